"""Kernels behind latent sizes that are not multiples of 4: the upsample gather of the implicit-GEMM convolution with a cropped
target, the stand-alone sized upsample and its adjoint, stride-2 convolutions on odd extents, and the token counts of the
1440x720 bucket (latent 90x180 -> 45x90 -> 23x45: 4050 and 1035 tokens) through the attention and norm kernels.

Reference: fp32 torch on the CPU on identical bf16-rounded inputs; bounds as tests/test_kernels_gpu.py applies to the same entry
points (relative Frobenius <= 4e-3 and max <= 2e-2; fused sums 4e-3 / 3e-2; attention / norm gradients as there), under the
same forced tiles."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_kernels_gpu import DEV, bf, check, ops, rnd, tile      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CROPS = [(0, 0), (1, 0), (0, 1), (1, 1)]


# ---- convolution with the cropped upsample gather ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Hs,Ws,Cin,Cout,crop_h,crop_w", [(2, 8, 8, 64, 64, 1, 1), (1, 6, 10, 128, 72, 1, 0), (2, 5, 7, 72, 40, 0, 1),
                                                            (1, 23, 45, 64, 64, 1, 0)])      # the last: the bucket's 23x45 -> 45x90 (4050 pixels)
def test_conv_with_cropped_upsample_gather(ops, tile, B, Hs, Ws, Cin, Cout, crop_h, crop_w):
    """Upsample2D with a target size (F.interpolate(size=(2n - 1, ...)) -> 3x3 conv) folded into the conv's operand gather: forward
    and weight gradient read the half-resolution tensor; a tap beyond the cropped edge is zero padding."""
    H, W = 2 * Hs - crop_h, 2 * Ws - crop_w
    x, w, b = rnd(B, Hs, Ws, Cin), rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5), rnd(Cout)
    xn = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    wn = w.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.conv2d(F.interpolate(xn, size=(H, W), mode="nearest"), wn, b.float(), padding=1)
    out = torch.empty(B, H, W, Cout, dtype=torch.bfloat16, device=DEV)
    ops.conv_fwd(x.to(DEV), w.to(DEV), out, bias=b.to(DEV), upsample=True)
    check(out, y.permute(0, 2, 3, 1), f"conv_fwd cropped upsample {B,Hs,Ws,Cin,Cout,crop_h,crop_w}")
    # the same through the stand-alone sized upsample and a plain convolution: bit-identical (same products, same order)
    xu = torch.empty(B, H, W, Cin, dtype=torch.bfloat16, device=DEV)
    ops.upsample_nearest_fwd(x.to(DEV), xu)
    out2 = torch.empty_like(out)
    ops.conv_fwd(xu, w.to(DEV), out2, bias=b.to(DEV))
    assert torch.equal(out, out2)
    dy = rnd(B, H, W, Cout)
    y.backward(dy.float().permute(0, 3, 1, 2))
    prev = rnd(Cout, 3, 3, Cin, scale=0.05)
    dw, bg = prev.to(DEV).clone(), torch.zeros(Cout, dtype=torch.bfloat16, device=DEV)
    ops.conv_wgrad(dy.to(DEV), x.to(DEV), dw, accumulate=True, split_k=0, bias_grad=bg, upsample=True)
    check(dw, prev.float() + wn.grad.permute(0, 2, 3, 1), f"conv_wgrad cropped upsample {B,Hs,Ws,Cin,Cout,crop_h,crop_w}")
    dw2 = prev.to(DEV).clone()
    ops.conv_wgrad(dy.to(DEV), xu, dw2, accumulate=True, split_k=0)
    assert torch.equal(dw, dw2)
    dw3 = prev.to(DEV).clone()
    ops.conv_wgrad(dy.to(DEV), x.to(DEV), dw3, accumulate=True, split_k=0, upsample=True)      # without the fused bias gradient
    assert torch.equal(dw, dw3)
    check(bg, dy.float().sum((0, 1, 2)), "bias grad", fro=4e-3, mx=3e-2)


def test_upsample_target_must_be_2n_or_2n_minus_1(ops):
    from aozora_sdxl_training_amd._lib import AozoraError, lib
    import ctypes
    x = torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16, device=DEV)
    for Ho, Wo in [(6, 8), (8, 9), (9, 8), (4, 4)]:
        y = torch.zeros(1, Ho, Wo, 8, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(AozoraError):
            ops.upsample_nearest_fwd(x, y)
        with pytest.raises(AozoraError):
            ops.upsample_nearest_bwd(y, x)
        with pytest.raises(AozoraError):      # the entry point itself refuses too, not only the Python wrapper
            lib().call("az_upsample_nearest_fwd", 1, 4, 4, Ho, Wo, 8, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        w = torch.zeros(8, 3, 3, 8, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(AozoraError):
            ops.conv_fwd(x, w, y, upsample=True)


# ---- stand-alone sized upsample and its adjoint -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C", [(2, 37, 29, 1280), (1, 5, 3, 8), (3, 1, 1, 16)])
@pytest.mark.parametrize("crop_h,crop_w", CROPS)
def test_sized_upsample_forward_and_adjoint_are_exact(ops, B, H, W, C, crop_h, crop_w):
    Ho, Wo = 2 * H - crop_h, 2 * W - crop_w
    x, dy = rnd(B, H, W, C), rnd(B, Ho, Wo, C)
    xn = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    ref = F.interpolate(xn, size=(Ho, Wo), mode="nearest")
    y = torch.full((B, Ho, Wo, C), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.upsample_nearest_fwd(x.to(DEV), y)
    assert torch.equal(y.cpu().float(), ref.detach().permute(0, 2, 3, 1))
    ref.backward(dy.float().permute(0, 3, 1, 2))       # fp32 sums of at most four bf16 values ...
    dx = torch.full((B, H, W, C), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.upsample_nearest_bwd(dy.to(DEV), dx)
    # ... rounded once.  Sums of up to four bf16 values are not always exact in fp32 order-independently, so the reference sums
    # them in the kernel's order (dy-row major) as well; both must agree with autograd to fp32 rounding and with the kernel bit for bit
    from tests.oddsize_ref import cropped_fold
    fold = cropped_fold(dy.permute(0, 3, 1, 2), H, W)
    assert torch.allclose(fold, xn.grad, rtol=0, atol=1e-5)
    assert torch.equal(dx.cpu(), bf(fold.permute(0, 2, 3, 1)))
    if (crop_h, crop_w) == (0, 0):        # the uncropped case is the existing nearest-2x pair, bit for bit
        y2, dx2 = torch.empty_like(y), torch.empty_like(dx)
        ops.upsample2x_fwd(x.to(DEV), y2)
        ops.upsample2x_bwd(dy.to(DEV), dx2)
        assert torch.equal(y, y2) and torch.equal(dx, dx2)


# ---- stride 2 on odd sides (45 -> 23) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 9, 7, 64, 128), (1, 45, 90, 64, 64), (1, 13, 11, 72, 40)])
def test_stride2_conv_on_odd_sides(ops, tile, B, H, W, Cin, Cout):
    x, w, b = rnd(B, H, W, Cin), rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5), rnd(Cout)
    xn = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    wn = w.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.conv2d(xn, wn, b.float(), stride=2, padding=1)
    Ho, Wo = y.shape[2], y.shape[3]
    assert (Ho, Wo) == ((H + 1) // 2, (W + 1) // 2)
    tag = f"{B,H,W,Cin,Cout}"
    out = torch.empty(B, Ho, Wo, Cout, dtype=torch.bfloat16, device=DEV)
    ops.conv_fwd(x.to(DEV), w.to(DEV), out, stride=2, bias=b.to(DEV))
    check(out, y.permute(0, 2, 3, 1), "stride-2 conv_fwd " + tag)
    dy = rnd(B, Ho, Wo, Cout)
    y.backward(dy.float().permute(0, 3, 1, 2))
    dyd = dy.to(DEV)
    dx = torch.empty(B, H, W, Cin, dtype=torch.bfloat16, device=DEV)
    ops.conv_dgrad(dyd, w.to(DEV), dx, stride=2, cout_real=Cout)
    check(dx, xn.grad.permute(0, 2, 3, 1), "stride-2 conv_dgrad " + tag)
    wt = w.permute(3, 1, 2, 0).contiguous().to(DEV)
    dx2 = torch.empty_like(dx)
    ops.conv_dgrad_wt(dyd, wt, dx2, stride=2)
    check(dx2, xn.grad.permute(0, 2, 3, 1), "stride-2 conv_dgrad_wt " + tag)
    prev = rnd(Cout, 3, 3, Cin, scale=0.05)
    dw = prev.to(DEV).clone()
    ops.conv_wgrad(dyd, x.to(DEV), dw, stride=2, accumulate=True, split_k=0)
    check(dw, prev.float() + wn.grad.permute(0, 2, 3, 1), "stride-2 conv_wgrad " + tag)
    dw2, bg = prev.to(DEV).clone(), torch.zeros(Cout, dtype=torch.bfloat16, device=DEV)
    ops.conv_wgrad(dyd, x.to(DEV), dw2, stride=2, accumulate=True, split_k=0, bias_grad=bg)
    assert torch.equal(dw2, dw), "the fused bias gradient must not change dW"
    check(bg, dy.float().sum((0, 1, 2)), "stride-2 fused bias grad " + tag, fro=4e-3, mx=3e-2)


# ---- the bucket's token counts through kernels that exist already -----------------------------------------------------------------
@pytest.mark.parametrize("B,heads,Tq,Tk", [(1, 2, 1035, 1035), (1, 1, 4050, 4050), (1, 2, 1035, 77)])
def test_attention_at_the_bucket_token_counts(ops, B, heads, Tq, Tk):
    from tests.test_kernels_gpu import test_attention_fwd_bwd
    test_attention_fwd_bwd(ops, B, heads, Tq, Tk)


@pytest.mark.parametrize("HW", [1035, 4050])
@pytest.mark.parametrize("C,G", [(64, 8), (320, 32)])      # the mini configuration's and SDXL's first level
def test_groupnorm_at_the_bucket_token_counts(ops, HW, C, G):
    from tests.test_kernels_gpu import test_groupnorm_fwd_bwd
    test_groupnorm_fwd_bwd(ops, 1, HW, C, G, True, 1e-5)


def test_layernorm_at_the_bucket_token_count(ops):
    from tests.test_kernels_gpu import test_layernorm_fwd_bwd
    test_layernorm_fwd_bwd(ops, 1035, 640)
