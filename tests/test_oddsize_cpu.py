"""Latent sizes that are not multiples of 4, CPU part: the odd-size oracle helper (tests/oddsize_ref.py) against the unmodified
oracle, and the two facts the kernels rest on -- F.interpolate(size=) to 2n or 2n - 1 reads source index dst >> 1, and its
adjoint is the 2x2 fold with fewer terms on a cropped edge."""
import pytest
import torch
import torch.nn.functional as F

from tests.oddsize_ref import OddSizeRefUNet, cropped_fold


def _mini():
    from aozora_sdxl_training_amd.unet_spec import mini_config
    from oracle.unet_ref import UNetConfig as OC, init_params
    pc = mini_config()
    oc = OC(block_out_channels=pc.block_out_channels, transformer_layers=pc.transformer_layers, head_dim=64,
            cross_attention_dim=pc.cross_attention_dim, addition_time_embed_dim=pc.addition_time_embed_dim,
            pooled_dim=pc.pooled_dim, norm_groups=pc.norm_groups)
    params = {k: v.bfloat16().float() for k, v in init_params(oc, seed=1234).items()}
    return pc, oc, params


def _inputs(B, h, w, pc, seed=7):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(B, 4, h, w, generator=g).bfloat16()
    noise = torch.randn(B, 4, h, w, generator=g)
    ctx = torch.randn(B, 77, pc.cross_attention_dim, generator=g).bfloat16()
    pooled = torch.randn(B, pc.pooled_dim, generator=g).bfloat16()
    tid = torch.tensor([[h * 8, w * 8, 0, 0, h * 8, w * 8]] * B, dtype=torch.bfloat16)
    return lat, noise, torch.tensor([37, 911][:B]), ctx, pooled, tid


@pytest.mark.parametrize("bf16", [False, True])
def test_helper_equals_oracle_bit_for_bit_on_a_multiple_of_4(bf16):
    from oracle.step_ref import RefTrainer
    pc, oc, params = _mini()
    args = _inputs(2, 16, 16, pc)
    a = RefTrainer(oc, params, mode="epsilon", bf16=bf16, ga=1, clip=1.0)
    b = RefTrainer(oc, params, mode="epsilon", bf16=bf16, ga=1, clip=1.0)
    b.net = OddSizeRefUNet(oc, b.params)
    la, lb = a.micro_step(*args), b.micro_step(*args)
    assert la == lb and torch.equal(a.last_pred, b.last_pred)
    ga, gb = a.grads(), b.grads()
    assert set(ga) == set(gb) == set(params)
    assert all(torch.equal(ga[k], gb[k]) for k in ga)


def test_unmodified_oracle_raises_and_helper_runs_on_18x10():
    from oracle.step_ref import RefTrainer
    pc, oc, params = _mini()
    args = _inputs(2, 18, 10, pc)
    with pytest.raises(RuntimeError):
        RefTrainer(oc, params, mode="epsilon", bf16=False, ga=1, clip=1.0).micro_step(*args)
    t = RefTrainer(oc, params, mode="epsilon", bf16=False, ga=1, clip=1.0)
    t.net = OddSizeRefUNet(oc, t.params)
    loss = t.micro_step(*args)
    assert loss == loss and t.last_pred.shape == (2, 4, 18, 10)
    g = t.grads()
    assert len(g) == len(params) and all(v.norm().item() > 1e-6 for v in g.values())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_nearest_to_size_reads_index_dst_shift_1(dtype):
    for n in range(1, 400):
        src = torch.arange(n, dtype=torch.float32).view(1, 1, n, 1)      # values are the source indices (exact in bf16 below 257:
        if dtype == torch.bfloat16:                                       # compare through a second channel of residues for larger n)
            src = torch.cat([(src // 256), (src % 256)], dim=1)
        for o in (2 * n - 1, 2 * n):
            got = F.interpolate(src.to(dtype), size=(o, 1), mode="nearest").float()
            idx = got[0, 0, :, 0] if dtype == torch.float32 else got[0, 0, :, 0] * 256 + got[0, 1, :, 0]
            assert torch.equal(idx.long(), torch.arange(o) >> 1), (n, o)


@pytest.mark.parametrize("H,W,ch,cw", [(5, 3, 0, 0), (5, 3, 1, 0), (5, 3, 0, 1), (5, 3, 1, 1), (1, 1, 1, 1), (23, 45, 1, 0)])
def test_cropped_fold_is_the_autograd_of_interpolate_to_size(H, W, ch, cw):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(2, 3, H, W, generator=g, requires_grad=True)
    Ho, Wo = 2 * H - ch, 2 * W - cw
    y = F.interpolate(x, size=(Ho, Wo), mode="nearest")
    dy = torch.randn(2, 3, Ho, Wo, generator=g)
    y.backward(dy)
    # the forward is the 2x image with its last row / column cropped
    assert torch.equal(y.detach(), F.interpolate(x.detach(), scale_factor=2.0, mode="nearest")[:, :, :Ho, :Wo])
    assert torch.allclose(cropped_fold(dy, H, W), x.grad, rtol=0, atol=1e-6)
    # a pixel on a cropped edge receives 2 or 1 contributions
    ones = cropped_fold(torch.ones(1, 1, Ho, Wo), H, W)
    assert ones[0, 0, H - 1, W - 1].item() == (2 - ch) * (2 - cw)
    assert H == 1 or W == 1 or ones[0, 0, 0, 0].item() == 4
