"""Float64 restatements of the adapter arithmetic on 3x3 convolutions (include/aozora_hip.h az_lora_conv_*, INTEGRATION.md "LoRA"):
the three gathered products with S = sum |a||b| for the exactness conditions of tests/lora_ref.exact_ok_scaled, and a
LoraConvRefUNet that adds the adapters to the oracle's convolutions.  The product never imports this file.  Plain torch on the CPU.

Activations are NHWC rows [B H W][C]; the down matrix is a [r][3][3][Cin] (the device layout: the base conv weight's own).  Pixel
m = (b, h, w) meets, at tap t = 3 kh + kw, pixel (b, h + kh - 1, w + kw - 1) -- the data gradient the mirrored (b, h - kh + 1,
w - kw + 1) -- and nothing outside image b.  The gather below is written with padded slices and shares no code with the index
tables of tests/gemm_ref.py; tests/test_lora_conv_ref_cpu.py checks it against F.conv2d and its autograd."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import lora_ref as LR                     # noqa: E402
from oddsize_ref import OddSizeRefUNet    # noqa: E402


def gather(x, geom, mirrored=False):
    """x [B H W][C] -> float64 [B H W][9][C]: tap t = 3 kh + kw holds the row of pixel (h + kh - 1, w + kw - 1) of the same image
    (mirrored: (h - kh + 1, w - kw + 1)), zeros where that pixel lies outside it."""
    B, H, W = geom
    C = x.shape[1]
    pad = F.pad(x.double().reshape(B, H, W, C), (0, 0, 1, 1, 1, 1))
    taps = []
    for kh in range(3):
        for kw in range(3):
            oh, ow = (2 - kh, 2 - kw) if mirrored else (kh, kw)
            taps.append(pad[:, oh:oh + H, ow:ow + W].reshape(B * H * W, C))
    return torch.stack(taps, 1)


def _finish(P, S, s, prev, exact):
    # a sum that starts from +0 is +0 when it is zero (round to nearest: +0 + -0 = +0); an einsum over a single term -- one pixel, a
    # tap outside the image times a negative partner -- would hand back that term's -0
    P = P + 0.0
    if exact:
        LR.exact_ok_scaled(S, s, prev)
    if prev is None:
        return s * P, s * S
    return prev.double() + s * P, s * S + prev.double().abs()


def down(x, a, geom, s, exact=True):
    """U[m][j] = s sum_t sum_c X[nbr(m, t)][c] A[j][t][c].  -> (ref [B H W][r], S)"""
    r = a.shape[0]
    G, a9 = gather(x, geom), a.double().reshape(r, 9, -1)
    return _finish(torch.einsum("mtc,jtc->mj", G, a9), torch.einsum("mtc,jtc->mj", G.abs(), a9.abs()), s, None, exact)


def dgrad(du, a, prev, geom, s, exact=True):
    """dX[m][c] = prev[m][c] + s sum_t sum_j dU[nbr'(m, t)][j] A[j][t][c] (mirrored taps).  -> (ref [B H W][Cin], S)"""
    r = a.shape[0]
    G, a9 = gather(du, geom, mirrored=True), a.double().reshape(r, 9, -1)
    return _finish(torch.einsum("mtj,jtc->mc", G, a9), torch.einsum("mtj,jtc->mc", G.abs(), a9.abs()), s, prev, exact)


def wgrad(du, x, prev, geom, s, exact=True):
    """dA[j][t][c] = (prev +) s sum_m dU[m][j] X[nbr(m, t)][c].  -> (ref [r][3][3][Cin], S)"""
    r, C = du.shape[1], x.shape[1]
    G, d = gather(x, geom), du.double()
    P, S = torch.einsum("mj,mtc->jtc", d, G).reshape(r, 3, 3, C), torch.einsum("mj,mtc->jtc", d.abs(), G.abs()).reshape(r, 3, 3, C)
    return _finish(P, S, s, prev, exact)


def to_nchw(x, geom):
    """[B H W][C] rows -> (B, C, H, W)."""
    B, H, W = geom
    return x.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def to_oihw(a):
    """device layout [r][3][3][Cin] -> logical (r, Cin, 3, 3) (what the parameter exposes and the adapter file holds)."""
    return a.permute(0, 3, 1, 2)


def merged_conv_weight(W, A, B, s):
    """W[o][c][kh][kw] + s sum_j B[o][j] A[j][c][kh][kw] in float64 (logical shapes; a 2-D A is a 1x1 convolution's)."""
    A4 = A.double() if A.dim() == 4 else A.double()[:, :, None, None]
    return W.double() + s * torch.einsum("oj,jchw->ochw", B.double(), A4)


class LoraConvRefUNet(LR.LoraRefUNet):
    """LoraRefUNet whose convolutions carry an adapter too wherever the parameter dict holds one: y = conv(x, W, b) + s conv1x1(
    conv(x, A), B), with s the module's own alpha / rank (`spec`: unet_spec.LoraSpec -- conv_rank / conv_alpha govern conv1 / conv2,
    rank / alpha the 1x1 conv_shortcut and every linear)."""

    def __init__(self, cfg, params, spec):
        super().__init__(cfg, params, spec.scale)
        self.spec = spec

    def _conv(self, x, name, stride=1, pad=1):
        y = super()._conv(x, name, stride, pad)
        A = self.p.get(name + ".lora_A.weight")
        if A is None:
            return y
        Bm = self.p[name + ".lora_B.weight"]
        if A.dim() == 4:
            assert stride == 1 and pad == 1, name
            u = F.conv2d(x, A, padding=1)
        else:
            assert stride == 1 and pad == 0, name
            u = F.conv2d(x, A[:, :, None, None])
        return y + self.spec.scale_of(name) * F.conv2d(u, Bm[:, :, None, None])


class LoraConvOddRefUNet(OddSizeRefUNet, LoraConvRefUNet):
    """The same at latent sizes that are no multiple of 4: tests/oddsize_ref.py's size-targeted upsamples around the adapted layers."""
