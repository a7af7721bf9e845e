"""Float64 restatements of the LoRA adapter arithmetic (include/aozora_hip.h az_lora_*, INTEGRATION.md "LoRA"): the three kernel shape
classes on exactly summable inputs, the six products of an adapted linear, and a LoraRefUNet that adds the adapters to the oracle's
linear layers.  The product never imports this file.  Plain torch on the CPU.

Exactly summable inputs follow tests/gemm_ref.py: operands are multiples of 2^-2 in [-4, 4], previous contents of an accumulated
output lie in [-8, 8], so every product is a multiple of 2^-4 and every partial sum is exact in fp32 while 16 S < 2^24 (S = sum of
|a||b|).  The adapter kernels multiply the finished sum by s = alpha / r before the previous contents are added.  For s in {1, 1/2, 2}
-- powers of two -- s * sum is exact, a multiple of 2^-5 at the finest, and so is s * sum + prev, whose magnitude is at most
s S + |prev|: representable while 32 (s S + |prev|) < 2^24 (and a contracted fma rounds the same exact value).  `exact_ok_scaled`
asserts both conditions; the expected output is then the one bf16 bit pattern gemm_ref.expected_bits gives."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import gemm_ref as R                      # noqa: E402
from oracle.unet_ref import RefUNet       # noqa: E402

EXACT_SCALES = (1.0, 0.5, 2.0)
RANKS = (4, 8, 16, 32, 64)


def exact_ok_scaled(S, s, prev=None):
    """gemm_ref.exact_ok extended for the factor s: the sum of products is exact (16 S < 2^24), s is a power of two among
    EXACT_SCALES, and s * sum (+ prev) is a multiple of 2^-5 below 2^24 * 2^-5."""
    assert float(s) in EXACT_SCALES, f"s = {s} is not one of the exact scales {EXACT_SCALES}"
    R.exact_ok(S)
    T = float(s) * S + (prev.double().abs() if prev is not None else 0.0)
    m = float(T.max()) if T.numel() else 0.0
    assert 32.0 * m < 2.0 ** 24, f"s * sum + prev is not exact in fp32: max = {m}"
    return True


# ---------------- the three kernel shape classes ------------------------------------------------------------------------------------
def down(x, w, parts, s, exact=True):
    """out[:, p r:(p+1) r] = s x_p w_p^T.  x [M][parts K] (one column slice per part), w [parts r][K].  -> (ref, S of s * sum)."""
    K = w.shape[1]
    r = w.shape[0] // parts
    P, S = [], []
    for p in range(parts):
        xp, wp = x[:, p * K:(p + 1) * K].double(), w[p * r:(p + 1) * r].double()
        P.append(xp @ wp.t()); S.append(xp.abs() @ wp.abs().t())
    P, S = torch.cat(P, 1), torch.cat(S, 1)
    if exact:
        exact_ok_scaled(S, s)
    return s * P, s * S


def up(u, w, y, parts, s, exact=True):
    """y[:, p N:(p+1) N] + s u_p w_p^T.  u [M][parts r], w [parts N][r], y [M][parts N].  -> (ref, S)."""
    r = w.shape[1]
    N = w.shape[0] // parts
    P, S = [], []
    for p in range(parts):
        up_, wp = u[:, p * r:(p + 1) * r].double(), w[p * N:(p + 1) * N].double()
        P.append(up_ @ wp.t()); S.append(up_.abs() @ wp.abs().t())
    P, S = torch.cat(P, 1), torch.cat(S, 1)
    if exact:
        exact_ok_scaled(S, s, y)
    return y.double() + s * P, s * S + y.double().abs()


def wgrad(small, big, prev, parts, s, small_major, exact=True):
    """(prev +) s small_p^T big_p.  small [M][parts ns], big [M][parts nb]; out [parts ns][nb] (small_major) or [parts nb][ns]."""
    ns, nb = small.shape[1] // parts, big.shape[1] // parts
    P, S = [], []
    for p in range(parts):
        sp, bp = small[:, p * ns:(p + 1) * ns].double(), big[:, p * nb:(p + 1) * nb].double()
        a, b = (sp.t() @ bp, sp.abs().t() @ bp.abs())
        P.append(a if small_major else a.t()); S.append(b if small_major else b.t())
    P, S = torch.cat(P, 0), torch.cat(S, 0)
    if exact:
        exact_ok_scaled(S, s, prev)
    if prev is None:
        return s * P, s * S
    return prev.double() + s * P, s * S + prev.double().abs()


# ---------------- the six products of one adapted linear ------------------------------------------------------------------------------
def bf(t):
    """Round to bf16 (nearest even) and return float64: what is stored between two kernels."""
    return t.float().bfloat16().double()


def lora_forward(x, y_base, A, B, s, rounded=True):
    """u = bf16(x A^T), y = bf16(y_base + s u B^T) (rounded=False: the same in exact float64 arithmetic).  -> (u, y)"""
    rd = bf if rounded else (lambda t: t)
    u = rd(x.double() @ A.double().t())
    return u, rd(y_base.double() + s * (u @ B.double().t()))


def lora_backward(x, u, dy, dx_base, A, B, s, dA_prev=None, dB_prev=None, rounded=True):
    """du = bf16(s dy B), dx = bf16(dx_base + du A), dA = bf16(dA_prev + du^T x), dB = bf16(dB_prev + s dy^T u).  -> (du, dx, dA, dB)"""
    rd = bf if rounded else (lambda t: t)
    du = rd(s * (dy.double() @ B.double()))
    dx = rd(dx_base.double() + du @ A.double())
    dA = rd((dA_prev.double() if dA_prev is not None else 0.0) + du.t() @ x.double())
    dB = rd((dB_prev.double() if dB_prev is not None else 0.0) + s * (dy.double().t() @ u))
    return du, dx, dA, dB


def merged_weight(W, A, B, s):
    """W + s B A in float64 (the trainer's save_merged forms it in fp32 and rounds once)."""
    return W.double() + s * (B.double() @ A.double())


# ---------------- the oracle UNet with adapters -------------------------------------------------------------------------------------
class LoraRefUNet(RefUNet):
    """RefUNet whose linear layers carry an adapter wherever the parameter dict holds `<module>.lora_A.weight` / `.lora_B.weight`:
    y = linear(x, W, b) + s linear(linear(x, A), B)."""

    def __init__(self, cfg, params, scale):
        super().__init__(cfg, params)
        self.scale = scale

    def _lin(self, x, name, bias=True):
        y = super()._lin(x, name, bias)
        A = self.p.get(name + ".lora_A.weight")
        if A is None:
            return y
        return y + self.scale * F.linear(F.linear(x, A), self.p[name + ".lora_B.weight"])
