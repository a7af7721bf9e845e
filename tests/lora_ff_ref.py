"""Float64 restatement of az_lora_up_geglu_bf16 (include/aozora_hip.h): the up product of ff.net.0.proj with the GEGLU in its epilogue.

    proj[m][n] = bf16(float(proj[m][n]) + s sum_{k < r} U[m][k] W[n][k])            n < 2 H       -- lora_ref.up with parts = 1
    out[m][h]  = bf16(float(proj[m][h]) * gelu_erf(float(proj[m][H + h])))          h < H         -- on the ROUNDED, stored proj

The first line is exact on the inputs of tests/lora_ref.py (one bf16 bit pattern per element: gemm_ref.expected_bits).  The second is
not -- gelu is transcendental -- so its bits are whatever az_geglu_fwd computes from the same stored proj (the rule the fused GEGLU
GEMM follows as well); `geglu` gives the float64 value those bits approximate.  The product never imports this file."""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lora_ref as LR                     # noqa: E402


def geglu(proj):
    """proj [M][2 H] (value | gate halves) -> value * gelu(gate) with the exact-erf GELU, float64."""
    p = proj.double()
    H = p.shape[1] // 2
    a, g = p[:, :H], p[:, H:]
    return a * (0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0))))


def up_geglu(u, w, y, s, exact=True):
    """u [M][r], w [2 H][r], y [M][2 H] (the previous proj).  -> (proj ref, S, out ref): proj ref and S are lora_ref.up's (parts = 1),
    out ref is the GEGLU of the proj the kernel STORES (proj ref rounded to bf16)."""
    assert w.shape[0] % 2 == 0 and y.shape == (u.shape[0], w.shape[0]) and u.shape[1] == w.shape[1]
    ref, S = LR.up(u, w, y, 1, s, exact=exact)
    return ref, S, geglu(LR.bf(ref))
