"""Numpy restatement of the stochastic-rounding parameter write of az_adamw_flat_sr / az_raven_step_sr (csrc/az_optim.hip):
Philox4x32-10, the 16 bits an element receives, the rounding rule, and the whole update built on elem_ref.adamw_bits' arithmetic.

Counter layout: key = (seed low word, seed high word); counter = (group low word, group high word, step, domain) with
group = e >> 3 for the element's GLOBAL index e; element e takes the low (e even) or high (e odd) half of output word (e & 7) >> 1."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import elem_ref as R        # noqa: E402

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape, key: two uint32 scalars -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                    # 32 x 32 -> 64 bits: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _MASK, p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def sr_bits16(seed, step, domain, e):
    """The 16 random bits of the elements with global indices e (int64 array) -> uint32 array in [0, 65536)."""
    e = np.asarray(e, dtype=np.int64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    grp = (e >> 3).astype(np.uint64)
    out = philox4x32_10((grp & _MASK, grp >> np.uint64(32), np.uint64(int(step) & 0xFFFFFFFF), np.uint64(int(domain) & 0xFFFFFFFF)),
                        (seed & 0xFFFFFFFF, seed >> 32))
    word = np.choose(((e & 7) >> 1).astype(np.int64), out)
    return (word >> ((e & 1) << 4).astype(np.uint32)) & np.uint32(0xFFFF)


def sr_round(pp_f32, r16):
    """fp32 array, uint32 array in [0, 65536) -> uint16 bf16 bits.  Non-finite values as round-to-nearest gives them; otherwise
    (bits + r) >> 16, truncation where that would carry into the all-ones exponent."""
    u = np.ascontiguousarray(pp_f32, dtype=np.float32).view(np.uint32)
    r = np.asarray(r16, dtype=np.uint32)
    o = (u + r) >> 16                                    # u <= 0xFF7FFFFF where it is used: no 32-bit overflow
    o = np.where((o & 0x7F80) == 0x7F80, u >> 16, o)
    nonfinite = (u & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
    return np.where(nonfinite, R.bf16_bits_np(pp_f32), o.astype(np.uint16)).astype(np.uint16)


def adamw_pp(p, g, m, v, hyper, coef=None):
    """elem_ref.adamw_bits' arithmetic up to the fp32 parameter value: -> (pp float32 numpy, m, v as adamw_bits stores them)."""
    mdtype = {torch.bfloat16: 0, torch.float32: 1, torch.float16: 2}[m.dtype]
    f = np.float32
    b1, b2, eps, wdf, step, sbc2 = (f(hyper[i]) for i in range(1, 7))
    omb1, omb2 = f(1.0) - b1, f(1.0) - b2
    with np.errstate(all="ignore"):
        gr = g.float().numpy() * (f(coef) if coef is not None else f(1.0))
        if g.dtype == torch.bfloat16:
            gr = R.bf16_round_np(gr)
        mm = R.fma32(gr, np.full_like(gr, omb1), m.float().numpy() * b1)
        vv = v.float().numpy() * b2
        vv = vv + ((omb2 * gr) * gr)
        pp = R.bf16_to_np(p) * wdf
        denom = np.sqrt(vv) / sbc2 + eps
        pp = pp + ((-step * mm) / denom)
    return pp, R._store(mm, mdtype), R._store(vv, mdtype)


def adamw_sr_bits(p, g, m, v, hyper, coef, seed, step, domain, elem0):
    """az_adamw_flat_sr on CPU tensors -> (p, m, v) new tensors.  m and v are those of elem_ref.adamw_bits; p is the same fp32 value
    written with stochastic rounding, element i using the bits of global index elem0 + i."""
    pp, m2, v2 = adamw_pp(p, g, m, v, hyper, coef)
    e = np.int64(elem0) + np.arange(pp.shape[0], dtype=np.int64)
    return R.bits_to_bf16(sr_round(pp, sr_bits16(seed, step, domain, e))), m2, v2


# ---- the drift experiment of the issue: uniform weights, constant gradient, the reference's default hyper-parameters ------------
DRIFT = dict(n=65536, p0=0.0234375, g=1.0, steps=64, lr=8e-7, betas=(0.9, 0.999), wd=0.01, eps=1e-8, debias=0.3, seeds=(42, 7, 123456789012))
DRIFT_ULP = 2.0 ** -13            # bf16 spacing at 0.0234375 (in [2^-6, 2^-5))
DRIFT_BOUND_ULP = 6.0 / 64.0      # six standard deviations: 64 per-step errors of variance <= ulp^2 / 4, mean of 65 536 elements


def drift_hyper(step):
    d = DRIFT
    return R.adamw_hyper(d["lr"], d["betas"], d["wd"], d["eps"], d["debias"], step)


def drift_master():
    """The fp32 master copy after DRIFT['steps'] steps (the kernel's arithmetic, p kept in fp32): a scalar (all elements alike)."""
    f = np.float32
    p, m, v = f(DRIFT["p0"]), f(0.0), f(0.0)
    g = np.array([DRIFT["g"]], dtype=f)
    p, m, v = np.array([p]), np.array([m]), np.array([v])
    for s in range(1, DRIFT["steps"] + 1):
        _, b1, b2, eps, wdf, step, sbc2, _ = (f(x) for x in drift_hyper(s))
        m = R.fma32(g, np.array([f(1.0) - b1]), m * b1)
        v = v * b2 + (((f(1.0) - b2) * g) * g)
        p = p * wdf
        p = p + ((-step * m) / (np.sqrt(v) / sbc2 + eps))
    return float(p[0])
