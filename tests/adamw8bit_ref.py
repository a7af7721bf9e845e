"""CPU restatement of the paged_adamw_8bit update: numpy float32, one rounding per operation, no
contraction.  The product never imports this file; tests compare the HIP kernel against it bit for bit.

Tensors here are in LOGICAL flat order (p.view(-1) of the reference's parameter).  Parameters are bf16 bit patterns (uint16),
gradients are their fp32 values, codes are uint8, absmax / moments fp32."""
import math

import numpy as np
import torch

BLOCK = 256
MIN_8BIT = 4096
F32 = np.float32


def dynamic_map(signed: bool) -> np.ndarray:
    """bitsandbytes' create_dynamic_map(signed, max_exponent_bits=7, total_bits=8)."""
    data = []
    for i in range(7):
        k = 2 ** i if signed else 2 ** (i + 1)
        b = torch.linspace(0.1, 1, k + 1)
        means = (b[:-1] + b[1:]) / 2.0
        data += ((10 ** (i - 6)) * means).tolist()
        if signed:
            data += (-(10 ** (i - 6)) * means).tolist()
    data += [0, 1.0]
    data.sort()
    q = np.array(data, dtype=np.float32)
    assert q.shape == (256,) and np.all(np.diff(q) > 0) and q.max() == 1.0 and int((q == 0).sum()) == 1
    return q


def hyper(lr, betas, eps, wd, t):
    """Per-step constants: float64 on the host, one rounding to fp32 each."""
    b1, b2 = float(betas[0]), float(betas[1])
    c1, c2 = 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)
    return dict(b1=F32(b1), b2=F32(b2), omb1=F32(1.0 - b1), omb2=F32(1.0 - b2), step_size=F32(-lr * c2 / c1),
                eps_c=F32(eps * c2), decay=F32(1.0 - lr * wd), wd_pos=wd > 0)


def bf16_round(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 (round to nearest even, NaN kept) -> fp32."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    nan = np.isnan(np.asarray(x, dtype=np.float32))
    r = np.where(nan, (u | 0x00400000) >> 16 << 16, r)
    return r.astype(np.uint32).view(np.float32)


def bf16_bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_bits(x: np.ndarray) -> np.ndarray:
    return (bf16_round(x).view(np.uint32) >> 16).astype(np.uint16)


def encode(x: np.ndarray, qmap: np.ndarray) -> np.ndarray:
    """Nearest map entry: lo = largest index with qmap[lo] <= x (0 if none; 8-step binary search), hi = min(lo+1, 255),
    hi iff (qmap[hi]-x) < (x-qmap[lo]) in fp32: ties go to lo.  A NaN x gives 0."""
    x = np.asarray(x, dtype=np.float32)
    lo = np.zeros(x.shape, dtype=np.int64)
    for step in (128, 64, 32, 16, 8, 4, 2, 1):
        lo = np.where(qmap[lo + step] <= x, lo + step, lo)
    hi = np.minimum(lo + 1, 255)
    pick_hi = (qmap[hi] - x) < (x - qmap[lo])
    return np.where(pick_hi, hi, lo)


def quantize(vals: np.ndarray, absmax, qmap: np.ndarray, signed: bool) -> np.ndarray:
    """Codes of values against their block's (new) absmax (a scalar or one per value), with bitsandbytes' sign rule on the
    signed map; absmax 0 gives the code of 0.0."""
    vals = np.asarray(vals, dtype=np.float32)
    absmax = np.broadcast_to(np.asarray(absmax, dtype=np.float32), vals.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = encode(vals / absmax, qmap)
    if signed:
        neg_code = np.signbit(qmap[c])
        c = np.where((vals > 0) & neg_code, c + 1, c)
        c = np.where((vals < 0) & ~neg_code, c - 1, c)
    c = np.where(absmax == 0, int(np.argmax(qmap == 0)), c)
    return c.astype(np.uint8)


def _grad(g, coef):
    g = np.asarray(g, dtype=np.float32)
    if coef is not None:
        g = bf16_round(g * F32(coef))
    return g


def _apply(p_bits, g, m, v, h):
    """Parameter update (both paths): only where g is finite; decay after the update."""
    p = bf16_bits_to_f32(p_bits)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        den = np.sqrt(v) + h["eps_c"]
        upd = h["step_size"] * (m / den)
        pn = bf16_round(p + upd)
        if h["wd_pos"]:
            pn = bf16_round(pn * h["decay"])
    fin = np.isfinite(g)
    return np.where(fin, f32_to_bf16_bits(pn), p_bits).astype(np.uint16)


def step_8bit(p_bits, g, c1, c2, absmax1, absmax2, q1, q2, h, coef=None):
    """One step of an 8-bit-state tensor.  Returns new (p_bits, c1, c2, absmax1, absmax2).  Blocks are rows of a [nb, 256]
    view; padding slots of a short last block are excluded from absmax and dropped."""
    g = _grad(g, coef)
    n = g.size
    nb = (n + BLOCK - 1) // BLOCK
    pad = nb * BLOCK - n

    def rows(x, fill):
        return np.concatenate([x, np.full(pad, fill, dtype=x.dtype)]).reshape(nb, BLOCK)
    G, C1, C2 = rows(g, F32(0)), rows(c1, 0), rows(c2, 0)
    valid = rows(np.ones(n, bool), False)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = q1[C1] * absmax1[:, None]
        v = q2[C2] * absmax2[:, None]
        v = v * h["b2"] + (h["omb2"] * G) * G
        m = m * h["b1"] + h["omb1"] * G
        a1 = np.fmax.reduce(np.where(valid, np.abs(m), F32(0)), axis=1, initial=F32(0)).astype(np.float32)   # NaN ignored
        a2 = np.fmax.reduce(np.where(valid, np.abs(v), F32(0)), axis=1, initial=F32(0)).astype(np.float32)
        m, v = m.reshape(-1)[:n], v.reshape(-1)[:n]
        pn = _apply(p_bits, g, m, v, h)
        blk = np.arange(n) // BLOCK
        c1n = quantize(m, a1[blk], q1, True)
        c2n = quantize(v, a2[blk], q2, False)
    return pn, c1n, c2n, a1, a2


def step_32bit(p_bits, g, m, v, h, coef=None):
    """One step of an fp32-state tensor (numel < 4096).  Returns new (p_bits, m, v)."""
    g = _grad(g, coef)
    with np.errstate(invalid="ignore", over="ignore"):
        m = m * h["b1"] + h["omb1"] * g
        v = v * h["b2"] + h["omb2"] * (g * g)
    return _apply(p_bits, g, m, v, h), m.astype(np.float32), v.astype(np.float32)


class RefAdamW8bit:
    """The restatement as an optimizer over a list of logical-order tensors (numpy)."""

    def __init__(self, sizes, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, min_8bit_size=MIN_8BIT):
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.q1, self.q2 = dynamic_map(True), dynamic_map(False)
        self.t = 0
        self.state = []
        for n in sizes:
            if n < min_8bit_size:
                self.state.append(dict(m=np.zeros(n, np.float32), v=np.zeros(n, np.float32)))
            else:
                nb = (n + BLOCK - 1) // BLOCK
                self.state.append(dict(c1=np.zeros(n, np.uint8), c2=np.zeros(n, np.uint8),
                                       a1=np.zeros(nb, np.float32), a2=np.zeros(nb, np.float32)))

    def step(self, params, grads, coef=None):
        """params: list of uint16 bf16 bit arrays (updated and returned); grads: list of fp32 arrays."""
        self.t += 1
        h = hyper(self.lr, self.betas, self.eps, self.wd, self.t)
        out = []
        for p, g, st in zip(params, grads, self.state):
            if "m" in st:
                p, st["m"], st["v"] = step_32bit(p, g, st["m"], st["v"], h, coef)
            else:
                p, st["c1"], st["c2"], st["a1"], st["a2"] = step_8bit(p, g, st["c1"], st["c2"], st["a1"], st["a2"],
                                                                       self.q1, self.q2, h, coef)
            out.append(p)
        return out
