"""DoRA (weight-decomposed LoRA, Liu et al. arXiv 2402.09353; include/aozora_hip.h az_dora_*, INTEGRATION.md "DoRA") restated on the
CPU: the contract in float64 and in its rounded steps (bf16 stores, fp32 sums), built on tests/lora_ref.py; bit-level restatements of
the three kernels in numpy float32; the bound on the kernel's fp32 n2; the inputs the tests share; and DoraRefUNet, the oracle UNet with
magnitudes.  The product never imports this file.

The contract (W [N][K], A [r][K], B [N][r], s = alpha / r, magnitude m [N], all bf16 in memory):
    n2[o] = sum_k (W[o][k] + s sum_j B[o][j] A[j][k])^2      inv[o] = 1 / sqrt(n2[o])      g[o] = m[o] inv[o]        (fp32 vectors)
    forward    v = bf16(x W^T), u = bf16(x A^T), v = bf16(v + s u B^T), y = bf16(fma(g[o], v, bias[o]) + residual)
    backward   dv = bf16(g[o] dy)   dm[o] = bf16(dm[o] + inv[o] sum_rows dy v)   then LoRA's backward on dv; the norm is a constant
    init       B = 0, m = bf16(sqrt(n2)): g = bf16(n) / n, within 2^-8 of 1 (half an ulp of bf16's 8 significant bits), not exactly 1
    merged     W'[o][:] = (m[o] / n[o]) (W + s B A)[o][:]

The bound on n2.  A kernel forms t = sum_j B A in fp32 from exact products (two bf16 values: 16 significant bits), val = fma(s, t, W)
and n2 = sum_k val^2 by fma.  With V[o][k] = |W| + |s| sum_j |B||A| >= |val|: t carries at most (r - 1) u |s| sum|B||A| in any order, the
fma one more rounding, so |d val| <= r u V; the K squares are exact inside their fma and their sum costs at most (K + 2) u sum val^2
(K - 1 additions and the three additions of the lanes of a row).  Worst case: (K + 2 r + 2) u sum_k V^2.  The issue that introduced
DoRA sets the check at (K + r + 4) u sum_k V^2 -- tighter for r > 2, and what n2_bound returns: rounding errors do not line up in the
worst case (test_dora_ref_cpu.py: an fp32 restatement with another summation order stays inside it on the Gaussian inputs).  Headroom
seen on an MI355X with the kernel's own order (tests/test_dora_gpu.py prints it per module): the error of inv, which is half the
relative error of n2 plus two roundings, reached at most 0.053 of its bound (module 0: K = 8) and 0.0007 to 0.035 elsewhere -- a
statistical expectation asserted as a hard bound, with a factor of about 20 to spare."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import elem_ref as R                      # noqa: E402
import lora_ref as LR                     # noqa: E402

U = 2.0 ** -24
SENTINEL = 0x4D4D
# (r, K, N) of the modules of one job table: every rank; K below one MFMA step, no multiple of 32, several chunks; N below a row tile,
# no multiple of it, beyond one workgroup's 64 rows (four tiles); the last module is a fresh adapter (B = 0)
CASES = [(4, 8, 8), (8, 40, 72), (16, 320, 200), (32, 40, 8), (64, 320, 72), (16, 72, 136)]
B_ZERO = 5
SCALES = (2.0, 0.5, 1.0, 2.0, 0.5, 1.0)


def f32(x):
    return np.float32(x)


def to_bits(x):
    b = R.bf16_bits_np(np.asarray(x, np.float32))
    assert np.array_equal((b.astype(np.uint32) << 16).view(np.float32).astype(np.float64), np.asarray(x, np.float64)), "not a bf16 value"
    return b


def from_bits(b):
    return (np.asarray(b).astype(np.uint32) << 16).view(np.float32)


def bf_np(x):
    """float -> the bf16 value nearest (even), float64."""
    return R.bf16_round_np(np.asarray(x, np.float32)).astype(np.float64)


# ---------------- the norm ---------------------------------------------------------------------------------------------------------------
def n2_64(W, A, B, s):
    W, A, B = (np.asarray(t, np.float64) for t in (W, A, B))
    return ((W + float(s) * (B @ A)) ** 2).sum(1)


def n2_f32(W, A, B, s):
    """The same in float32 with numpy's own orders (a BLAS product, then a pairwise sum): not the kernel's order."""
    W, A, B = (np.asarray(t, np.float32) for t in (W, A, B))
    val = (W + f32(s) * (B @ A)).astype(np.float32)
    return (val * val).sum(1, dtype=np.float32)


def n2_bound(W, A, B, s):
    """(K + r + 4) 2^-24 sum_k (|W| + |s| sum_j |B||A|)^2 per row (module docstring)."""
    W, A, B = (np.abs(np.asarray(t, np.float64)) for t in (W, A, B))
    r, K = A.shape
    return (K + r + 4) * U * ((W + abs(float(s)) * (B @ A)) ** 2).sum(1)


def gains32(n2, m_bits=None):
    """(inv, g, m bits) as the kernel forms them from ITS fp32 n2: root = sqrtf(n2), inv = 1 / root, m = bf16(root) when m_bits is
    None (init), g = float(m) * inv; every step correctly rounded."""
    with np.errstate(all="ignore"):
        root = np.sqrt(np.asarray(n2, np.float32))
        inv = (f32(1.0) / root).astype(np.float32)
        mb = R.bf16_bits_np(root) if m_bits is None else np.asarray(m_bits, np.uint16)
        return inv, (from_bits(mb) * inv).astype(np.float32), mb


def inv_bound(n2, bound):
    """|inv_got - 1 / sqrt(n2)| for |n2_got - n2| <= bound: (1 + d)^-1/2 to second order, plus the roundings of root and quotient."""
    d = bound / n2
    return (0.5 * d + 0.375 * d * d + 2.0 * U * (1.0 + d)) / np.sqrt(n2)


# ---------------- scale and backward kernels, bit level ---------------------------------------------------------------------------------
def scale_bits(v_bits, g, bias_bits=None, res_bits=None):
    """az_dora_scale_bf16: bf16(fmaf(g[o], v, bias[o] or 0) + (residual or nothing)) -> uint16 [M][N]."""
    v = from_bits(v_bits)
    gg = np.broadcast_to(np.asarray(g, np.float32)[None, :], v.shape)
    b = np.broadcast_to(from_bits(bias_bits)[None, :], v.shape) if bias_bits is not None else np.zeros_like(v)
    t = R.fma32(gg, v, b)
    if res_bits is not None:
        t = (t + from_bits(res_bits)).astype(np.float32)
    return R.bf16_bits_np(t)


def dv_bits(dy_bits, g):
    return R.bf16_bits_np((np.asarray(g, np.float32)[None, :] * from_bits(dy_bits)).astype(np.float32))


def dm_64(dy_bits, v_bits, inv, dm_prev_bits):
    """(float64 dm before its rounding, S = inv sum |dy v|)."""
    dy, v = from_bits(dy_bits).astype(np.float64), from_bits(v_bits).astype(np.float64)
    inv = np.asarray(inv, np.float64)
    return from_bits(dm_prev_bits).astype(np.float64) + inv * (dy * v).sum(0), inv * np.abs(dy * v).sum(0)


# ---------------- the adapted linear, float64 and rounded ------------------------------------------------------------------------------
def forward(x, W, A, B, m, s, bias=None, residual=None, rounded=True, n=None):
    """-> (u, v, y, n).  n: the row norms to use (None: of W + s B A, float64; the rounded form takes fp32 inv and g from them)."""
    rd = LR.bf if rounded else (lambda t: t)
    d = lambda t: t.double()
    if n is None:
        n = torch.from_numpy(np.sqrt(n2_64(d(W).numpy(), d(A).numpy(), d(B).numpy(), s)))
    u, v = LR.lora_forward(x, rd(d(x) @ d(W).t()), A, B, s, rounded)
    g = d(m) / n
    if rounded:
        g = (d(m).float() * (1.0 / n.float())).double()
    y = g * v + (d(bias) if bias is not None else 0.0)
    if rounded:
        y = y.float().double()
    return u, v, rd(y + (d(residual) if residual is not None else 0.0)), n


def backward(x, u, v, dy, W, A, B, m, s, n, rounded=True):
    """Hand-written backward with n constant -> dict(dv, dm, du, dx, dA, dB, dbias, dres)."""
    rd = LR.bf if rounded else (lambda t: t)
    d = lambda t: t.double()
    inv = (1.0 / n.float()).double() if rounded else 1.0 / n
    g = (d(m).float() * inv.float()).double() if rounded else d(m) * inv
    dv = rd(g * d(dy))
    dm = rd(inv * (d(dy) * d(v)).sum(0))
    du, dx, dA, dB = LR.lora_backward(x, u, dv, rd(dv @ d(W)), A, B, s, rounded=rounded)
    return dict(dv=dv, dm=dm, du=du, dx=dx, dA=dA, dB=dB, dbias=rd(d(dy).sum(0)), dres=d(dy))


def merged_weight(W, A, B, m, s):
    Wp = LR.merged_weight(W, A, B, s)
    return (m.double() / Wp.norm(dim=1))[:, None] * Wp


# ---------------- shared inputs -------------------------------------------------------------------------------------------------------
def exact_inputs():
    """W multiples of 1/4 in [-2.25, 2.25], A and B multiples of 1/2 in [-1, 1], s a power of two: t = sum_j B A is a multiple of 1/4,
    val of 1/8, val^2 of 2^-6, and every partial sum of n2 in ANY order is at most S = sum_k (|W| + |s| sum_j |B||A|)^2 with
    64 S < 2^24 (asserted): exact in fp32.  -> [(W, A, B, s)] float64."""
    rng = np.random.default_rng(11)
    out = []
    for i, ((r, K, N), s) in enumerate(zip(CASES, SCALES)):
        W = rng.integers(-4, 5, (N, K)).astype(np.float64) / 2.0
        A, B = (rng.integers(-2, 3, shp).astype(np.float64) / 2.0 for shp in ((r, K), (N, r)))
        W[:, 0] += 0.25                                  # no zero row
        if i == B_ZERO:
            B[:] = 0.0
        S = ((np.abs(W) + abs(s) * (np.abs(B) @ np.abs(A))) ** 2).sum(1).max()
        assert 64.0 * S < 2.0 ** 24, (i, S)
        out.append((W, A, B, s))
    return out


def gauss_inputs():
    rng = np.random.default_rng(12)
    out = []
    for i, ((r, K, N), s) in enumerate(zip(CASES, SCALES)):
        W, A, B = bf_np(rng.standard_normal((N, K)) / np.sqrt(K)), bf_np(rng.standard_normal((r, K)) / np.sqrt(K)), bf_np(0.3 * rng.standard_normal((N, r)))
        if i == B_ZERO:
            B[:] = 0.0
        out.append((W, A, B, s))
    return out


def layout(mods):
    """Slots of one flat bf16 buffer: W, A, B, m of every module in whole 64-element slots with 64 sentinel elements in front of,
    between and behind them -> ([(oW, oA, oB, om)], total)."""
    off, offs = 64, []
    for W, A, B, _ in mods:
        row = []
        for n in (W.size, A.size, B.size, W.shape[0]):
            row.append(off)
            off += ((n + 63) // 64) * 64 + 64
        offs.append(tuple(row))
    return offs, off


# ---------------- the oracle UNet with magnitudes ---------------------------------------------------------------------------------------
class DoraRefUNet(LR.LoraRefUNet):
    """LoraRefUNet whose adapted linears carry a magnitude wherever the parameter dict holds `<module>.dora_scale`:
    y = (m / ||W + s B A||_row) (x W^T + s (x A^T) B^T) + bias, the norm detached.  In the fp32 oracle these linears are evaluated in
    float64; under the bf16 oracle (autocast) the products run in bf16 and the gain in fp32."""

    def _lin(self, x, name, bias=True):
        m = self.p.get(name + ".dora_scale")
        if m is None:
            return super()._lin(x, name, bias)
        W, A, B = self.p[name + ".weight"], self.p[name + ".lora_A.weight"], self.p[name + ".lora_B.weight"]
        b = self.p[name + ".bias"] if bias else None
        if x.dtype == torch.float32 and W.dtype == torch.float32:
            hi = torch.float64
            n = (W.to(hi) + self.scale * (B.to(hi) @ A.to(hi))).norm(dim=1).detach()
            v = F.linear(x.to(hi), W.to(hi)) + self.scale * F.linear(F.linear(x.to(hi), A.to(hi)), B.to(hi))
            y = (m.to(hi) / n) * v
            return (y + b.to(hi) if b is not None else y).to(x.dtype)
        n = (W.float() + self.scale * (B.float() @ A.float())).norm(dim=1).detach()
        v = F.linear(x, W) + self.scale * F.linear(F.linear(x, A), B)
        y = (m.float() / n) * v.float()
        return (y + b.float() if b is not None else y).to(v.dtype)
