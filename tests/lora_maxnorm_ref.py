"""LoRA max-norm regularisation (kohya-ss scale_weight_norms; include/aozora_hip.h az_lora_max_norm_bf16) restated in numpy: the rule
in float64, the norm both by the Gram identity and by the materialised product, the element update for a given fp32 q, a worst-case
bound for the kernel's fp32 n2 and the bound on q that follows from it, and the inputs the tests share.  The rule, per module with
A [r][K], B [out][r] (bf16 values) and s = alpha / rank:
    n2 = s^2 sum_ij (A A^T)_ij (B^T B)_ij = || s B A ||_F^2,  norm = sqrt(n2)
    norm > max_norm:  q = sqrt(max_norm / norm), every element x <- bf16_rn(fl32(x) q)   (with a master: w <- w q in fp32, x <- bf16_rn(w))
    otherwise q = 1 and nothing is written (a NaN norm compares false).
Written from kohya-ss's apply_max_norm_regularization as understood (its clamp(min = max_norm / 2) only keeps 0 / 0 out of the
ratio); unpinned against the package."""
import numpy as np

import elem_ref as R

U = 2.0 ** -24                      # unit roundoff of fp32
SENTINEL = 0x4D4D
MAX_NORM = 1.0
# (r, K, out): rank 4 and 8 (padded tiles), a 3x3 convolution with Cin 8 (K = 72), out beyond one 128-row stage and no multiple of it,
# K beyond one round of the four waves' k-steps and no multiple of 32, every tile count (1, 2, 4), and a fresh adapter (B = 0)
CASES = [(4, 8, 8), (8, 72, 24), (16, 40, 328), (32, 320, 64), (64, 136, 72), (16, 64, 16)]
B_ZERO = 5                          # index of the module whose B is 0


def f32(x):
    return np.float32(x)


# ---------------- the rule -------------------------------------------------------------------------------------------------------------
def n2_gram(A, B, s):
    """|| s B A ||_F^2 by the Gram identity, float64.  A [r][K], B [out][r] float64 arrays of bf16 values."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return float(s) ** 2 * float(((A @ A.T) * (B.T @ B)).sum())


def n2_product(A, B, s):
    """The same by the materialised product (kohya-ss's form), float64."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return float(((float(s) * (B @ A)) ** 2).sum())


def rule64(n2, max_norm):
    """(norm, q, over) in float64."""
    norm = np.sqrt(n2)
    over = bool(norm > max_norm)
    return norm, (np.sqrt(max_norm / norm) if over else 1.0), over


def rule32(n2, max_norm):
    """(norm, q, over) as the kernel forms them from ITS fp32 n2: norm = sqrtf(n2); q = sqrtf(max_norm / norm), each correctly rounded."""
    with np.errstate(all="ignore"):
        norm = np.sqrt(f32(n2))
        over = bool(norm > f32(max_norm))
        return norm, (np.sqrt(f32(max_norm) / norm) if over else f32(1.0)), over


def scale_bits(bits, q):
    """uint16 bf16 bits -> bf16_rn(fl32(x) * q) for the fp32 q, as bits."""
    x = (bits.astype(np.uint32) << 16).view(np.float32)
    with np.errstate(all="ignore"):
        return R.bf16_bits_np(x * f32(q))


def scale_master(w, q):
    """fp32 master w -> (w * q in fp32, bf16_rn of it as bits)."""
    with np.errstate(all="ignore"):
        wn = (np.asarray(w, np.float32) * f32(q)).astype(np.float32)
    return wn, R.bf16_bits_np(wn)


# ---------------- bounds (derived, not fitted) ---------------------------------------------------------------------------------------------
def n2_bound(A, B, s):
    """|n2_got - n2_64| <= (K + out + r^2 + 8) 2^-24 s^2 sum_ij Ghat_A[i][j] Ghat_B[i][j], Ghat the Gram matrices of the absolute
    values: the products of two bf16 values are exact in fp32, so an entry of G_A carries at most K u Ghat_A of accumulation error in
    any summation order (the standard n u bound), an entry of G_B out u Ghat_B, the sum of the r^2 products r^2 u more, and the product
    of two entries, s * s and the two multiplications by it a handful of roundings (8 covers them with the second-order terms)."""
    A, B = np.abs(np.asarray(A, np.float64)), np.abs(np.asarray(B, np.float64))
    r, K = A.shape
    out = B.shape[0]
    return (K + out + r * r + 8) * U * float(s) ** 2 * float(((A @ A.T) * (B.T @ B)).sum())


def q_bound(A, B, s):
    """Relative bound on q = (max_norm^2 / n2)^(1/4): a quarter of the relative bound x on n2 (|(1 + x)^(-1/4) - 1| <= |x| / 4 (1 + |x|)
    for |x| <= 1/2), plus three fp32 roundings (sqrtf of n2, the division, sqrtf of the ratio)."""
    n2 = n2_gram(A, B, s)
    if n2 == 0.0:
        return 0.0
    x = n2_bound(A, B, s) / n2
    assert x <= 0.5
    return x / 4.0 * (1.0 + x) + 3.0 * U


# ---------------- inputs ---------------------------------------------------------------------------------------------------------------------
def _hadamard(h):
    H = np.ones((1, 1))
    while H.shape[0] < h:
        H = np.block([[H, H], [H, -H]])
    return H


# exactly summable inputs: (s, norm) per module; A's rows are rows of a Sylvester-Hadamard matrix tiled over a power-of-two number of
# columns (the rest 0), so G_A = a I with every partial sum a small integer; B holds +-0.5, +-1, +-2 at random places with
# || B ||_F^2 = T = norm^2 / (s^2 a).  Every partial sum is exact in fp32 in any order, n2 = s^2 a T is a perfect square and max_norm / norm is a
# power of 4 for the three modules above the limit; module 1 sits exactly ON the limit (not above it: untouched).
EXACT = [(0.5, 4.0), (2.0 ** -4, 1.0), (0.125, 16.0), (2.0 ** -7, 0.5), (0.25, 64.0), (1.0, 0.0)]


def exact_inputs():
    """-> [(A float64 [r][K], B float64 [out][r], s)] for CASES."""
    rng = np.random.default_rng(20240607)
    outp = []
    for i, ((r, K, out), (s, norm)) in enumerate(zip(CASES, EXACT)):
        h = max(r, 8)
        tiles = 1 << int(np.log2(K // h))
        a = h * tiles
        A = np.zeros((r, K))
        A[:, :a] = np.tile(_hadamard(h)[:r], (1, tiles))
        B = np.zeros(out * r)
        if i != B_ZERO:
            T = norm * norm / (s * s * a)
            assert T >= 1 and T == int(T)
            rest = int(T) - 1
            n4 = rest // 8
            n1 = rest - 4 * n4
            vals = np.concatenate([np.full(4, 0.5), np.full(n1, 1.0), np.full(n4, 2.0)])
            assert vals.size <= B.size and float((vals ** 2).sum()) == T
            pos = rng.permutation(B.size)[:vals.size]
            B[pos] = vals * rng.choice([-1.0, 1.0], vals.size)
        outp.append((A, B.reshape(out, r), s))
    return outp


# Gaussian inputs: norm / max_norm per module, set through the module's scale (three above the limit, two below, B = 0)
GAUSS_RATIO = [2.5, 0.6, 7.0, 0.3, 1.5, 0.0]


def gauss_inputs(seed=7):
    """-> [(A, B, s)] for CASES: bf16 Gaussian values, s an fp32 value that puts norm / MAX_NORM near GAUSS_RATIO."""
    rng = np.random.default_rng(seed)
    outp = []
    for i, ((r, K, out), ratio) in enumerate(zip(CASES, GAUSS_RATIO)):
        A = R.bf16_round_np((rng.standard_normal((r, K)) / np.sqrt(K)).astype(np.float32)).astype(np.float64)
        B = R.bf16_round_np((rng.standard_normal((out, r)) * 0.05).astype(np.float32)).astype(np.float64)
        if i == B_ZERO:
            B[:] = 0.0
            s = 1.0
        else:
            s = float(f32(ratio * MAX_NORM / np.sqrt(n2_gram(A, B, 1.0))))
        outp.append((A, B, s))
    return outp


def to_bits(x):
    """float64 array of bf16 values -> uint16 bits (exact)."""
    b = R.bf16_bits_np(np.asarray(x, np.float32))
    assert np.array_equal((b.astype(np.uint32) << 16).view(np.float32).astype(np.float64), np.asarray(x, np.float64))
    return b


def layout(mods):
    """Slots of one flat bf16 buffer: every matrix in a whole number of 64-element slots, 64 sentinel elements in front of, between and
    behind them -> (offsets [(oA, oB)], total elements)."""
    off, offs = 64, []
    for A, B, _ in mods:
        pair = []
        for m in (A, B):
            pair.append(off)
            off += (m.size + 63) // 64 * 64 + 64
        offs.append(tuple(pair))
    return offs, off
