"""Closed-form attention for aozora_sdxl_training_amd/csrc/az_attn.hip: inputs for which every output of the forward and the
backward is ONE bit pattern per element, the float64 closed form of those outputs, an fp32 emulation with the kernels' rounding
points, and a mirror of the host dispatch.  The product never imports this file; tests/test_attn_exact_gpu.py compares the HIP
kernels with it and tests/test_attn_ref_cpu.py checks it without a GPU.  Plain numpy on the CPU.

Selector inputs (head dim 64, scale 0.125, every operand a small integer, exact in bf16).  Every key belongs to a group of 1, 2 or 4
keys.  The group index is written as NBITS bits, each bit REPS times as +-1 in NBITS * REPS "code" columns of K; the remaining
"free" columns of K hold integers in [-4, 4].  Query q carries amp_q * code(pi(q)) in the code columns (amp_q is 128 or 256, so
neighbouring queries have different row maxima and different lse) and zeros in the free columns.  The scores are integers, exact in
the MFMA; every key of group pi(q) scores the row maximum NBITS * REPS * amp_q and every other key at least 2 * REPS * 128 = 1280
less, which is 230.8 in the base-2 exponent: its probability is exactly 0 in fp32, flushed or not.  P is then exactly 1/g on the
group: the running sum is g, 1/g is exact, O is the mean of g integer rows of V, lse2 = m c + log2(g).  Groups are neighbours
("near": k // g) or spread over the key axis ("far": k % ngroups) so that equal maxima arrive in different key tiles, ring slots
and query splits.  A key count that is no multiple of g ends in groups of 2 and 1.

Backward: P is recomputed from lse to ~1e-4 relative, which rounds to exactly 1/g in bf16.  V is in [-2, 2] and dO has two
non-zeros of {+-1, +-2} per row (or the other way round, `dense_do`), so delta, dP - delta and dS are multiples of 1/16 of at most
8 significant bits: the bf16 rounding of dS is exact, and dQ, dK, dV are sums of exact terms -- exact in fp32 in any order and
through any query split.  With g = 1 dQ and dK vanish: the backward cases use g >= 2.

Bias column.  Zero-filled padded keys score 0, far below the maximum: a missing key mask would go unnoticed.  With `bias` one more
column holds -16384 in every row of Q and +1 in every row of K: every valid score is negative and an unmasked padded key wins the
softmax.  Every case with a ragged Tq or Tk has it.

Per head the 64 columns of Q and K are permuted, by a rotation of 18 (h + rot) columns: scores do not change, and the free
columns -- where dQ is non-zero -- sweep all 64 positions over four consecutive values of h + rot.  pi, amp, V and dO differ per
(batch, head).

`build` draws a case from its fields alone and skips draws whose expected outputs are not bf16-representable (a sum of dS over the
queries of one group can need a ninth bit): the seed of the draw that `exact_ok` accepts is part of the case's data."""
import functools
import math
from collections import namedtuple

import numpy as np

D = 64
SCALE = 0.125
C64 = SCALE * math.log2(math.e)
C32 = np.float32(SCALE) * np.float32(1.4426950408889634)      # the kernels' `scale * LOG2E`
NBITS, REPS = 9, 5
NCODE = NBITS * REPS
AMPS = (128, 256)
FREE_STEP = D - NCODE - 1          # the 18 free columns of a head with a bias column
BIAS_Q = -16384.0
TILE = 64
POISON = 3.0 * 2.0 ** 40          # finite and bf16-exact; a poisoned row read as a key would win every softmax
SENTINEL = -5.0 * 2.0 ** 33       # fills output buffers: no kernel here produces it

# B H Tq Tk | g: keys per group | layout "near" / "far" | bias column | dense_do: dense dO and two-non-zero V rows |
# rot: head h's columns are rotated by 18 (h + rot)
Case = namedtuple("Case", "B H Tq Tk g layout bias dense_do rot", defaults=(2, "near", False, False, 0))
Data = namedtuple("Data", "case Q K V dO grp pi seed")


def ragged(c):
    return c.Tq % 128 != 0 or c.Tk % 128 != 0


def case_id(c):
    return f"{c.B}x{c.H}x{c.Tq}x{c.Tk}-g{c.g}{c.layout}{'-bias' if c.bias else ''}{'-ddo' if c.dense_do else ''}-r{c.rot}"


# ---------------- bf16 / fp32 helpers ------------------------------------------------------------------------------------------
def bf16_round(x):
    """fp32 -> the nearest bf16 (ties to even, f2bf of az_common.h), returned as fp32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def is_bf16(x):
    x = np.asarray(x, dtype=np.float64)
    return bool(np.all(bf16_round(x.astype(np.float32)).astype(np.float64) == x))


def is_f32(x):
    x = np.asarray(x, dtype=np.float64)
    return bool(np.all(x.astype(np.float32).astype(np.float64) == x))


def _fma32(a, b, c):
    """fp32 a * b + c with one rounding (the product of two fp32 is exact in float64)."""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)


def _exp2_flush(x):
    """The raw hardware exponential: results below 2^-126 flush to zero."""
    with np.errstate(over="ignore", under="ignore"):
        y = np.exp2(x.astype(np.float32)).astype(np.float32)
    return np.where(y < np.float32(2.0 ** -126), np.float32(0), y)


# ---------------- builders -----------------------------------------------------------------------------------------------------
def key_groups(Tk, g, layout):
    """-> (grp[Tk], number of groups); every group has 1, 2 or 4 keys."""
    assert g in (1, 2, 4) and layout in ("near", "far")
    nfull = Tk // g
    grp = np.empty(Tk, np.int64)
    k = np.arange(nfull * g)
    if nfull:
        grp[:nfull * g] = k // g if layout == "near" else k % nfull
    nxt, pos, rem = nfull, nfull * g, Tk - nfull * g
    for size in (2, 1):
        if rem >= size:
            grp[pos:pos + size] = nxt
            nxt, pos, rem = nxt + 1, pos + size, rem - size
    assert rem == 0 and nxt <= 2 ** NBITS
    return grp, nxt


def _two_nonzero_rows(rng, shape):
    n = int(np.prod(shape[:-1]))
    flat = np.zeros((n, shape[-1]))
    cols = np.argsort(rng.random((n, shape[-1])), axis=1)[:, :2]
    flat[np.arange(n)[:, None], cols] = rng.choice([-2.0, -1.0, 1.0, 2.0], size=(n, 2))
    return flat.reshape(shape)


def _draw(c, seed):
    rng = np.random.default_rng([c.B, c.H, c.Tq, c.Tk, c.g, c.layout == "far", c.bias, c.dense_do, c.rot, seed])
    grp, ng = key_groups(c.Tk, c.g, c.layout)
    code = ((((np.arange(ng)[:, None] >> np.arange(NBITS)) & 1) * 2 - 1).repeat(REPS, axis=1)).astype(np.float64)   # (ng, NCODE)
    Q = np.zeros((c.B, c.H, c.Tq, D))
    K = np.zeros((c.B, c.H, c.Tk, D))
    pi = np.empty((c.B, c.H, c.Tq), np.int64)
    nfree0 = NCODE + (1 if c.bias else 0)
    for b in range(c.B):
        for h in range(c.H):
            pi[b, h] = rng.permutation(ng)[np.arange(c.Tq) % ng]
            amp = rng.choice(AMPS, size=c.Tq).astype(np.float64)
            Q[b, h, :, :NCODE] = amp[:, None] * code[pi[b, h]]
            K[b, h, :, :NCODE] = code[grp]
            if c.bias:
                Q[b, h, :, NCODE] = BIAS_Q
                K[b, h, :, NCODE] = 1.0
            K[b, h, :, nfree0:] = rng.integers(-4, 5, size=(c.Tk, D - nfree0))
    for h in range(c.H):              # one column permutation per head, the same for Q and K
        Q[:, h] = np.roll(Q[:, h], FREE_STEP * (h + c.rot), axis=-1)
        K[:, h] = np.roll(K[:, h], FREE_STEP * (h + c.rot), axis=-1)
    if c.dense_do:
        V = _two_nonzero_rows(rng, (c.B, c.H, c.Tk, D))
        dO = rng.integers(-2, 3, size=(c.B, c.H, c.Tq, D)).astype(np.float64)
    else:
        V = rng.integers(-2, 3, size=(c.B, c.H, c.Tk, D)).astype(np.float64)
        dO = _two_nonzero_rows(rng, (c.B, c.H, c.Tq, D))
    return Data(c, Q, K, V, dO, grp, pi, seed)


@functools.lru_cache(maxsize=None)
def build(c):
    """The first draw of the case whose expected outputs are all bf16-representable (see the module docstring)."""
    for seed in range(32):
        d = _draw(c, seed)
        e = closed_form(d)
        if all(is_bf16(e[n]) for n in ("O", "dQ", "dK", "dV", "dS")) and is_f32(e["delta"]):
            return d
    raise AssertionError(f"no representable draw for {case_id(c)}")


# ---------------- the closed form (float64) ------------------------------------------------------------------------------------
def closed_form(d):
    """Expected O, lse2, delta, dQ, dK, dV (+ P, dS, the exponent gap) with P from `score == row maximum`."""
    Q, K, V, dO = d.Q, d.K, d.V, d.dO
    S = Q @ K.swapaxes(-1, -2)
    m = S.max(-1, keepdims=True)
    sel = S == m
    cnt = sel.sum(-1, keepdims=True).astype(np.float64)
    P = sel / cnt
    O = P @ V
    lse = m[..., 0] * C64 + np.log2(cnt[..., 0])
    delta = (dO * O).sum(-1)
    dP = dO @ V.swapaxes(-1, -2)
    dS = P * (dP - delta[..., None])
    dS = np.where(sel, dS, 0.0)
    second = np.where(sel, -np.inf, S).max(-1)
    gap = (m[..., 0] - second) * C64          # +inf where the group is the whole key axis
    return {"O": O, "lse": lse, "delta": delta, "dQ": SCALE * (dS @ K), "dK": SCALE * (dS.swapaxes(-1, -2) @ Q),
            "dV": P.swapaxes(-1, -2) @ dO, "P": P, "dS": dS, "gap": gap, "S": S, "cnt": cnt[..., 0]}


def exact_ok(c):
    """The conditions under which the expected outputs of case `c` are one bit pattern each."""
    d = build(c)
    e = closed_form(d)
    for n in ("Q", "K", "V", "dO"):
        assert is_bf16(getattr(d, n)), f"{n} is not bf16-representable"
    assert float(e["gap"].min()) >= 160.0, f"exponent gap {float(e['gap'].min())}"
    assert set(np.unique(e["cnt"])) <= {1.0, 2.0, 4.0}
    for n in ("O", "dQ", "dK", "dV", "dS"):
        assert is_bf16(e[n]), f"expected {n} is not bf16-representable"
    assert is_f32(e["delta"])
    # every partial sum is a multiple of its resolution and at most sum |a||b|: exact in fp32 below 2^24 resolutions
    aQ, aK, aV, adO, adS, aP = (np.abs(x) for x in (d.Q, d.K, d.V, d.dO, e["dS"], e["P"]))
    sums = {"S": (aQ @ aK.swapaxes(-1, -2), 1.0), "O": (aP @ aV * e["cnt"][..., None], 1.0), "delta": ((adO * np.abs(e["O"])).sum(-1), 0.25),
            "dP": (adO @ aV.swapaxes(-1, -2) + np.abs(e["delta"])[..., None], 0.25), "dQ": (adS @ aK, 1.0 / 16),
            "dK": (adS.swapaxes(-1, -2) @ aQ, 128.0 / 16), "dV": (aP.swapaxes(-1, -2) @ adO, 0.25)}      # Q holds multiples of 128
    assert np.all(d.Q % 128.0 == 0)
    for n, (s, res) in sums.items():
        assert float(s.max()) < 2.0 ** 24 * res, f"{n}: sum magnitude {float(s.max())} at resolution {res}"
    for n, res in (("dS", 1.0 / 16), ("delta", 0.25), ("O", 0.25), ("dV", 0.25), ("dQ", 1.0 / 128), ("dK", 1.0 / 128)):
        assert np.all(e[n] / res == np.round(e[n] / res)), f"{n} is no multiple of {res}"
    return True


# ---------------- fp32 emulation with the kernels' rounding points -------------------------------------------------------------
DEFECTS = ("drop_key", "mask_short", "mask_long", "unmasked", "lse_neighbour", "swap_rows", "drop_slab", "delta_wrong_head")


ATTN_THR2 = np.float32(4.0)


def _online_plain(S, Vp):
    """attn_fwd_kernel: key tiles of 64 in order; a probability is rounded to bf16 RELATIVE TO THE RUNNING MAXIMUM of its tile (the
    rounding errors are not those of exp2(s - final maximum)); O and l are rescaled when the maximum moves.  -> (o, l, m)"""
    f = np.float32
    m = np.full(S.shape[:-1], -np.inf, f)
    l = np.zeros(S.shape[:-1], f)
    o = np.zeros(S.shape[:-1] + (Vp.shape[-1],), f)
    for kt in range(S.shape[-1] // TILE):
        st = S[..., kt * TILE:(kt + 1) * TILE]
        m_new = np.maximum(m, st.max(-1))
        alpha = _exp2_flush(((m - m_new) * C32).astype(f))          # 1 where the maximum stays, 0 in front of the first tile
        pb = bf16_round(_exp2_flush(_fma32(st, C32, -(m_new * C32).astype(f)[..., None])))
        l = (l * alpha + pb.sum(-1, dtype=f)).astype(f)
        o = (o * alpha[..., None] + pb @ Vp[..., kt * TILE:(kt + 1) * TILE, :]).astype(f)
        m = m_new
    return o, l, m


def _online_dma(S, Vp):
    """attn_fwd_dma_kernel (Tq % 128 == 0, Tk % 128 == 0): query block bx of nx visits the key tiles rotated by (bx * ntiles) / nx;
    the running maximum starts as the first tile's and is raised -- for the 32 queries of a wave together -- only when some tile
    maximum of the wave exceeds it by more than 2^4 in the exponent; until then probabilities stand against the stale maximum."""
    f = np.float32
    Tq, ntiles = S.shape[-2], S.shape[-1] // TILE
    nx = Tq // 128
    assert Tq % 128 == 0 and ntiles % 2 == 0
    o = np.zeros(S.shape[:-1] + (Vp.shape[-1],), f)
    l = np.zeros(S.shape[:-1], f)
    m = np.empty(S.shape[:-1], f)
    for bx in range(nx):
        rot = (bx * ntiles) // nx
        rows = slice(bx * 128, (bx + 1) * 128)
        tile = lambda i: slice(((i + rot) % ntiles) * TILE, ((i + rot) % ntiles + 1) * TILE)      # noqa: E731
        mb = S[..., rows, tile(0)].max(-1)
        lb = np.zeros_like(mb)
        ob = np.zeros(mb.shape + (Vp.shape[-1],), f)
        for kt in range(ntiles):
            pb = bf16_round(_exp2_flush(_fma32(S[..., rows, tile(kt)], C32, -(mb * C32).astype(f)[..., None])))
            lb = (lb + pb.sum(-1, dtype=f)).astype(f)
            ob = (ob + pb @ Vp[..., tile(kt), :]).astype(f)
            if kt + 1 < ntiles:
                mx = S[..., rows, tile(kt + 1)].max(-1)
                raise_ = (((mx - mb) * C32).astype(f) > ATTN_THR2).reshape(mb.shape[:-1] + (4, 32)).any(-1)      # per wave
                raise_ = np.repeat(raise_, 32, axis=-1)
                m_new = np.where(raise_, np.maximum(mb, mx), mb)
                alpha = _exp2_flush(((mb - m_new) * C32).astype(f))
                lb, ob, mb = (lb * alpha).astype(f), (ob * alpha[..., None]).astype(f), m_new
        o[..., rows, :], l[..., rows], m[..., rows] = ob, lb, mb
    return o, l, m


def emulate_arrays(Q, K, V, dO, defect=None, fwd="plain"):
    """Forward and backward as az_attn.hip computes them: fp32 scores and sums, the online softmax of the forward kernel named by
    `fwd` ("plain": attn_fwd_kernel, "dma": attn_fwd_dma_kernel), P and dS rounded to bf16 in front of their products, the bf16 O
    feeding delta, lse in fp32, keys padded with zero rows to whole 64-key tiles and masked.  `defect` plants one of DEFECTS
    (tests/test_attn_ref_cpu.py shows that the comparison rejects each)."""
    assert defect is None or defect in DEFECTS
    f = np.float32
    Q, K, V, dO = (np.asarray(x, dtype=f) for x in (Q, K, V, dO))
    Tq, Tk = Q.shape[-2], K.shape[-2]
    Tkp = -(-Tk // TILE) * TILE
    pad = [(0, 0)] * (K.ndim - 2) + [(0, Tkp - Tk), (0, 0)]
    Kp, Vp = np.pad(K, pad), np.pad(V, pad)
    nvalid = {"mask_short": Tk - 1, "mask_long": min(Tk + 1, Tkp), "unmasked": Tkp}.get(defect, Tk)
    valid = np.arange(Tkp) < nvalid
    if defect == "drop_key":
        valid[Tk // 2] = False
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        S = np.where(valid, Q @ Kp.swapaxes(-1, -2), f(-np.inf)).astype(f)
        o, l, m = (_online_dma if fwd == "dma" else _online_plain)(S, Vp)
        O = bf16_round(o * (f(1.0) / l).astype(f)[..., None])
        lse = ((m * C32).astype(f) + np.log2(l).astype(f)).astype(f)
        # backward
        lse_b = np.roll(lse, 1, axis=-1) if defect == "lse_neighbour" else lse
        delta = (O * dO).sum(-1, dtype=f)
        delta_b = np.roll(delta, 1, axis=-2) if defect == "delta_wrong_head" else delta
        P = _exp2_flush(_fma32(S, C32, -lse_b[..., None]))
        dp = (dO @ Vp.swapaxes(-1, -2) - delta_b[..., None]).astype(f)
        dS = bf16_round(P * dp)
        Pb = bf16_round(P)
        dQ = bf16_round(f(SCALE) * (dS @ Kp))
        dSk, Pk = dS, Pb
        if defect == "drop_slab":          # the second 64-query slab is left out of the dK / dV sum
            dSk, Pk = dS.copy(), Pb.copy()
            dSk[..., 64:128, :] = 0
            Pk[..., 64:128, :] = 0
        dK = bf16_round(f(SCALE) * (dSk.swapaxes(-1, -2) @ Q))[..., :Tk, :]
        dV = bf16_round(Pk.swapaxes(-1, -2) @ dO)[..., :Tk, :]
    if defect == "swap_rows":
        O, dQ = O.copy(), dQ.copy()
        for x in (O, dQ):
            x[..., [3, 17], :] = x[..., [17, 3], :]
    return {"O": O, "lse": lse, "delta": delta, "dQ": dQ, "dK": dK, "dV": dV}


def emulate(d, defect=None, fwd="plain"):
    return emulate_arrays(d.Q, d.K, d.V, d.dO, defect, fwd)


# ---------------- the comparison the GPU test uses -----------------------------------------------------------------------------
def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def mismatches(got, exp, names=("O", "lse", "delta", "dQ", "dK", "dV"), lse_ulps=4.0):
    """-> list of messages, empty when `got` (fp32 arrays holding the kernels' bf16 / fp32 outputs, (B, H, T, 64) or (B, H, Tq))
    is what the closed form `exp` demands: the bf16 outputs and delta equal (as torch.equal: NaN equals nothing), lse2 within
    `lse_ulps` fp32 ulp of the float64 value."""
    out = []
    for n in names:
        g = np.asarray(got[n], dtype=np.float64)
        e = np.asarray(exp[n], dtype=np.float64)
        if g.shape != e.shape:
            out.append(f"{n}: shape {g.shape} != {e.shape}")
            continue
        if n == "lse":
            with np.errstate(invalid="ignore"):
                bad = ~(np.abs(g - e) <= lse_ulps * ulp32(e))
        else:
            ee = e.astype(np.float32).astype(np.float64) if n == "delta" else bf16_round(e.astype(np.float32)).astype(np.float64)
            bad = ~(g == ee)
        if bad.any():
            i = tuple(int(v) for v in np.argwhere(bad)[0])
            out.append(f"{n}: {int(bad.sum())} of {bad.size} elements differ, first at {i}: got {g[i]!r}, expected {e[i]!r}")
    return out


# ---------------- float64 attention on arbitrary inputs (the peaked layer) -----------------------------------------------------
def reference64(Q, K, V, dO):
    Q, K, V, dO = (np.asarray(x, dtype=np.float64) for x in (Q, K, V, dO))
    S = (Q @ K.swapaxes(-1, -2)) * SCALE
    m = S.max(-1, keepdims=True)
    E = np.exp(S - m)
    l = E.sum(-1, keepdims=True)
    P = E / l
    O = P @ V
    delta = (dO * O).sum(-1)
    dS = P * (dO @ V.swapaxes(-1, -2) - delta[..., None])
    return {"O": O, "lse": (m[..., 0] + np.log(l[..., 0])) * math.log2(math.e), "delta": delta, "dQ": SCALE * (dS @ K),
            "dK": SCALE * (dS.swapaxes(-1, -2) @ Q), "dV": P.swapaxes(-1, -2) @ dO, "P": P}


def row_rel_l2(got, ref):
    """Relative L2 error of every row (last axis) of `got` against `ref`."""
    g, r = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.sqrt(((g - r) ** 2).sum(-1)) / np.sqrt((r ** 2).sum(-1))


def peaked_inputs(B, H, Tq, Tk, seed):
    """Gaussian bf16 q, k, v, dO with q scaled so that the median over rows of the largest probability is about 0.5."""
    rng = np.random.default_rng([B, H, Tq, Tk, seed])
    q0, K, V, dO = (bf16_round(rng.standard_normal((B, H, T, D)).astype(np.float32)) for T in (Tq, Tk, Tk, Tq))
    best = None
    for a in np.geomspace(0.25, 16.0, 49):
        Q = bf16_round((a * q0).astype(np.float32))
        S = (Q.astype(np.float64) @ K.astype(np.float64).swapaxes(-1, -2)) * SCALE
        E = np.exp(S - S.max(-1, keepdims=True))
        pmax = float(np.median((E / E.sum(-1, keepdims=True)).max(-1)))
        if best is None or abs(pmax - 0.5) < abs(best[0] - 0.5):
            best = (pmax, Q)
    return best[1], K, V, dO, best[0]


# ---------------- mirror of the host dispatch (az_attn_fwd / az_attn_bwd) ------------------------------------------------------
WS_DEFAULT = 96 << 20


def fwd_kernel(Tq, Tk, pipe=15):
    if (pipe & 1) and Tq % 128 == 0 and Tk % 128 == 0:
        return "fwd_dma"
    return "fwd_full" if Tq % 128 == 0 and Tk % 64 == 0 else "fwd_general"


def bwd_kernels(B, H, Tq, Tk, pipe=15, target=384, parts=7, ws_bytes=WS_DEFAULT):
    """-> the kernels one az_attn_bwd call launches, in order; ws_bytes = 0 stands for workspace == NULL."""
    parts = parts or 7
    BH = B * H
    dma = bool(pipe & 8) and Tq % 128 == 0 and Tk % 128 == 0
    if parts == 7 and (pipe & 2) and Tq == Tk and Tq % 128 == 0 and (Tq // 128) * BH <= 768:
        return ["delta", "merged_dma" if dma else "merged"]
    if parts == 7 and Tk <= 128 and (pipe & 4):
        ntile = (Tq + 127) // 128
        ns = min(-(-target // BH), ntile)
        if ns > 1 and not ws_bytes:
            ns = 1
        while ns > 1 and ns * BH * 128 * 128 * 4 > ws_bytes:
            ns -= 1
        tpw = -(-ntile // ns)
        ns = -(-ntile // tpw)
        return [f"cross[{ns}]"] + (["reduce"] if ns > 1 else [])
    out = []
    if (parts & 1) and not (parts & 2):
        out.append("delta")
    if parts & 2:
        fd = "fused" if parts & 1 else "plain"
        out.append(f"dq_dma_{fd}" if dma else f"dq_{fd}_{'full' if Tq % 128 == 0 and Tk % 64 == 0 else 'general'}")
    if not (parts & 4):
        return out
    kb, qtiles = (Tk + 127) // 128, (Tq + TILE - 1) // TILE
    ns = 1
    if kb * BH < 384 and qtiles >= 4 and ws_bytes:
        ns = min(-(-target // (kb * BH)), qtiles // 2)
        while ns > 1 and ns * BH * kb * 128 * 128 * 4 > ws_bytes:
            ns -= 1
        ns = max(ns, 1)
    tps = -(-qtiles // ns)
    ns = -(-qtiles // tps)
    if dma and ns == 1:
        return out + ["dkv_dma"]
    return out + [f"dkv[{ns}]"] + (["reduce"] if ns > 1 else [])
