"""Restatements of the element-wise, reduction and optimizer kernels (csrc/az_elem.hip, csrc/az_optim.hip) with per-element error
bounds.  The product never imports this file; tests/test_elem_gpu.py compares the HIP kernels against it and
tests/test_elem_ref_cpu.py checks it (and derives the constants K below) without a GPU.  Plain torch / numpy on the CPU.

Two kinds of reference:
  * float64 restatements (torch) of what a kernel approximates in fp32: GEGLU with the exact erf GELU, SiLU, nearest-2x upsample,
    column sums, reduce_segs, the weighted MSE, the timestep embedding, the sum of squares and the clip coefficient.  Each comes
    with S, the sum of the magnitudes of the terms the kernel combined in fp32 for that element;
  * bit-level restatements (numpy float32 / integer arithmetic) where a kernel promises bits: the bf16 cast, scale_bf16 / scale_f32,
    titan_offload, add_rows, noise_target and the AdamW element update.  The library is built without fast-math, so fp32 division
    and sqrtf are correctly rounded and numpy's float32 operators restate them exactly.  Python 3.10 has no math.fma: `fma32` forms
    the product exactly in float64, the sum in float64 ROUNDED TO ODD (the exact error of the float64 addition, from TwoSum, decides
    the sticky bit) and rounds that once to fp32 -- with 53 >= 2 * 24 + 2 bits this is the correctly rounded fma, no double rounding,
    so the fp32-moment tests ask for bits as well.

Bound of an output stored in bf16 whose fp32 value approximates ref:
    |out - ref| <= half_ulp_bf16(ref) + K[q] * 2^-24 * S  (+ 2^-126 * flush where hardware flushes fp32 denormals)
half_ulp_bf16(ref) = 2^(floor(log2 |ref|) - 8) is what one round-to-nearest to bf16 (8 significant bits) can cost.  It lies between
2^-9 |ref| and 2^-8 |ref|: a rounding term of 2^-9 |ref| itself is NOT attainable -- the correctly rounded bf16 of 1 + 2^-8 - tiny is
off by 2^-8 (tests/test_elem_ref_cpu.py shows torch's own cast violating it) -- and 2^-8 |ref| would give away up to a factor two;
half an ulp of ref's own binade is the tightest term a correct kernel always meets.  fp32 outputs pass rounding = 2^-24 |ref|.

K: one constant per quantity.  Not invented: tests/test_elem_ref_cpu.py evaluates each kernel's own formula in float32 torch (the
Abramowitz & Stegun 7.1.26 polynomial with the constants of az_common.h, x * 1 / (1 + exp(-x)), the kernels' summation orders ...),
measures the K that needs against float64 over the test inputs (in brackets below) and requires K >= 4 x measured; the table holds
4 x measured rounded up to a power of two (never below 1): the margin is for the hardware reciprocal (1 ulp), __expf and the wave
butterfly sums, which the CPU cannot reproduce.

Not covered on purpose: the 64-bit branch of `divmod` (flat indices above 2^32: tens of gigabytes), the transposes and
az_stage_inputs (exact tests exist), anything that inspects generated code."""
import math

import numpy as np
import torch

U_F32 = 2.0 ** -24
TINY = 2.0 ** -126
GRID_CAP = 4096 * 256               # work items of one sweep of the element-wise grid-stride loops (grid_for in az_elem / az_optim)
SUMSQ_SWEEP = 1024 * 256 * 8        # bf16 elements of one sweep of az_sumsq's 8-wide path

K = {
    "geglu_out": 16.0,     # [3.57]  a * gelu(g): the polynomial's absolute error (2.1e-7 = 3.5 x 2^-24) on top of the product's rounding
    "geglu_da": 16.0,      # [3.57]  dout * gelu(g)
    "geglu_dg": 32.0,      # [4.91]  dout * a * gelu'(g)
    "silu_y": 16.0,        # [2.76]  x / (1 + exp(-x))
    "silu_dx": 16.0,       # [3.53]  dy * s (1 + x (1 - s)) (+ dx)
    "upsample_dx": 1.0,    # [0.00]  four bf16 terms: their fp32 sums are exact
    "colsum": 2.0,         # [0.29]  lane, block and chunk partial sums in fp32
    "reduce_segs": 8.0,    # [1.58]
    "mse_dpred": 16.0,     # [2.52]  k * (pred - target): k (four fp32 operations), the difference and the product rounded
    "mse_mean": 8.0,       # [1.40]  (pred - target)^2 summed over HW * C terms: thread, block, sample
    "mse_loss": 8.0,       # [1.16]
    "temb": 4.0,           # [0.96]  cos / sin of t * exp(-ln(1e4) j / half): the fp32 argument's error scales with |t|
    "sumsq": 8.0,          # [1.14]  fp32 per thread and block, double across blocks
    "clip_coef": 8.0,      # [1.07]  sqrt, add, divide, multiply
}


# ---------------- bounds -------------------------------------------------------------------------------------------------------
def half_ulp_bf16(ref):
    """Half the spacing of bf16 numbers at ref (float64): 2^(floor(log2 |ref|) - 8), the denormal spacing below 2^-126."""
    _, e = torch.frexp(ref.abs())                       # |ref| = m 2^e, m in [0.5, 1)
    e = torch.where(ref == 0, torch.full_like(e, -125), e).clamp_min(-125)
    return torch.ldexp(torch.ones_like(ref), e - 9)


def bound(ref, S, k, rounding=None, flush=None):
    """Per-element bound of a kernel output whose exact value is `ref` (float64).  rounding: defaults to one bf16 rounding; flush: a
    per-element factor on 2^-126 where the kernel's approximate exp / reciprocal flush a denormal intermediate."""
    b = (half_ulp_bf16(ref) if rounding is None else rounding) + K[k] * U_F32 * S
    return b if flush is None else b + TINY * flush


def excess(out, ref, S, rounding=None, flush=None):
    """The K an output needed: max over elements of (|out - ref| - rounding - flush) / (2^-24 S), >= 0."""
    d = (out.double() - ref).abs() - (half_ulp_bf16(ref) if rounding is None else rounding)
    if flush is not None:
        d = d - TINY * flush
    r = d / (U_F32 * S).clamp_min(1e-300)
    return max(float(r.max()), 0.0) if r.numel() else 0.0


def f32_rounding(ref):
    return U_F32 * ref.abs()


# ---------------- GEGLU --------------------------------------------------------------------------------------------------------
SQRT_HALF, INV_SQRT_2PI = math.sqrt(0.5), 1.0 / math.sqrt(2.0 * math.pi)
ERFC_P, ERFC_A = 0.3275911, (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)     # az_common.h gelu_pair


def gelu64(g):
    """(gelu, gelu') of float64 g with the exact erf; the negative tail from erfc (no cancellation)."""
    phi = 0.5 * torch.special.erfc(-g * SQRT_HALF)
    return g * phi, phi + g * torch.exp(-0.5 * g * g) * INV_SQRT_2PI


def gelu_pair_formula(g):
    """az_common.h gelu_pair in the dtype of g (float32: the kernel's formula with correctly rounded exp and reciprocal -- its fmaf
    steps, 0.3275911 x + 1, the Horner steps and the derivative's last step, are restated here as a rounded product and a rounded
    sum each; float64: the polynomial itself)."""
    x = g.abs() * SQRT_HALF
    t = 1.0 / (ERFC_P * x + 1.0)
    e = torch.exp(-x * x)
    poly = t * (ERFC_A[0] + t * (ERFC_A[1] + t * (ERFC_A[2] + t * (ERFC_A[3] + t * ERFC_A[4]))))
    hc = 0.5 * poly * e
    phi = torch.where(g >= 0, 1.0 - hc, hc)
    return g * phi, g * 0.3989422804014327 * e + phi


def geglu_fwd_ref(proj):
    """proj [M][2H] (value | gate) -> out [M][H] = a * gelu(g), S."""
    H = proj.shape[1] // 2
    a, g = proj[:, :H].double(), proj[:, H:].double()
    ge, _ = gelu64(g)
    return a * ge, a.abs() * ge.abs().clamp_min(1.0)


def geglu_bwd_ref(proj, dout):
    """-> dproj [M][2H] = (dout * gelu(g) | dout * a * gelu'(g)), S."""
    H = proj.shape[1] // 2
    a, g, d = proj[:, :H].double(), proj[:, H:].double(), dout.double()
    ge, dge = gelu64(g)
    return (torch.cat([d * ge, d * a * dge], 1),
            torch.cat([d.abs() * ge.abs().clamp_min(1.0), (d * a).abs() * dge.abs().clamp_min(1.0)], 1))


def geglu_fwd_f32(proj):
    H = proj.shape[1] // 2
    return proj[:, :H].float() * gelu_pair_formula(proj[:, H:].float())[0]


def geglu_bwd_f32(proj, dout):
    H = proj.shape[1] // 2
    a, d = proj[:, :H].float(), dout.float()
    ge, dge = gelu_pair_formula(proj[:, H:].float())
    return torch.cat([d * ge, d * a * dge], 1)


# ---------------- SiLU ---------------------------------------------------------------------------------------------------------
def silu_fwd_ref(x):
    """-> y = x s, S, flush.  s = 1 / (1 + e^-x).  The kernel's __expf takes x log2(e) rounded to fp32: a relative error |x| 2^-24 on
    e^-x, |x| (1 - s) 2^-24 on s -- S carries that factor.  flush: below x ~ -87.3 s is an fp32 denormal, which the hardware
    reciprocal may flush: |x| 2^-126 on y."""
    xd = x.double()
    s = 1.0 / (1.0 + torch.exp(-xd))
    return xd * s, (xd * s).abs() * (1.0 + xd.abs() * (1.0 - s)), xd.abs()


def silu_bwd_ref(x, dy, dx_old=None):
    """-> dx = dy s (1 + x (1 - s)) (+ dx_old), S, flush.  The kernel forms 1 - s from the rounded s (absolute error 2^-24 s, times |x|)."""
    xd, d = x.double(), dy.double()
    s = 1.0 / (1.0 + torch.exp(-xd))
    out = d * s * (1.0 + xd * (1.0 - s))
    S = d.abs() * s * (1.0 + xd.abs()) * (1.0 + xd.abs() * (1.0 - s))
    if dx_old is not None:
        out, S = out + dx_old.double(), S + dx_old.double().abs()
    return out, S, d.abs() * (1.0 + xd.abs())


def silu_fwd_f32(x):
    xf = x.float()
    return xf * (1.0 / (1.0 + torch.exp(-xf)))


def silu_bwd_f32(x, dy, dx_old=None):
    xf = x.float()
    s = 1.0 / (1.0 + torch.exp(-xf))
    v = dy.float() * (s * (1.0 + xf * (1.0 - s)))
    return v if dx_old is None else v + dx_old.float()


# ---------------- add_rows, upsample --------------------------------------------------------------------------------------------
def add_rows_bits(a, b):
    """bf16(a + b): one fp32 addition, exact restatement."""
    return (a.float() + b.float()).bfloat16()


def upsample_fwd_ref(x):
    """x [B][H][W][C] -> [B][2H][2W][C], a copy."""
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def upsample_bwd_ref(dy):
    """dy [B][2H][2W][C] -> dx [B][H][W][C] = the four taps' sum, S."""
    B, H2, W2, C = dy.shape
    t = dy.double().reshape(B, H2 // 2, 2, W2 // 2, 2, C)
    return t.sum((2, 4)), t.abs().sum((2, 4))


def upsample_bwd_f32(dy):
    B, H2, W2, C = dy.shape
    t = dy.float().reshape(B, H2 // 2, 2, W2 // 2, 2, C)
    return ((t[:, :, 0, :, 0] + t[:, :, 0, :, 1]) + t[:, :, 1, :, 0]) + t[:, :, 1, :, 1]


# ---------------- column sums --------------------------------------------------------------------------------------------------
# (rows, C, rows_per_seg) and the branches of colsum_geom each case is there for (tests/test_elem_ref_cpu.py asserts them)
COLSUM_CASES = [
    ((64, 8, 64), ("bx1", "by_clamped", "rpc_floor", "chunks_256", "ragged", "small_block")),
    ((77 * 7, 40, 7), ("by_clamped", "rpc_floor", "ragged", "small_block")),        # bx = 5: 160-thread blocks
    ((3 * 1000, 320, 1000), ("rpc_floor", "chunks_256", "ragged", "small_block")),
    ((5000, 320, 5000), ("rpc_floor", "chunks_256", "ragged", "small_block")),
    ((4200, 8, 2), ("bx1", "by_clamped", "rpc_floor", "chunks_1", "ragged", "small_block")),   # nseg * zb > 2048
    ((4 * 96, 1024, 96), ("rpc_floor", "chunks_256")),
    ((2 * 100, 1032, 100), ("zb2", "rpc_floor", "chunks_256", "ragged")),                        # the second column block has one live lane
    ((2 * 64, 2560, 64), ("zb3", "rpc_floor", "chunks_256")),
    ((5, 72, 1), ("rpc_floor", "chunks_256", "ragged", "small_block")),
    ((2103, 1024, 2103), ("chunks_256", "rpc_above_floor", "ragged")),             # a neighbour: 211 chunks of 10 rows, the last of 3
]


def colsum_geom(rows, C, rows_per_seg):
    """Python port of colsum_geom (az_elem.hip) -> dict(bx, by, zb, rpc, nchunk, nseg) and the set of branches taken."""
    cch = C // 8
    bx = min(cch, 128)
    by0 = 256 // bx
    by = min(max(by0, 1), 32)
    zb = (cch + bx - 1) // bx
    nseg = rows // rows_per_seg
    want0 = 2048 // (nseg * zb)
    want = min(max(want0, 1), 256)
    rpc0 = (rows_per_seg + want - 1) // want
    rpc1 = max(rpc0, 4 * by)
    rpc = (rpc1 + by - 1) // by * by
    nchunk = (rows_per_seg + rpc - 1) // rpc
    br = set()
    if bx == 1:
        br.add("bx1")
    if by0 > 32:
        br.add("by_clamped")
    br.add("rpc_floor" if rpc0 < 4 * by else "rpc_above_floor")
    if want0 < 1:
        br.add("chunks_1")
    if want0 > 256:
        br.add("chunks_256")
    if zb in (2, 3):
        br.add(f"zb{zb}")
    if rows_per_seg % rpc:
        br.add("ragged")
    if bx * by < 256:
        br.add("small_block")
    return dict(bx=bx, by=by, zb=zb, rpc=rpc, nchunk=nchunk, nseg=nseg), br


def colsum_ref(x, rows_per_seg):
    """x [rows][C] -> [nseg][C] float64 sums, S."""
    xd = x.double().reshape(-1, rows_per_seg, x.shape[1])
    return xd.sum(1), xd.abs().sum(1)


def colsum_grad_ref(x, rows_per_seg, bias_old, n_real):
    """-> seg [nseg][C], S_seg, bias [C] (entries >= n_real unchanged), S_bias."""
    seg, S = colsum_ref(x, rows_per_seg)
    live = (torch.arange(x.shape[1]) < n_real).double()
    return seg, S, bias_old.double() + live * seg.sum(0), bias_old.double().abs() + live * S.sum(0)


def colsum_partials_f32(x, rows_per_seg):
    """colsum_kernel's partial[seg][chunk][C] in its own order: a lane's rows one after the other, the block's lanes one after
    the other."""
    rows, C = x.shape
    g, _ = colsum_geom(rows, C, rows_per_seg)
    xf = x.float().reshape(g["nseg"], rows_per_seg, C)
    part = torch.zeros(g["nseg"], g["nchunk"], C)
    for ch in range(g["nchunk"]):
        blk = xf[:, ch * g["rpc"]:(ch + 1) * g["rpc"]]
        lanes = torch.zeros(g["nseg"], g["by"], C)
        for j in range(0, blk.shape[1], g["by"]):
            r = blk[:, j:j + g["by"]]
            lanes[:, :r.shape[1]] += r
        a = torch.zeros(g["nseg"], C)
        for y in range(g["by"]):
            a = a + lanes[:, y]
        part[:, ch] = a
    return part


def _slices_f32(part, nsl):
    """sum over chunks the way the final kernels do: nsl interleaved slices, each serial, then the slices serial."""
    tot = torch.zeros(part.shape[0], part.shape[2])
    for sl in range(nsl):
        a = torch.zeros_like(tot)
        for k in range(sl, part.shape[1], nsl):
            a = a + part[:, k]
        tot = tot + a
    return tot


def colsum_f32(x, rows_per_seg):
    return _slices_f32(colsum_partials_f32(x, rows_per_seg), 4)


def colsum_grad_f32(x, rows_per_seg, bias_old, n_real):
    seg = _slices_f32(colsum_partials_f32(x, rows_per_seg), 8)
    tot = torch.zeros(x.shape[1])
    for s in range(seg.shape[0]):
        tot = tot + seg[s]
    bias = torch.where(torch.arange(x.shape[1]) < n_real, bias_old.float() + tot, bias_old.float())
    return seg, bias


def reduce_segs_ref(src, nseg, n, dst_old=None):
    """src fp32 [nseg][n] -> float64 [n] (+ dst_old), S."""
    s = src.double().reshape(nseg, n)
    out, S = s.sum(0), s.abs().sum(0)
    if dst_old is not None:
        out, S = out + dst_old.double(), S + dst_old.double().abs()
    return out, S


def reduce_segs_f32(src, nseg, n, dst_old=None):
    a = torch.zeros(n)
    for k in range(nseg):
        a = a + src.reshape(nseg, n)[k]
    return a if dst_old is None else a + dst_old.float()


# ---------------- weighted MSE -------------------------------------------------------------------------------------------------
def mse_ref(pred, target, w, gscale):
    """pred [B][HW][ldp] bf16 (channels c < C live), target [B][C][HW] fp32, w [B] fp32 -> dict(dpred [B][HW][C], S_dpred,
    mean [B], S_mean, loss, S_loss) in float64."""
    B, C, HW = target.shape
    d = pred[..., :C].double() - target.double().permute(0, 2, 1)
    k = gscale * w.double() * 2.0 / (C * HW * B)
    mean = (d * d).sum((1, 2)) / (C * HW)
    # the difference of two exactly known values is rounded once: every term is relative to its own magnitude
    return dict(dpred=k[:, None, None] * d, S_dpred=(k[:, None, None] * d).abs(), mean=mean, S_mean=mean,
                loss=(mean * w.double()).sum() / B, S_loss=(mean * w.double().abs()).sum() / B)


def mse_f32(pred, target, w, gscale):
    """mse_kernel / mse_finalize_kernel in float32 in their own order: a thread's pixels and channels one after the other, the block,
    the sample's blocks one after the other."""
    B, C, HW = target.shape
    gx = min((HW + 255) // 256, 64)
    d = pred[..., :C].float() - target.permute(0, 2, 1)
    k = torch.tensor(gscale, dtype=torch.float32) * w * 2.0 / (torch.tensor(float(C)) * float(HW) * float(B))
    sweep = gx * 256
    nsw = (HW + sweep - 1) // sweep
    dd = torch.zeros(B, nsw * sweep, C)
    dd[:, :HW] = d * d
    acc = torch.zeros(B, sweep)
    for s in range(nsw):
        for c in range(C):
            acc = acc + dd[:, s * sweep:(s + 1) * sweep, c]
    blocks = acc.reshape(B, gx, 256).sum(2)
    ps = torch.zeros(B)
    for j in range(gx):
        ps = ps + blocks[:, j]
    mean = ps / (torch.tensor(float(C)) * float(HW))
    loss = torch.zeros(())
    for b in range(B):
        loss = loss + mean[b] * w[b]
    return k[:, None, None] * d, mean, loss / float(B)


# ---------------- noise and target (bits) -----------------------------------------------------------------------------------------
def bf16_round_np(x):
    """float32 array -> float32 array holding the bf16 value (round to nearest even; NaN stays NaN)."""
    return (bf16_bits_np(x).astype(np.uint32) << 16).view(np.float32)


def bf16_bits_np(x):
    """float32 array -> uint16 bf16 bits, round to nearest even; a NaN becomes the quiet NaN 0x7FC0 (sign kept)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u + (np.uint32(0x7FFF) + ((u >> 16) & 1))) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((u >> 16) & 0x8000).astype(np.uint16) | np.uint16(0x7FC0), r)


def bits_to_bf16(b):
    """uint16 numpy bits -> torch bf16 tensor."""
    return torch.from_numpy(b.astype(np.int16)).view(torch.bfloat16)


def bf16_to_np(t):
    """torch bf16 tensor -> float32 numpy (exact)."""
    return t.float().numpy()


def noise_target_bits(mode, lat, noise, ca, cb, cpad):
    """noise_target_kernel: lat [B][C][HW] bf16, noise [B][C][HW] fp32, ca / cb [B] fp32 -> noisy [B][HW][cpad] bf16 (padding 0),
    target [B][C][HW] fp32.  Separate fp32 operations, no contraction; the DDPM modes (0 epsilon, 1 v) round coefficient x latent
    products to bf16."""
    x, nz = bf16_to_np(lat), noise.numpy()
    a, s = ca.numpy()[:, None, None], cb.numpy()[:, None, None]
    with np.errstate(all="ignore"):
        if mode == 2:
            xt, tg = a * x + s * nz, nz - x
        else:
            xt = bf16_round_np(a * x) + s * nz
            tg = (a * nz - bf16_round_np(s * x)) if mode == 1 else nz.copy()
    B, C, HW = x.shape
    noisy = np.zeros((B, HW, cpad), dtype=np.uint16)
    noisy[..., :C] = bf16_bits_np(xt).transpose(0, 2, 1)
    return bits_to_bf16(noisy), torch.from_numpy(np.ascontiguousarray(tg, dtype=np.float32))


# ---------------- timestep embedding -------------------------------------------------------------------------------------------
LN_1E4_F32 = 9.210340371976184


def temb_ref(t, dim):
    """t [n] fp32 -> [n][dim] float64 (cos | sin), S.  arg = t exp(-ln(1e4) j / half): the kernel's fp32 exponent, expf and product
    leave a relative error ~(|expo| + 2) 2^-24 on arg, i.e. |arg| (|expo| + 2) 2^-24 absolute on cos / sin (about 1000 x 2^-24 at
    t ~ 1000) on top of their own rounding (values <= 1)."""
    half = dim // 2
    j = torch.arange(half, dtype=torch.float64)
    expo = -LN_1E4_F32 * j / half
    arg = t.double()[:, None] * torch.exp(expo)[None]
    S = 1.0 + arg.abs() * (expo.abs()[None] + 2.0)
    return torch.cat([torch.cos(arg), torch.sin(arg)], 1), torch.cat([S, S], 1)


def temb_f32(t, dim):
    half = dim // 2
    j = torch.arange(half, dtype=torch.float32)
    expo = (torch.tensor(-LN_1E4_F32, dtype=torch.float32) * j) / float(half)
    arg = t.float()[:, None] * torch.exp(expo)[None]
    return torch.cat([torch.cos(arg), torch.sin(arg)], 1)


# ---------------- sum of squares, clip coefficient ---------------------------------------------------------------------------------
def sumsq_ref(g, prev=0.0):
    """-> float64 sum of squares (+ prev), S."""
    s = float((g.double() ** 2).sum())
    return torch.tensor(prev + s, dtype=torch.float64), torch.tensor(abs(prev) + s, dtype=torch.float64)


def sumsq_f32(g, prev=0.0):
    """sumsq_partial_kernel / sumsq_final_kernel: fp32 per thread (8-wide vectors first for 2-byte types, then the tail) and per
    block, double across blocks."""
    n = g.numel()
    nblk = min(max((n + 255) // 256, 1), 1024)
    T = nblk * 256
    x = g.float().reshape(-1)
    acc = torch.zeros(T)
    if g.element_size() == 2:
        n8 = n // 8
        v = x[:n8 * 8].reshape(n8, 4, 2)
        pair = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]
        nsw = (n8 + T - 1) // T
        pp = torch.zeros(nsw * T, 4)
        pp[:n8] = pair
        for s in range(nsw):
            for e in range(4):
                acc = acc + pp[s * T:(s + 1) * T, e]
        tail = x[n8 * 8:]
        acc[:tail.numel()] += tail * tail
    else:
        nsw = (n + T - 1) // T
        pp = torch.zeros(nsw * T)
        pp[:n] = x * x
        for s in range(nsw):
            acc = acc + pp[s * T:(s + 1) * T]
    blocks = acc.reshape(nblk, 256).sum(1)
    return torch.tensor(prev, dtype=torch.float32) + blocks.double().sum().float()


def clip_coef_ref(sumsq, max_norm, unscale):
    """-> (coef, norm) float64: norm = sqrt(sumsq) unscale, coef = min(max_norm / (norm + 1e-6), 1) unscale."""
    nrm = math.sqrt(sumsq) * unscale
    c = max_norm / (nrm + float(np.float32(1e-6)))
    return min(c, 1.0) * unscale, nrm


def clip_coef_f32(sumsq, max_norm, unscale):
    with np.errstate(all="ignore"):
        nrm = np.sqrt(np.float32(sumsq)) * np.float32(unscale)
        c = np.float32(max_norm) / (nrm + np.float32(1e-6))
        return float((c if c < 1 else np.float32(1.0)) * np.float32(unscale)), float(nrm)


# ---------------- casts, scales, offload (bits) ------------------------------------------------------------------------------------
def cast_edges():
    """fp32 bit patterns: ties to even and to odd, the largest finite value that rounds to inf, denormals, +-0, +-inf, NaNs."""
    u = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F818001, 0x3F817FFF, 0xBF808000, 0xBF818000,
                  0x7F7F8000, 0x7F7F7FFF, 0x7F7FFFFF, 0xFF7F8000, 0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80008000,
                  0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC12345, 0x7FFFFFFF], dtype=np.uint32)
    return torch.from_numpy(u.view(np.float32).copy())


def f32_to_bf16_bits(x):
    """fp32 torch tensor -> bf16 torch tensor, round to nearest even (integer arithmetic on the bits)."""
    return bits_to_bf16(bf16_bits_np(x.numpy()))


def scale_bf16_bits(g, c):
    """scale_bf16_kernel: bf16(float(g) * c); the buffer untouched (NaN payloads included) when c == 1."""
    if np.float32(c) == np.float32(1.0):
        return g.clone()
    with np.errstate(all="ignore"):
        return bits_to_bf16(bf16_bits_np(bf16_to_np(g) * np.float32(c)))


def scale_f32_bits(x, c):
    with np.errstate(all="ignore"):
        return torch.from_numpy(x.numpy() * np.float32(c))


def titan_offload_bits(g, gh_old, accumulate):
    """offload_kernel: gh = float(g), or gh + float(g)."""
    with np.errstate(all="ignore"):
        return torch.from_numpy(gh_old.numpy() + bf16_to_np(g)) if accumulate else g.float()


# ---------------- AdamW (bits) -----------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """Correctly rounded float32 a * b + c (numpy float32 arrays): exact product and round-to-odd sum in float64, one rounding."""
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)          # exact: 48 bits
        cd = c.astype(np.float64)
        s = p + cd
        bb = s - p
        err = (p - (s - bb)) + (cd - bb)                            # TwoSum: s + err = p + c exactly
        inexact = np.isfinite(err) & (err != 0) & np.isfinite(s)
        other = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        even = (s.view(np.int64) & 1) == 0
        s = np.where(inexact & even, other, s)                      # of the two doubles around the exact sum, the odd one
        return s.astype(np.float32)


def adamw_hyper(lr, betas, wd, eps, debias, step):
    """The hyper vector RavenAdamW.step hands the kernel (optimizers/raven.py), as fp32: [lr, b1, b2, eps, wd_factor, step_size,
    sqrt_bc2, 0]."""
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    if debias < 1.0:
        bc1, bc2 = 1.0 - (1.0 - bc1) * debias, 1.0 - (1.0 - bc2) * debias
    wdf = 1.0 - lr * wd if wd != 0 else 1.0
    return np.array([lr, b1, b2, eps, wdf, lr / bc1, math.sqrt(bc2), 0.0], dtype=np.float32)


_MOMENT = {0: torch.bfloat16, 1: torch.float32, 2: torch.float16}


def moment_dtype(mdtype):
    return _MOMENT[mdtype]


def _store(x, mdtype):
    if mdtype == 0:
        return bits_to_bf16(bf16_bits_np(x))
    with np.errstate(all="ignore"):
        return torch.from_numpy(x.astype(np.float16) if mdtype == 2 else x.copy())


def adamw_bits(p, g, m, v, hyper, coef=None):
    """adamw_kernel, operation for operation (its comment): p bf16, g bf16 | fp32, m / v bf16 | fp32 | fp16 torch CPU tensors, hyper a
    float32 numpy vector, coef None or a float -> (p, m, v) new tensors of the same dtypes.  One fused multiply-add (exp_avg); every
    other product, quotient, sqrt and sum rounded to fp32; a bf16 gradient times the coefficient is rounded to bf16 again."""
    mdtype = {torch.bfloat16: 0, torch.float32: 1, torch.float16: 2}[m.dtype]
    f = np.float32
    b1, b2, eps, wdf, step, sbc2 = (f(hyper[i]) for i in range(1, 7))
    omb1, omb2 = f(1.0) - b1, f(1.0) - b2
    with np.errstate(all="ignore"):
        gr = g.float().numpy() * (f(coef) if coef is not None else f(1.0))
        if g.dtype == torch.bfloat16:
            gr = bf16_round_np(gr)
        mm = fma32(gr, np.full_like(gr, omb1), m.float().numpy() * b1)
        vv = v.float().numpy() * b2
        vv = vv + ((omb2 * gr) * gr)
        pp = bf16_to_np(p) * wdf
        denom = np.sqrt(vv) / sbc2 + eps
        pp = pp + ((-step * mm) / denom)
    return bits_to_bf16(bf16_bits_np(pp)), _store(mm, mdtype), _store(vv, mdtype)


# ---------------- inputs ---------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def gate_values(shape, seed):
    """GEGLU gates: Gaussian bulk, a quarter uniform over [-40, 40], +-0 and the interval's ends."""
    g = gen(seed)
    x = 1.5 * torch.randn(*shape, generator=g)
    u = torch.rand(*shape, generator=g) * 80.0 - 40.0
    x = torch.where(torch.rand(*shape, generator=g) < 0.25, u, x)
    f = x.reshape(-1)
    for i, val in enumerate((0.0, -0.0, 40.0, -40.0, -13.5, 5.0)):
        if i < f.numel():
            f[i] = val
    return x.bfloat16()


def geglu_inputs(M, H, seed):
    """proj [M][2H] bf16 (value | gate), dout [M][H] bf16."""
    g = gen(seed + 1)
    a = torch.randn(M, H, generator=g).bfloat16()
    return torch.cat([a, gate_values((M, H), seed)], 1), torch.randn(M, H, generator=g).bfloat16()


def silu_inputs(n, seed):
    """x over [-100, 100] (where __expf(-x) overflows and where s is denormal) with a Gaussian bulk and +-0; dy, dx_old."""
    g = gen(seed)
    x = 2.0 * torch.randn(n, generator=g)
    x = torch.where(torch.rand(n, generator=g) < 0.25, torch.rand(n, generator=g) * 200.0 - 100.0, x)
    for i, val in enumerate((0.0, -0.0, 100.0, -100.0, -88.0, -87.5, -89.0, 88.0)):
        if i < n:
            x[i] = val
    return x.bfloat16(), torch.randn(n, generator=g).bfloat16(), torch.randn(n, generator=g).bfloat16()


def ints_bf16(shape, seed, lim=4):
    """bf16 integers in [-lim, lim]: every partial sum of fewer than 2^24 / lim of them is exact in fp32 in any order."""
    return torch.randint(-lim, lim + 1, shape, generator=gen(seed)).bfloat16()


def gauss_bf16(shape, seed, scale=1.0):
    return (scale * torch.randn(*shape, generator=gen(seed))).bfloat16()


def adamw_grads(n, seed, f32):
    """Gradients with a 0, a NaN, an inf and a magnitude whose square overflows fp16 moments among the first four elements."""
    g = 1e-2 * torch.randn(n, generator=gen(seed))
    for i, val in enumerate((0.0, float("nan"), float("inf"), 1.0e4)):
        if i < n - 1:
            g[i] = val
    return g if f32 else g.bfloat16()
