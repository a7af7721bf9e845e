"""Float64 restatement of the GroupNorm / LayerNorm kernels (csrc/az_norm.hip), with per-element error bounds.  The product never
imports this file; tests/test_norms_gpu.py compares the HIP kernels against it.

Plain torch float64 on the CPU, written out as formulas (no autograd) so that the statistics the backward reads can be modelled:
  * forwards use exact statistics (variance about the mean, two passes);
  * backwards take the fp32 statistics the kernel's forward wrote, rounded to bf16 when NORM_STAT_BF16 = 1 (`stat_round` in
    az_norm.hip).  GroupNorm evaluates SiLU' at z formed from the UNROUNDED pair, its own formula uses the rounded pair;
  * dx = dx_add + gradient, dgamma / dbeta = prev + sum: each rounded once to bf16 by the kernel.

GroupNorm tensors are NHWC as the kernels see them: x [B][HW][C].  LayerNorm tensors are [M][C].

Every reference value comes with S, the sum of the absolute values of the terms the kernel combined in fp32 for that element, and
    bound = rounding + K * 2^-24 * S
where `rounding` is one rounding to the format the kernel stores: 2^-8 |ref| for bf16 outputs (the unit roundoff: a correctly
rounded value is never further from the exact one; a full ulp would let a coherent 2^-9 scale error through), 2^-24 |ref| for the
fp32 statistics (R_mean / R_var / R_rstd in the forward references).  K is one constant per quantity (table K below): the fp32 slack of the kernel's summation
orders and approximate SiLU.  Because S carries the magnitudes that were combined, the bounds stay tight on large values and do not
fail where the result cancels."""
import torch

U_BF16 = 2.0 ** -8
U_F32 = 2.0 ** -24

# Slack in units of 2^-24 * S, per quantity.  Measured on an MI355X over every case of tests/test_norms_gpu.py, both NORM_STAT_BF16
# values and every GN_RPT / GN_RPT_BWD / LN_RPB value tested: the largest (|err| - rounding) / (2^-24 S) observed is in brackets.
# Each K is about twice that, rounded up to a power of two, and never below 1 (one fp32 rounding of the terms combined).
K = {
    "gn_y": 4.0,        # [1.94] x*sc + sf, SiLU through exp and a hardware reciprocal
    "gn_mean": 1.0,     # [0.16] fp32 partial sums over a thread's rows, the block's rows and channels; double across chunks
    "gn_var": 4.0,      # [1.22] one-pass: (sum x^2) / n - mean^2 in double from the same fp32 partial sums
    "gn_dx": 1.0,       # [0.29] dz, x_hat, the fp32 channel / group sums behind k1, k2
    "gn_dparam": 1.0,   # [0.07] fp32 sums over rows, chunks, samples
    "ln_y": 2.0,        # [0.97]
    "ln_mean": 1.0,     # [0.37]
    "ln_var": 8.0,      # [2.81] two-pass in fp32, rsqrtf (an approximate reciprocal square root: its error doubles in var)
    "ln_dx": 1.0,       # [0.21]
    "ln_dparam": 1.0,   # [0.03]
}


def bound(ref, S, k, rounding=None):
    """Per-element bound of a kernel output whose exact value is `ref` (float64); `rounding` defaults to one bf16 rounding."""
    return (U_BF16 * ref.abs() if rounding is None else rounding) + K[k] * U_F32 * S


def excess(out, ref, S, rounding=None):
    """The K an output needed: max over elements of (|out - ref| - rounding) / (2^-24 S), >= 0."""
    d = (out.double() - ref).abs() - (U_BF16 * ref.abs() if rounding is None else rounding)
    r = d / (U_F32 * S.clamp_min(1e-300))
    return max(float(r.max()), 0.0) if r.numel() else 0.0


def _stat_terms(mean, var, eps):
    """S and rounding allowances of the statistics.  mean: within K 2^-24 of the RMS (+ its own fp32 rounding).  var, the variance
    the kernel's rstd stands for (var_from_rstd): within K 2^-24 (mean^2 + var + eps), + 2^-23 (var + eps) for the fp32 rounding of
    rstd.  rstd itself (checked where it is saved in bf16): the same variance error, as 0.5 rstd dvar / (var + eps)."""
    rstd = 1.0 / torch.sqrt(var + eps)
    S_var = mean * mean + var + eps
    return dict(S_mean=torch.sqrt(mean * mean + var), R_mean=U_F32 * mean.abs(), S_var=S_var, R_var=2.0 * U_F32 * (var + eps),
                S_rstd=0.5 * rstd * S_var / (var + eps), R_rstd=U_F32 * rstd)


def stat_round(t):
    """fp32 -> bf16 -> fp32 (round to nearest even) of fp32 statistics, as float64."""
    return t.float().bfloat16().double()


def _sigmoid(z):
    return 1.0 / (1.0 + torch.exp(-z))


# ---------------- GroupNorm ----------------------------------------------------------------------------------------------------
def _chan(t, C):
    """[B][G] per-group values -> [B][1][C] per channel."""
    return t.repeat_interleave(C // t.shape[1], dim=1)[:, None, :]


def gn_fwd_ref(x, gamma, beta, G, eps, silu):
    """-> dict(y, S_y, mean, var, rstd [B][G], and S_ / R_ mean, var, rstd: _stat_terms).  x [B][HW][C]; gamma, beta [C]."""
    B, HW, C = x.shape
    xd, ga, be = x.double(), gamma.double(), beta.double()
    xg = xd.reshape(B, HW, G, C // G)
    mean = xg.mean((1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
    rstd = 1.0 / torch.sqrt(var + eps)
    mc, rc = _chan(mean, C), _chan(rstd, C)
    z = (xd - mc) * rc * ga + be
    y = z * _sigmoid(z) if silu else z
    # the kernel: z = x * sc + sf, sc = rstd * gamma, sf = beta - mean * rstd * gamma
    S_y = (xd.abs() + mc.abs()) * (rc * ga).abs() + be.abs() + y.abs()
    return dict(y=y, S_y=S_y, mean=mean, var=var, rstd=rstd, **_stat_terms(mean, var, eps))


def gn_bwd_ref(x, gamma, beta, stats, dy, G, silu, stat_bf16, dx_add=None, dgamma_prev=None, dbeta_prev=None):
    """stats: [B][G][2] (mean, rstd) as the forward kernel wrote them (fp32 values).  -> dict(dx, S_dx, dgamma, S_dgamma, dbeta,
    S_dbeta); dx includes dx_add, dgamma / dbeta include their previous values."""
    B, HW, C = x.shape
    st = stats.double().reshape(B, G, 2).repeat_interleave(C // G, dim=1)
    return gn_bwd_ref_chan(x, gamma, beta, st, dy, G, silu, stat_bf16, dx_add, dgamma_prev, dbeta_prev)


def gn_bwd_ref_chan(x, gamma, beta, stats_c, dy, G, silu, stat_bf16, dx_add=None, dgamma_prev=None, dbeta_prev=None, k_rows=None,
                    r_scale=None):
    """gn_bwd_ref with the statistics given per CHANNEL, stats_c [B][C][2], the rows whose terms enter k1 / k2 (all unless `k_rows`,
    a slice, says otherwise) and a per-channel factor [C] on the rstd the formula reads (after any rounding): the tightness tests
    build wrong kernels from these."""
    B, HW, C = x.shape
    cpg, n = C // G, HW * (C // G)
    xd, ga, be, d = x.double(), gamma.double(), beta.double(), dy.double()
    st = stats_c.double()[:, None, :, :]                              # [B][1][C][2]
    m32, r32 = st[..., 0], st[..., 1]
    m, r = (stat_round(m32), stat_round(r32)) if stat_bf16 else (m32, r32)
    if r_scale is not None:
        r = r * r_scale.double()
    if silu:
        z = (xd - m32) * r32 * ga + be
        s = _sigmoid(z)
        dz = d * (s * (1.0 + z * (1.0 - s)))
        E = dz.abs() + d.abs() * ((xd.abs() + m32.abs()) * (r32 * ga).abs() + be.abs())   # dz and what the z it was taken at combined
    else:
        dz = d
        E = d.abs()
    xh = (xd - m) * r
    A, Bs = dz.sum(1), (dz * xh).sum(1)                               # [B][C]
    Ak, Bk = (A, Bs) if k_rows is None else (dz[:, k_rows].sum(1), (dz * xh)[:, k_rows].sum(1))
    k1 = (ga * Ak).reshape(B, G, cpg).sum(-1) / n                      # [B][G]
    k2 = (ga * Bk).reshape(B, G, cpg).sum(-1) / n
    EA, EB = E.sum(1), (E * xh.abs()).sum(1)
    k1a = (ga.abs() * EA).reshape(B, G, cpg).sum(-1) / n
    k2a = (ga.abs() * EB).reshape(B, G, cpg).sum(-1) / n
    dx = r * (dz * ga - _chan(k1, C) - xh * _chan(k2, C))
    S_dx = r.abs() * (E * ga.abs() + _chan(k1a, C) + xh.abs() * _chan(k2a, C))
    if dx_add is not None:
        dx = dx + dx_add.double()
        S_dx = S_dx + dx_add.double().abs()
    pg = dgamma_prev.double() if dgamma_prev is not None else torch.zeros(C, dtype=torch.float64)
    pb = dbeta_prev.double() if dbeta_prev is not None else torch.zeros(C, dtype=torch.float64)
    return dict(dx=dx, S_dx=S_dx, dgamma=pg + Bs.sum(0), S_dgamma=pg.abs() + EB.sum(0), dbeta=pb + A.sum(0), S_dbeta=pb.abs() + EA.sum(0))


# ---------------- LayerNorm ----------------------------------------------------------------------------------------------------
def ln_fwd_ref(x, gamma, beta, eps):
    """-> dict(y, S_y, mean, var, rstd [M], and S_ / R_ mean, var, rstd: _stat_terms).  x [M][C]."""
    xd, ga, be = x.double(), gamma.double(), beta.double()
    mean = xd.mean(1)
    var = ((xd - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (xd - mean[:, None]) * rstd[:, None] * ga + be
    S_y = (xd.abs() + mean.abs()[:, None]) * (rstd[:, None] * ga).abs() + be.abs()
    return dict(y=y, S_y=S_y, mean=mean, var=var, rstd=rstd, **_stat_terms(mean, var, eps))


def ln_bwd_ref(x, gamma, stats, dy, stat_bf16, dx_add=None, dgamma_prev=None, dbeta_prev=None):
    """stats: [M][2] as the forward kernel SAVED them (already bf16 values when NORM_STAT_BF16 = 1: the LayerNorm backward kernels
    read them as they are; rounding them again here changes nothing).  -> dict(dx, S_dx, dgamma, S_dgamma, dbeta, S_dbeta)."""
    M, C = x.shape
    xd, ga, d = x.double(), gamma.double(), dy.double()
    st = stats.double().reshape(M, 2)
    if stat_bf16:
        st = stat_round(st)
    m, r = st[:, :1], st[:, 1:]
    xh = (xd - m) * r
    g = d * ga
    c1, c2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    c1a, c2a = g.abs().mean(1, keepdim=True), (g * xh).abs().mean(1, keepdim=True)
    dx = r * (g - c1 - xh * c2)
    S_dx = r.abs() * (g.abs() + c1a + xh.abs() * c2a)
    if dx_add is not None:
        dx = dx + dx_add.double()
        S_dx = S_dx + dx_add.double().abs()
    pg = dgamma_prev.double() if dgamma_prev is not None else torch.zeros(C, dtype=torch.float64)
    pb = dbeta_prev.double() if dbeta_prev is not None else torch.zeros(C, dtype=torch.float64)
    return dict(dx=dx, S_dx=S_dx, dgamma=pg + (d * xh).sum(0), S_dgamma=pg.abs() + (d * xh).abs().sum(0),
                dbeta=pb + d.sum(0), S_dbeta=pb.abs() + d.abs().sum(0))


def var_from_rstd(rstd, eps):
    """The variance a kernel's rstd stands for (float64)."""
    return 1.0 / (rstd.double() ** 2) - eps


def gn_rows_per_chunk(HW, C, rpt):
    """Rows of one chunk of a GroupNorm row pass (gn_geom in az_norm.hip), rpt already clamped to [4, 64]."""
    py = max(256 // (C // 8), 1)
    want = max((HW + 1023) // 1024, rpt * py)
    return (want + py - 1) // py * py



# ---------------- inputs -------------------------------------------------------------------------------------------------------
def gn_inputs(B, HW, C, G, seed, edges=False):
    """bf16 CPU tensors x [B][HW][C], gamma, beta [C], dy [B][HW][C].  edges: group 3 of every sample is a large-offset group (mean
    ~6, std ~0.05: the one-pass variance), group 5 a constant one (var = 0, rstd = 1/sqrt(eps))."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, HW, C, generator=g) * 1.5 + 0.3
    if edges:
        cpg = C // G
        x[:, :, 3 * cpg:4 * cpg] = 6.0 + 0.05 * torch.randn(B, HW, cpg, generator=g)
        x[:, :, 5 * cpg:6 * cpg] = 0.75
    gamma = 1.0 + 0.2 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    dy = torch.randn(B, HW, C, generator=g)
    return x.bfloat16(), gamma.bfloat16(), beta.bfloat16(), dy.bfloat16()


def ln_inputs(M, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g) * 2.0 - 0.5
    gamma = 1.0 + 0.2 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    dy = torch.randn(M, C, generator=g)
    return x.bfloat16(), gamma.bfloat16(), beta.bfloat16(), dy.bfloat16()


def small_bf16(shape, seed, scale=0.1):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).bfloat16()
