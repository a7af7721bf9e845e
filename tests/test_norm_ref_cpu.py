"""The float64 GroupNorm / LayerNorm restatement (tests/norm_ref.py) without a GPU: it equals torch's float64 autograd with exact
statistics, it follows a hand-rounded restatement with NORM_STAT_BF16 = 1, and its bounds are tight enough to REJECT the kernel
errors the GPU tests are there to catch (a bound that accepts them proves nothing) while accepting the correctly rounded result."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import norm_ref as R        # noqa: E402


def close(a, b, tol=1e-12):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


def rounded(t):
    """What a kernel that got `t` exactly right stores: one rounding to bf16."""
    return t.float().bfloat16()


def within(out, ref, S, k, rounding=None):
    return bool(((out.double() - ref).abs() <= R.bound(ref, S, k, rounding)).all())


def fp32_stats(fw):
    """[B][G][2] fp32 statistics as a kernel's forward writes them, from the exact ones."""
    return torch.stack([fw["mean"], fw["rstd"]], -1).float()


# ---------------- equal to autograd -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW,C,G,silu,eps", [(2, 37, 64, 8, True, 1e-5), (1, 50, 96, 32, False, 1e-6), (3, 9, 24, 3, True, 1e-5)])
def test_groupnorm_reference_equals_float64_autograd(B, HW, C, G, silu, eps):
    x, gamma, beta, dy = R.gn_inputs(B, HW, C, G, seed=B * 100 + C)
    add, pg, pb = R.small_bf16((B, HW, C), 1), R.small_bf16((C,), 2), R.small_bf16((C,), 3)
    xf = x.double().permute(0, 2, 1).requires_grad_(True)
    gf, bf_ = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.group_norm(xf, G, gf, bf_, eps)
    if silu:
        y = F.silu(y)
    y.backward(dy.double().permute(0, 2, 1))
    fw = R.gn_fwd_ref(x, gamma, beta, G, eps, silu)
    assert close(fw["y"], y.detach().permute(0, 2, 1))
    stats = torch.stack([fw["mean"], fw["rstd"]], -1)        # exact float64 statistics: nothing rounded
    bw = R.gn_bwd_ref(x, gamma, beta, stats, dy, G, silu, stat_bf16=False, dx_add=add, dgamma_prev=pg, dbeta_prev=pb)
    assert close(bw["dx"], add.double() + xf.grad.permute(0, 2, 1))
    assert close(bw["dgamma"], pg.double() + gf.grad) and close(bw["dbeta"], pb.double() + bf_.grad)


@pytest.mark.parametrize("M,C", [(5, 64), (3, 520), (1, 8)])
def test_layernorm_reference_equals_float64_autograd(M, C):
    x, gamma, beta, dy = R.ln_inputs(M, C, seed=M + C)
    add = R.small_bf16((M, C), 4)
    xf = x.double().requires_grad_(True)
    gf, bf_ = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.layer_norm(xf, (C,), gf, bf_, 1e-5)
    y.backward(dy.double())
    fw = R.ln_fwd_ref(x, gamma, beta, 1e-5)
    assert close(fw["y"], y.detach())
    bw = R.ln_bwd_ref(x, gamma, torch.stack([fw["mean"], fw["rstd"]], -1), dy, stat_bf16=False, dx_add=add)
    assert close(bw["dx"], add.double() + xf.grad)
    assert close(bw["dgamma"], gf.grad) and close(bw["dbeta"], bf_.grad)


# ---------------- NORM_STAT_BF16 = 1: a hand-rounded restatement -------------------------------------------------------------
def test_groupnorm_rounded_statistics_follow_a_hand_rounded_restatement():
    """Group by group, in loops: SiLU' at the fp32 statistics, the rest with the bf16-rounded pair."""
    B, HW, C, G, eps = 2, 23, 48, 4, 1e-5
    x, gamma, beta, dy = R.gn_inputs(B, HW, C, G, seed=5)
    st32 = fp32_stats(R.gn_fwd_ref(x, gamma, beta, G, eps, True))
    bw = R.gn_bwd_ref(x, gamma, beta, st32, dy, G, True, stat_bf16=True)
    cpg = C // G
    dx = torch.empty(B, HW, C, dtype=torch.float64)
    dg, db = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for b in range(B):
        for g in range(G):
            cs = slice(g * cpg, (g + 1) * cpg)
            m32, r32 = float(st32[b, g, 0]), float(st32[b, g, 1])
            m = float(torch.tensor(m32).bfloat16())
            r = float(torch.tensor(r32).bfloat16())
            xs, ga, be, d = x[b, :, cs].double(), gamma[cs].double(), beta[cs].double(), dy[b, :, cs].double()
            z = (xs - m32) * r32 * ga + be
            dz = d * torch.autograd.functional.jacobian(lambda t: F.silu(t).sum(), z)      # SiLU' by autograd, elementwise
            xh = (xs - m) * r
            dz_g = dz * ga
            dx[b, :, cs] = r * (dz_g - dz_g.mean() - xh * (dz_g * xh).mean())
            dg[cs] += (dz * xh).sum(0)
            db[cs] += dz.sum(0)
    assert close(bw["dx"], dx, 1e-11) and close(bw["dgamma"], dg, 1e-11) and close(bw["dbeta"], db, 1e-11)
    # and it is not the unrounded one
    assert not close(R.gn_bwd_ref(x, gamma, beta, st32, dy, G, True, stat_bf16=False)["dx"], dx, 1e-6)


def test_layernorm_rounded_statistics_follow_a_hand_rounded_restatement():
    M, C = 6, 40
    x, gamma, beta, dy = R.ln_inputs(M, C, seed=6)
    fw = R.ln_fwd_ref(x, gamma, beta, 1e-5)
    saved = torch.stack([fw["mean"], fw["rstd"]], -1).float().bfloat16().float()       # what the forward saves with the option on
    bw = R.ln_bwd_ref(x, gamma, saved, dy, stat_bf16=True)
    for i in range(M):
        m, r = float(saved[i, 0]), float(saved[i, 1])
        xh = (x[i].double() - m) * r
        g = dy[i].double() * gamma.double()
        assert close(bw["dx"][i], r * (g - g.mean() - xh * (g * xh).mean()), 1e-11)
    assert close(bw["dgamma"], sum(dy[i].double() * (x[i].double() - float(saved[i, 0])) * float(saved[i, 1]) for i in range(M)), 1e-11)


# ---------------- tightness: the bounds reject the errors the GPU tests look for -----------------------------------------------
_CACHE = {}


def gn_case(B, HW, C, G, silu, eps, stat_bf16, seed):
    key = (B, HW, C, G, silu, eps, stat_bf16, seed)
    if key not in _CACHE:
        x, gamma, beta, dy = R.gn_inputs(B, HW, C, G, seed, edges=HW >= 4096)
        fw = R.gn_fwd_ref(x, gamma, beta, G, eps, silu)
        st = fp32_stats(fw)
        bw = R.gn_bwd_ref(x, gamma, beta, st, dy, G, silu, stat_bf16)
        _CACHE[key] = (x, gamma, beta, dy, fw, st, bw)
    return _CACHE[key]


# the 896^2 level (ragged last row chunk), and the 128^2 level's conv_norm_out (cpg 10: groups straddle 8-channel chunks, SiLU)
GN_TIGHT = [(1, 12544, 640, 32, False, 1e-5), (1, 16384, 320, 32, True, 1e-5)]


@pytest.mark.parametrize("stat_bf16", [0, 1])
@pytest.mark.parametrize("case", GN_TIGHT, ids=lambda c: f"B{c[0]}_HW{c[1]}_C{c[2]}_G{c[3]}_silu{int(c[4])}")
def test_groupnorm_bounds_accept_the_rounded_result_and_reject_kernel_errors(case, stat_bf16):
    B, HW, C, G, silu, eps = case
    x, gamma, beta, dy, fw, st, bw = gn_case(*case, stat_bf16, seed=11)
    cpg = C // G
    # the correctly rounded result is accepted (with K = 0 even: nothing but one rounding)
    assert within(rounded(fw["y"]), fw["y"], fw["S_y"], "gn_y")
    for q in ("dx", "dgamma", "dbeta"):
        assert within(rounded(bw[q]), bw[q], bw["S_" + q], "gn_dx" if q == "dx" else "gn_dparam"), q

    def rejected(fake, q):
        k = "gn_dx" if q == "dx" else "gn_dparam"
        return not within(rounded(fake[q]), bw[q], bw["S_" + q], k)

    stc = st.double().repeat_interleave(cpg, dim=1)               # [B][C][2] per channel
    # (1) rstd scaled by (1 + 2^-9) in one group: forward and backward
    g1 = 7
    y_bad = fw["y"].clone()
    z = (x[..., g1 * cpg:(g1 + 1) * cpg].double() - fw["mean"][:, g1, None, None]) * (fw["rstd"][:, g1, None, None] * (1 + 2 ** -9)) \
        * gamma[g1 * cpg:(g1 + 1) * cpg].double() + beta[g1 * cpg:(g1 + 1) * cpg].double()
    y_bad[..., g1 * cpg:(g1 + 1) * cpg] = z * torch.sigmoid(z) if silu else z
    assert not within(rounded(y_bad), fw["y"], fw["S_y"], "gn_y"), "rstd * (1 + 2^-9) in one group passes the forward bound"
    scale = torch.ones(C, dtype=torch.float64)
    scale[g1 * cpg:(g1 + 1) * cpg] = 1 + 2 ** -9
    assert rejected(R.gn_bwd_ref_chan(x, gamma, beta, stc, dy, G, silu, stat_bf16, r_scale=scale), "dx"), "rstd * (1 + 2^-9): backward"
    # (2) the statistics rounding left out (or put in where it does not belong)
    assert rejected(R.gn_bwd_ref(x, gamma, beta, st, dy, G, silu, not stat_bf16), "dx"), "stat rounding toggled: dx"
    # (3) one channel read with its neighbour group's statistics: the last channel of a group that an 8-channel chunk straddles
    c = next(cc for cc in range(cpg - 1, C, cpg) if (cc + 1) % 8)
    s_bad = stc.clone()
    s_bad[:, c] = stc[:, c + 1]
    assert rejected(R.gn_bwd_ref_chan(x, gamma, beta, s_bad, dy, G, silu, stat_bf16), "dx"), f"channel {c} with group {c // cpg + 1}'s stats"
    g_c = c // cpg
    y_bad = fw["y"].clone()
    z = (x[..., c].double() - fw["mean"][:, g_c + 1, None]) * fw["rstd"][:, g_c + 1, None] * float(gamma[c]) + float(beta[c])
    y_bad[..., c] = z * torch.sigmoid(z) if silu else z
    assert not within(rounded(y_bad), fw["y"], fw["S_y"], "gn_y"), "neighbour statistics pass the forward bound"
    # (4) the last row chunk of the backward's partial sums left out of k1 / k2
    rpc = R.gn_rows_per_chunk(HW, C, 32)          # GN_RPT_BWD's default
    last = (HW - 1) // rpc * rpc
    fake = R.gn_bwd_ref_chan(x, gamma, beta, stc, dy, G, silu, stat_bf16, k_rows=slice(0, last))
    assert rejected(fake, "dx"), f"rows {last}..{HW} dropped from k1 / k2"


def test_groupnorm_parameter_gradient_bound_rejects_a_missing_sample():
    case = (2, 4096, 640, 32, False, 1e-6)
    x, gamma, beta, dy, fw, st, bw = gn_case(*case, 1, seed=12)
    one = R.gn_bwd_ref(x[:1], gamma, beta, st[:1], dy[:1], 32, False, 1)
    for q in ("dgamma", "dbeta"):
        assert within(rounded(bw[q]), bw[q], bw["S_" + q], "gn_dparam")
        assert not within(rounded(one[q]), bw[q], bw["S_" + q], "gn_dparam"), q


@pytest.mark.parametrize("stat_bf16", [0, 1])
def test_layernorm_bounds_accept_the_rounded_result_and_reject_kernel_errors(stat_bf16):
    M, C = 4096, 1280
    x, gamma, beta, dy = R.ln_inputs(M, C, seed=13)
    fw = R.ln_fwd_ref(x, gamma, beta, 1e-5)
    st32 = torch.stack([fw["mean"], fw["rstd"]], -1).float()
    saved = st32.bfloat16().float() if stat_bf16 else st32
    bw = R.ln_bwd_ref(x, gamma, saved, dy, stat_bf16)
    assert within(rounded(fw["y"]), fw["y"], fw["S_y"], "ln_y")
    for q in ("dx", "dgamma", "dbeta"):
        assert within(rounded(bw[q]), bw[q], bw["S_" + q], "ln_dx" if q == "dx" else "ln_dparam"), q
    # rstd * (1 + 2^-9) in one row
    bad = saved.clone()
    bad[100, 1] *= 1 + 2 ** -9
    assert not within(rounded(R.ln_bwd_ref(x, gamma, bad, dy, False)["dx"]), bw["dx"], bw["S_dx"], "ln_dx")
    y_bad = fw["y"].clone()
    y_bad[100] = (x[100].double() - fw["mean"][100]) * fw["rstd"][100] * (1 + 2 ** -9) * gamma.double() + beta.double()
    assert not within(rounded(y_bad), fw["y"], fw["S_y"], "ln_y")
    # the statistics rounding left out / put in
    other = st32 if stat_bf16 else st32.bfloat16().float()
    assert not within(rounded(R.ln_bwd_ref(x, gamma, other, dy, False)["dx"]), bw["dx"], bw["S_dx"], "ln_dx")
    # a row's terms missing from the parameter gradients
    part = R.ln_bwd_ref(x[1:], gamma, saved[1:], dy[1:], stat_bf16)
    for q in ("dgamma", "dbeta"):
        assert not within(rounded(part[q]), bw[q], bw["S_" + q], "ln_dparam"), q


@pytest.mark.parametrize("stat_bf16", [0, 1])
def test_layernorm_statistics_bounds_reject_a_2_to_minus_12_error(stat_bf16):
    """The statistics the LayerNorm forward saves: fp32 (one fp32 rounding of slack) or bf16 (one bf16 rounding)."""
    M, C = 4096, 1280
    x, gamma, beta, dy = R.ln_inputs(M, C, seed=13)
    fw = R.ln_fwd_ref(x, gamma, beta, 1e-5)
    st = torch.stack([fw["mean"], fw["rstd"]], -1).float()
    if stat_bf16:
        st = st.bfloat16().float()
        mean_ok = lambda m: within(m, fw["mean"], fw["S_mean"], "ln_mean")             # noqa: E731
        rstd_ok = lambda r: within(r, fw["rstd"], fw["S_rstd"], "ln_var")              # noqa: E731
        scale = 2 ** -7            # below a bf16 step a scaled saved value is no kernel error: it is still the rounded one
    else:
        mean_ok = lambda m: within(m, fw["mean"], fw["S_mean"], "ln_mean", fw["R_mean"])                              # noqa: E731
        rstd_ok = lambda r: within(R.var_from_rstd(r, 1e-5), fw["var"], fw["S_var"], "ln_var", fw["R_var"])       # noqa: E731
        scale = 2 ** -12
    assert mean_ok(st[:, 0]) and rstd_ok(st[:, 1])
    for k in (0, 1):
        bad = st.clone()
        bad[100, k] *= 1 + scale
        assert not (mean_ok(bad[:, 0]) and rstd_ok(bad[:, 1])), (k, scale)


def test_groupnorm_statistics_bounds_are_fp32_tight():
    """The GroupNorm forward writes fp32 statistics: the bounds allow one fp32 rounding plus K 2^-24 (mean^2 + var) and no bf16
    slack.  A (1 + 2^-12) error in the mean is rejected in every group (the large-offset and the constant one included), in the
    rstd of an ordinary group too.  In the large-offset group (mean^2 / var ~ 1.4e4) the stated variance bound K 2^-24 (mean^2 +
    var) is what a one-pass fp32 variance may legitimately miss by, ~2^-11 of rstd: there a 2^-9 rstd error is rejected."""
    B, HW, C, G, silu, eps = 1, 16384, 320, 32, True, 1e-5
    x, gamma, beta, dy = R.gn_inputs(B, HW, C, G, seed=11, edges=True)
    fw = R.gn_fwd_ref(x, gamma, beta, G, eps, silu)
    st = fp32_stats(fw)

    def ok(s):
        return (within(s[..., 0], fw["mean"], fw["S_mean"], "gn_mean", fw["R_mean"])
                and within(R.var_from_rstd(s[..., 1], eps), fw["var"], fw["S_var"], "gn_var", fw["R_var"]))

    assert ok(st), "correctly rounded fp32 statistics rejected"
    assert float(fw["var"][0, 5]) == 0.0 and float(fw["mean"][0, 3]) > 5.5       # the constant and the large-offset group
    for g in (0, 3, 5, 17):
        bad = st.clone()
        bad[0, g, 0] *= 1 + 2 ** -12
        assert not ok(bad), f"mean * (1 + 2^-12) in group {g}"
    for g, scale in ((0, 2 ** -12), (17, 2 ** -12), (3, 2 ** -9)):
        bad = st.clone()
        bad[0, g, 1] *= 1 + scale
        assert not ok(bad), f"rstd * (1 + {scale}) in group {g}"


def test_rows_per_chunk_restatement_at_known_geometries():
    """gn_rows_per_chunk against chunk sizes worked out by hand from gn_geom in az_norm.hip."""
    assert R.gn_rows_per_chunk(16384, 320, 4) == 24 and R.gn_rows_per_chunk(12544, 640, 32) == 96
    assert R.gn_rows_per_chunk(1, 320, 4) == 24 and R.gn_rows_per_chunk(16, 4096, 4) == 4
