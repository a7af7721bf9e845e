"""GroupNorm / LayerNorm kernels (csrc/az_norm.hip) against the float64 restatement of their semantics (tests/norm_ref.py), element by
element within condition-aware bounds, at the model's shapes and at the geometry edges of the kernels: ragged last row chunks,
groups that an 8-channel chunk straddles, groups narrower than a chunk, blocks with fewer threads than groups, the widest rows
gn_check allows, LayerNorm's lane groups and its rows-per-block growth.  Every call form the executor issues, both NORM_STAT_BF16
values, the chunking options and their clamping, strided views, batch independence and the scratch sizes are covered; where two
forms share their arithmetic the results are compared bit for bit.

AZ_NORM_K_REPORT=<file>: write the largest K each quantity needed (norm_ref.excess) as JSON at the end of the module."""
import contextlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import norm_ref as R        # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -1234.5            # sentinel of scratch tails and padding columns (exact in bf16 and fp32)
TAIL = 1024


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd import ops as _ops
    return _ops


OBSERVED = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("AZ_NORM_K_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(OBSERVED, f, indent=1, sort_keys=True)


def within(out, ref, S, k, what, rounding=None):
    """out (device, any dtype) against ref / S (device float64) under norm_ref's bound for quantity k; `rounding`: the allowance of
    the stored format (default one bf16 rounding; the fp32 statistics pass their own)."""
    assert out.shape == ref.shape, (what, tuple(out.shape), tuple(ref.shape))
    o = out.double()
    assert torch.isfinite(o).all(), f"{what}: non-finite output"
    OBSERVED[k] = max(OBSERVED.get(k, 0.0), R.excess(o, ref, S, rounding))
    err = (o - ref).abs()
    b = R.bound(ref, S, k, rounding)
    bad = err > b
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at flat {i}: "
                             f"out={float(o.reshape(-1)[i]):.7g} ref={float(ref.reshape(-1)[i]):.7g} err={float(err.reshape(-1)[i]):.3g} "
                             f"bound={float(b.reshape(-1)[i]):.3g}; K needed {R.excess(o, ref, S, rounding):.1f} > {R.K[k]}")


def same(a, b, what):
    assert torch.equal(a, b), f"{what}: not bit-identical (max |diff| {float((a.double() - b.double()).abs().max()):.3g})"


@contextlib.contextmanager
def options(**kw):
    from aozora_sdxl_training_amd._lib import set_option, get_option
    old = {k: get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            set_option(k, v)


def dev(d):
    return {k: v.to(DEV) for k, v in d.items() if torch.is_tensor(v)}


# ---------------- GroupNorm ----------------------------------------------------------------------------------------------------
GN_CASES = [
    (1, 16384, 320, 32, True, 1e-5),      # 128^2: down 0, conv_norm_out -- cpg 10 straddles 8-channel chunks
    (1, 16384, 960, 32, True, 1e-5),      # up 2 norm1: cpg 30
    (2, 4096, 640, 32, False, 1e-6),      # transformer norm
    (1, 4096, 1920, 32, True, 1e-5),      # up 1: py = 1
    (2, 1024, 2560, 32, True, 1e-5),      # up 0: cpg 80
    (1, 12544, 640, 32, False, 1e-5),     # the 896^2 level: ragged last row chunk
    (3, 1, 320, 32, True, 1e-5),          # HW below one chunk
    (2, 9, 1280, 32, True, 1e-5),
    (2, 100, 24, 3, True, 1e-5),          # cpg 8 exactly, C / 8 = 3
    (1, 16, 4096, 1024, True, 1e-5),      # cpg 4 < 8; fewer threads than groups (the tiny-block loop of gn_partial_kernel)
    (1, 64, 8192, 64, False, 1e-5),       # gn_check's limits: C / 8 = 1024, cpg 128
]
GN_IDS = [f"B{c[0]}_HW{c[1]}_C{c[2]}_G{c[3]}{'_silu' if c[4] else ''}" for c in GN_CASES]


def gn_data(ops, case):
    """Inputs on the device and the kernel's forward at the default options."""
    B, HW, C, G, silu, eps = case
    x, gamma, beta, dy = R.gn_inputs(B, HW, C, G, seed=HW + C + G, edges=HW >= 4096)
    add = R.small_bf16((B, HW, C), seed=C + 1)
    pg, pb = R.small_bf16((C,), seed=C + 2), R.small_bf16((C,), seed=C + 3)
    d = dict(x=x.to(DEV), gamma=gamma.to(DEV), beta=beta.to(DEV), dy=dy.to(DEV), add=add.to(DEV), pg=pg.to(DEV), pb=pb.to(DEV),
             cpu=(x, gamma, beta, dy))
    d["y"] = torch.empty(B, HW, C, dtype=torch.bfloat16, device=DEV)
    d["stats"] = torch.empty(B * G * 2, dtype=torch.float32, device=DEV)
    ops.groupnorm_fwd(d["x"], d["gamma"], d["beta"], d["y"], d["stats"], G, eps, silu)
    return d


@pytest.fixture(scope="module", params=GN_CASES, ids=GN_IDS)
def gn(request, ops):
    """(case, data): the forward reference and the backward references built on the kernel's fp32 statistics (NORM_STAT_BF16 = 0
    and 1), computed once per case -- the module-scoped parameter keeps one case's tests together."""
    case = request.param
    B, HW, C, G, silu, eps = case
    d = gn_data(ops, case)
    x, gamma, beta, dy = d.pop("cpu")
    d["fwd"] = dev(R.gn_fwd_ref(x, gamma, beta, G, eps, silu))
    st = d["stats"].cpu().reshape(B, G, 2)
    d["bwd"] = {on: dev(R.gn_bwd_ref(x, gamma, beta, st, dy, G, silu, on)) for on in (0, 1)}
    return case, d


def check_gn_forward(d, case, y, stats, what):
    B, HW, C, G, silu, eps = case
    f = d["fwd"]
    within(y, f["y"], f["S_y"], "gn_y", what + " y")
    st = stats.reshape(B, G, 2)
    # fp32 statistics: one fp32 rounding each, no bf16 slack; the variance is the one the fp32 rstd stands for
    within(st[..., 0], f["mean"], f["S_mean"], "gn_mean", what + " mean", rounding=f["R_mean"])
    within(R.var_from_rstd(st[..., 1], eps), f["var"], f["S_var"], "gn_var", what + " var", rounding=f["R_var"])


def gn_fwd_private(ops, d, case):
    """az_groupnorm_fwd with a private scratch buffer of exactly az_gn_scratch_floats floats and a sentinel tail."""
    from aozora_sdxl_training_amd._lib import lib
    B, HW, C, G, silu, eps = case
    n = ops.gn_scratch_floats(B, HW, C, G)
    buf = torch.full((n + TAIL,), SENT, dtype=torch.float32, device=DEV)
    y = torch.empty(B, HW, C, dtype=torch.bfloat16, device=DEV)
    stats = torch.empty(B * G * 2, dtype=torch.float32, device=DEV)
    x = d["x"]
    lib().call("az_groupnorm_fwd", B, HW, C, G, float(eps), int(silu), ops._ptr(x), x.stride(1), ops._ptr(d["gamma"]),
               ops._ptr(d["beta"]), ops._ptr(y), y.stride(1), ops._ptr(stats), ops._ptr(buf), ops._stream())
    assert bool((buf[n:] == SENT).all()), "az_groupnorm_fwd wrote past az_gn_scratch_floats"
    return y, stats


def gn_bwd_private(ops, d, case, stats, dx_add=True, params=True):
    """az_groupnorm_bwd_ex with a private scratch buffer and a sentinel tail; dx = add + gradient, dgamma / dbeta from prev."""
    from aozora_sdxl_training_amd._lib import lib
    B, HW, C, G, silu, eps = case
    n = ops.gn_scratch_floats(B, HW, C, G)
    buf = torch.full((n + TAIL,), SENT, dtype=torch.float32, device=DEV)
    dx = torch.full((B, HW, C), 3.0, dtype=torch.bfloat16, device=DEV)
    dg, db = (d["pg"].clone(), d["pb"].clone()) if params else (None, None)
    x, dy, add = d["x"], d["dy"], d["add"] if dx_add else None
    lib().call("az_groupnorm_bwd_ex", B, HW, C, G, int(silu), ops._ptr(x), x.stride(1), ops._ptr(d["gamma"]), ops._ptr(d["beta"]),
               ops._ptr(stats), ops._ptr(dy), dy.stride(1), ops._ptr(dx), dx.stride(1), ops._ptr(add), add.stride(1) if add is not None else 0,
               ops._ptr(dg), ops._ptr(db), ops._ptr(buf), ops._stream())
    assert bool((buf[n:] == SENT).all()), "az_groupnorm_bwd_ex wrote past az_gn_scratch_floats"
    return dx, dg, db


def test_groupnorm_forward_within_float64_bounds_under_every_chunking(ops, gn):
    case, d = gn
    check_gn_forward(d, case, d["y"], d["stats"], "gn_fwd")
    outs = {}
    for rpt in (0, 1, 4, 16, 64, 1000):
        with options(GN_RPT=rpt):
            outs[rpt] = gn_fwd_private(ops, d, case)
        if rpt in (4, 16, 64):
            check_gn_forward(d, case, *outs[rpt], f"gn_fwd GN_RPT={rpt}")
    same(outs[4][0], d["y"], "private scratch vs ops y"); same(outs[4][1], d["stats"], "private scratch vs ops stats")
    for lo, eq in ((0, 4), (1, 4), (1000, 64)):         # out-of-range values clamp to [4, 64]
        same(outs[lo][0], outs[eq][0], f"GN_RPT={lo} vs {eq} y"); same(outs[lo][1], outs[eq][1], f"GN_RPT={lo} vs {eq} stats")


@pytest.mark.parametrize("stat_bf16", [0, 1])
def test_groupnorm_backward_every_call_form_within_float64_bounds(ops, gn, stat_bf16):
    """Every call form against the reference of this NORM_STAT_BF16 value, then -- under the same value -- the GN_RPT_BWD /
    GN_RPT_APPLY sweeps with their clamping, each call with a private scratch buffer and a sentinel tail."""
    case, d = gn
    B, HW, C, G, silu, eps = case
    r = d["bwd"][stat_bf16]
    x, gm, bt, st, dy, add = d["x"], d["gamma"], d["beta"], d["stats"], d["dy"], d["add"]
    with options(NORM_STAT_BF16=stat_bf16):
        # (dx, dgamma, dbeta): the executor's data-gradient chain, parameter gradients on top of previous values
        dx = torch.full_like(x, 3.0)
        dg, db = d["pg"].clone(), d["pb"].clone()
        ops.groupnorm_bwd(x, gm, bt, st, dy, dx, dg, db, G, silu)
        within(dx, r["dx"], r["S_dx"], "gn_dx", "dx")
        within(dg, r["dgamma"] + d["pg"].double(), r["S_dgamma"] + d["pg"].double().abs(), "gn_dparam", "dgamma")
        within(db, r["dbeta"] + d["pb"].double(), r["S_dbeta"] + d["pb"].double().abs(), "gn_dparam", "dbeta")
        # (dx only): the same dx
        dx1 = torch.full_like(x, 3.0)
        ops.groupnorm_bwd(x, gm, bt, st, dy, dx1, None, None, G, silu)
        same(dx1, dx, "dx without parameter gradients")
        # (dgamma, dbeta only): gn_bwd_param_kernel, the apply kernel's arithmetic
        dg2, db2 = d["pg"].clone(), d["pb"].clone()
        ops.groupnorm_bwd(x, gm, bt, st, dy, None, dg2, db2, G, silu)
        same(dg2, dg, "param-only dgamma"); same(db2, db, "param-only dbeta")
        # (dgamma only), with and without a data gradient
        dg3 = d["pg"].clone()
        ops.groupnorm_bwd(x, gm, bt, st, dy, None, dg3, None, G, silu)
        same(dg3, dg, "dgamma-only (param kernel)")
        dg4, dx4 = d["pg"].clone(), torch.full_like(x, 3.0)
        ops.groupnorm_bwd(x, gm, bt, st, dy, dx4, dg4, None, G, silu)
        same(dg4, dg, "dgamma-only (apply kernel)"); same(dx4, dx, "dx beside dgamma only")
        # dx_add in place and out of place
        dx5, dg5, db5 = add.clone(), d["pg"].clone(), d["pb"].clone()
        ops.groupnorm_bwd(x, gm, bt, st, dy, dx5, dg5, db5, G, silu, accumulate_dx=True)
        within(dx5, r["dx"] + add.double(), r["S_dx"] + add.double().abs(), "gn_dx", "dx += gradient")
        same(dg5, dg, "dgamma beside dx_add")
        src = add.clone()
        dx6 = torch.full_like(x, 3.0)
        ops.groupnorm_bwd(x, gm, bt, st, dy, dx6, None, None, G, silu, dx_add=src)
        same(dx6, dx5, "dx = dx_add + gradient out of place"); same(src, add, "dx_add source")
        # chunking of the partial sums (GN_RPT_BWD): within bounds; of the element-wise pass (GN_RPT_APPLY): bitwise neutral;
        # out-of-range values clamp.  Every call with a private scratch buffer of exactly az_gn_scratch_floats floats.
        ref_dx, ref_S = r["dx"] + add.double(), r["S_dx"] + add.double().abs()
        got = {}
        for rb in (0, 1, 4, 32, 64, 1000):
            with options(GN_RPT_BWD=rb):
                got[rb] = gn_bwd_private(ops, d, case, st)
            if rb in (4, 32, 64):
                dxo, dgo, dbo = got[rb]
                within(dxo, ref_dx, ref_S, "gn_dx", f"dx GN_RPT_BWD={rb}")
                within(dgo, r["dgamma"] + d["pg"].double(), r["S_dgamma"] + d["pg"].double().abs(), "gn_dparam", f"dgamma GN_RPT_BWD={rb}")
                within(dbo, r["dbeta"] + d["pb"].double(), r["S_dbeta"] + d["pb"].double().abs(), "gn_dparam", f"dbeta GN_RPT_BWD={rb}")
        for lo, eq in ((0, 4), (1, 4), (1000, 64)):
            for k, q in enumerate(("dx", "dgamma", "dbeta")):
                same(got[lo][k], got[eq][k], f"GN_RPT_BWD={lo} vs {eq} {q}")
        app = {}
        for ra in (0, 1, 4, 32, 64, 1000):
            with options(GN_RPT_APPLY=ra):
                app[ra] = gn_bwd_private(ops, d, case, st)
        for ra in (0, 1, 4, 64, 1000):
            for k, q in enumerate(("dx", "dgamma", "dbeta")):
                same(app[ra][k], app[32][k], f"GN_RPT_APPLY={ra} vs 32 {q}")
        same(app[32][0], dx5, "private scratch vs ops dx")


@pytest.mark.parametrize("case", GN_CASES, ids=GN_IDS)
def test_groupnorm_strided_views_equal_the_contiguous_run(ops, case):
    """unet.py hands the norms row-strided views (slices of concat buffers): x / dy / dx / dx_add with row strides C + 8 and C + 64
    give the contiguous run's bits, and the padding columns stay untouched."""
    B, HW, C, G, silu, eps = case
    d = gn_data(ops, case)

    def padded(pad, fill=None):
        buf = torch.full((B, HW, C + pad), SENT, dtype=torch.bfloat16, device=DEV)
        if fill is not None:
            buf[..., :C] = fill
        return buf, buf[..., :C]

    xb, xv = padded(8, d["x"])
    yb, yv = padded(64)
    stats = torch.empty(B * G * 2, dtype=torch.float32, device=DEV)
    ops.groupnorm_fwd(xv, d["gamma"], d["beta"], yv, stats, G, eps, silu)
    same(yv, d["y"], "strided y"); same(stats, d["stats"], "strided stats")
    assert bool((yb[..., C:] == SENT).all()) and bool((xb[..., C:] == SENT).all()), "padding columns written"
    dyb, dyv = padded(64, d["dy"])
    ab, av = padded(64, d["add"])
    dxb, dxv = padded(8)
    dg, db = d["pg"].clone(), d["pb"].clone()
    ops.groupnorm_bwd(xv, d["gamma"], d["beta"], stats, dyv, dxv, dg, db, G, silu, dx_add=av)
    dx, dg1, db1 = d["add"].clone(), d["pg"].clone(), d["pb"].clone()
    ops.groupnorm_bwd(d["x"], d["gamma"], d["beta"], stats, d["dy"], dx, dg1, db1, G, silu, accumulate_dx=True)
    same(dxv, dx, "strided dx"); same(dg, dg1, "strided dgamma"); same(db, db1, "strided dbeta")
    assert bool((dxb[..., C:] == SENT).all()), "dx padding written"
    same(av, d["add"], "strided dx_add source")
    assert bool((ab[..., C:] == SENT).all()) and bool((dyb[..., C:] == SENT).all())
    # in place through a strided view: dx_add is dx itself
    dxb2, dxv2 = padded(64, d["add"])
    ops.groupnorm_bwd(xv, d["gamma"], d["beta"], stats, dyv, dxv2, None, None, G, silu, accumulate_dx=True)
    same(dxv2, dx, "strided in-place dx"); assert bool((dxb2[..., C:] == SENT).all())


@pytest.mark.parametrize("case", [c for c in GN_CASES if c[0] > 1], ids=[i for c, i in zip(GN_CASES, GN_IDS) if c[0] > 1])
def test_groupnorm_samples_are_independent_of_the_batch(ops, case):
    """The row chunking depends on HW only: sample b of a batch gives the bits of a batch of one."""
    B, HW, C, G, silu, eps = case
    d = gn_data(ops, case)
    dx = torch.empty_like(d["x"])
    ops.groupnorm_bwd(d["x"], d["gamma"], d["beta"], d["stats"], d["dy"], dx, None, None, G, silu)
    for b in range(B):
        xb, dyb = d["x"][b:b + 1].clone(), d["dy"][b:b + 1].clone()
        y1 = torch.empty_like(xb)
        s1 = torch.empty(G * 2, dtype=torch.float32, device=DEV)
        ops.groupnorm_fwd(xb, d["gamma"], d["beta"], y1, s1, G, eps, silu)
        same(y1, d["y"][b:b + 1], f"y of sample {b}"); same(s1, d["stats"].reshape(B, -1)[b], f"stats of sample {b}")
        dx1 = torch.empty_like(xb)
        ops.groupnorm_bwd(xb, d["gamma"], d["beta"], s1, dyb, dx1, None, None, G, silu)
        same(dx1, dx[b:b + 1], f"dx of sample {b}")


# ---------------- LayerNorm ----------------------------------------------------------------------------------------------------
LN_CASES = [(16384, 640), (4096, 1280), (77, 2048), (3, 520), (1, 8), (36000, 640)]      # last: rows > 1024 x LN_RPB's default


@pytest.fixture(scope="module", params=LN_CASES, ids=[f"M{m}_C{c}" for m, c in LN_CASES])
def ln(request, ops):
    """(case, data): inputs, the kernel's forward under both NORM_STAT_BF16 values and the backward references on what it saved."""
    case = request.param
    M, C = case
    x, gamma, beta, dy = R.ln_inputs(M, C, seed=M + C)
    add = R.small_bf16((M, C), seed=C + 5)
    pg, pb = R.small_bf16((C,), seed=C + 6), R.small_bf16((C,), seed=C + 7)
    d = dict(x=x.to(DEV), gamma=gamma.to(DEV), beta=beta.to(DEV), dy=dy.to(DEV), add=add.to(DEV), pg=pg.to(DEV), pb=pb.to(DEV))
    d["fwd"] = dev(R.ln_fwd_ref(x, gamma, beta, 1e-5))
    for on in (0, 1):
        y = torch.empty(M, C, dtype=torch.bfloat16, device=DEV)
        st = torch.empty(2 * M, dtype=torch.float32, device=DEV)
        with options(NORM_STAT_BF16=on):
            ops.layernorm_fwd(d["x"], d["gamma"], d["beta"], y, st)
        d[("y", on)], d[("stats", on)] = y, st
        d[("bwd", on)] = dev(R.ln_bwd_ref(x, gamma, st.cpu().reshape(M, 2), dy, on))
    return case, d


@pytest.mark.parametrize("stat_bf16", [0, 1])
def test_layernorm_within_float64_bounds_and_every_form_agrees(ops, ln, stat_bf16):
    (M, C), d = ln
    f, r = d["fwd"], d[("bwd", stat_bf16)]
    x, gm, dy, add = d["x"], d["gamma"], d["dy"], d["add"]
    st = d[("stats", stat_bf16)]
    within(d[("y", stat_bf16)], f["y"], f["S_y"], "ln_y", "ln y")
    sm, sr = st.reshape(M, 2)[:, 0], st.reshape(M, 2)[:, 1]
    if stat_bf16:          # saved as bf16 values: one rounding on top of the fp32 statistics
        assert torch.equal(st, st.bfloat16().float()), "saved statistics are not bf16 values"
        within(sm, f["mean"], f["S_mean"], "ln_mean", "ln saved mean")
        within(sr, f["rstd"], f["S_rstd"], "ln_var", "ln saved rstd")
    else:                  # fp32: one fp32 rounding each
        within(sm, f["mean"], f["S_mean"], "ln_mean", "ln mean", rounding=f["R_mean"])
        within(R.var_from_rstd(sr, 1e-5), f["var"], f["S_var"], "ln_var", "ln var", rounding=f["R_var"])
    pgd, pbd = d["pg"].double(), d["pb"].double()
    with options(NORM_STAT_BF16=stat_bf16):
        # fused: dx + parameter gradients in one pass
        dx = torch.full_like(x, 3.0)
        dg, db = d["pg"].clone(), d["pb"].clone()
        ops.layernorm_bwd(x, gm, st, dy, dx, dg, db)
        within(dx, r["dx"], r["S_dx"], "ln_dx", "ln dx")
        within(dg, r["dgamma"] + pgd, r["S_dgamma"] + pgd.abs(), "ln_dparam", "ln dgamma")
        within(db, r["dbeta"] + pbd, r["S_dbeta"] + pbd.abs(), "ln_dparam", "ln dbeta")
        # split forms
        dx1 = torch.full_like(x, 3.0)
        ops.layernorm_bwd(x, gm, st, dy, dx1, None, None)
        same(dx1, dx, "dx-only form")
        dg1, db1 = d["pg"].clone(), d["pb"].clone()
        ops.layernorm_bwd(x, gm, st, dy, None, dg1, db1)
        within(dg1, r["dgamma"] + pgd, r["S_dgamma"] + pgd.abs(), "ln_dparam", "ln dgamma (param-only)")
        within(db1, r["dbeta"] + pbd, r["S_dbeta"] + pbd.abs(), "ln_dparam", "ln dbeta (param-only)")
        # dx_add out of place
        dx2 = torch.full_like(x, 3.0)
        ops.layernorm_bwd(x, gm, st, dy, dx2, None, None, dx_add=add)
        within(dx2, r["dx"] + add.double(), r["S_dx"] + add.double().abs(), "ln_dx", "ln dx = dx_add + gradient")
        # every LN_RPB (growth past 1024 blocks included): fused and parked partial sums + ln_param_finish_multi
        for rpb in (4, 32, 101, 1000):
            with options(LN_RPB=rpb):
                dx3 = torch.full_like(x, 3.0)
                dg3, db3 = d["pg"].clone(), d["pb"].clone()
                ops.layernorm_bwd(x, gm, st, dy, dx3, dg3, db3)
                same(dx3, dx, f"fused dx LN_RPB={rpb}")
                within(dg3, r["dgamma"] + pgd, r["S_dgamma"] + pgd.abs(), "ln_dparam", f"ln dgamma LN_RPB={rpb}")
                within(db3, r["dbeta"] + pbd, r["S_dbeta"] + pbd.abs(), "ln_dparam", f"ln dbeta LN_RPB={rpb}")
                nblk = ops.ln_partial_blocks(M)
                assert 1 <= nblk <= 1024 and nblk * ((M + nblk - 1) // nblk) >= M
                part = torch.full((nblk * C * 2 + TAIL,), SENT, dtype=torch.float32, device=DEV)
                dx4 = torch.full_like(x, 3.0)
                ops.layernorm_bwd_partial(x, gm, st, dy, dx4, part[:nblk * C * 2])
                assert bool((part[nblk * C * 2:] == SENT).all()), "partial sums written past nblk * C * 2"
                same(dx4, dx, f"partial-form dx LN_RPB={rpb}")
                dg4, db4 = d["pg"].clone(), d["pb"].clone()
                table = torch.tensor([[part.data_ptr(), dg4.data_ptr(), db4.data_ptr(), nblk, C, 0]], dtype=torch.int64, device=DEV)
                ops.ln_param_finish_multi(table, 1, (C + 31) // 32)
                same(dg4, dg3, f"parked dgamma LN_RPB={rpb}"); same(db4, db3, f"parked dbeta LN_RPB={rpb}")


def test_ln_param_finish_multi_finishes_jobs_of_different_widths_in_one_launch(ops):
    """Three jobs, C = 8 / 520 / 1280, different part counts, one without dbeta and one without dgamma, in one launch: each equals
    its own single-job finish bit for bit and the float64 sum within bounds, and the bytes beside every output stay untouched."""
    jobs = [(8, 3, True, True), (520, 37, True, False), (1280, 1000, False, True)]
    g = torch.Generator().manual_seed(99)
    parts, outs, table, start = [], [], [], 0
    for C, nparts, with_g, with_b in jobs:
        p = torch.randn(nparts * C * 2, generator=g).to(DEV)
        prev = R.small_bf16((2, C), seed=C).to(DEV)
        bufs = []
        for k, on in enumerate((with_g, with_b)):
            buf = torch.full((C + 64,), SENT, dtype=torch.bfloat16, device=DEV)
            buf[32:32 + C] = prev[k]
            bufs.append((buf, on))
        parts.append(p); outs.append((bufs, prev))
        table.append([p.data_ptr(), bufs[0][0][32:].data_ptr() if with_g else 0, bufs[1][0][32:].data_ptr() if with_b else 0, nparts, C, start])
        start += (C + 31) // 32
    ops.ln_param_finish_multi(torch.tensor(table, dtype=torch.int64, device=DEV), len(jobs), start)
    torch.cuda.synchronize()
    for (C, nparts, with_g, with_b), p, (bufs, prev), row in zip(jobs, parts, outs, table):
        single = []
        for k, (buf, on) in enumerate(bufs):
            assert bool((buf[:32] == SENT).all()) and bool((buf[32 + C:] == SENT).all()), f"C={C}: bytes beside output {k} written"
            if not on:
                same(buf[32:32 + C], prev[k], f"C={C}: output {k} without a job pointer changed")
        b2 = [torch.full((C + 64,), SENT, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
        for k in range(2):
            b2[k][32:32 + C] = prev[k]
        t1 = torch.tensor([[p.data_ptr(), b2[0][32:].data_ptr() if with_g else 0, b2[1][32:].data_ptr() if with_b else 0, nparts, C, 0]],
                          dtype=torch.int64, device=DEV)
        ops.ln_param_finish_multi(t1, 1, (C + 31) // 32)
        sums = p.double().reshape(nparts, C, 2).sum(0)
        S = p.double().abs().reshape(nparts, C, 2).sum(0)
        for k, (buf, on) in enumerate(bufs):
            same(buf, b2[k], f"C={C}: output {k}, multi-job vs single-job finish")
            if on:
                within(buf[32:32 + C], prev[k].double() + sums[:, k], S[:, k] + prev[k].double().abs(), "ln_dparam", f"C={C} finish {k}")
