"""Element-wise, reduction and optimizer kernels (csrc/az_elem.hip, csrc/az_optim.hip) against tests/elem_ref.py, element by element,
at the edges of their launch geometry: past the 4096 x 256 cap of the grid-stride loops (the second sweep), past one sweep of
az_sumsq, every branch of colsum_geom, ragged last chunks of the Raven chunk pipeline, strided operands, and the call forms the
executor issues but no other test exercised.  Where a kernel promises bits the comparison is bit for bit; reductions run first on
integer-valued inputs whose every partial sum is exact in fp32 in any order, so a dropped or doubled row fails outright, then on
Gaussian data within elem_ref's bound.  Strided destinations and scratch buffers carry sentinels.

Not covered on purpose: the 64-bit branch of `divmod` (flat indices above 2^32 need tens of gigabytes), the transposes and
az_stage_inputs (exact tests exist), anything that inspects generated code.

AZ_ELEM_K_REPORT=<file>: write the largest K each quantity needed (elem_ref.excess) as JSON at the end of the module."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import elem_ref as R        # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -1232.0            # sentinel of scratch tails and padding columns (exact in bf16, fp16 and fp32)
TAIL = 1024
BF16, F32 = torch.bfloat16, torch.float32
BIG = R.GRID_CAP + 77


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
    path = os.environ.get("AZ_ELEM_K_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(observed=OBSERVED, table=R.K), f, indent=1, sort_keys=True)


def within(out, ref, S, k, what, rounding=None, flush=None):
    """out (device, any dtype) against ref / S (CPU or device float64) under elem_ref's bound for quantity k."""
    ref, S = ref.to(DEV), S.to(DEV)
    rounding = rounding.to(DEV) if rounding is not None else None
    flush = flush.to(DEV) if flush is not None else None
    assert out.shape == ref.shape, (what, tuple(out.shape), tuple(ref.shape))
    o = out.double()
    assert bool(torch.isfinite(o).all()), f"{what}: non-finite output"
    need = R.excess(o, ref, S, rounding, flush)
    OBSERVED[k] = max(OBSERVED.get(k, 0.0), need)
    err = (o - ref).abs()
    b = R.bound(ref, S, k, rounding, flush)
    bad = err > b
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at flat {i}: "
                             f"out={float(o.reshape(-1)[i]):.7g} ref={float(ref.reshape(-1)[i]):.7g} err={float(err.reshape(-1)[i]):.3g} "
                             f"bound={float(b.reshape(-1)[i]):.3g}; K needed {need:.1f} > {R.K[k]}")


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b, what, nan_equal=False):
    """Bit equality (+0 and -0 differ); nan_equal: a NaN counts as equal to a NaN whatever its payload."""
    a, b = a.to(DEV), b.to(DEV)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, tuple(a.shape), tuple(b.shape), a.dtype, b.dtype)
    eq = bits(a) == bits(b)
    if nan_equal:
        eq = eq | (a.isnan() & b.isnan())
    if not bool(eq.all()):
        i = int((~eq).reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int((~eq).sum())} of {eq.numel()} elements differ; first at flat {i}: "
                             f"{float(a.reshape(-1)[i])!r} vs {float(b.reshape(-1)[i])!r}")


def padded(rows, width, pad, fill=None, dtype=BF16):
    """[rows][width + pad] buffer full of sentinels and its [rows][width] view (filled from a CPU tensor)."""
    buf = torch.full((rows, width + pad), SENT, dtype=dtype, device=DEV)
    if fill is not None:
        buf[:, :width] = fill.to(DEV)
    return buf, buf[:, :width]


def intact(buf, width, what):
    assert bool((buf[:, width:] == SENT).all()), f"{what}: padding columns written"


def tailed(n, dtype, fill=None):
    """n elements + a sentinel tail; -> (buffer, view of the first n)."""
    buf = torch.full((n + TAIL,), SENT, dtype=dtype, device=DEV)
    if fill is not None:
        buf[:n] = fill.to(DEV).reshape(-1)
    return buf, buf[:n]


def tail_ok(buf, n, what):
    assert bool((buf[n:] == SENT).all()), f"{what}: wrote past its {n} elements"


def call(name, *args):
    from aozora_sdxl_training_amd._lib import lib
    return lib().call(name, *args)


def refused(name, *args):
    """The entry point returns an argument error (before any launch)."""
    from aozora_sdxl_training_amd._lib import AozoraError
    with pytest.raises(AozoraError, match="argument error"):
        call(name, *args)


def vp(x):
    return ctypes.c_void_p(x)


# ---------------- GEGLU ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,H", [(1100, 7688), (1, 8), (300, 200)])
def test_geglu_forward_and_backward_past_the_grid_cap_on_strided_operands(ops, M, H):
    assert (M * H // 8 > R.GRID_CAP) == (M == 1100)
    proj, dout = R.geglu_inputs(M, H, seed=M + H)
    pb, pv = padded(M, 2 * H, 8, proj)
    ob, ov = padded(M, H, 8)
    ops.geglu_fwd(pv, ov)
    ref, S = R.geglu_fwd_ref(proj)
    within(ov, ref, S, "geglu_out", "geglu out"); intact(ob, H, "geglu out"); intact(pb, 2 * H, "geglu proj")
    db, dv = padded(M, H, 8, dout)
    gb, gv = padded(M, 2 * H, 8)
    ops.geglu_bwd(pv, dv, gv)
    ref, S = R.geglu_bwd_ref(proj, dout)
    within(gv[:, :H], ref[:, :H], S[:, :H], "geglu_da", "geglu dproj (value half)")
    within(gv[:, H:], ref[:, H:], S[:, H:], "geglu_dg", "geglu dproj (gate half)")
    intact(gb, 2 * H, "geglu dproj"); intact(db, H, "geglu dout")
    # the contiguous run gives the same bits
    oc = torch.empty(M, H, dtype=BF16, device=DEV)
    ops.geglu_fwd(proj.to(DEV), oc)
    same(oc, ov, "contiguous vs strided out")


def test_geglu_refuses_leading_dimensions_off_the_vector_grid(ops):
    M, H = 4, 16
    p, o, d = (torch.zeros(M, w + 4, dtype=BF16, device=DEV) for w in (2 * H, H, H))
    good_p, good_o = torch.zeros(M, 2 * H, dtype=BF16, device=DEV), torch.zeros(M, H, dtype=BF16, device=DEV)
    refused("az_geglu_fwd", M, H, ops._ptr(p), 2 * H + 4, ops._ptr(good_o), H, ops._stream())
    refused("az_geglu_fwd", M, H, ops._ptr(good_p), 2 * H, ops._ptr(o), H + 4, ops._stream())
    refused("az_geglu_bwd", M, H, ops._ptr(good_p), 2 * H, ops._ptr(d), H + 4, ops._ptr(good_p), 2 * H, ops._stream())
    refused("az_geglu_bwd", M, H, ops._ptr(good_p), 2 * H, ops._ptr(good_o), H, ops._ptr(p), 2 * H + 4, ops._stream())


# ---------------- SiLU -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [R.GRID_CAP + 4099, 1])
def test_silu_forward_backward_and_accumulate(ops, n):
    x, dy, old = R.silu_inputs(n, seed=n)
    xd, dyd = x.to(DEV), dy.to(DEV)
    yb, y = tailed(n, BF16)
    ops.silu_fwd(xd, y)
    ref, S, fl = R.silu_fwd_ref(x)
    within(y, ref, S, "silu_y", "silu y", flush=fl); tail_ok(yb, n, "silu y")
    db, dx = tailed(n, BF16, torch.full((n,), float("nan")))          # accumulate = 0 must not read dx
    ops.silu_bwd(xd, dyd, dx, accumulate=False)
    ref, S, fl = R.silu_bwd_ref(x, dy)
    within(dx, ref, S, "silu_dx", "silu dx", flush=fl); tail_ok(db, n, "silu dx")
    ab, acc = tailed(n, BF16, old)
    ops.silu_bwd(xd, dyd, acc, accumulate=True)
    ref, S, fl = R.silu_bwd_ref(x, dy, old)
    within(acc, ref, S, "silu_dx", "silu dx += gradient", flush=fl); tail_ok(ab, n, "silu dx +=")
    if n > 1:
        assert not torch.equal(acc, dx)


# ---------------- add_rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", [(4100, 2056), (1, 8), (37, 72)])
def test_add_rows_bit_exact_with_three_leading_dimensions(ops, rows, C):
    assert (rows * C // 8 > R.GRID_CAP) == (rows == 4100)
    a, b = R.gauss_bf16((rows, C), seed=rows), R.gauss_bf16((rows, C), seed=rows + 1)
    ab, av = padded(rows, C, 8, a)
    bb, bv = padded(rows, C, 16, b)
    yb, yv = padded(rows, C, 24)
    ops.add_rows(av, None, yv)
    same(yv, a, "add_rows copy"); intact(yb, C, "add_rows y")
    ops.add_rows(av, bv, yv)
    same(yv, R.add_rows_bits(a, b), "add_rows sum"); intact(yb, C, "add_rows y"); intact(ab, C, "add_rows a"); intact(bb, C, "add_rows b")
    ops.add_rows(yv, bv, yv)                                          # in place, as the residual chain calls it
    same(yv, R.add_rows_bits(R.add_rows_bits(a, b), b), "add_rows in place")


# ---------------- upsample ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C", [(2, 37, 29, 1280), (1, 5, 3, 8), (3, 1, 1, 16)])
def test_upsample_forward_is_a_copy_and_backward_sums_four_taps(ops, B, H, W, C):
    assert (B * 4 * H * W * C // 8 > R.GRID_CAP) == (B == 2)
    x = R.gauss_bf16((B, H, W, C), seed=H)
    n = B * 4 * H * W * C
    yb, y = tailed(n, BF16)
    ops.upsample2x_fwd(x.to(DEV), y.view(B, 2 * H, 2 * W, C))
    same(y.view(B, 2 * H, 2 * W, C), R.upsample_fwd_ref(x), "upsample fwd"); tail_ok(yb, n, "upsample y")
    for dy, exact in ((R.ints_bf16((B, 2 * H, 2 * W, C), seed=W, lim=32), True), (R.gauss_bf16((B, 2 * H, 2 * W, C), seed=W + 1), False)):
        db, dx = tailed(n // 4, BF16)
        ops.upsample2x_bwd(dy.to(DEV), dx.view(B, H, W, C))
        ref, S = R.upsample_bwd_ref(dy)
        if exact:
            same(dx.view(B, H, W, C), ref.bfloat16(), "upsample bwd on integers")
        else:
            within(dx.view(B, H, W, C), ref, S, "upsample_dx", "upsample bwd")
        tail_ok(db, n // 4, "upsample dx")


def test_upsample_backward_past_the_grid_cap_is_exact_on_integers(ops):
    B, H, W, C = 2, 59, 58, 1280
    assert B * H * W * C // 8 > R.GRID_CAP
    dy = R.ints_bf16((B, 2 * H, 2 * W, C), seed=1, lim=32)
    db, dx = tailed(B * H * W * C, BF16)
    ops.upsample2x_bwd(dy.to(DEV), dx.view(B, H, W, C))
    same(dx.view(B, H, W, C), R.upsample_bwd_ref(dy)[0].bfloat16(), "upsample bwd"); tail_ok(db, B * H * W * C, "upsample dx")


def test_upsample_refuses_channels_off_the_vector_grid(ops):
    x = torch.zeros(1, 2, 2, 16, dtype=BF16, device=DEV)
    y = torch.zeros(1, 4, 4, 16, dtype=BF16, device=DEV)
    refused("az_upsample2x_fwd", 1, 2, 2, 12, ops._ptr(x), ops._ptr(y), ops._stream())
    refused("az_upsample2x_bwd", 1, 2, 2, 12, ops._ptr(y), ops._ptr(x), ops._stream())


# ---------------- column sums ---------------------------------------------------------------------------------------------------
def run_colsum(ops, xv, rps, scratch_floats):
    rows, C = xv.shape
    nseg = rows // rps
    sb, _ = tailed(scratch_floats, F32)
    ob, out = tailed(nseg * C, F32)
    call("az_colsum", rows, C, rps, ops._ptr(xv), xv.stride(0), ops._ptr(out), ops._ptr(sb), ops._stream())
    tail_ok(sb, scratch_floats, "az_colsum scratch"); tail_ok(ob, nseg * C, "az_colsum out")
    return out.view(nseg, C)


def run_colsum_grad(ops, xv, rps, scratch_floats, bias_old, n_real, seg=True, bias=True):
    rows, C = xv.shape
    nseg = rows // rps
    sb, _ = tailed(scratch_floats, F32)
    gb, so = tailed(nseg * C, BF16)
    bb, bo = tailed(C, BF16, bias_old)
    call("az_colsum_grad", rows, C, rps, ops._ptr(xv), xv.stride(0), ops._ptr(so if seg else None), ops._ptr(bo if bias else None),
         n_real, ops._ptr(sb), ops._stream())
    tail_ok(sb, scratch_floats, "az_colsum_grad scratch"); tail_ok(gb, nseg * C, "seg_out"); tail_ok(bb, C, "bias")
    if not seg:
        assert bool((so == SENT).all()), "seg_out written although not asked for"
    return so.view(nseg, C), bo


@pytest.mark.parametrize("case", [c for c, _ in R.COLSUM_CASES], ids=[f"rows{c[0]}_C{c[1]}_seg{c[2]}" for c, _ in R.COLSUM_CASES])
def test_colsum_and_colsum_grad_on_every_geometry_branch(ops, case):
    from aozora_sdxl_training_amd._lib import lib
    rows, C, rps = case
    g, _ = R.colsum_geom(rows, C, rps)
    nf = int(lib().raw("az_colsum_scratch_floats")(rows, C, rps))
    assert nf == g["nseg"] * g["nchunk"] * C, (nf, g)
    n_reals = sorted({C, C - 3, max(C - 40, 0)})
    for exact in (True, False):
        x = R.ints_bf16((rows, C), seed=rows + C) if exact else R.gauss_bf16((rows, C), seed=rows + C + 1)
        bias_old = R.ints_bf16((C,), seed=C, lim=64) if exact else R.gauss_bf16((C,), seed=C + 1, scale=3.0)
        xb = torch.full((rows, C + 16), 3.0, dtype=BF16, device=DEV)           # integer sentinel columns: a wrong column shows
        xb[:, :C] = x.to(DEV)
        xv = xb[:, :C]
        ref, S = R.colsum_ref(x, rps)
        out = run_colsum(ops, xv, rps, nf)
        if exact:
            same(out, ref.float(), "colsum on integers")
        else:
            within(out, ref, S, "colsum", "colsum", rounding=R.f32_rounding(ref))
        for n_real in n_reals:
            seg_ref, S_seg, b_ref, S_b = R.colsum_grad_ref(x, rps, bias_old, n_real)
            so, bo = run_colsum_grad(ops, xv, rps, nf, bias_old, n_real)
            if exact:
                same(so, seg_ref.bfloat16(), f"seg_out on integers (n_real {n_real})")
                same(bo, b_ref.bfloat16(), f"bias on integers (n_real {n_real})")
            else:
                within(so, seg_ref, S_seg, "colsum", f"seg_out (n_real {n_real})")
                within(bo, b_ref, S_b, "colsum", f"bias (n_real {n_real})")
            same(bo[n_real:], bias_old[n_real:], f"bias entries at and beyond n_real {n_real}")
            so2, bo2 = run_colsum_grad(ops, xv, rps, nf, bias_old, n_real)
            same(so2, so, "seg_out of a repeated call"); same(bo2, bo, "bias of a repeated call")
            so3, bo3 = run_colsum_grad(ops, xv, rps, nf, bias_old, n_real, bias=False)
            same(so3, so, "seg_out alone"); same(bo3, bias_old, "bias although not asked for")
            _, bo4 = run_colsum_grad(ops, xv, rps, nf, bias_old, n_real, seg=False)
            same(bo4, bo, "bias alone")
        assert bool((xb[:, C:] == 3.0).all())


def test_colsum_refuses_bad_shapes(ops):
    x = torch.zeros(64, 32, dtype=BF16, device=DEV)
    o = torch.zeros(64 * 32, dtype=F32, device=DEV)
    s = torch.zeros(64 * 32, dtype=F32, device=DEV)
    b = torch.zeros(64, dtype=BF16, device=DEV)
    sg = torch.zeros(64 * 32, dtype=BF16, device=DEV)
    st = ops._stream()
    refused("az_colsum_grad", 64, 32, 16, ops._ptr(x), 32, ops._ptr(sg), ops._ptr(b), 33, ops._ptr(s), st)      # n_real > C
    refused("az_colsum_grad", 64, 32, 24, ops._ptr(x), 32, ops._ptr(sg), ops._ptr(b), 32, ops._ptr(s), st)      # rows % rows_per_seg
    refused("az_colsum_grad", 64, 28, 16, ops._ptr(x), 32, ops._ptr(sg), ops._ptr(b), 28, ops._ptr(s), st)      # C % 8
    refused("az_colsum", 64, 32, 24, ops._ptr(x), 32, ops._ptr(o), ops._ptr(s), st)
    refused("az_colsum", 64, 28, 16, ops._ptr(x), 32, ops._ptr(o), ops._ptr(s), st)
    refused("az_colsum", 64, 32, 16, ops._ptr(x), 36, ops._ptr(o), ops._ptr(s), st)                               # ldx % 8


@pytest.mark.parametrize("n", [1, 255, 257, 1000])
@pytest.mark.parametrize("nseg", [1, 5])
def test_reduce_segs_to_bf16(ops, n, nseg):
    for exact in (True, False):
        src = R.ints_bf16((nseg, n), seed=n).float() if exact else torch.randn(nseg, n, generator=R.gen(n + nseg))
        old = R.ints_bf16((n,), seed=n + 1, lim=32) if exact else R.gauss_bf16((n,), seed=n + 2)
        for acc in (0, 1):
            db, dst = tailed(n, BF16, old)
            ops.reduce_segs_to_bf16(src.to(DEV), nseg, n, dst, acc)
            ref, S = R.reduce_segs_ref(src, nseg, n, old if acc else None)
            if exact:
                same(dst, ref.bfloat16(), f"reduce_segs on integers acc={acc}")
            else:
                within(dst, ref, S, "reduce_segs", f"reduce_segs acc={acc}")
            tail_ok(db, n, "reduce_segs dst")


# ---------------- MSE -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,HW,ldp,cpad", [(1, 4, 1, 4, 4), (3, 4, 255, 8, 8), (2, 4, 257, 4, 8), (2, 4, 16384 + 300, 8, 8)])
def test_mse_loss_dpred_and_the_form_without_dpred(ops, B, C, HW, ldp, cpad):
    pred = R.gauss_bf16((B, HW, ldp), seed=HW)
    target = torch.randn(B, C, HW, generator=R.gen(HW + 1))
    w = torch.tensor([1.3, 0.0, 0.7][:B])                      # a zero weight among them
    gs = 0.5
    r = R.mse_ref(pred, target, w, gs)
    pd, td, wd = pred.to(DEV).view(B, 1, HW, ldp), target.to(DEV).view(B, C, 1, HW), w.to(DEV)
    lb, loss = tailed(1, F32)
    sb, per = tailed(B, F32)
    db, dp = tailed(B * HW * cpad, BF16)
    ops.mse_loss_fwd_bwd(pd, td, wd, gs, loss, per, dp.view(B, 1, HW, cpad))
    dpv = dp.view(B, HW, cpad)
    within(dpv[..., :C], r["dpred"], r["S_dpred"], "mse_dpred", "mse dpred")
    assert bool((bits(dpv[..., C:]) == 0).all()), "padding channels of dpred are not +0"
    within(per, r["mean"], r["S_mean"], "mse_mean", "mse per-sample means", rounding=R.f32_rounding(r["mean"]))
    within(loss.reshape(()), r["loss"], r["S_loss"], "mse_loss", "mse loss", rounding=R.f32_rounding(r["loss"]))
    tail_ok(lb, 1, "loss"); tail_ok(sb, B, "per_sample"); tail_ok(db, B * HW * cpad, "dpred")
    lb2, loss2 = tailed(1, F32)
    sb2, per2 = tailed(B, F32)
    ops.mse_loss_fwd_bwd(pd, td, wd, gs, loss2, per2, None)
    same(loss2, loss, "loss without dpred"); same(per2, per, "per-sample means without dpred")
    tail_ok(lb2, 1, "loss"); tail_ok(sb2, B, "per_sample")


# ---------------- noise and target ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW,cpad", [(2, 600001, 4), (2, 600001, 8), (1, 1, 8)])
def test_noise_and_target_bit_for_bit_in_all_three_modes(ops, B, HW, cpad):
    C = 4
    assert (B * HW > R.GRID_CAP) == (B == 2)
    lat = R.gauss_bf16((B, C, HW), seed=HW)
    noise = torch.randn(B, C, HW, generator=R.gen(HW + 3))
    ca, cb = torch.tensor([0.8359375, 0.3173828125][:B]), torch.tensor([0.548828125, 0.9482421875][:B])
    ld, nd = lat.to(DEV).view(B, C, 1, HW), noise.to(DEV).view(B, C, 1, HW)
    for mode in (0, 1, 2):
        nb, noisy = tailed(B * HW * cpad, BF16)
        tb, tg = tailed(B * C * HW, F32)
        ops.noise_target(mode, ld, nd, ca.to(DEV), cb.to(DEV), noisy.view(B, 1, HW, cpad), tg.view(B, C, 1, HW))
        want_noisy, want_tg = R.noise_target_bits(mode, lat, noise, ca, cb, cpad)
        same(noisy.view(B, HW, cpad), want_noisy, f"noisy latents mode {mode}")
        same(tg.view(B, C, HW), want_tg, f"target mode {mode}")
        tail_ok(nb, B * HW * cpad, "noisy"); tail_ok(tb, B * C * HW, "target")


# ---------------- layout ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W,cpad", [(2, 4, 1, 600001, 8), (2, 4, 5, 7, 8), (1, 3, 1, 1, 4), (3, 4, 9, 9, 4)])
def test_layout_kernels_are_exact_permutations(ops, B, C, H, W, cpad):
    assert (B * H * W > R.GRID_CAP) == (W == 600001)
    HW = H * W
    for src in (torch.randn(B, C, H, W, generator=R.gen(HW)), R.gauss_bf16((B, C, H, W), seed=HW + 1)):
        db, dst = tailed(B * HW * cpad, BF16)
        ops.nchw_to_nhwc_pad(src.to(DEV), dst.view(B, H, W, cpad), C)
        want = torch.zeros(B, H, W, cpad, dtype=BF16)
        want[..., :C] = src.bfloat16().permute(0, 2, 3, 1)
        same(dst.view(B, H, W, cpad), want, f"nchw -> nhwc from {src.dtype}"); tail_ok(db, B * HW * cpad, "nhwc")
    nhwc = R.gauss_bf16((B, H, W, cpad + 8), seed=HW + 2)              # ldsrc > C
    for dt in (BF16, F32):
        for c_live in (C, cpad):
            ob, out = tailed(B * c_live * HW, dt)
            ops.nhwc_to_nchw(nhwc.to(DEV), out.view(B, c_live, H, W), c_live)
            same(out.view(B, c_live, H, W), nhwc[..., :c_live].permute(0, 3, 1, 2).to(dt).contiguous(), f"nhwc -> nchw into {dt}")
            tail_ok(ob, B * c_live * HW, "nchw")


# ---------------- timestep embedding --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim", [(1, 2), (3, 170), (1, 514), (5, 320)])
def test_timestep_embedding_with_a_strided_destination(ops, n, dim):
    t = torch.tensor([999.0, 0.0, 37.0, 500.5, 1.0][:n])
    ob, ov = padded(n, dim, 8)
    ops.timestep_embed(t.to(DEV), dim, ov)
    ref, S = R.temb_ref(t, dim)
    within(ov, ref, S, "temb", "timestep embedding"); intact(ob, dim, "timestep embedding")
    refused("az_timestep_embed", n, dim + 1, ops._ptr(t.to(DEV)), ops._ptr(ov), dim + 8, ops._stream())


# ---------------- casts and scales -----------------------------------------------------------------------------------------------------
def test_f32_to_bf16_rounds_to_nearest_even(ops):
    x = torch.cat([R.cast_edges(), torch.randn(BIG, generator=R.gen(21)) * 100.0])
    n = x.numel()
    db, d = tailed(n, BF16)
    ops.f32_to_bf16(x.to(DEV), d)
    same(d, x.bfloat16(), "cast vs torch's CPU cast", nan_equal=True)
    same(d, R.f32_to_bf16_bits(x), "cast vs the integer restatement", nan_equal=True)
    assert bool((d.isnan().cpu() == x.isnan()).all()), "NaN-ness changed"
    tail_ok(db, n, "cast")


def test_scale_bf16_and_scale_f32(ops):
    g = torch.cat([R.cast_edges().bfloat16(), bits_nan_payloads(), R.gauss_bf16((BIG,), seed=22, scale=30.0)])
    n = g.numel()
    for c in (1.0, 0.37):
        coef = torch.tensor([c], dtype=F32, device=DEV)
        gb, gv = tailed(n, BF16, g)
        call("az_scale_bf16", n, ops._ptr(gv), ops._ptr(coef), ops._stream())
        same(gv, R.scale_bf16_bits(g, c), f"scale_bf16 c={c}", nan_equal=(c != 1.0)); tail_ok(gb, n, "scale_bf16")
        x = torch.randn(BIG, generator=R.gen(23))
        xb, xv = tailed(BIG, F32, x)
        call("az_scale_f32", BIG, ops._ptr(xv), ops._ptr(coef), ops._stream())
        same(xv, R.scale_f32_bits(x, c), f"scale_f32 c={c}"); tail_ok(xb, BIG, "scale_f32")
    refused("az_scale_bf16", 0, ops._ptr(gv), ops._ptr(coef), ops._stream())
    refused("az_scale_f32", -1, ops._ptr(xv), ops._ptr(coef), ops._stream())


def bits_nan_payloads():
    return R.bits_to_bf16(np.array([0x7FC1, 0x7F81, 0xFFFF, 0x7FA5], dtype=np.uint16))


class HostBuf:
    """Memory from az_host_alloc as a numpy byte array."""

    def __init__(self, nbytes):
        p = ctypes.c_void_p()
        call("az_host_alloc", ctypes.byref(p), nbytes)
        assert p.value
        self.ptr = p.value
        self.bytes = np.frombuffer((ctypes.c_uint8 * nbytes).from_address(p.value), dtype=np.uint8)

    def tensor(self, dtype):
        return torch.from_numpy(self.bytes).view(dtype)

    def free(self):
        self.bytes = None
        call("az_host_free", vp(self.ptr))


@pytest.mark.parametrize("where", ["device", "host"])
def test_titan_offload(ops, where):
    n = BIG
    g = R.gauss_bf16((n,), seed=24)
    old = torch.randn(n, generator=R.gen(25))
    hb = HostBuf((n + TAIL) * 4) if where == "host" else None
    try:
        for acc in (0, 1):
            if hb is not None:
                gh = hb.tensor(F32)
                gh[:n], gh[n:] = old, SENT
                ptr = hb.ptr
            else:
                gh = torch.full((n + TAIL,), SENT, dtype=F32, device=DEV)
                gh[:n] = old.to(DEV)
                ptr = gh.data_ptr()
            torch.cuda.synchronize()
            call("az_titan_offload", n, ops._ptr(g.to(DEV)), vp(ptr), vp(0), acc, ops._stream())
            torch.cuda.synchronize()
            same(gh[:n].clone(), R.titan_offload_bits(g, old, acc), f"titan_offload acc={acc} into {where} memory")
            assert bool((gh[n:] == SENT).all())
    finally:
        if hb is not None:
            gh = None
            hb.free()
    refused("az_titan_offload", 0, ops._ptr(g.to(DEV)), vp(0), vp(0), 0, ops._stream())


# ---------------- sum of squares, clip coefficient ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,f32", [(1, False), (7, False), (8, False), (9, False), (R.SUMSQ_SWEEP + 8 * 300 + 5, False), (1, True), (262144 + 3, True)])
def test_sumsq_exact_on_integers_and_within_bounds(ops, n, f32):
    for exact in (True, False):
        g = R.ints_bf16((n,), seed=n) if exact else R.gauss_bf16((n,), seed=n + 1)
        if f32:
            g = g.float() if exact else torch.randn(n, generator=R.gen(n + 2))
        gd = g.to(DEV)
        for acc, prev in ((0, 777.0), (1, 123.5)):
            ob, out = tailed(1, F32, torch.tensor([prev]))
            ops.sumsq(gd, out, acc)
            ref, S = R.sumsq_ref(g, prev if acc else 0.0)
            if exact:
                total = np.float32(float((g.double() ** 2).sum()))
                same(out, torch.tensor([np.float32(prev) + total if acc else total], dtype=F32), f"sumsq on integers acc={acc}")
            else:
                within(out.reshape(()), ref, S, "sumsq", f"sumsq acc={acc}", rounding=R.f32_rounding(ref))
            tail_ok(ob, 1, "sumsq out")


def test_sumsq_refuses_misaligned_bf16_and_empty_input(ops):
    g = torch.zeros(64, dtype=BF16, device=DEV)
    out = torch.zeros(1, dtype=F32, device=DEV)
    ws = ops.workspace(out.device)
    refused("az_sumsq", 16, ops._ptr(g[1:]), 0, ops._ptr(out), 0, ops._ptr(ws.scratch), ops._stream())
    refused("az_sumsq", 0, ops._ptr(g), 0, ops._ptr(out), 0, ops._ptr(ws.scratch), ops._stream())
    refused("az_sumsq", -5, ops._ptr(g), 1, ops._ptr(out), 0, ops._ptr(ws.scratch), ops._stream())


@pytest.mark.parametrize("unscale", [1.0, 1.0 / 128])
@pytest.mark.parametrize("max_norm", [0.5, float("inf")])
@pytest.mark.parametrize("ss", [0.0, 7.5, float("inf")])
def test_clip_coef(ops, unscale, max_norm, ss):
    s = torch.tensor([ss], dtype=F32, device=DEV)
    cb, coef = tailed(1, F32)
    nb, norm = tailed(1, F32)
    ops.clip_coef(s, max_norm, coef, norm, unscale=unscale)
    c, nrm = float(coef), float(norm)
    assert np.isfinite(c) and 0.0 <= c <= unscale, (c, unscale)
    tail_ok(cb, 1, "coef"); tail_ok(nb, 1, "norm")
    if np.isfinite(ss):
        c_ref, n_ref = R.clip_coef_ref(ss, max_norm, unscale)
        ref = torch.tensor([c_ref, n_ref], dtype=torch.float64)
        within(torch.stack([coef[0], norm[0]]), ref, ref.abs(), "clip_coef", "clip coefficient and norm", rounding=R.f32_rounding(ref))
    else:
        assert nrm == float("inf") and c == (0.0 if np.isfinite(max_norm) else unscale)


# ---------------- AdamW ------------------------------------------------------------------------------------------------------------------
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), wd=0.01, eps=1e-8, debias=0.3)


def adamw_state(n, mdtype, f32_grads, seed):
    """p, three gradients, zero m / v (CPU) and the three hyper vectors."""
    p = R.gauss_bf16((n,), seed=seed, scale=0.1)
    grads = [R.adamw_grads(n, seed + 1 + s, f32_grads) for s in range(3)]
    m = torch.zeros(n, dtype=R.moment_dtype(mdtype))
    hyper = [R.adamw_hyper(step=s + 1, **HYPER) for s in range(3)]
    return p, grads, m, m.clone(), hyper


def hyper_dev(hyper):
    return torch.from_numpy(np.stack(hyper)).to(DEV)


@pytest.mark.parametrize("mdtype,gdtype", [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)])
def test_adamw_flat_three_steps_bit_for_bit(ops, mdtype, gdtype):
    for n in (BIG, 5):
        for coef in (None, 0.37):
            p, grads, m, v, hyper = adamw_state(n, mdtype, gdtype == 1, seed=n + mdtype)
            pb, pd = tailed(n, BF16, p)
            mb, md = tailed(n, m.dtype, m)
            vb, vd = tailed(n, v.dtype, v)
            hd = hyper_dev(hyper)
            cd = torch.tensor([coef], dtype=F32, device=DEV) if coef is not None else None
            for s in range(3):
                gd = grads[s].to(DEV)
                if gdtype == 0 and s == 0:          # the entry point without a gradient type takes bf16 gradients
                    call("az_adamw_flat", n, ops._ptr(pd), ops._ptr(gd), ops._ptr(md), ops._ptr(vd), mdtype, ops._ptr(hd[s]), ops._ptr(cd), ops._stream())
                else:
                    call("az_adamw_flat_ex", n, ops._ptr(pd), ops._ptr(gd), gdtype, ops._ptr(md), ops._ptr(vd), mdtype, ops._ptr(hd[s]),
                         ops._ptr(cd), ops._stream())
                p, m, v = R.adamw_bits(p, grads[s], m, v, hyper[s], coef)
                what = f"n={n} coef={coef} step {s + 1}"
                same(md, m, "m " + what, nan_equal=True); same(vd, v, "v " + what, nan_equal=True); same(pd, p, "p " + what, nan_equal=True)
                if s == 0 and coef is None and n > 4:       # element 3 holds 1e4: its square overflows fp16 moments and no other type
                    assert bool(torch.isinf(vd[3])) == (mdtype == 2), f"v of the 1e4 gradient: {float(vd[3])} ({what})"
            assert bool(p.isnan().any()) and bool(torch.isfinite(p.float()).any())
            tail_ok(pb, n, "p"); tail_ok(mb, n, "m"); tail_ok(vb, n, "v")


def test_adamw_refuses_unknown_types(ops):
    n = 8
    p, g, m = (torch.zeros(n, dtype=BF16, device=DEV) for _ in range(3))
    h = hyper_dev([R.adamw_hyper(step=1, **HYPER)])
    refused("az_adamw_flat", n, ops._ptr(p), ops._ptr(g), ops._ptr(m), ops._ptr(m), 3, ops._ptr(h), vp(0), ops._stream())
    refused("az_adamw_flat_ex", n, ops._ptr(p), ops._ptr(g), 0, ops._ptr(m), ops._ptr(m), 3, ops._ptr(h), vp(0), ops._stream())
    refused("az_adamw_flat_ex", n, ops._ptr(p), ops._ptr(g), 2, ops._ptr(m), ops._ptr(m), 0, ops._ptr(h), vp(0), ops._stream())
    refused("az_adamw_flat_ex", 0, ops._ptr(p), ops._ptr(g), 0, ops._ptr(m), ops._ptr(m), 0, ops._ptr(h), vp(0), ops._stream())
    assert bool((p == 0).all())


# ---------------- the Raven chunk pipeline ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three_streams(ops):
    from aozora_sdxl_training_amd import streams
    sc = streams.pick(DEV, what="compute")
    sh = streams.pick(DEV, beside=[sc], what="h2d")
    sd = streams.pick(DEV, beside=[sc, sh], what="d2h")
    return sc, sh, sd


@pytest.mark.parametrize("mdtype,gdtype", [(0, 0), (1, 1), (2, 0)])
@pytest.mark.parametrize("n,chunk", [(1000, 4096), (1000, 1000), (2000, 1000), (4 * 3000 + 77, 3000), (7, 1)],
                         ids=["one_chunk", "chunk_equals_n", "two_chunks", "five_chunks_ragged", "n7_chunk1"])
def test_raven_step_equals_flat_steps_on_host_moments(ops, three_streams, mdtype, gdtype, n, chunk):
    """Two az_raven_step_ex calls back to back on the same three streams (the event pool is reused), moments in az_host_alloc memory:
    p, m, v equal two az_adamw_flat_ex steps bit for bit; staging beyond 2 x 2 x chunk elements, host moments beyond n and the
    parameters beyond n stay sentinel (every buffer has a whole chunk of room behind n, so a last chunk taken at full length shows
    as a broken sentinel, not as a fault).  Each case runs once."""
    sc, sh, sd = three_streams
    mdt = R.moment_dtype(mdtype)
    esz = 4 if mdtype == 1 else 2
    p0, grads, _, _, hyper = adamw_state(n, mdtype, gdtype == 1, seed=n + chunk)
    g = torch.Generator().manual_seed(n)
    m0 = (1e-3 * torch.randn(n, generator=g)).to(mdt)
    v0 = (1e-4 * torch.rand(n, generator=g)).to(mdt)
    hd = hyper_dev(hyper)
    cd = torch.tensor([0.37], dtype=F32, device=DEV)
    gds = [torch.cat([x, torch.zeros(chunk, dtype=x.dtype)]).to(DEV) for x in grads]
    # flat steps on device moments
    pf, mf, vf = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    for s in range(2):
        call("az_adamw_flat_ex", n, ops._ptr(pf), ops._ptr(gds[s]), gdtype, ops._ptr(mf), ops._ptr(vf), mdtype, ops._ptr(hd[s]), ops._ptr(cd),
             ops._stream())
    # the pipeline on host moments
    hm, hv = HostBuf((n + chunk) * esz), HostBuf((n + chunk) * esz)
    try:
        mh, vh = hm.tensor(mdt), hv.tensor(mdt)
        mh[:n], vh[:n], mh[n:], vh[n:] = m0, v0, SENT, SENT
        used = 2 * 2 * chunk * esz
        staging = torch.full((used + TAIL,), 0xA5, dtype=torch.uint8, device=DEV)
        pbuf = torch.full((n + chunk,), SENT, dtype=BF16, device=DEV)
        pr = pbuf[:n]
        pr.copy_(p0)
        torch.cuda.synchronize()
        for s in range(2):
            call("az_raven_step_ex", n, ops._ptr(pr), ops._ptr(gds[s]), gdtype, vp(hm.ptr), vp(hv.ptr), mdtype, ops._ptr(hd[s]), ops._ptr(cd),
                 ops._ptr(staging), chunk, vp(sc.cuda_stream), vp(sh.cuda_stream), vp(sd.cuda_stream))
        sc.synchronize()                  # the compute stream joins the last write-backs
        torch.cuda.synchronize()
        same(pr, pf, "p", nan_equal=True)
        same(mh[:n].clone(), mf, "m", nan_equal=True); same(vh[:n].clone(), vf, "v", nan_equal=True)
        assert bool((mh[n:] == SENT).all()) and bool((vh[n:] == SENT).all()), "host moments beyond n written"
        assert bool((pbuf[n:] == SENT).all()), "parameters beyond n written"
        assert bool((staging[used:] == 0xA5).all()), "staging beyond 2 x 2 x chunk elements written"
        assert not torch.equal(bits(mf.cpu()), bits(m0))
    finally:
        mh = vh = None
        hm.free(); hv.free()


def test_raven_step_refuses_bad_arguments(ops, three_streams):
    sc, sh, sd = three_streams
    n = 8
    p, g = torch.zeros(n, dtype=BF16, device=DEV), torch.zeros(n, dtype=BF16, device=DEV)
    h = hyper_dev([R.adamw_hyper(step=1, **HYPER)])
    st = torch.zeros(256, dtype=torch.uint8, device=DEV)
    hb = HostBuf(64)
    try:
        for chunk, mdtype in ((0, 0), (-4, 0), (8, 3)):
            refused("az_raven_step_ex", n, ops._ptr(p), ops._ptr(g), 0, vp(hb.ptr), vp(hb.ptr + 32), mdtype, ops._ptr(h), vp(0), ops._ptr(st), chunk,
                    vp(sc.cuda_stream), vp(sh.cuda_stream), vp(sd.cuda_stream))
    finally:
        hb.free()
