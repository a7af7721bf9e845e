"""az_robust_loss_fwd_bwd (csrc/az_elem.hip: l1, huber, smooth_l1) against tests/loss_ref.py, element by element, within its bounds
(derived in tests/test_loss_ref_cpu.py, which also shows that a kernel spelling the pseudo-Huber loss as a difference would fail
here): one pixel, both sides of a 256-thread block, more than one sweep, ldp != cpad != C; unit-scale, tiny and exactly zero
residuals, per-sample widths that differ, a zero weight, and a sample with c = 2^20 whose huber mean must meet az_mse_loss_fwd_bwd's.
Then the drop-in seam loss.weighted_sdxl_loss."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import elem_ref as R        # noqa: E402
import loss_ref as LR       # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -1232.0            # sentinel of guard tails (exact in bf16 and fp32)
TAIL = 1024
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd import ops as _ops
    return _ops


def within(out, ref, S, k, what, rounding=None):
    """out (device) against ref / S (float64) under loss_ref's bound for quantity k; prints the K it needed before it asserts."""
    ref, S = ref.to(DEV), S.to(DEV)
    rounding = rounding.to(DEV) if rounding is not None else None
    assert out.shape == ref.shape, (what, tuple(out.shape), tuple(ref.shape))
    o = out.double()
    assert bool(torch.isfinite(o).all()), f"{what}: non-finite output"
    need = R.excess(o, ref, S, rounding)
    print(f"{what}: K needed {need:.3f} of {LR.K[k]}")
    err = (o - ref).abs()
    b = LR.bound(ref, S, k, rounding)
    bad = err > b
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at flat {i}: "
                             f"out={float(o.reshape(-1)[i]):.7g} ref={float(ref.reshape(-1)[i]):.7g} err={float(err.reshape(-1)[i]):.3g} "
                             f"bound={float(b.reshape(-1)[i]):.3g}; K needed {need:.1f} > {LR.K[k]}")


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all()), what


def tailed(n, dtype):
    buf = torch.full((n + TAIL,), SENT, dtype=dtype, device=DEV)
    return buf, buf[:n]


def tail_ok(buf, n, what):
    assert bool((buf[n:] == SENT).all()), f"{what}: wrote past its {n} elements"


_REFS = {}


def case(kind, variant, shape):
    """Inputs and float64 reference of one case, computed once."""
    key = (kind, variant, shape)
    if key not in _REFS:
        B, C, HW, ldp, _ = shape
        pred, target, w, c = LR.inputs(variant, B, C, HW, ldp)
        _REFS[key] = (pred, target, w, c, LR.robust_ref(kind, pred, target, w, c, LR.GSCALE))
    return _REFS[key]


def run(ops, kind, pred, target, w, c, cpad, with_dpred=True):
    """-> (loss, per, dpred [B][HW][cpad] or None), guard tails checked."""
    B, C, HW = target.shape
    ldp = pred.shape[2]
    pd, td = pred.to(DEV).view(B, 1, HW, ldp), target.to(DEV).view(B, C, 1, HW)
    lb, loss = tailed(1, F32)
    sb, per = tailed(B, F32)
    db, dp = tailed(B * HW * cpad, BF16) if with_dpred else (None, None)
    ops.robust_loss_fwd_bwd(kind, pd, td, w.to(DEV), None if kind == "l1" else c.to(DEV), LR.GSCALE, loss, per,
                            dp.view(B, 1, HW, cpad) if with_dpred else None)
    tail_ok(lb, 1, "loss"); tail_ok(sb, B, "per_sample")
    if with_dpred:
        tail_ok(db, B * HW * cpad, "dpred")
    return loss, per, dp.view(B, HW, cpad) if with_dpred else None


@pytest.mark.parametrize("shape", LR.SHAPES, ids=lambda s: "B%d_C%d_HW%d_ldp%d_cpad%d" % s)
@pytest.mark.parametrize("kind", list(LR.KINDS))
def test_robust_loss_against_float64(ops, kind, shape):
    B, C, HW, ldp, cpad = shape
    for variant in LR.VARIANTS:
        pred, target, w, c, r = case(kind, variant, shape)
        loss, per, dp = run(ops, kind, pred, target, w, c, cpad)
        tag = f"{kind} {variant}"
        within(dp[..., :C], r["dpred"], r["S_dpred"], "robust_dpred", f"{tag} dpred")
        assert bool((bits(dp[..., C:]) == 0).all()), f"{tag}: padding channels of dpred are not +0"
        within(per, r["mean"], r["S_mean"], "robust_mean", f"{tag} per-sample means", rounding=R.f32_rounding(r["mean"]))
        within(loss.reshape(()), r["loss"], r["S_loss"], "robust_loss", f"{tag} loss", rounding=R.f32_rounding(r["loss"]))
        if variant == "zero":
            assert bool((bits(dp) == 0).all()), f"{tag}: dpred of zero residuals is not +0 everywhere"
            assert float(loss) == 0.0 and bool((per == 0).all()), f"{tag}: loss of zero residuals"
        # the form without dpred: same loss and means, bit for bit
        loss2, per2, _ = run(ops, kind, pred, target, w, c, cpad, with_dpred=False)
        same(loss2, loss, f"{tag}: loss without dpred"); same(per2, per, f"{tag}: per-sample means without dpred")


@pytest.mark.parametrize("shape", LR.SHAPES, ids=lambda s: "B%d_C%d_HW%d_ldp%d_cpad%d" % s)
def test_huber_at_c_2_to_20_meets_the_mse_kernel(ops, shape):
    """Sample 0 of the huge-c input: the pseudo-Huber loss is the squared error to 2^-42 there.  Reference: az_mse_loss_fwd_bwd on the
    same data; bound: the two kernels' `mean` bounds added (each: one fp32 rounding of the mean + K 2^-24 S)."""
    B, C, HW, ldp, cpad = shape
    pred, target, w, c, _ = case("huber", "huge_c", shape)
    assert float(c[0]) == 2.0 ** 20
    _, per, _ = run(ops, "huber", pred, target, w, c, cpad)
    pd, td = pred.to(DEV).view(B, 1, HW, ldp), target.to(DEV).view(B, C, 1, HW)
    loss_m = torch.empty(1, dtype=F32, device=DEV)
    per_m = torch.empty(B, dtype=F32, device=DEV)
    ops.mse_loss_fwd_bwd(pd, td, w.to(DEV), LR.GSCALE, loss_m, per_m, None)
    m = R.mse_ref(pred, target, w, LR.GSCALE)["mean"][0]
    b = (R.U_F32 * m + R.K["mse_mean"] * R.U_F32 * m) + (R.U_F32 * m + LR.K["robust_mean"] * R.U_F32 * m)
    err = abs(float(per[0].double()) - float(per_m[0].double()))
    print(f"huber(c=2^20) mean {float(per[0])!r} mse mean {float(per_m[0])!r} err {err:.3g} bound {float(b):.3g}")
    assert err <= float(b)


def test_argument_refusals(ops):
    from aozora_sdxl_training_amd._lib import lib, AozoraError
    B, C, HW = 2, 4, 16
    pred = torch.zeros(B, HW, 8, dtype=BF16, device=DEV)
    target = torch.zeros(B, C, HW, dtype=F32, device=DEV)
    w = torch.ones(B, dtype=F32, device=DEV)
    c = torch.full((B,), 0.1, dtype=F32, device=DEV)
    loss, per = torch.zeros(1, dtype=F32, device=DEV), torch.zeros(B, dtype=F32, device=DEV)
    dp = torch.zeros(B, HW, 8, dtype=BF16, device=DEV)
    scratch = torch.zeros(64 * B, dtype=F32, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(kind, cw, cpad, ldp=8):
        lib().call("az_robust_loss_fwd_bwd", kind, B, C, HW, vp(pred), ldp, vp(target), vp(w), vp(cw), 1.0, vp(loss), vp(per), vp(dp), cpad,
                   vp(scratch), st)
    for kind, cw, cpad, ldp in ((0, c, 8, 8), (4, c, 8, 8), (-1, c, 8, 8), (2, c, 3, 8), (1, None, 3, 8), (2, None, 8, 8), (3, None, 8, 8),
                                (2, c, 8, 3)):
        with pytest.raises(AozoraError, match="argument error"):
            call(kind, cw, cpad, ldp)
    call(1, None, 8)            # l1 takes no widths
    call(2, c, 8)
    torch.cuda.synchronize()
    assert float(loss) == 0.0 and bool((bits(dp) == 0).all())


@pytest.mark.parametrize("kind", list(LR.KINDS))
def test_a_nan_in_pred_or_target_gives_a_nan_loss(ops, kind):
    shape = LR.SHAPES[2]
    B, C, HW, ldp, cpad = shape
    pred, target, w, c, _ = case(kind, "unit", shape)
    for where in ("pred", "target", "pred_inf"):
        p, t = pred.clone(), target.clone()
        if where == "target":
            t[0, 3, HW - 1] = float("nan")
        else:
            p[0, HW - 1, 2] = float("nan") if where == "pred" else float("inf")
        loss, per, _ = run(ops, kind, p, t, w, c, cpad)
        assert not bool(torch.isfinite(loss).any()) and not bool(torch.isfinite(per[0])), (kind, where, float(loss))
        assert bool(torch.isfinite(per[1])), "the other sample's mean is its own"


# ---------------- the drop-in seam ------------------------------------------------------------------------------------------------
def _seam_inputs():
    g = R.gen(5)
    B, C, H, W = 3, 4, 9, 7
    pred = torch.randn(B, C, H, W, generator=g).bfloat16()
    target = torch.randn(B, C, H, W, generator=g)
    ts = torch.tensor([10, 900, 1500])                        # the last one past the curve: clamped
    curve = torch.linspace(0.25, 1.75, 1000)
    return pred, target, ts, curve


@pytest.mark.parametrize("kind", list(LR.KINDS))
def test_seam_backward_against_float64(ops, kind):
    """weighted_sdxl_loss(...).backward() seeded by a scalar: loss and the gradient against the float64 restatement; the gradient is
    dpred of the kernel (bound robust_dpred) scaled by the seed in bf16 (one more rounding: half an ulp of bf16)."""
    from aozora_sdxl_training_amd.loss import weighted_sdxl_loss
    pred, target, ts, curve = _seam_inputs()
    B = pred.shape[0]
    n = pred[0].numel()
    cw = torch.tensor([0.05, 0.4, 1.5])
    seed = 0.25                                                # a power of two: the bf16 scaling by the seed is exact
    p = pred.to(DEV).requires_grad_(True)
    loss = weighted_sdxl_loss(p, target.to(DEV), ts.to(DEV), curve.to(DEV), loss_type=f"{kind}", c=None if kind == "l1" else cw.to(DEV))
    (loss * seed).backward()
    w = curve[ts.clamp(0, 999)]
    r = LR.robust_ref(kind, pred.reshape(B, n, 1), target.reshape(B, 1, n), w, cw, 1.0)
    within(loss.detach().reshape(()), r["loss"], r["S_loss"], "robust_loss", f"seam {kind} loss", rounding=R.f32_rounding(r["loss"]))
    within(p.grad.reshape(B, n, 1), seed * r["dpred"], seed * r["S_dpred"], "robust_dpred", f"seam {kind} gradient")
    assert p.grad.dtype == BF16 and p.grad.shape == pred.shape
    # c = None takes the spec's constant
    l1 = weighted_sdxl_loss(pred.to(DEV), target.to(DEV), ts.to(DEV), None, loss_type=f"{kind}:c=0.4" if kind != "l1" else "l1")
    l2 = weighted_sdxl_loss(pred.to(DEV), target.to(DEV), ts.to(DEV), None, loss_type=kind, c=None if kind == "l1" else torch.full((B,), 0.4))
    assert float(l1) == float(l2)


def test_seam_mse_is_weighted_sdxl_mse_loss_bit_for_bit(ops):
    from aozora_sdxl_training_amd.loss import weighted_sdxl_loss, weighted_sdxl_mse_loss
    pred, target, ts, curve = _seam_inputs()
    out = []
    for fn in (lambda p: weighted_sdxl_mse_loss(p, target.to(DEV), ts.to(DEV), curve.to(DEV)),
               lambda p: weighted_sdxl_loss(p, target.to(DEV), ts.to(DEV), curve.to(DEV), loss_type="MSE"),
               lambda p: weighted_sdxl_loss(p, target.to(DEV), ts.to(DEV), curve.to(DEV))):
        p = pred.to(DEV).requires_grad_(True)
        loss = fn(p)
        (loss * 0.5).backward()
        out.append((loss.detach().clone(), p.grad.clone()))
    for l, g in out[1:]:
        same(l.reshape(1), out[0][0].reshape(1), "loss"); same(g, out[0][1], "gradient")
    with pytest.raises(ValueError):
        weighted_sdxl_loss(pred.to(DEV), target.to(DEV), ts.to(DEV), None, loss_type="MSE", c=torch.ones(3))
    with pytest.raises(ValueError):
        weighted_sdxl_loss(pred.to(DEV), target.to(DEV), ts.to(DEV), None, loss_type="huber:min_snr_gamma=5")
    with pytest.raises(ValueError):
        weighted_sdxl_loss(pred.to(DEV), target.to(DEV), ts.to(DEV), None, loss_type="logcosh")
