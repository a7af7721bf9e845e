"""tests/loss_ref.py and the host side of LOSS_TYPE without a GPU: the table K of the robust losses is derived here (the kernel's own
formula in float32 torch against the float64 restatement over the inputs of tests/test_loss_gpu.py; an entry below 4 x measured
fails), the inputs are shown to discriminate (the difference spelling 2c (sqrt(x^2 + c^2) - c) leaves the robust_mean bound on the
tiny-residual and on the huge-c input), and loss.parse_loss_type, loss.loss_widths and loss.min_snr_factors are checked against
their contract (INTEGRATION.md "Loss types")."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import elem_ref as R        # noqa: E402
import loss_ref as LR       # noqa: E402

from aozora_sdxl_training_amd import loss as L                            # noqa: E402
from aozora_sdxl_training_amd.schedule import ddpm_alphas_cumprod         # noqa: E402

ZERO = torch.zeros((), dtype=torch.float64)
MEASURED = {}


def measure(quantity, out32, ref, S, rounding=None):
    """elem_ref's derivation: the K the float32 value itself needs (no storage rounding) against the table with the 4x margin; then
    the value rounded as the kernel stores it stays inside the bound."""
    k = R.excess(out32, ref, S, ZERO)
    MEASURED[quantity] = max(MEASURED.get(quantity, 0.0), k)
    assert LR.K[quantity] >= 4.0 * k, f"K[{quantity}] = {LR.K[quantity]} is below 4 x the measured {k:.3f}"
    stored = out32.bfloat16() if rounding is None else out32
    assert bool(((stored.double() - ref).abs() <= LR.bound(ref, S, quantity, rounding)).all()), quantity
    return k


# ---------------- K -------------------------------------------------------------------------------------------------------------
def test_k_of_the_robust_losses_is_derived_from_the_kernel_formula():
    MEASURED.clear()
    for B, C, HW, ldp, _ in LR.SHAPES:
        for variant in LR.VARIANTS:
            pred, target, w, c = LR.inputs(variant, B, C, HW, ldp)
            for kind in LR.KINDS:
                r = LR.robust_ref(kind, pred, target, w, c, LR.GSCALE)
                dp, mean, loss = LR.robust_f32(kind, pred, target, w, c, LR.GSCALE)
                measure("robust_dpred", dp, r["dpred"], r["S_dpred"])
                measure("robust_mean", mean, r["mean"], r["S_mean"], rounding=R.f32_rounding(r["mean"]))
                measure("robust_loss", loss, r["loss"], r["S_loss"], rounding=R.f32_rounding(r["loss"]))
    for q, k in sorted(MEASURED.items()):
        print(f"K[{q}] measured {k:.3f} table {LR.K[q]}")
    assert set(MEASURED) == set(LR.K)
    assert all(v >= 1.0 and float(np.log2(v)).is_integer() for v in LR.K.values())
    # the table is 4 x measured rounded up to a power of two -- not wider
    for q, k in MEASURED.items():
        assert LR.K[q] == max(1.0, 2.0 ** math.ceil(math.log2(max(4.0 * k, 1e-30)))), (q, k, LR.K[q])


@pytest.mark.parametrize("kind", ["huber", "smooth_l1"])
@pytest.mark.parametrize("variant", ["tiny", "huge_c"])
def test_the_difference_spelling_leaves_the_bound_on_these_inputs(kind, variant):
    """2c (sqrt(x^2 + c^2) - c) in float32: cancellation once |x| << c.  The per-sample means it gives are outside the robust_mean
    bound on the tiny-residual input (every sample) and on the huge-c input (the sample with c = 2^20, where it is exactly 0), at every
    shape -- a kernel written that way fails tests/test_loss_gpu.py; the stable spelling passes on the same inputs (above)."""
    for B, C, HW, ldp, _ in LR.SHAPES:
        pred, target, w, c = LR.inputs(variant, B, C, HW, ldp)
        r = LR.robust_ref(kind, pred, target, w, c, LR.GSCALE)
        _, mean, loss = LR.robust_f32(kind, pred, target, w, c, LR.GSCALE, naive=True)
        b = LR.bound(r["mean"], r["S_mean"], "robust_mean", R.f32_rounding(r["mean"]))
        err = (mean.double() - r["mean"]).abs()
        bad = err > b
        if variant == "tiny":
            if HW > 1:                # one pixel: four terms, the error of a single term may happen to be small
                assert bool(bad.all()), (kind, HW, (err / r["mean"]).tolist())
        else:
            assert bool(bad[0]) and float(mean[0]) == 0.0, (kind, HW, float(mean[0]), float(r["mean"][0]))
            if B == 1:
                assert float(loss) == 0.0 and float(r["loss"]) > 0.0


def test_float64_restatement_is_the_published_form():
    """The stable spelling equals 2c (sqrt(x^2 + c^2) - c) / 2 (sqrt(x^2 + c^2) - c) where that does not cancel (float64, |x| ~ c),
    its derivative is the analytic one, l1 is |x| with sign(x) and +0 at 0, and huber at c = 2^20 is the squared error to x^2 / (4 c^2) (2^-42 at |x| = 1)."""
    x = torch.randn(10000, dtype=torch.float64, generator=R.gen(11))
    c = torch.full_like(x, 0.7)
    for kind, lead in (("huber", 2.0 * c), ("smooth_l1", torch.full_like(c, 2.0))):
        l, dl = LR.elem(kind, x, c)
        want = lead * (torch.sqrt(x * x + c * c) - c)
        assert float((l - want).abs().max()) < 1e-14          # absolute: the difference spelling itself cancels at small |x|
        h = 1e-6
        num = (LR.elem(kind, x + h, c)[0] - LR.elem(kind, x - h, c)[0]) / (2 * h)
        assert float((dl - num).abs().max()) < 1e-8
    l, dl = LR.elem("l1", torch.tensor([-2.0, 0.0, 3.0], dtype=torch.float64), None)
    assert l.tolist() == [2.0, 0.0, 3.0] and dl.tolist() == [-1.0, 0.0, 1.0] and not math.copysign(1.0, float(dl[1])) < 0
    l, dl = LR.elem("huber", x, torch.full_like(x, 2.0 ** 20))
    assert float(x.abs().max()) < 8.0           # relative distance x^2 / (4 c^2) (loss) and x^2 / (2 c^2) (derivative): below 2^-36 / 2^-35
    assert float(((l - x * x).abs() / (x * x)).max()) < 2.0 ** -36 and float(((dl - 2 * x).abs() / x.abs()).max()) < 2.0 ** -35


# ---------------- parser --------------------------------------------------------------------------------------------------------
def test_parser_defaults_and_letter_case():
    for s in (None, "", "MSE", "mse", " Mse "):
        for mode in L.PREDICTION_TYPES:
            assert L.parse_loss_type(s, mode) == L.LossSpec("mse", None, None, None)
    assert L.parse_loss_type("L1", "rectified_flow") == L.LossSpec("l1", None, None, None)
    assert L.parse_loss_type("Huber", "epsilon") == L.LossSpec("huber", 0.1, "snr", None)
    assert L.parse_loss_type("SMOOTH_L1", "v_prediction") == L.LossSpec("smooth_l1", 0.1, "snr", None)
    assert L.parse_loss_type("huber:C=0.25,Schedule=Exponential", "epsilon") == L.LossSpec("huber", 0.25, "exponential", None)
    assert L.parse_loss_type("Huber:c=1048576,schedule=constant", "rectified_flow") == L.LossSpec("huber", 1048576.0, "constant", None)
    assert L.parse_loss_type("MSE:min_snr_gamma=5", "epsilon") == L.LossSpec("mse", None, None, 5.0)
    assert L.parse_loss_type("l1:MIN_SNR_GAMMA=1.5", "v_prediction") == L.LossSpec("l1", None, None, 1.5)
    assert L.parse_loss_type("smooth_l1: c = 1e-2 , min_snr_gamma = 5", "epsilon") == L.LossSpec("smooth_l1", 0.01, "snr", 5.0)
    spec = L.parse_loss_type("huber:c=0.3", "epsilon")
    assert L.parse_loss_type(spec, "rectified_flow") is spec and spec.needs_c and not L.parse_loss_type("l1", "epsilon").needs_c


@pytest.mark.parametrize("s,mode", [
    ("logcosh", "epsilon"), ("huber2", "epsilon"), ("mse:huber_scale=1", "epsilon"), ("huber:delta=1", "epsilon"),      # unknown kind / key
    ("huber:c", "epsilon"), ("huber:c=0.1,c=0.2", "epsilon"), ("huber:,", "epsilon"),                                       # malformed
    ("mse:c=0.1", "epsilon"), ("l1:c=0.1", "epsilon"), ("mse:schedule=snr", "epsilon"), ("l1:schedule=constant", "epsilon"),
    ("huber:c=0", "epsilon"), ("huber:c=-1", "epsilon"), ("smooth_l1:c=nan", "epsilon"), ("huber:c=inf", "epsilon"),
    ("huber:c=abc", "epsilon"), ("huber:schedule=linear", "epsilon"),
    ("mse:min_snr_gamma=5", "rectified_flow"), ("huber:min_snr_gamma=5", "rectified_flow"), ("l1:min_snr_gamma=0", "epsilon"),
    ("l1:min_snr_gamma=-5", "v_prediction"), ("mse:min_snr_gamma=inf", "epsilon")])
def test_parser_refusals(s, mode):
    with pytest.raises(ValueError, match="LOSS_TYPE"):
        L.parse_loss_type(s, mode)


def test_a_spec_with_min_snr_is_refused_for_rectified_flow_too():
    with pytest.raises(ValueError, match="min_snr_gamma"):
        L.parse_loss_type(L.LossSpec("mse", None, None, 5.0), "rectified_flow")


def test_trainer_refuses_an_unreadable_loss_type_before_anything_is_loaded(tmp_path, monkeypatch, capsys):
    """trainer.train raises before the checkpoint is touched; trainer.main prints ERROR: and returns 2, as for MIXED_PRECISION."""
    import json
    import types
    from aozora_sdxl_training_amd import checkpoint as C
    from aozora_sdxl_training_amd import config as CF
    from aozora_sdxl_training_amd import trainer

    def no_load(*a, **k):
        raise AssertionError("a UNet was loaded")
    monkeypatch.setattr(C, "load_unet", no_load)
    for mode, bad in (("v_prediction", "logcosh"), ("rectified_flow", "huber:min_snr_gamma=5"), ("epsilon", "huber:c=-1")):
        cfg = types.SimpleNamespace(OPTIMIZER_TYPE="raven", RAVEN_PARAMS={}, GRADIENT_ACCUMULATION_STEPS=2, PREDICTION_TYPE=mode,
                                    LOSS_TYPE=bad, SINGLE_FILE_CHECKPOINT_PATH=str(tmp_path / "none.safetensors"), SEED=1)
        with pytest.raises(ValueError, match="LOSS_TYPE"):
            trainer.train(cfg, unet=None, device="cpu")
    key = {v: k for k, v in CF.block_keys("sdxl").items()}
    preset = tmp_path / "preset.json"
    preset.write_text(json.dumps({"active_mode": "sdxl", "sdxl": {key["LOSS_TYPE"]: "LogCosh", key["PREDICTION_TYPE"]: "epsilon"}}))
    assert trainer.main(["--config", str(preset)]) == 2
    out = capsys.readouterr().out
    assert "ERROR: LOSS_TYPE: unknown loss 'logcosh'" in out
    assert CF.flat_defaults()["LOSS_TYPE"] == "MSE"


# ---------------- widths --------------------------------------------------------------------------------------------------------
def test_width_schedules_at_the_ends_of_the_timestep_range():
    ac = ddpm_alphas_cumprod().double()
    ts = torch.tensor([0, 999, 500])
    c = 0.1
    for mode in ("epsilon", "v_prediction"):
        got = L.loss_widths(L.parse_loss_type("huber:schedule=constant", mode), mode, ts)
        assert got.dtype == torch.float32 and got.tolist() == [np.float32(c)] * 3
        got = L.loss_widths(L.parse_loss_type("huber:schedule=exponential", mode), mode, ts)
        want = [1.0, math.exp(math.log(c) * 0.999), math.exp(math.log(c) * 0.5)]
        assert got.tolist() == [float(np.float32(v)) for v in want]
        got = L.loss_widths(L.parse_loss_type("smooth_l1:schedule=snr", mode), mode, ts)
        want = [(1 - c) / (1 + math.sqrt((1 - float(ac[t])) / float(ac[t]))) ** 2 + c for t in (0, 999, 500)]
        assert np.allclose(got.double().numpy(), want, rtol=2.0 ** -23, atol=0)
        assert c < got[1] < got[2] < got[0] < 1.0 and float(got[1]) - c < 5e-3          # sigma_999 ~ 14.6: 0.9 / 243 above c
    # rectified flow: tau = clamp((t + jitter) / 1000, 0, 1)
    ts, jit = torch.tensor([0, 999, 250]), torch.tensor([0.0, 1.0, 0.5])
    spec = L.parse_loss_type("huber:c=0.2", "rectified_flow")
    got = L.loss_widths(spec, "rectified_flow", ts, jit)
    assert got[0] == 1.0 and got[1] == np.float32(0.2)                              # tau = 0: sigma = 0 -> 1; tau = 1 -> c
    tau = 0.2505
    assert float(got[2]) == float(np.float32((1 - 0.2) / (1 + tau / (1 - tau)) ** 2 + 0.2))
    got = L.loss_widths(L.parse_loss_type("huber:c=0.2,schedule=exponential", "rectified_flow"), "rectified_flow", ts, jit)
    assert got[0] == 1.0 and got[1] == np.float32(0.2)
    assert L.loss_widths(L.parse_loss_type("huber:c=0.2,schedule=constant", "rectified_flow"), "rectified_flow", ts, None).tolist() == [float(np.float32(0.2))] * 3
    with pytest.raises(ValueError):
        L.loss_widths(spec, "rectified_flow", ts, None)
    with pytest.raises(ValueError):
        L.loss_widths(L.parse_loss_type("l1", "epsilon"), "epsilon", ts)
    # clamped: jitter past the range
    assert L.loss_widths(spec, "rectified_flow", torch.tensor([999]), torch.tensor([5.0]))[0] == np.float32(0.2)


# ---------------- min-SNR -------------------------------------------------------------------------------------------------------
def test_min_snr_table():
    ac = ddpm_alphas_cumprod().double()
    snr = ac / (1 - ac)
    g = 5.0
    m = L.min_snr_factors(g, "epsilon")
    assert m.dtype == torch.float64 and m.shape == (1000,)
    low = snr <= g
    assert bool(low.any()) and bool((~low).any())
    assert bool((m[low] == 1.0).all())
    assert torch.equal(m[~low], g / snr[~low]) or float(((m[~low] - g / snr[~low]).abs() / m[~low]).max()) < 2.0 ** -50
    mv = L.min_snr_factors(g, "v_prediction")
    want = torch.minimum(snr, torch.full_like(snr, g)) / (snr + 1.0)
    assert float(((mv - want).abs() / want).max()) < 2.0 ** -50
    assert bool((mv < 1.0).all()) and bool((mv[low] == (snr / (snr + 1.0))[low]).all())
    with pytest.raises(ValueError):
        L.min_snr_factors(g, "rectified_flow")
    # folded into the curve in float64, rounded to fp32 once; without the key the curve is the object itself
    curve = torch.linspace(0.5, 1.5, 1000)
    spec = L.parse_loss_type("mse:min_snr_gamma=5", "epsilon")
    assert torch.equal(L.fold_min_snr(curve, spec, "epsilon"), (curve.double() * m).float())
    assert L.fold_min_snr(curve, L.parse_loss_type("huber", "epsilon"), "epsilon") is curve
