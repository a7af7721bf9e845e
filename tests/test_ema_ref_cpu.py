"""The EMA of the weights without a GPU: the decay schedule's known answers (tests/ema_ref.py AND the package's host code), the
refusal of invalid decays, the error bound of the three-rounding update, and the trainer's option reader."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ema_ref as E        # noqa: E402

KNOWN = [  # (decay, k, warm-up, bits of omd)
    (0.999, 1, True, 0x3f51745d), (0.999, 2, True, 0x3f400000), (0.999, 90, True, 0x3db851ec), (0.999, 8989, True, 0x3a831629),
    (0.999, 8990, True, 0x3a83126f), (0.999, 8991, True, 0x3a83126f), (0.999, 10 ** 6, True, 0x3a83126f),
    (0.9999, 1, False, 0x38d1b717), (0.9999, 12345, False, 0x38d1b717)]


def _bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


@pytest.mark.parametrize("decay,k,warmup,want", KNOWN)
def test_decay_schedule_known_answers(decay, k, warmup, want):
    from aozora_sdxl_training_amd import ema
    assert E.omd_bits(decay, k, warmup) == want
    got = ema.one_minus_decay(decay, k, warmup)
    assert isinstance(got, float) and _bits(got) == want and float(np.float32(got)) == got      # already an fp32 value


def test_schedule_of_the_package_equals_the_restatement_over_many_steps():
    from aozora_sdxl_training_amd import ema
    for decay in (0.5, 0.9, 0.99, 0.999, 0.9999):
        for k in list(range(1, 200)) + [8989, 8990, 89989, 89990, 89991, 10 ** 7]:
            for w in (True, False):
                assert _bits(ema.one_minus_decay(decay, k, w)) == E.omd_bits(decay, k, w), (decay, k, w)


@pytest.mark.parametrize("bad", [0, 1, -0.1, 1.5, "x", None])
def test_invalid_decay_is_a_value_error(bad):
    from aozora_sdxl_training_amd import ema
    with pytest.raises(ValueError):
        E.check_decay(bad)
    with pytest.raises(ValueError):
        ema.check_decay(bad)
    with pytest.raises(ValueError):
        ema.EmaWeights(None, bad)                      # refused at construction, before the UNet is looked at
    with pytest.raises(ValueError):
        ema.read_options({"ema_decay": bad})


@pytest.mark.parametrize("omd", [1.0, 9.0 / 11.0, 1.0 - 0.999, 1.0 - 0.9999])
def test_restatement_stays_within_three_roundings_per_step(omd):
    """Constant bf16-representable target c, random start e0 (2^16 standard normals each): after K updates the fp32 restatement is
    within 3 K 2^-24 (|e0| + |c|) per element of the same recurrence in float64 with the same fp32 omd -- each of the three
    operations rounds a value of magnitude <= |e0| + |c| (the iterate stays between e0 and c) by at most 2^-24 relative."""
    rng = np.random.default_rng(7)
    n = 1 << 16
    e0 = rng.standard_normal(n).astype(np.float32)
    c = E.bf16_bits_to_f32((rng.standard_normal(n).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16))
    omd = np.float32(omd)
    e, ref = e0.copy(), e0.astype(np.float64)
    worst = {}
    for k in range(1, 401):
        e = E.ema_update(e, c, omd)
        ref = E.ema_update_f64(ref, c, omd)
        if k in (1, 64, 400):
            bound = 3.0 * k * 2.0 ** -24 * (np.abs(e0).astype(np.float64) + np.abs(c).astype(np.float64))
            err = np.abs(e.astype(np.float64) - ref)
            worst[k] = float((err / bound).max())
            print(f"omd={float(omd):.6g} K={k}: worst error / bound = {worst[k]:.3f}")
            assert bool((err <= bound).all()), (float(omd), k, worst[k])
    assert set(worst) == {1, 64, 400}


def test_update_is_the_three_operation_form():
    """One element by hand: the three roundings are visible (a fused or reordered form gives another last bit)."""
    e, p, omd = np.float32(1.0000001), np.float32(0.33203125), np.float32(1.0 - 0.999)
    t = np.float32(e - p); t = np.float32(omd * t); want = np.float32(e - t)
    assert E.ema_update(np.array([e]), np.array([p]), omd)[0] == want
    # IEEE propagation, no special case: e = inf gives inf - omd * inf = nan; omd == 1 with finite operands gives p up to rounding
    got = E.ema_update(np.array([np.inf, np.nan, 1.0, 2.0], np.float32), np.array([1.0, 1.0, np.nan, np.inf], np.float32), omd)
    assert np.isnan(got[:3]).all() and got[3] == np.inf
    assert E.ema_update(np.array([3.0], np.float32), np.array([-0.5], np.float32), np.float32(1.0))[0] == np.float32(-0.5)


def test_option_reader():
    from aozora_sdxl_training_amd.ema import read_options
    assert read_options(None) == (None, True) and read_options({}) == (None, True) and read_options({"betas": (0.9, 0.999)}) == (None, True)
    assert read_options({"ema_warmup": False}) == (None, True)                  # no decay: the option is off whatever else is set
    assert read_options({"ema_decay": 0.99}) == (0.99, True)
    assert read_options({"ema_decay": 0.5, "ema_warmup": False}) == (0.5, False)
    for s, want in (("true", True), ("True", True), ("1", True), ("yes", True), (" y ", True), ("false", False), ("0", False), ("no", False), ("", False)):
        assert read_options({"ema_decay": 0.9, "ema_warmup": s}) == (0.9, want), s
    assert read_options({"ema_decay": 0.9, "ema_warmup": 0}) == (0.9, False)
    for bad in (True, float("nan"), float("inf"), [0.9]):
        with pytest.raises(ValueError):
            read_options({"ema_decay": bad})
