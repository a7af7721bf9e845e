"""The fp32-master-weights option without a GPU: the numpy restatement tests/master_ref.py (its first step is the default update's, the
drift experiment follows sr_ref.drift_master bit for bit while round to nearest never moves), and the option in the trainer's
configuration (absent means off, the three combinations it refuses)."""
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import elem_ref as R        # noqa: E402
import master_ref as M      # noqa: E402
import sr_ref as S          # noqa: E402

HYPER = dict(lr=1e-3, betas=(0.9, 0.999), wd=0.01, eps=1e-8, debias=0.3)


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.dtype, b.dtype)
    eq = (bits(a) == bits(b)) | (a.isnan() & b.isnan())
    assert bool(eq.all()), f"{what}: {int((~eq).sum())} of {eq.numel()} elements differ"


# ---------------- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mdtype", [0, 1, 2])
@pytest.mark.parametrize("f32_grads", [False, True])
@pytest.mark.parametrize("coef", [None, 0.37])
def test_first_step_from_w_equal_float_p_is_the_default_step(mdtype, f32_grads, coef):
    n = 4099
    p = R.gauss_bf16((n,), seed=5, scale=0.1)
    g = R.adamw_grads(n, 6, f32_grads)
    gen = R.gen(7)
    m = (1e-3 * torch.randn(n, generator=gen)).to(R.moment_dtype(mdtype))
    v = (1e-4 * torch.rand(n, generator=gen)).to(R.moment_dtype(mdtype))
    hyper = R.adamw_hyper(step=1, **HYPER)
    p1, w1, m1, v1 = M.adamw_master_bits(p.float(), g, m, v, hyper, coef)
    pd, md, vd = R.adamw_bits(p, g, m, v, hyper, coef)
    same(p1, pd, "p"); same(m1, md, "m"); same(v1, vd, "v")
    assert w1.dtype == torch.float32
    same(R.f32_to_bf16_bits(w1), p1, "p against bf16(w)")
    # the second step differs from the default's somewhere: the master kept what the bf16 write discarded
    g2 = R.adamw_grads(n, 8, f32_grads)
    hyper2 = R.adamw_hyper(step=2, **HYPER)
    p2 = M.adamw_master_bits(w1, g2, m1, v1, hyper2, coef)[0]
    pd2 = R.adamw_bits(pd, g2, md, vd, hyper2, coef)[0]
    assert int((bits(p2) != bits(pd2)).sum()) > 0


def test_nan_and_inf_go_through_both_outputs():
    w = torch.tensor([1.0, 2.0, 3.0, 4.0, float("inf"), float("nan")])
    g = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, 0.0, 0.0])
    z = torch.zeros(6)
    p1, w1, m1, v1 = M.adamw_master_bits(w, g, z, z.clone(), R.adamw_hyper(step=1, **HYPER))
    assert bool(w1[:3].isnan().all()) and bool(p1[:3].isnan().all())          # nan; inf / inf; -inf / inf
    assert float(w1[3]) == float(np.float32(4.0) * R.adamw_hyper(step=1, **HYPER)[4]) and bool(w1[4].isinf()) and bool(p1[4].isinf()) and bool(w1[5].isnan())


def test_drift_master_follows_while_round_to_nearest_never_moves():
    d = S.DRIFT
    n = d["n"]
    g = torch.full((n,), d["g"], dtype=torch.float32)
    w = torch.full((n,), d["p0"], dtype=torch.float32)
    m, v = torch.zeros(n), torch.zeros(n)
    p_rn = torch.full((n,), d["p0"], dtype=torch.bfloat16)
    m_rn, v_rn = torch.zeros(n), torch.zeros(n)
    for s in range(1, d["steps"] + 1):
        p, w, m, v = M.adamw_master_bits(w, g, m, v, S.drift_hyper(s))
        p_rn, m_rn, v_rn = R.adamw_bits(p_rn, g, m_rn, v_rn, S.drift_hyper(s))
    master = S.drift_master()
    assert w.numpy().view(np.uint32).tolist() == [int(np.array([master], dtype=np.float32).view(np.uint32)[0])] * n     # bit for bit, every element
    same(p, R.f32_to_bf16_bits(w), "p == bf16(w)")
    assert bool((p.float() == d["p0"] - 2 * S.DRIFT_ULP).all())                # p0 - 2 bf16 ulp ...
    assert abs((master - d["p0"]) / S.DRIFT_ULP - (-1.955)) < 0.002             # ... for a master that moved -1.955 ulp
    assert bool((p_rn.float() == d["p0"]).all())                                # round to nearest without a master: still p0


# ---------------- configuration --------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    return types.SimpleNamespace(**kw)


def test_key_absent_or_false_is_off_and_true_is_on():
    from aozora_sdxl_training_amd import config as C
    from aozora_sdxl_training_amd.trainer import _master_option
    assert "master_weights" not in C.flat_defaults()["RAVEN_PARAMS"] and "master_weights" not in C.flat_defaults()["TITAN_PARAMS"]
    for kind, key in (("raven", "RAVEN_PARAMS"), ("titan", "TITAN_PARAMS")):
        assert _master_option(_cfg(OPTIMIZER_TYPE=kind, **{key: dict(C.flat_defaults()[key])})) is False
        assert _master_option(_cfg(OPTIMIZER_TYPE=kind)) is False
        assert _master_option(_cfg(OPTIMIZER_TYPE=kind, **{key: {"master_weights": False}})) is False
        assert _master_option(_cfg(OPTIMIZER_TYPE=kind, **{key: {"master_weights": "false"}})) is False
        assert _master_option(_cfg(OPTIMIZER_TYPE=kind, **{key: {"master_weights": True}})) is True
        assert _master_option(_cfg(OPTIMIZER_TYPE=kind, **{key: {"master_weights": "true"}})) is True
        assert _master_option(_cfg(OPTIMIZER_TYPE=kind, TITAN_HOST_GRADIENTS=False, **{key: {"master_weights": True, "stochastic_rounding": False}})) is True
    assert _master_option(_cfg(OPTIMIZER_TYPE="paged_adamw_8bit", PAGED_ADAMW_8BIT_PARAMS={"betas": [0.9, 0.999]})) is False
    # the key of the OTHER optimizer's dictionary is not read
    assert _master_option(_cfg(OPTIMIZER_TYPE="raven", RAVEN_PARAMS={}, TITAN_PARAMS={"master_weights": True})) is False
    flat = C.flatten_preset({"active_mode": "sdxl", "sdxl": {"sdxl_raven_params": {"betas": [0.9, 0.999], "master_weights": True}}})
    assert flat["RAVEN_PARAMS"]["master_weights"] is True


def test_the_three_refusals():
    from aozora_sdxl_training_amd.trainer import _master_option, _optimizer_8bit
    with pytest.raises(ValueError, match="master_weights is an option of raven and titan"):
        _master_option(_cfg(OPTIMIZER_TYPE="paged_adamw_8bit", PAGED_ADAMW_8BIT_PARAMS={"master_weights": True}))
    with pytest.raises(ValueError, match="master_weights is an option of raven and titan"):
        _optimizer_8bit(_cfg(LR_CUSTOM_CURVE=[], LEARNING_RATE=1e-4, PAGED_ADAMW_8BIT_PARAMS={"master_weights": True}), [])
    for kind, key in (("raven", "RAVEN_PARAMS"), ("titan", "TITAN_PARAMS")):
        with pytest.raises(ValueError, match="master_weights and stochastic_rounding do not combine"):
            _master_option(_cfg(OPTIMIZER_TYPE=kind, **{key: {"master_weights": True, "stochastic_rounding": True}}))
    with pytest.raises(ValueError, match="TITAN_HOST_GRADIENTS"):
        _master_option(_cfg(OPTIMIZER_TYPE="titan", TITAN_HOST_GRADIENTS=True, TITAN_PARAMS={"master_weights": True}))
    # host gradients without the key, and the key under raven with the (unused) Titan switch set: fine
    assert _master_option(_cfg(OPTIMIZER_TYPE="titan", TITAN_HOST_GRADIENTS=True, TITAN_PARAMS={})) is False
    assert _master_option(_cfg(OPTIMIZER_TYPE="raven", TITAN_HOST_GRADIENTS=True, RAVEN_PARAMS={"master_weights": True})) is True


def test_optimizer_keyword_and_its_refusal_before_anything_is_touched():
    from aozora_sdxl_training_amd.dist import ShardedRaven, ShardedTitan
    assert inspect.signature(ShardedRaven.__init__).parameters["master_weights"].default is False
    for cls in (ShardedRaven, ShardedTitan):
        with pytest.raises(ValueError, match="master_weights and stochastic_rounding do not combine"):
            cls(None, master_weights=True, stochastic_rounding=True)         # (no UNet: the refusal comes before anything reads it)


def test_entry_point_is_declared_with_its_citation_and_wrapped():
    from aozora_sdxl_training_amd import _lib as L, ops, tape
    ret, args = L.parse_header()["az_adamw_flat_master"]
    assert ret == "int" and [a for _, a in args] == ["n", "p", "w_f32", "g", "gdtype", "m", "v", "mdtype", "hyper", "coef", "stream"]
    above = open(L.HEADER).read().split("int az_adamw_flat_master(")[0]
    assert above.rstrip().endswith("*/") and above[above.rindex("/*"):].startswith("/* ref: raven.py:109-147")
    assert "az_adamw_flat_master" in tape._KERNEL_ENTRIES and callable(ops.adamw_flat_master)
