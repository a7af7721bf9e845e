"""The stochastic-rounding option in the trainer's configuration (no GPU): absent means off, the seed is the run's SEED, and the 8-bit
optimizer refuses the key."""
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_preset_key_reaches_the_optimizer_keywords():
    from aozora_sdxl_training_amd import config as C
    from aozora_sdxl_training_amd.trainer import _sr_args
    cfg = types.SimpleNamespace(SEED=1234)
    assert "stochastic_rounding" not in C.flat_defaults()["RAVEN_PARAMS"] and "stochastic_rounding" not in C.flat_defaults()["TITAN_PARAMS"]
    assert _sr_args(cfg, dict(C.flat_defaults()["RAVEN_PARAMS"])) == dict(stochastic_rounding=False, sr_seed=1234)
    assert _sr_args(cfg, {"stochastic_rounding": True}) == dict(stochastic_rounding=True, sr_seed=1234)
    assert _sr_args(cfg, {"stochastic_rounding": "true"})["stochastic_rounding"] is True
    assert _sr_args(cfg, {"stochastic_rounding": "false"})["stochastic_rounding"] is False
    # a preset's dictionary reaches the flat configuration whole
    flat = C.flatten_preset({"active_mode": "sdxl", "sdxl": {"sdxl_raven_params": {"betas": [0.9, 0.999], "stochastic_rounding": True}}})
    assert flat["RAVEN_PARAMS"]["stochastic_rounding"] is True


def test_optimizer_classes_take_the_keywords():
    import inspect
    from aozora_sdxl_training_amd.dist import ShardedRaven
    from aozora_sdxl_training_amd.optimizers import RavenAdamW, TitanAdamW
    for cls in (RavenAdamW, TitanAdamW, ShardedRaven):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["stochastic_rounding"].default is False and sig["sr_seed"].default == 0, cls


def test_trainer_refuses_the_key_for_the_8bit_optimizer():
    from aozora_sdxl_training_amd.trainer import _optimizer_8bit
    cfg = types.SimpleNamespace(LR_CUSTOM_CURVE=[], LEARNING_RATE=1e-4, PAGED_ADAMW_8BIT_PARAMS={"stochastic_rounding": True})
    with pytest.raises(ValueError, match="stochastic_rounding is an option of raven and titan"):
        _optimizer_8bit(cfg, [])
