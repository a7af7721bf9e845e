"""ADAFACTOR_PARAMS: read from `<mode>_adafactor_params` of the preset's active block without a row in the key table (the flattened
preset stays key for key the reference's), default {}, kept out of as_dict(), and everything trainer.adafactor_options refuses -- on a
machine without a GPU."""
import json
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from aozora_sdxl_training_amd import config as C        # noqa: E402


def _preset(tmp_path, block, mode="sdxl"):
    p = tmp_path / "preset.json"
    p.write_text(json.dumps({"config_version": C.CONFIG_VERSION, "active_mode": mode, mode: block}))
    return str(p)


def test_adafactor_params_are_read_from_the_active_block(tmp_path, capsys):
    hp = {"scale_parameter": False, "relative_step": False, "warmup_init": False, "stochastic_rounding": True, "weight_decay": 0.01}
    cfg = C.TrainingConfig(["--config", _preset(tmp_path, {"sdxl_optimizer_type": "adafactor", "sdxl_adafactor_params": hp, "sdxl_batch_size": 3})])
    assert cfg.ADAFACTOR_PARAMS == hp and cfg.OPTIMIZER_TYPE == "adafactor" and cfg.BATCH_SIZE == 3 and cfg.PRODIGY_PARAMS == {}
    other = C.TrainingConfig(["--config", _preset(tmp_path, {"anima_adafactor_params": hp}, mode="anima")])
    assert other.ADAFACTOR_PARAMS == hp
    inactive = tmp_path / "inactive.json"
    inactive.write_text(json.dumps({"active_mode": "sdxl", "sdxl": {}, "anima": {"anima_adafactor_params": hp}}))
    assert C.TrainingConfig(["--config", str(inactive)]).ADAFACTOR_PARAMS == {}


def test_default_is_an_empty_dictionary(tmp_path, capsys):
    assert C.TrainingConfig([]).ADAFACTOR_PARAMS == {}
    assert C.TrainingConfig(["--config", _preset(tmp_path, {"sdxl_batch_size": 2})]).ADAFACTOR_PARAMS == {}
    assert C.TrainingConfig(["--config", _preset(tmp_path, {"sdxl_adafactor_params": "not a dictionary"})]).ADAFACTOR_PARAMS == {}
    assert C.TrainingConfig(["--config", "/nonexistent/preset.json"]).ADAFACTOR_PARAMS == {}


def test_flattened_preset_is_unchanged():
    hp = {"beta1": 0.9}
    assert all(name != "ADAFACTOR_PARAMS" for name, _, _, _ in C._TABLE)
    with_key = {"active_mode": "sdxl", "sdxl": {"sdxl_batch_size": 3, "sdxl_adafactor_params": hp}}
    without = {"active_mode": "sdxl", "sdxl": {"sdxl_batch_size": 3}}
    assert C.flatten_preset(with_key) == C.flatten_preset(without)
    assert "ADAFACTOR_PARAMS" not in C.flatten_preset(with_key) and "ADAFACTOR_PARAMS" not in C.flat_defaults()
    assert C.normalize_preset(with_key) == C.normalize_preset(without)
    assert "ADAFACTOR_PARAMS" not in C.TrainingConfig([]).as_dict()


def _cfg(**hp):
    return types.SimpleNamespace(OPTIMIZER_TYPE="adafactor", ADAFACTOR_PARAMS=hp, SEED=42)


def test_options_reach_the_optimizer_keywords():
    from aozora_sdxl_training_amd.trainer import adafactor_options
    assert adafactor_options(types.SimpleNamespace(OPTIMIZER_TYPE="adafactor")) == {"sr_seed": 0}
    assert adafactor_options(_cfg()) == {"sr_seed": 42}
    kw = adafactor_options(_cfg(eps=["1e-30", 1e-3], clip_threshold="0.5", decay_rate=-0.7, beta1=0.9, weight_decay=0.01, scale_parameter="true",
                                relative_step=True, warmup_init="yes", stochastic_rounding=True, ema_decay=0.999, ema_warmup=True))
    assert kw == dict(eps=(1e-30, 1e-3), clip_threshold=0.5, decay_rate=-0.7, beta1=0.9, weight_decay=0.01, scale_parameter=True, relative_step=True,
                      warmup_init=True, stochastic_rounding=True, sr_seed=42)
    assert adafactor_options(_cfg(beta1=None, scale_parameter=False, relative_step=False, warmup_init=False)) == dict(
        beta1=None, scale_parameter=False, relative_step=False, warmup_init=False, sr_seed=42)           # the customary recipe


@pytest.mark.parametrize("hp,world,match", [
    ({}, 2, "one rank only"),
    ({"param_groups": []}, 1, "param_groups is an option of raven, titan and paged_adamw_8bit"),
    ({"master_weights": True}, 1, "keeps no fp32 master copy"),
    ({"master_weights": False}, 1, "keeps no fp32 master copy"),
    ({"betas": [0.9, 0.99]}, 1, "unknown key"),
    ({"lr": 1e-6}, 1, "unknown key"),
    ({"sr_seed": 1}, 1, "unknown key"),
    ({"warmup_init": True}, 1, "warmup_init=True needs relative_step=True"),
    ({"clip_threshold": 0.0}, 1, "clip_threshold must be > 0"),
    ({"clip_threshold": -1}, 1, "clip_threshold must be > 0"),
    ({"beta1": 1.0}, 1, r"beta1 must lie in \[0, 1\)"),
    ({"beta1": -0.5}, 1, r"beta1 must lie in \[0, 1\)"),
    ({"decay_rate": 0.8}, 1, "decay_rate must be <= 0"),
    ({"weight_decay": -0.1}, 1, "weight_decay must be >= 0"),
    ({"eps": 1e-30}, 1, "cannot be read as a number"),
    ({"eps": [1e-30]}, 1, "cannot be read as a number"),
    ({"eps": [-1.0, 1e-3]}, 1, "eps must be two values >= 0"),
    ({"clip_threshold": "wide"}, 1, "cannot be read as a number"),
    ({"beta1": "momentum"}, 1, "cannot be read as a number"),
])
def test_refusals(hp, world, match):
    from aozora_sdxl_training_amd.trainer import adafactor_options
    with pytest.raises(ValueError, match=match):
        adafactor_options(_cfg(**hp), world)


def test_main_refuses_before_anything_runs(tmp_path, capsys, monkeypatch):
    """trainer.main prints the refusal and returns 2 -- for a bad ADAFACTOR_PARAMS and for more than one rank."""
    from aozora_sdxl_training_amd import trainer
    bad = _preset(tmp_path, {"sdxl_optimizer_type": "adafactor", "sdxl_adafactor_params": {"warmup_init": True}})
    assert trainer.main(["--config", bad]) == 2
    assert "warmup_init=True needs relative_step=True" in capsys.readouterr().out
    ok = _preset(tmp_path, {"sdxl_optimizer_type": "adafactor", "sdxl_adafactor_params": {}})
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert trainer.main(["--config", ok]) == 2
    assert "one rank only" in capsys.readouterr().out
