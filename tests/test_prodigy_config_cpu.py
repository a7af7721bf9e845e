"""PRODIGY_PARAMS: read from `<mode>_prodigy_params` of the preset's active block without a row in the key table (the flattened preset
stays key for key the reference's), default {}, and everything trainer.prodigy_options refuses -- on a machine without a GPU."""
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


def test_prodigy_params_are_read_from_the_active_block(tmp_path, capsys):
    hp = {"d_coef": 2.0, "weight_decay": 0.01, "safeguard_warmup": True, "betas": [0.9, 0.99]}
    cfg = C.TrainingConfig(["--config", _preset(tmp_path, {"sdxl_optimizer_type": "prodigy", "sdxl_prodigy_params": hp, "sdxl_batch_size": 3})])
    assert cfg.PRODIGY_PARAMS == hp and cfg.OPTIMIZER_TYPE == "prodigy" and cfg.BATCH_SIZE == 3
    # the other mode's block is not the active one
    other = C.TrainingConfig(["--config", _preset(tmp_path, {"anima_prodigy_params": hp}, mode="anima")])
    assert other.PRODIGY_PARAMS == hp
    inactive = tmp_path / "inactive.json"
    inactive.write_text(json.dumps({"active_mode": "sdxl", "sdxl": {}, "anima": {"anima_prodigy_params": hp}}))
    assert C.TrainingConfig(["--config", str(inactive)]).PRODIGY_PARAMS == {}


def test_default_is_an_empty_dictionary(tmp_path, capsys):
    assert C.TrainingConfig([]).PRODIGY_PARAMS == {}
    assert C.TrainingConfig(["--config", _preset(tmp_path, {"sdxl_batch_size": 2})]).PRODIGY_PARAMS == {}
    assert C.TrainingConfig(["--config", _preset(tmp_path, {"sdxl_prodigy_params": "not a dictionary"})]).PRODIGY_PARAMS == {}
    assert C.TrainingConfig(["--config", "/nonexistent/preset.json"]).PRODIGY_PARAMS == {}


def test_flattened_preset_is_unchanged():
    hp = {"d_coef": 2.0}
    assert all(name != "PRODIGY_PARAMS" for name, _, _, _ in C._TABLE)
    with_key = {"active_mode": "sdxl", "sdxl": {"sdxl_batch_size": 3, "sdxl_prodigy_params": hp}}
    without = {"active_mode": "sdxl", "sdxl": {"sdxl_batch_size": 3}}
    assert C.flatten_preset(with_key) == C.flatten_preset(without)
    assert "PRODIGY_PARAMS" not in C.flatten_preset(with_key) and "PRODIGY_PARAMS" not in C.flat_defaults()
    assert C.normalize_preset(with_key) == C.normalize_preset(without)
    assert "PRODIGY_PARAMS" not in C.TrainingConfig([]).as_dict()


def _cfg(**hp):
    return types.SimpleNamespace(OPTIMIZER_TYPE="prodigy", PRODIGY_PARAMS=hp)


def test_options_reach_the_optimizer_keywords():
    from aozora_sdxl_training_amd.trainer import prodigy_options
    assert prodigy_options(types.SimpleNamespace(OPTIMIZER_TYPE="prodigy")) == {}
    assert prodigy_options(_cfg()) == {}
    kw = prodigy_options(_cfg(betas=[0.9, 0.99], beta3=0.95, eps="1e-9", weight_decay=0.01, use_bias_correction="true", safeguard_warmup=False,
                              d0=1e-5, d_coef=2, growth_rate=1.02, ema_decay=0.999, ema_warmup=True))
    assert kw == dict(betas=(0.9, 0.99), beta3=0.95, eps=1e-9, weight_decay=0.01, use_bias_correction=True, safeguard_warmup=False, d0=1e-5,
                      d_coef=2.0, growth_rate=1.02)


@pytest.mark.parametrize("hp,world,match", [
    ({}, 2, "one rank only"),
    ({"stochastic_rounding": True}, 1, "stochastic_rounding is an option of raven and titan"),
    ({"stochastic_rounding": False}, 1, "stochastic_rounding is an option of raven and titan"),
    ({"master_weights": True}, 1, "master_weights is an option of raven and titan"),
    ({"param_groups": []}, 1, "param_groups is an option of raven, titan and paged_adamw_8bit"),
    ({"debias_strength": 0.3}, 1, "unknown key"),
    ({"lr": 1.0}, 1, "unknown key"),
    ({"eps": 0.0}, 1, "eps must be > 0"),
    ({"eps": -1e-8}, 1, "eps must be > 0"),
    ({"d0": 0.0}, 1, "d0 must be > 0"),
    ({"d0": -1e-6}, 1, "d0 must be > 0"),
    ({"betas": [1.0, 0.999]}, 1, r"betas must lie in \[0, 1\)"),
    ({"betas": [0.9, -0.1]}, 1, r"betas must lie in \[0, 1\)"),
    ({"betas": [0.9]}, 1, r"betas must lie in \[0, 1\)"),
    ({"beta3": 1.0}, 1, r"beta3 must lie in \[0, 1\)"),
    ({"eps": "tiny"}, 1, "cannot be read as a number"),
])
def test_refusals(hp, world, match):
    from aozora_sdxl_training_amd.trainer import prodigy_options
    with pytest.raises(ValueError, match=match):
        prodigy_options(_cfg(**hp), world)


def test_main_refuses_before_anything_runs(tmp_path, capsys, monkeypatch):
    """trainer.main prints the refusal and returns 2 -- for a bad PRODIGY_PARAMS and for more than one rank."""
    from aozora_sdxl_training_amd import trainer
    bad = _preset(tmp_path, {"sdxl_optimizer_type": "prodigy", "sdxl_prodigy_params": {"eps": 0}})
    assert trainer.main(["--config", bad]) == 2
    assert "eps must be > 0" in capsys.readouterr().out
    ok = _preset(tmp_path, {"sdxl_optimizer_type": "prodigy", "sdxl_prodigy_params": {}})
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert trainer.main(["--config", ok]) == 2
    assert "one rank only" in capsys.readouterr().out
