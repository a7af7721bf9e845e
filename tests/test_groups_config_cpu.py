"""The "param_groups" option without a GPU: the rules (param_groups.parse_rules / option), the resolver on a fake slot table
(first match wins, schedule.trainable_mask's keyword reading, equal groups merge, padding belongs to its slot, frozen slots are ignored),
every refusal, the host arithmetic of the per-group table, a nested GUI preset reaching TrainingConfig whole, the trainer's torch groups
for the 8-bit optimizer and main()'s exit status."""
import json
import math
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from aozora_sdxl_training_amd import param_groups as PG      # noqa: E402

#        name                              offset  elements   (slots are padded to 64: the next one starts on a multiple of it)
SLOTS = [("conv_in.weight",                     0,     100),
         ("conv_in.bias",                     128,      10),
         ("down_blocks.0.norm1.weight",       192,      64),
         ("down_blocks.0.conv1.weight",       256,      65),
         ("down_blocks.1.conv1.weight",       384,     128),
         ("mid_block.attn.to_q.weight",       512,      64),
         ("mid_block.attn.to_q.bias",         576,       3),
         ("conv_out.weight",                  640,     200)]
ALL = [True] * len(SLOTS)
RULES = [{"match": "bias, norm", "weight_decay": 0.0}, {"match": ["down_blocks.0.*", "conv_in"], "lr_scale": 0.25}]


def resolve(rules, trainable=ALL, base=0.01, flat=4096):
    return PG.resolve(SLOTS, trainable, PG.parse_rules(rules, base), base, flat)


def test_first_match_wins_and_the_table_covers_the_flat_buffer():
    r = resolve(RULES)
    assert r.groups == [(1.0, 0.01), (1.0, 0.0), (0.25, 0.01)]                 # group 0 is the base
    assert r.param_gid == {"conv_in.weight": 2, "conv_in.bias": 1, "down_blocks.0.norm1.weight": 1, "down_blocks.0.conv1.weight": 2,
                           "down_blocks.1.conv1.weight": 0, "mid_block.attn.to_q.weight": 0, "mid_block.attn.to_q.bias": 1, "conv_out.weight": 0}
    # conv_in.bias matches both rules: the first one takes it.  Adjacent slots of one group merge; padding stays with its slot
    # (conv_in.weight: 100 elements, its segment ends at 128; to_q.bias: 3 elements, its segment ends at 640); the last end is flat_numel
    assert r.seg_end == [128, 256, 384, 576, 640, 4096] and r.seg_gid == [2, 1, 2, 0, 1, 0]
    assert all(e % PG.ALIGN == 0 for e in r.seg_end)
    assert r.counts == [(3, 392), (3, 77), (2, 165)]
    assert len(PG.describe(r)) == 3 and "lr_scale 0.25" in PG.describe(r)[2] and "(base)" in PG.describe(r)[0]


def test_keywords_read_as_the_freeze_mask_reads_them():
    from aozora_sdxl_training_amd.schedule import trainable_mask
    names = [s[0] for s in SLOTS]
    for kws in (["bias"], ["down_blocks.0.*"], ["down_blocks.0"], ["*.weight"], ["conv"], ["mid_block.attn.to_q.bias"], ["*mid*", "conv_out"]):
        assert [PG.matches(n, kws) for n in names] == [not t for t in trainable_mask(names, kws)], kws
    assert not PG.matches("x.down_blocks.0.conv1.weight", ["down_blocks.0.*"]) and PG.matches("x.down_blocks.0.conv1.weight", ["down_blocks.0"])
    # a string and a list are the same rule; blanks around keywords do not count
    assert PG.parse_rules([{"match": " bias ,norm, "}], 0.01) == PG.parse_rules([{"match": ["bias", "norm"]}], 0.01)


def test_equal_groups_merge_and_a_neutral_list_is_one_group():
    r = resolve([{"match": "bias", "weight_decay": 0.0}, {"match": "norm", "weight_decay": 0.0, "lr_scale": 1.0}, {"match": "conv_out", "lr_scale": 1}])
    assert r.groups == [(1.0, 0.01), (1.0, 0.0)]                               # rules 0 and 1 share a group, rule 2 is the base
    assert r.param_gid["conv_out.weight"] == 0 and r.param_gid["down_blocks.0.norm1.weight"] == 1
    n = resolve([{"match": "bias, norm", "weight_decay": 0.01}, {"match": "conv_in", "lr_scale": 1.0}, {"match": "mid_block"}])
    assert n.groups == [(1.0, 0.01)] and n.seg_end == [4096] and n.seg_gid == [0] and n.counts == [(8, 634)]
    # weight_decay defaults to the dictionary's own value and is absolute
    assert PG.parse_rules([{"match": "x", "lr_scale": 2}], 0.05) == [PG.Rule(("x",), 2.0, 0.05)]
    off = PG.resolve(SLOTS, ALL, [], 0.01, 4096)
    assert off.groups == [(1.0, 0.01)] and off.seg_gid == [0]
    assert PG.parse_rules(None, 0.01) == [] and PG.parse_rules([], 0.01) == []


def test_frozen_parameters_are_ignored():
    tr = [n not in ("conv_in.bias", "down_blocks.0.norm1.weight") for n, _, _ in SLOTS]
    r = resolve(RULES, tr)
    assert "conv_in.bias" not in r.param_gid and r.counts[1] == (1, 3)
    assert r.seg_end == [384, 576, 640, 4096] and r.seg_gid == [2, 0, 1, 0]      # the frozen slots ride with the segment in front of them
    with pytest.raises(ValueError, match="matches no trainable parameter"):      # every "norm" parameter is frozen now
        resolve([{"match": "norm", "weight_decay": 0.0}], tr)
    assert resolve([{"match": "bias", "lr_scale": 0.5}, {"match": "to_q.bias", "lr_scale": 0.1}]).param_gid["mid_block.attn.to_q.bias"] == 1   # shadowed: legal


@pytest.mark.parametrize("spec,msg", [
    ({"match": "bias"}, "list of dictionaries"), ("bias", "list of dictionaries"), ([["bias"]], "list of dictionaries"), ([None], "list of dictionaries"),
    ([{"match": "bias", "betas": [0.9, 0.99]}], "unknown key"), ([{"match": "bias", "lr": 1e-4}], "unknown key"),
    ([{"weight_decay": 0.0}], "missing or empty"), ([{"match": ""}], "missing or empty"), ([{"match": " , "}], "missing or empty"), ([{"match": []}], "missing or empty"),
    ([{"match": 3}], "comma-separated string or a list"), ([{"match": ["bias", 3]}], "comma-separated string or a list"),
    ([{"match": "bias", "lr_scale": True}], "must be a number"), ([{"match": "bias", "weight_decay": False}], "must be a number"),
    ([{"match": "bias", "lr_scale": "0.5"}], "must be a number"), ([{"match": "bias", "weight_decay": None}], "must be a number"),
    ([{"match": "bias", "lr_scale": float("nan")}], "finite and >= 0"), ([{"match": "bias", "weight_decay": float("inf")}], "finite and >= 0"),
    ([{"match": "bias", "lr_scale": -0.5}], "finite and >= 0"), ([{"match": "bias", "weight_decay": -1e-9}], "finite and >= 0"),
    ([{"match": "bias", "weight_decay": 0.0}, {"match": "biass", "lr_scale": 0.5}], "matches no trainable parameter")])
def test_refusals(spec, msg):
    with pytest.raises(ValueError, match=msg):
        resolve(spec)


def test_more_than_255_groups_are_refused():
    many = [{"match": "conv", "lr_scale": 1.0 + k} for k in range(1, 255)]
    assert len(resolve(many).groups) == 255
    with pytest.raises(ValueError, match="at most 255"):
        resolve(many + [{"match": "conv", "lr_scale": 0.5}])


def test_option_reads_the_active_dictionary_and_refuses_the_host_paths():
    pg = [{"match": "bias", "weight_decay": 0.0}]
    cfg = lambda **kw: types.SimpleNamespace(**kw)
    assert PG.option(cfg(OPTIMIZER_TYPE="raven", RAVEN_PARAMS={"weight_decay": 0.02})) == []
    assert PG.option(cfg(OPTIMIZER_TYPE="raven", RAVEN_PARAMS={"param_groups": []})) == []
    assert PG.option(cfg(OPTIMIZER_TYPE="raven", RAVEN_PARAMS=None)) == []
    assert PG.option(cfg(OPTIMIZER_TYPE="raven", RAVEN_PARAMS={"param_groups": pg}, TITAN_PARAMS={"param_groups": "junk"})) == [PG.Rule(("bias",), 1.0, 0.0)]
    assert PG.option(cfg(OPTIMIZER_TYPE="titan", RAVEN_PARAMS={"param_groups": "junk"}, TITAN_PARAMS={"weight_decay": 0.5, "param_groups": [{"match": "norm"}]})) == [PG.Rule(("norm",), 1.0, 0.5)]
    assert PG.option(cfg(OPTIMIZER_TYPE="paged_adamw_8bit", PAGED_ADAMW_8BIT_PARAMS={"param_groups": pg})) == [PG.Rule(("bias",), 1.0, 0.0)]
    for bad in (cfg(OPTIMIZER_TYPE="titan", TITAN_PARAMS={"param_groups": pg}, TITAN_HOST_GRADIENTS=True),
                cfg(OPTIMIZER_TYPE="raven", RAVEN_PARAMS={"param_groups": pg}, RAVEN_STATE_ON_HOST=True),
                cfg(OPTIMIZER_TYPE="titan", TITAN_PARAMS={"param_groups": pg}, RAVEN_STATE_ON_HOST=True)):
        with pytest.raises(ValueError, match="pinned-host memory.*no segmented form of the chunk pipeline"):
            PG.option(bad)
    # off: the host paths stay available
    assert PG.option(cfg(OPTIMIZER_TYPE="titan", TITAN_PARAMS={}, TITAN_HOST_GRADIENTS=True, RAVEN_STATE_ON_HOST=True)) == []
    with pytest.raises(ValueError, match="list of dictionaries"):
        PG.option(cfg(OPTIMIZER_TYPE="raven", RAVEN_PARAMS={"param_groups": {"match": "bias"}}))


def test_group_hyper_rows_are_the_single_group_arithmetic():
    """wd_factor and step_size per group exactly as dist.ShardedRaven._hyper forms them for its one group."""
    lr, b1, deb, t = 3e-5, 0.9, 0.3, 7
    bc1 = 1.0 - b1 ** t
    bc1 = 1.0 - (1.0 - bc1) * deb
    rows = PG.ghyper_rows([(1.0, 0.01), (0.25, 0.0), (0.0, 0.0), (2.0, 0.1)], lr, bc1)
    assert rows[0] == [1.0 - lr * 0.01, lr / bc1]
    assert rows[1] == [1.0, (lr * 0.25) / bc1]
    assert rows[2] == [1.0, 0.0]
    assert rows[3] == [1.0 - (lr * 2.0) * 0.1, (lr * 2.0) / bc1]


def test_a_nested_gui_preset_reaches_training_config_whole(tmp_path):
    from aozora_sdxl_training_amd import config as C
    preset = {"active_mode": "sdxl", "sdxl": {"sdxl_raven_params": {"betas": [0.9, 0.999], "weight_decay": 0.02, "param_groups": RULES}}}
    flat = C.flatten_preset(preset)
    assert flat["RAVEN_PARAMS"]["param_groups"] == RULES
    p = tmp_path / "preset.json"
    p.write_text(json.dumps(preset))
    c = C.TrainingConfig(["--config", str(p)])
    assert c.RAVEN_PARAMS["param_groups"] == RULES and c.RAVEN_PARAMS["weight_decay"] == 0.02
    assert PG.option(c) == [PG.Rule(("bias", "norm"), 1.0, 0.0), PG.Rule(("down_blocks.0.*", "conv_in"), 0.25, 0.02)]
    assert "param_groups" not in C.flat_defaults()["RAVEN_PARAMS"] and "param_groups" not in C.flat_defaults()["PAGED_ADAMW_8BIT_PARAMS"]


def test_main_turns_a_refusal_into_an_error_line(tmp_path, capsys):
    from aozora_sdxl_training_amd.trainer import main
    for params in ({"param_groups": [{"match": "bias", "lr_scale": -1}]}, {"param_groups": [{"match": "bias", "decay": 0}]}):
        p = tmp_path / "preset.json"
        p.write_text(json.dumps({"active_mode": "sdxl", "sdxl": {"sdxl_raven_params": params}}))
        assert main(["--config", str(p)]) == 2
        out = capsys.readouterr().out
        assert "ERROR: param_groups[0]" in out


def test_train_refuses_before_anything_is_loaded(tmp_path, monkeypatch):
    from aozora_sdxl_training_amd import checkpoint as C
    from aozora_sdxl_training_amd import trainer

    def no_load(*a, **k):
        raise AssertionError("a UNet was loaded")
    monkeypatch.setattr(C, "load_unet", no_load)
    for over, msg in ((dict(RAVEN_PARAMS={"param_groups": [{"match": "bias", "weight_decay": -1}]}), "finite and >= 0"),
                      (dict(RAVEN_PARAMS={"param_groups": [{"match": "bias"}]}, RAVEN_STATE_ON_HOST=True), "RAVEN_STATE_ON_HOST"),
                      (dict(OPTIMIZER_TYPE="titan", TITAN_PARAMS={"param_groups": [{"match": "bias"}]}, TITAN_HOST_GRADIENTS=True), "TITAN_HOST_GRADIENTS")):
        cfg = types.SimpleNamespace(**{**dict(OPTIMIZER_TYPE="raven", RAVEN_PARAMS={}, GRADIENT_ACCUMULATION_STEPS=2, PREDICTION_TYPE="epsilon",
                                              SINGLE_FILE_CHECKPOINT_PATH=str(tmp_path / "none.safetensors"), SEED=1), **over})
        with pytest.raises(ValueError, match=msg):
            trainer.train(cfg, unet=None, device="cpu")


def test_optimizer_classes_take_the_keyword():
    import inspect
    from aozora_sdxl_training_amd import ops
    from aozora_sdxl_training_amd.dist import ShardedRaven
    assert inspect.signature(ShardedRaven.__init__).parameters["groups"].default is None
    assert inspect.signature(ops.adamw_range).parameters["groups"].default is None
    assert math.isfinite(PG.MAX_GROUPS)
