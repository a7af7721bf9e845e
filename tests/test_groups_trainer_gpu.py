"""The "param_groups" option through trainer.train on the synthetic cache: a block given lr_scale 0 and weight_decay 0 comes back bit for
bit while every other trainable parameter moves (wd_factor 1, step_size 0: p + (-0 * m) / denom = p -- the test that fails without the
option, which trains every parameter alike); weight_decay 0 on "bias, norm" leaves the first update of every other weight untouched and
changes later ones only through the gradients; a neutral list changes nothing; the reported learning rate stays the curve's; a resumed
run ends bitwise like the uninterrupted one and the training state holds nothing of the option; the 8-bit optimizer gets its torch
groups; the refusals surface through train() and main().  (The helpers are those of tests/test_ema_trainer_gpu.py.)"""
import json
import gc
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import test_ema_trainer_gpu as T        # noqa: E402

pytestmark = pytest.mark.gpu
DEV, MODE = T.DEV, T.MODE
# a learning rate at which one update is several bf16 spacings of a weight of magnitude 1 (the norm scales): lr / bc1 * m / denom is about
# 3.7 lr on the first step (debias_strength 0.3), the spacing below 1.0 is 2^-8
CURVE = [[0.0, 4e-3], [1.0, 1e-3]]
RAVEN = dict(T.RAVEN)
FROZEN = [{"match": "mid_block", "lr_scale": 0.0, "weight_decay": 0.0}]
STATE_KEYS = {"global_step", "micro_step", "optimizer_state", "sampler_seed", "sampler_epoch", "timestep_sampler_state", "random_state",
              "numpy_state", "torch_cpu_state", "torch_cuda_state"}


@pytest.fixture(autouse=True)
def _collect_cycles():
    """Optimizers and UNets sit in reference cycles that hold device objects: they are collected here, when the test that made them
    ends, not by whichever later test happens to trigger the collector."""
    yield
    gc.collect()


def _run(tmp, **over):
    cfg = T._config(tmp, MODE, **{"LR_CUSTOM_CURVE": CURVE, "RAVEN_PARAMS": dict(RAVEN), **over})
    if not os.path.exists(cfg.SINGLE_FILE_CHECKPOINT_PATH):
        T._base_checkpoint(cfg.SINGLE_FILE_CHECKPOINT_PATH, T._model())
    unet, h, out = T._train(cfg, cfg.RESUME_MODEL_PATH if cfg.RESUME_TRAINING else cfg.SINGLE_FILE_CHECKPOINT_PATH)
    return cfg, unet, h, out


def _params(unet):
    return {n: p.detach().clone() for n, p in unet.named_parameters()}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The initial parameters, the default run and the run with the mid block frozen by its group, 8 micro-steps = 4 optimizer steps."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import types
    from aozora_sdxl_training_amd import checkpoint as C
    tmp = str(tmp_path_factory.mktemp("groups_trainer"))
    cfg0, unet0, h0, out0 = _run(tmp, OUTPUT_DIR=os.path.join(tmp, "out_default"))
    start = _params(C.load_unet(cfg0.SINGLE_FILE_CHECKPOINT_PATH, DEV, T._model()))
    cfg, unet, h, out = _run(tmp, RAVEN_PARAMS=dict(RAVEN, param_groups=FROZEN))
    trainable = {n for n, p in unet.named_parameters() if p.requires_grad}
    return types.SimpleNamespace(tmp=tmp, start=start, trainable=trainable, cfg0=cfg0, h0=h0, out0=out0, p0=_params(unet0), pflat0=unet0.pflat.clone(),
                                 cfg=cfg, h=h, out=out, p=_params(unet), pflat=unet.pflat.clone())


def test_a_group_with_zero_rate_and_decay_comes_back_bit_for_bit_and_the_rest_moves(runs):
    r = runs
    assert r.h["micro_step"] == 8 and r.h["optimizer_step"] == 4 and all(l == l for l in r.h["losses"])
    frozen = sorted(n for n in r.trainable if "mid_block" in n)
    others = sorted(n for n in r.trainable if "mid_block" not in n)
    assert len(frozen) > 10 and len(others) > 100 and len(r.trainable) < len(r.start)             # (conv1 / conv2 are frozen by the mask)
    changed = [n for n in frozen if not torch.equal(r.p[n], r.start[n])]
    still = [n for n in others if torch.equal(r.p[n], r.start[n])]
    print(f"frozen-by-group parameters that changed: {changed}; other trainable parameters that did not move: {still}")
    assert not changed, changed
    assert not still, still
    # the default run (the parent's behaviour) moves the block
    assert all(not torch.equal(r.p0[n], r.start[n]) for n in frozen)
    for n in r.start:
        if n not in r.trainable:
            assert torch.equal(r.p[n], r.start[n]), n


def test_info_lines_and_the_reported_learning_rate(runs):
    r = runs
    assert r.out.count("INFO: parameter groups are ON") == 1 and "an option outside the reference" in r.out
    lines = [l for l in r.out.splitlines() if l.startswith("INFO: parameter group ")]
    assert len(lines) == 2 and "(base)" in lines[0] and "lr_scale 0.0, weight_decay 0.0" in lines[1]
    n_frozen = sum(1 for n in r.trainable if "mid_block" in n)
    assert f": {n_frozen} parameters, " in lines[1] and f": {len(r.trainable) - n_frozen} parameters, " in lines[0]
    assert "parameter group" not in r.out0
    # the progress lines report the curve's value, unscaled, whatever the groups hold
    assert r.h["lrs"] == r.h0["lrs"] and len(r.h["lrs"]) == 4 and r.h["lrs"][0] <= 4e-3 and r.h["lrs"][-1] == pytest.approx(1e-3)
    _, _, h_q, _ = _run(r.tmp, RAVEN_PARAMS=dict(RAVEN, param_groups=[{"match": "*", "lr_scale": 0.25}]), OUTPUT_DIR=os.path.join(r.tmp, "out_quarter"),
                        SAVE_EVERY_N_STEPS=0)
    assert h_q["lrs"] == r.h0["lrs"] and h_q["losses"][:2] == r.h0["losses"][:2] and h_q["losses"] != r.h0["losses"]


def test_no_decay_on_bias_and_norm_reaches_the_other_weights_only_through_the_gradients(runs, tmp_path):
    """One optimizer step: bias / norm parameters lose their decay, every other parameter is updated with the same values from the same
    gradients -- bit for bit the default run's.  (weight_decay 0.5: at 0.01 the decay of one step is far below a bf16 spacing.)"""
    r = runs
    base = dict(RAVEN, weight_decay=0.5)
    rule = [{"match": "bias, norm", "weight_decay": 0.0}]
    one = dict(MAX_TRAIN_STEPS=2, SAVE_EVERY_N_STEPS=0)
    _, u_a, h_a, _ = _run(r.tmp, RAVEN_PARAMS=dict(base), OUTPUT_DIR=str(tmp_path / "a"), **one)
    _, u_b, h_b, out_b = _run(r.tmp, RAVEN_PARAMS=dict(base, param_groups=rule), OUTPUT_DIR=str(tmp_path / "b"), **one)
    assert h_a["optimizer_step"] == h_b["optimizer_step"] == 1 and h_a["losses"] == h_b["losses"] and h_a["grad_norms"] == h_b["grad_norms"]
    a, b = _params(u_a), _params(u_b)
    small = [n for n in r.trainable if "bias" in n or "norm" in n]
    for n in r.trainable:
        if n not in small:
            assert torch.equal(a[n], b[n]), n
    assert any(not torch.equal(a[n], b[n]) for n in small)
    assert "weight_decay 0.0" in out_b and "weight_decay 0.5" in out_b
    # a list that resolves to the base values: the default run, bit for bit
    _, u_n, h_n, out_n = _run(r.tmp, RAVEN_PARAMS=dict(base, param_groups=[{"match": "bias, norm", "weight_decay": 0.5}, {"match": "conv_in", "lr_scale": 1.0}]),
                              OUTPUT_DIR=str(tmp_path / "n"), **one)
    assert torch.equal(u_n.pflat, u_a.pflat) and h_n["losses"] == h_a["losses"] and out_n.count("INFO: parameter group ") == 1
    # over the whole run the two differ everywhere: the forward saw other biases
    _, u_c, h_c, _ = _run(r.tmp, RAVEN_PARAMS=dict(base, param_groups=rule), OUTPUT_DIR=str(tmp_path / "c"), SAVE_EVERY_N_STEPS=0, MAX_TRAIN_STEPS=4)
    _, u_d, h_d, _ = _run(r.tmp, RAVEN_PARAMS=dict(base), OUTPUT_DIR=str(tmp_path / "d"), SAVE_EVERY_N_STEPS=0, MAX_TRAIN_STEPS=4)
    assert h_c["losses"][:2] == h_d["losses"][:2] and h_c["losses"][2:] != h_d["losses"][2:]


def test_resumed_run_ends_bitwise_and_the_state_holds_nothing_of_the_option(runs):
    r = runs
    od, out2 = r.cfg.OUTPUT_DIR, os.path.join(r.tmp, "out_resumed")
    for step in (2, 4):
        assert set(T._state(os.path.join(od, f"mini_run_training_state_step_{step}.pt"))) == STATE_KEYS
    _, unet2, h2, out = _run(r.tmp, RAVEN_PARAMS=dict(RAVEN, param_groups=FROZEN), OUTPUT_DIR=out2, RESUME_TRAINING=True,
                             RESUME_MODEL_PATH=os.path.join(od, "mini_run_step_2.safetensors"),
                             RESUME_STATE_PATH=os.path.join(od, "mini_run_training_state_step_2.pt"))
    assert h2["micro_step"] == 8 and h2["optimizer_step"] == 4 and h2["losses"] == r.h["losses"][4:] and h2["grad_norms"] == r.h["grad_norms"][2:]
    assert h2["lrs"] == r.h["lrs"][2:] and out.count("INFO: parameter groups are ON") == 1        # read from the preset again
    assert torch.equal(unet2.pflat, r.pflat)


@pytest.mark.parametrize("kind,extra", [("raven", dict(stochastic_rounding=True)), ("raven", dict(master_weights=True, ema_decay=0.99)), ("titan", {})])
def test_the_option_combines_with_the_other_options(runs, tmp_path, kind, extra):
    r = runs
    hp = dict(RAVEN, param_groups=FROZEN, **extra)
    _, unet, h, out = _run(r.tmp, OPTIMIZER_TYPE=kind, TITAN_PARAMS=hp, RAVEN_PARAMS=hp, OUTPUT_DIR=str(tmp_path / "o"), MAX_TRAIN_STEPS=4, SAVE_EVERY_N_STEPS=0,
                           LOSS_TYPE="huber:c=0.5")
    assert h["optimizer_step"] == 2 and out.count("INFO: parameter groups are ON") == 1
    p = _params(unet)
    assert all(torch.equal(p[n], r.start[n]) for n in r.trainable if "mid_block" in n)
    assert all(not torch.equal(p[n], r.start[n]) for n in r.trainable if "mid_block" not in n)


def test_8bit_optimizer_gets_torch_groups_with_the_base_group_last(runs, tmp_path):
    r = runs
    hp8 = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    _, unet, h, out = _run(r.tmp, OPTIMIZER_TYPE="paged_adamw_8bit", PAGED_ADAMW_8BIT_PARAMS=dict(hp8, param_groups=FROZEN), OUTPUT_DIR=str(tmp_path / "o"),
                           MAX_TRAIN_STEPS=4, SAVE_EVERY_N_STEPS=0)
    _, _, h_0, _ = _run(r.tmp, OPTIMIZER_TYPE="paged_adamw_8bit", PAGED_ADAMW_8BIT_PARAMS=dict(hp8), OUTPUT_DIR=str(tmp_path / "p"), MAX_TRAIN_STEPS=4,
                        SAVE_EVERY_N_STEPS=0)
    assert h["optimizer_step"] == 2 and h["lrs"] == h_0["lrs"] and h["lrs"][0] > 1e-3            # the base group's rate, not the frozen group's 0
    assert out.count("INFO: parameter group ") == 2
    p = _params(unet)
    assert all(torch.equal(p[n], r.start[n]) for n in r.trainable if "mid_block" in n)
    assert sum(not torch.equal(p[n], r.start[n]) for n in r.trainable if "mid_block" not in n) > 100


def test_refusals_surface_through_train_and_main(runs, tmp_path, monkeypatch, capsys):
    from aozora_sdxl_training_amd import config as CF
    from aozora_sdxl_training_amd import trainer
    r = runs
    before = [
        (dict(RAVEN_PARAMS=dict(RAVEN, param_groups={"match": "bias"})), "list of dictionaries"),
        (dict(RAVEN_PARAMS=dict(RAVEN, param_groups=[{"match": "bias", "lr": 1.0}])), "unknown key"),
        (dict(RAVEN_PARAMS=dict(RAVEN, param_groups=[{"lr_scale": 1.0}])), "missing or empty"),
        (dict(RAVEN_PARAMS=dict(RAVEN, param_groups=[{"match": "bias", "lr_scale": True}])), "must be a number"),
        (dict(RAVEN_PARAMS=dict(RAVEN, param_groups=[{"match": "bias", "weight_decay": float("nan")}])), "finite and >= 0"),
        (dict(RAVEN_PARAMS=dict(RAVEN, param_groups=FROZEN), RAVEN_STATE_ON_HOST=True), "RAVEN_STATE_ON_HOST"),
        (dict(OPTIMIZER_TYPE="titan", TITAN_PARAMS=dict(RAVEN, param_groups=FROZEN), TITAN_HOST_GRADIENTS=True), "TITAN_HOST_GRADIENTS"),
        (dict(OPTIMIZER_TYPE="paged_adamw_8bit", PAGED_ADAMW_8BIT_PARAMS=dict(weight_decay=0.01, param_groups=[{"match": "bias", "lr_scale": -1}])), "finite and >= 0"),
    ]
    for i, (over, msg) in enumerate(before):
        cfg = T._config(str(tmp_path / str(i)), MODE, **{"RAVEN_PARAMS": dict(RAVEN), **over})
        with pytest.raises(ValueError, match=msg):
            trainer.train(cfg, unet=None, device=DEV)          # (no base checkpoint exists: the refusal comes before the model is read)
    # a rule that matches no trainable parameter: known once the freeze mask is set, refused before the optimizer is built
    for rules in ([{"match": "mid_blok", "lr_scale": 0.5}], [{"match": "conv1", "lr_scale": 0.5}]):       # a typo; a name the mask freezes
        with pytest.raises(ValueError, match="matches no trainable parameter"):
            _run(r.tmp, RAVEN_PARAMS=dict(RAVEN, param_groups=rules), OUTPUT_DIR=str(tmp_path / "never"))
    assert not os.path.exists(str(tmp_path / "never"))
    # main(): `ERROR: ...` and exit status 2, whether the refusal comes before the model is loaded or from train()
    key = {v: k for k, v in CF.block_keys("sdxl").items()}
    preset = tmp_path / "preset.json"
    preset.write_text(json.dumps({"active_mode": "sdxl", "sdxl": {key["RAVEN_PARAMS"]: {"param_groups": [{"match": "bias", "lr_scale": "fast"}]}}}))
    assert trainer.main(["--config", str(preset)]) == 2
    assert "ERROR: param_groups[0]: lr_scale must be a number" in capsys.readouterr().out

    def late(config, **kw):
        raise trainer.pgroups.GroupsError("param_groups[0] (match 'mid_blok') matches no trainable parameter")
    monkeypatch.setattr(trainer, "train", late)
    # (main() binds the process to CPUs, caps its threads and seeds every generator before it calls train(): not from inside a test suite)
    from aozora_sdxl_training_amd import affinity
    monkeypatch.setattr(affinity, "bind_rank", lambda *a, **k: dict(n_cpus=0, cpus="", threads=0, how="left alone"))
    monkeypatch.setattr(trainer, "set_seed", lambda seed: None)
    preset.write_text(json.dumps({"active_mode": "sdxl", "sdxl": {key["RAVEN_PARAMS"]: {"param_groups": [{"match": "mid_blok"}]},
                                                                  key["OUTPUT_DIR"]: str(tmp_path / "main_out")}}))
    assert trainer.main(["--config", str(preset)]) == 2
    assert "ERROR: param_groups[0] (match 'mid_blok') matches no trainable parameter." in capsys.readouterr().out
