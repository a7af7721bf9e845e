"""The "master_weights" option through trainer.train: the INFO line, "master_state" in the training-state file, a resumed run that ends
bitwise like the uninterrupted one (parameters AND master), resumes across the option, the refusals, and -- key absent -- no trace of
the option.  (The helpers are those of tests/test_ema_trainer_gpu.py.)"""
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
DEV, MODE, RAVEN = T.DEV, T.MODE, T.RAVEN
MASTER = dict(RAVEN, master_weights=True)
# the keys of the reference's training-state file (train.py:2513-2531), which is all a run without the option writes
STATE_KEYS = {"global_step", "micro_step", "optimizer_state", "sampler_seed", "sampler_epoch", "timestep_sampler_state", "random_state",
              "numpy_state", "torch_cpu_state", "torch_cuda_state"}


def _run(tmp, **over):
    cfg = T._config(tmp, MODE, **over)
    if not os.path.exists(cfg.SINGLE_FILE_CHECKPOINT_PATH):
        T._base_checkpoint(cfg.SINGLE_FILE_CHECKPOINT_PATH, T._model())
    unet, h, out = T._train(cfg, cfg.RESUME_MODEL_PATH if cfg.RESUME_TRAINING else cfg.SINGLE_FILE_CHECKPOINT_PATH)
    return cfg, unet, h, out


@pytest.fixture(scope="module")
def full_run(tmp_path_factory):
    """The uninterrupted 8-micro-step run with RAVEN_PARAMS["master_weights"] = true, and the same run with the key absent."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import types
    tmp = str(tmp_path_factory.mktemp("master_trainer"))
    cfg, unet, h, out = _run(tmp, RAVEN_PARAMS=dict(MASTER))
    cfg0, unet0, h0, out0 = _run(tmp, RAVEN_PARAMS=dict(RAVEN), OUTPUT_DIR=os.path.join(tmp, "out_absent"))
    return types.SimpleNamespace(tmp=tmp, cfg=cfg, h=h, out=out, pflat=unet.pflat.clone(), trainable=unet.trainable_ranges(),
                                 cfg0=cfg0, h0=h0, out0=out0, pflat0=unet0.pflat.clone())


def _resume_args(od, step=2):
    return dict(RESUME_TRAINING=True, RESUME_MODEL_PATH=os.path.join(od, f"mini_run_step_{step}.safetensors"),
                RESUME_STATE_PATH=os.path.join(od, f"mini_run_training_state_step_{step}.pt"))


def test_trains_prints_the_line_and_writes_master_state(full_run):
    r = full_run
    assert r.h["micro_step"] == 8 and r.h["optimizer_step"] == 4 and all(l == l and 0.0 < l < 10.0 for l in r.h["losses"])
    n_train = sum(b - a for a, b in r.trainable)
    assert r.out.count("INFO: fp32 master weights are ON") == 1 and f"({4 * n_train} bytes of fp32 on this rank)" in r.out
    assert "an option outside the reference" in r.out
    for step in (2, 4):
        st = T._state(os.path.join(r.cfg.OUTPUT_DIR, f"mini_run_training_state_step_{step}.pt"))
        assert set(st) == STATE_KEYS | {"master_state"}
        ms = st["master_state"]
        assert set(ms) == {"world", "rank", "ranges", "master"} and (ms["world"], ms["rank"]) == (1, 0)
        assert ms["master"].dtype == torch.float32 and ms["master"].numel() == n_train == sum(b - a for rs in ms["ranges"] for a, b in rs)
    # the model file holds pflat = bf16(master): the last checkpoint is the end of this run
    flat = r.pflat.cpu()
    o = 0
    for rs in ms["ranges"]:
        for a, b in rs:
            assert torch.equal(ms["master"][o:o + (b - a)].bfloat16(), flat[a:b])
            o += b - a
    assert not torch.equal(r.pflat, r.pflat0)                                # the option selects results ...
    assert r.h["losses"][:2] == r.h0["losses"][:2]                           # ... from the second optimizer step on: the first window is shared


def test_resumed_run_ends_bitwise_like_the_uninterrupted_one(full_run):
    r = full_run
    od, out2 = r.cfg.OUTPUT_DIR, os.path.join(r.tmp, "out_resumed")
    _, unet2, h2, out = _run(r.tmp, RAVEN_PARAMS=dict(MASTER), OUTPUT_DIR=out2, **_resume_args(od))
    assert h2["micro_step"] == 8 and h2["optimizer_step"] == 4 and h2["losses"] == r.h["losses"][4:] and h2["grad_norms"] == r.h["grad_norms"][2:]
    assert "fp32 master weights restored from the training state" in out
    assert torch.equal(unet2.pflat, r.pflat)
    a = T._state(os.path.join(od, "mini_run_training_state_step_4.pt"))["master_state"]
    b = T._state(os.path.join(out2, "mini_run_training_state_step_4.pt"))["master_state"]
    assert a["ranges"] == b["ranges"] and torch.equal(a["master"].view(torch.int32), b["master"].view(torch.int32))


def test_resume_across_the_option(full_run, tmp_path):
    r = full_run
    od = r.cfg.OUTPUT_DIR
    # option off, file with the key: ignored, with a line saying so; no master is kept or written
    _, _, h_off, out_off = _run(r.tmp, RAVEN_PARAMS=dict(RAVEN), OUTPUT_DIR=str(tmp_path / "off"), **_resume_args(od))
    assert "holds fp32 master weights" in out_off and "ignored" in out_off and "master weights are ON" not in out_off
    assert set(T._state(str(tmp_path / "off" / "mini_run_training_state_step_4.pt"))) == STATE_KEYS
    # option on, file without the key: the master starts from the loaded parameters, with a line saying so
    st = T._state(os.path.join(od, "mini_run_training_state_step_2.pt"))
    st.pop("master_state")
    bare = str(tmp_path / "bare_state.pt")
    torch.save(st, bare)
    _, unet_on, h_on, out_on = _run(r.tmp, RAVEN_PARAMS=dict(MASTER), OUTPUT_DIR=str(tmp_path / "on"),
                                    **{**_resume_args(od), "RESUME_STATE_PATH": bare})
    assert "holds no fp32 master weights" in out_on and "starts from the loaded parameters" in out_on
    assert h_on["optimizer_step"] == 4 and "master_state" in T._state(str(tmp_path / "on" / "mini_run_training_state_step_4.pt"))


def test_key_absent_leaves_no_trace(full_run, tmp_path):
    """Key absent: no line, the reference's state-file keys and nothing else, and history and parameters bit for bit those of a run whose
    dictionary says false -- neither run allocates a master or calls the new entry point."""
    r = full_run
    assert "master weights" not in r.out0 and "master_state" not in r.out0
    for step in (2, 4):
        assert set(T._state(os.path.join(r.cfg0.OUTPUT_DIR, f"mini_run_training_state_step_{step}.pt"))) == STATE_KEYS
    assert r.h0["saved"] == r.h["saved"] and set(r.h0) == set(r.h)
    _, unet_f, h_f, out_f = _run(r.tmp, RAVEN_PARAMS=dict(RAVEN, master_weights=False), OUTPUT_DIR=str(tmp_path / "false"))
    assert "master weights" not in out_f
    assert {k: v for k, v in h_f.items() if k != "final_model"} == {k: v for k, v in r.h0.items() if k != "final_model"}
    assert torch.equal(unet_f.pflat, r.pflat0)


def test_refusals_surface_through_train(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd.trainer import train
    cases = [
        (dict(OPTIMIZER_TYPE="paged_adamw_8bit", PAGED_ADAMW_8BIT_PARAMS=dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, master_weights=True)),
         "master_weights is an option of raven and titan"),
        (dict(RAVEN_PARAMS=dict(MASTER, stochastic_rounding=True)), "master_weights and stochastic_rounding do not combine"),
        (dict(OPTIMIZER_TYPE="titan", TITAN_PARAMS=dict(MASTER, stochastic_rounding=True)), "master_weights and stochastic_rounding do not combine"),
        (dict(OPTIMIZER_TYPE="titan", TITAN_PARAMS=dict(MASTER), TITAN_HOST_GRADIENTS=True), "TITAN_HOST_GRADIENTS"),
    ]
    for i, (over, msg) in enumerate(cases):
        cfg = T._config(str(tmp_path / str(i)), MODE, **{"RAVEN_PARAMS": dict(RAVEN), **over})
        with pytest.raises(ValueError, match=msg):
            train(cfg, unet=None, device=DEV)          # (no base checkpoint exists: the refusal comes before the model is read)


def test_titan_trains_with_a_master(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg, unet, h, out = _run(str(tmp_path), OPTIMIZER_TYPE="titan", RAVEN_PARAMS=dict(RAVEN), TITAN_PARAMS=dict(MASTER), MAX_TRAIN_STEPS=4)
    assert h["optimizer_step"] == 2 and out.count("INFO: fp32 master weights are ON") == 1
    ms = T._state(os.path.join(cfg.OUTPUT_DIR, "mini_run_training_state_step_2.pt"))["master_state"]
    assert ms["master"].numel() == sum(b - a for a, b in unet.trainable_ranges())
