"""NOISE_MODE through trainer.train (the helpers of tests/test_trainer_gpu.py, a handful of micro-steps): "pyramid" trains with finite
losses that are not the "normal" run's -- before NOISE_MODE was read both were the same run; "normal" and the attribute absent are the
same run bit for bit; a run stopped and resumed is bitwise the uninterrupted one (the draws depend on SEED and the micro-step
alone); a NOISE_MODE that cannot be read is refused before a UNet is loaded."""
import contextlib
import io
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import test_trainer_gpu as T        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ABSENT = object()
_RUNS = {}
PYRAMID = "pyramid:levels=3,offset=0.05,perturb=0.1"


def run(tmp_factory, noise_mode, mode="v_prediction", steps=4, save_every=0, resume_from=None):
    """History, final parameters, output and config of a run with this NOISE_MODE (ABSENT: no such attribute), once per module."""
    key = (noise_mode if noise_mode is not ABSENT else None, noise_mode is ABSENT, mode, steps, save_every, resume_from)
    if key in _RUNS:
        return _RUNS[key]
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd import checkpoint as C
    from aozora_sdxl_training_amd.trainer import train
    from aozora_sdxl_training_amd.telemetry import Reporter
    from aozora_sdxl_training_amd.unet_spec import mini_config
    model = mini_config(ctx_dim=64, pooled=32)
    over = dict(MAX_TRAIN_STEPS=steps, SAVE_EVERY_N_STEPS=save_every)
    if noise_mode is not ABSENT:
        over["NOISE_MODE"] = noise_mode
    if resume_from is None:
        tmp = str(tmp_factory.mktemp("noise_run"))
        cfg = T._config(tmp, mode, **over)
        T._base_checkpoint(cfg.SINGLE_FILE_CHECKPOINT_PATH, model)
        src = cfg.SINGLE_FILE_CHECKPOINT_PATH
    else:
        tmp, out_dir = resume_from
        cfg = T._config(tmp, mode, RESUME_TRAINING=True, RESUME_MODEL_PATH=os.path.join(out_dir, "mini_run_step_1.safetensors"),
                        RESUME_STATE_PATH=os.path.join(out_dir, "mini_run_training_state_step_1.pt"), **over)
        src = cfg.RESUME_MODEL_PATH
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        unet = C.load_unet(src, DEV, model)
        h = train(cfg, unet=unet, device=DEV, reporter=Reporter(cfg.MAX_TRAIN_STEPS, asynchronous=False))
    torch.cuda.synchronize()
    assert h["micro_step"] == steps
    _RUNS[key] = (h, unet.pflat.clone(), buf.getvalue(), (tmp, cfg.OUTPUT_DIR))
    return _RUNS[key]


def test_normal_and_the_absent_key_are_the_same_run(tmp_path_factory):
    h0, p0, out0, _ = run(tmp_path_factory, ABSENT)
    h1, p1, out1, _ = run(tmp_path_factory, "normal")
    assert h1["losses"] == h0["losses"] and h1["grad_norms"] == h0["grad_norms"] and torch.equal(p1, p0)
    assert "NOISE_MODE" not in out0 and "NOISE_MODE" not in out1


def test_pyramid_trains_with_finite_losses_that_are_not_the_normal_ones(tmp_path_factory):
    h0, p0, _, _ = run(tmp_path_factory, "normal")
    h, p, out, _ = run(tmp_path_factory, "pyramid")
    print(f"losses: pyramid {h['losses']!r} normal {h0['losses']!r}")
    assert len(h["losses"]) == 4 and all(l == l and 0.0 < l < 10.0 for l in h["losses"]) and all(g > 0 and g == g for g in h["grad_norms"])
    assert all(a != b for a, b in zip(h["losses"], h0["losses"])) and not torch.equal(p, p0)
    assert "INFO: NOISE_MODE: pyramid (6 levels, discount 0.3, per-sample unit std)" in out


def test_a_stopped_and_resumed_run_is_bitwise_the_uninterrupted_one(tmp_path_factory):
    h, p, _, where = run(tmp_path_factory, PYRAMID, steps=4, save_every=1)
    assert ("mini_run_step_1.safetensors", "mini_run_training_state_step_1.pt") in h["saved"]
    h2, p2, _, _ = run(tmp_path_factory, PYRAMID, steps=4, save_every=0, resume_from=where)
    assert h2["optimizer_step"] == h["optimizer_step"] == 2
    assert h2["losses"] == h["losses"][2:] and h2["grad_norms"] == h["grad_norms"][1:]
    assert torch.equal(p2, p)


def test_a_bad_noise_mode_is_refused_before_a_unet_is_loaded(tmp_path, monkeypatch):
    from aozora_sdxl_training_amd import checkpoint as C
    from aozora_sdxl_training_amd.trainer import train

    def no_load(*a, **k):
        raise AssertionError("a UNet was loaded")
    monkeypatch.setattr(C, "load_unet", no_load)
    for bad in ("pyramyd", "pyramid:levels=9", "normal:offset=0.1", "offset:offset=-1"):
        cfg = T._config(str(tmp_path), "v_prediction", NOISE_MODE=bad)
        assert not os.path.exists(cfg.SINGLE_FILE_CHECKPOINT_PATH)
        with pytest.raises(ValueError, match="NOISE_MODE"):
            train(cfg, unet=None, device=DEV)
