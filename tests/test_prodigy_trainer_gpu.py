"""OPTIMIZER_TYPE = "prodigy" through trainer.train on the mini UNet (the helpers of test_trainer_gpu.py, 4 micro-steps): the loop
builds optimizers.Prodigy -- it used to build Raven for any unknown value --, reports d after every optimizer step, says what is on,
resumes bit for bit from its own checkpoint, and refuses what it does not combine with before a UNet is loaded."""
import contextlib
import io
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
DEV = "cuda:0"
CURVE = [[0.0, 1.0], [1.0, 0.5]]
PARAMS = dict(d0=1e-5, weight_decay=0.01, safeguard_warmup=True)


def _run(tmp, capture=None, **over):
    """One trainer.train over the mini UNet -> (hist, unet, what it printed)."""
    from test_trainer_gpu import _base_checkpoint, _config
    from aozora_sdxl_training_amd import checkpoint as C
    from aozora_sdxl_training_amd.telemetry import Reporter
    from aozora_sdxl_training_amd.trainer import train
    from aozora_sdxl_training_amd.unet_spec import mini_config
    model = mini_config(ctx_dim=64, pooled=32)
    over.setdefault("MAX_TRAIN_STEPS", 4)
    cfg = _config(tmp, "v_prediction", **over)
    if not os.path.exists(cfg.SINGLE_FILE_CHECKPOINT_PATH):
        _base_checkpoint(cfg.SINGLE_FILE_CHECKPOINT_PATH, model)
    seen = {}
    if capture is not None:
        import aozora_sdxl_training_amd.trainer as T
        real = T.Prodigy

        def spy(*a, **k):
            seen["optimizer"] = real(*a, **k)
            return seen["optimizer"]
        capture.setattr(T, "Prodigy", spy)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        unet = C.load_unet(cfg.RESUME_MODEL_PATH if over.get("RESUME_TRAINING") else cfg.SINGLE_FILE_CHECKPOINT_PATH, DEV, model)
        h = train(cfg, unet=unet, device=DEV, reporter=Reporter(cfg.MAX_TRAIN_STEPS, asynchronous=False))
    torch.cuda.synchronize()
    return h, unet, buf.getvalue(), seen.get("optimizer")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tmp = str(tmp_path_factory.mktemp("prodigy"))
    mp = pytest.MonkeyPatch()
    try:
        h, unet, out, opt = _run(tmp, capture=mp, OPTIMIZER_TYPE="prodigy", PRODIGY_PARAMS=dict(PARAMS), LR_CUSTOM_CURVE=CURVE, SAVE_EVERY_N_STEPS=1)
    finally:
        mp.undo()
    hr, unet_r, _, _ = _run(tmp, OPTIMIZER_TYPE="raven", LR_CUSTOM_CURVE=CURVE, SAVE_EVERY_N_STEPS=0)
    return dict(tmp=tmp, h=h, pflat=unet.pflat.clone(), out=out, opt=opt, raven=unet_r.pflat.clone(), trainable=unet.trainable_ranges())


def test_the_loop_builds_prodigy_and_reports_d(runs):
    from aozora_sdxl_training_amd.optimizers import Prodigy
    h, opt = runs["h"], runs["opt"]
    assert isinstance(opt, Prodigy), "OPTIMIZER_TYPE = 'prodigy' must not silently build another optimizer"
    g = opt.param_groups[0]
    assert (g["d0"], g["weight_decay"], g["safeguard_warmup"], g["use_bias_correction"]) == (1e-5, 0.01, True, False)
    assert h["micro_step"] == 4 and h["optimizer_step"] == 2 and len(h["losses"]) == 4 and len(h["grad_norms"]) == 2
    assert all(math.isfinite(l) and 0.0 < l < 10.0 for l in h["losses"])
    d = h["prodigy_d"]
    assert len(d) == 2 and all(math.isfinite(x) for x in d) and 1e-5 <= d[0] <= d[1]
    assert opt.scalars()["k"] == 2.0 and opt.d_value() == d[1]
    assert [(a, b) for _, a, b in opt.ranges] == list(runs["trainable"])
    assert h["lrs"] == pytest.approx([1.0 - 0.5 * 2 / 3, 0.5])


def test_parameters_differ_from_a_raven_run(runs):
    assert runs["pflat"].shape == runs["raven"].shape and int((runs["pflat"] != runs["raven"]).sum()) > 0


def test_info_lines(runs, tmp_path):
    out = runs["out"]
    assert "INFO: OPTIMIZER_TYPE prodigy is ON" in out and f"{runs['opt'].state_bytes} bytes of fp32 state" in out
    assert "belongs near 1" not in out
    assert out.count("(prodigy d = ") == 2                  # the checkpoint banner of both saves
    # a learning-rate curve of AdamW's scale gets the second line
    h, _, low, _ = _run(str(tmp_path), OPTIMIZER_TYPE="prodigy", PRODIGY_PARAMS={}, MAX_TRAIN_STEPS=2, SAVE_EVERY_N_STEPS=0)
    assert "INFO: OPTIMIZER_TYPE prodigy is ON" in low and "belongs near 1" in low and "0.0001" in low
    assert len(h["prodigy_d"]) == 1


def test_a_run_resumed_at_optimizer_step_one_equals_the_uninterrupted_run(runs):
    tmp, h = runs["tmp"], runs["h"]
    assert h["saved"][0] == ("mini_run_step_1.safetensors", "mini_run_training_state_step_1.pt")
    out_dir = os.path.join(tmp, "out")
    h2, unet2, _, _ = _run(tmp, OPTIMIZER_TYPE="prodigy", PRODIGY_PARAMS=dict(PARAMS), LR_CUSTOM_CURVE=CURVE, SAVE_EVERY_N_STEPS=0, RESUME_TRAINING=True,
                           RESUME_MODEL_PATH=os.path.join(out_dir, "mini_run_step_1.safetensors"),
                           RESUME_STATE_PATH=os.path.join(out_dir, "mini_run_training_state_step_1.pt"))
    assert h2["micro_step"] == 4 and h2["optimizer_step"] == 2
    assert h2["losses"] == h["losses"][2:] and h2["grad_norms"] == h["grad_norms"][1:] and h2["prodigy_d"] == h["prodigy_d"][1:]
    assert torch.equal(unet2.pflat, runs["pflat"])


@pytest.mark.parametrize("hp,match", [
    ({"stochastic_rounding": True}, "stochastic_rounding is an option of raven and titan"),
    ({"master_weights": True}, "master_weights is an option of raven and titan"),
    ({"param_groups": [{"match": "bias", "weight_decay": 0.0}]}, "param_groups is an option of raven, titan"),
    ({"momentum_dtype": "bfloat16"}, "unknown key"),
    ({"eps": 0}, "eps must be > 0"),
    ({"d0": 0}, "d0 must be > 0"),
    ({"betas": [0.9, 1.0]}, "betas must lie"),
    ({"ema_decay": 1.5}, "decay"),
])
def test_refusals_come_before_a_unet_is_loaded(tmp_path, hp, match):
    """SINGLE_FILE_CHECKPOINT_PATH does not exist: reaching the loader would be a different error."""
    from test_trainer_gpu import _config
    from aozora_sdxl_training_amd.trainer import train
    cfg = _config(str(tmp_path), "v_prediction", OPTIMIZER_TYPE="prodigy", PRODIGY_PARAMS=hp, LR_CUSTOM_CURVE=CURVE)
    assert not os.path.exists(cfg.SINGLE_FILE_CHECKPOINT_PATH)
    with pytest.raises(ValueError, match=match):
        train(cfg, unet=None, device=DEV)


def test_more_than_one_rank_is_refused_before_a_unet_is_loaded(tmp_path, monkeypatch):
    import torch.distributed as tdist
    from test_trainer_gpu import _config
    from aozora_sdxl_training_amd.trainer import train
    monkeypatch.setattr(tdist, "is_initialized", lambda: True)
    monkeypatch.setattr(tdist, "get_world_size", lambda *a, **k: 2)
    monkeypatch.setattr(tdist, "get_rank", lambda *a, **k: 0)
    cfg = _config(str(tmp_path), "v_prediction", OPTIMIZER_TYPE="prodigy", PRODIGY_PARAMS={}, LR_CUSTOM_CURVE=CURVE)
    with pytest.raises(ValueError, match="one rank only"):
        train(cfg, unet=None, device=DEV)
