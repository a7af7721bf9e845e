"""OPTIMIZER_TYPE = "adafactor" through trainer.train on the mini UNet (the helpers of test_trainer_gpu.py, 4 micro-steps): the loop
builds optimizers.Adafactor, says what is on, resumes bit for bit from its own checkpoint with stochastic rounding on, trains LoRA
adapters alone, and refuses what it does not combine with before a UNet is loaded."""
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
CURVE = [[0.0, 2e-3], [1.0, 1e-3]]
PARAMS = dict(scale_parameter=False, relative_step=False, warmup_init=False, stochastic_rounding=True, weight_decay=0.01)


def _run(tmp, capture=None, **over):
    """One trainer.train over the mini UNet -> (hist, unet, what it printed, the optimizer, the parameters before)."""
    from test_trainer_gpu import _base_checkpoint, _config
    from aozora_sdxl_training_amd import checkpoint as C, lora
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
        real = T.Adafactor

        def spy(*a, **k):
            seen["optimizer"] = real(*a, **k)
            return seen["optimizer"]
        capture.setattr(T, "Adafactor", spy)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        spec = lora.options(cfg, cfg=model)[0] if getattr(cfg, "LORA_PARAMS", None) else None
        if spec is None:
            unet = C.load_unet(cfg.RESUME_MODEL_PATH if over.get("RESUME_TRAINING") else cfg.SINGLE_FILE_CHECKPOINT_PATH, DEV, model)
        else:
            unet = lora.load_unet(cfg.SINGLE_FILE_CHECKPOINT_PATH, DEV, model, spec, cfg.SEED, None)
        before = unet.pflat.clone()
        h = train(cfg, unet=unet, device=DEV, reporter=Reporter(cfg.MAX_TRAIN_STEPS, asynchronous=False))
    torch.cuda.synchronize()
    return h, unet, buf.getvalue(), seen.get("optimizer"), before


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tmp = str(tmp_path_factory.mktemp("adafactor"))
    mp = pytest.MonkeyPatch()
    try:
        h, unet, out, opt, _ = _run(tmp, capture=mp, OPTIMIZER_TYPE="adafactor", ADAFACTOR_PARAMS=dict(PARAMS), LR_CUSTOM_CURVE=CURVE, SAVE_EVERY_N_STEPS=1)
    finally:
        mp.undo()
    _, unet_r, _, _, _ = _run(tmp, OPTIMIZER_TYPE="raven", LR_CUSTOM_CURVE=CURVE, SAVE_EVERY_N_STEPS=0)
    return dict(tmp=tmp, h=h, pflat=unet.pflat.clone(), out=out, opt=opt, raven=unet_r.pflat.clone(), trainable=unet.trainable_ranges(),
                names=[n for n, p in unet.named_parameters() if p.requires_grad])


def test_the_loop_builds_adafactor(runs):
    from aozora_sdxl_training_amd.optimizers import Adafactor
    h, opt = runs["h"], runs["opt"]
    assert isinstance(opt, Adafactor), "OPTIMIZER_TYPE = 'adafactor' must not silently build another optimizer"
    g = opt.param_groups[0]
    assert (g["weight_decay"], g["stochastic_rounding"], g["sr_seed"], g["scale_parameter"], g["relative_step"], g["beta1"]) == (0.01, True, 42, False, False, None)
    assert h["micro_step"] == 4 and h["optimizer_step"] == 2 and len(h["losses"]) == 4 and len(h["grad_norms"]) == 2
    assert all(math.isfinite(l) and 0.0 < l < 10.0 for l in h["losses"])
    assert opt.optimizer_step == 2 and sorted(e["name"] for e in opt.entries) == sorted(runs["names"])
    assert h["lrs"] == pytest.approx([2e-3 - 1e-3 * 2 / 3, 1e-3])


def test_parameters_differ_from_a_raven_run(runs):
    assert runs["pflat"].shape == runs["raven"].shape and int((runs["pflat"] != runs["raven"]).sum()) > 0


def test_info_lines(runs, tmp_path):
    out = runs["out"]
    assert "INFO: OPTIMIZER_TYPE adafactor is ON" in out and f"{runs['opt'].state_bytes} bytes of fp32 state" in out
    assert "arithmetic of transformers.optimization.Adafactor, pinned by tests/golden/adafactor_golden.pt" in out
    assert "do not move at all" not in out and "relative_step is ON" not in out
    # the customary tiny learning rate without stochastic rounding gets the warning; relative_step says the curve is ignored
    _, _, low, _, _ = _run(str(tmp_path), OPTIMIZER_TYPE="adafactor", ADAFACTOR_PARAMS={}, LR_CUSTOM_CURVE=[[0.0, 0.0], [1.0, 1e-6]], MAX_TRAIN_STEPS=2,
                           SAVE_EVERY_N_STEPS=0)
    assert "INFO: OPTIMIZER_TYPE adafactor is ON" in low and "do not move at all" in low and "1e-06" in low
    _, _, rel, _, _ = _run(str(tmp_path), OPTIMIZER_TYPE="adafactor", ADAFACTOR_PARAMS=dict(relative_step=True, scale_parameter=True, warmup_init=True),
                           MAX_TRAIN_STEPS=2, SAVE_EVERY_N_STEPS=0)
    assert "relative_step is ON" in rel and "the reported learning rate is the curve's" in rel and "do not move at all" not in rel


def test_a_run_resumed_at_optimizer_step_one_equals_the_uninterrupted_run(runs):
    """With stochastic rounding on: the bits are a function of (SEED, optimizer step, flat offset), and the step count is restored."""
    tmp, h = runs["tmp"], runs["h"]
    assert h["saved"][0] == ("mini_run_step_1.safetensors", "mini_run_training_state_step_1.pt")
    out_dir = os.path.join(tmp, "out")
    h2, unet2, _, _, _ = _run(tmp, OPTIMIZER_TYPE="adafactor", ADAFACTOR_PARAMS=dict(PARAMS), LR_CUSTOM_CURVE=CURVE, SAVE_EVERY_N_STEPS=0, RESUME_TRAINING=True,
                              RESUME_MODEL_PATH=os.path.join(out_dir, "mini_run_step_1.safetensors"),
                              RESUME_STATE_PATH=os.path.join(out_dir, "mini_run_training_state_step_1.pt"))
    assert h2["micro_step"] == 4 and h2["optimizer_step"] == 2
    assert h2["losses"] == h["losses"][2:] and h2["grad_norms"] == h["grad_norms"][1:]
    assert torch.equal(unet2.pflat, runs["pflat"])


def test_lora_moves_only_adapters(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    h, unet, out, _, before = _run(str(tmp_path), OPTIMIZER_TYPE="adafactor", ADAFACTOR_PARAMS=dict(PARAMS), LR_CUSTOM_CURVE=CURVE, SAVE_EVERY_N_STEPS=0,
                                   LORA_PARAMS=dict(rank=4, alpha=4, scope="attention"))
    assert "LoRA is ON" in out and "INFO: OPTIMIZER_TYPE adafactor is ON" in out
    assert h["optimizer_step"] == 2 and all(math.isfinite(l) for l in h["losses"])
    lo = unet._slots["conv_out.bias"][0] + 64
    assert torch.equal(unet.pflat[:lo], before[:lo]), "a frozen base parameter changed"
    names = [n for n, p in unet.named_parameters() if p.requires_grad]
    assert names and all(".lora_" in n for n in names)
    assert all(bool(t.any()) for n, t in unet.lora_state_dict().items() if n.endswith(".lora_B.weight")), "an up matrix did not move"
    assert int((unet.pflat[lo:] != before[lo:]).sum()) > 0


@pytest.mark.parametrize("hp,match", [
    ({"param_groups": [{"match": "bias", "weight_decay": 0.0}]}, "param_groups is an option of raven, titan"),
    ({"master_weights": True}, "keeps no fp32 master copy"),
    ({"momentum_dtype": "bfloat16"}, "unknown key"),
    ({"clip_threshold": "wide"}, "cannot be read as a number"),
    ({"warmup_init": True}, "warmup_init=True needs relative_step=True"),
    ({"clip_threshold": 0}, "clip_threshold must be > 0"),
    ({"beta1": 1.0}, "beta1 must lie"),
    ({"ema_decay": 1.5}, "decay"),
])
def test_refusals_come_before_a_unet_is_loaded(tmp_path, hp, match):
    """SINGLE_FILE_CHECKPOINT_PATH does not exist: reaching the loader would be a different error."""
    from test_trainer_gpu import _config
    from aozora_sdxl_training_amd.trainer import train
    cfg = _config(str(tmp_path), "v_prediction", OPTIMIZER_TYPE="adafactor", ADAFACTOR_PARAMS=hp, LR_CUSTOM_CURVE=CURVE)
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
    cfg = _config(str(tmp_path), "v_prediction", OPTIMIZER_TYPE="adafactor", ADAFACTOR_PARAMS={}, LR_CUSTOM_CURVE=CURVE)
    with pytest.raises(ValueError, match="one rank only"):
        train(cfg, unet=None, device=DEV)
