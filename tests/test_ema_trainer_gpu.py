"""The "ema_decay" option through trainer.train: the _ema model files next to every checkpoint and at the end, the fp32 state in the
training-state file, a resumed run that ends bitwise like the uninterrupted one (parameters AND EMA), the module-optimizer branch
(paged_adamw_8bit), and -- key absent -- no trace of the option.  (The helpers are copies of tests/test_trainer_gpu.py's.)"""
import contextlib
import glob
import io
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
DEV = "cuda:0"
MODE = "v_prediction"
RAVEN = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, debias_strength=0.3, momentum_dtype="bfloat16")


def _config(tmp, mode, **over):
    import synth_cache
    synth_cache.build(os.path.join(tmp, "set0"), n_items=23, json_mode=False, seed=0, rf=(mode == "rectified_flow"))
    cfg = types.SimpleNamespace(
        INSTANCE_DATASETS=[{"path": os.path.join(tmp, "set0"), "repeats": 1}], CAPTION_SOURCE_TYPE="txt", SEED=42,
        MAX_TRAIN_STEPS=8, BATCH_SIZE=2, GRADIENT_ACCUMULATION_STEPS=2, PREDICTION_TYPE=mode, CLIP_GRAD_NORM=1.0,
        LR_CUSTOM_CURVE=[[0.0, 0.0], [0.2, 1e-4], [1.0, 2e-5]], LEARNING_RATE=1e-4, OPTIMIZER_TYPE="raven",
        RAVEN_PARAMS=dict(RAVEN, ema_decay=0.99),
        UNET_EXCLUDE_TARGETS="conv1, conv2", SAVE_EVERY_N_STEPS=2, OUTPUT_DIR=os.path.join(tmp, "out"), OUTPUT_NAME="mini_run",
        SINGLE_FILE_CHECKPOINT_PATH=os.path.join(tmp, "base.safetensors"), RESUME_TRAINING=False,
        TIMESTEP_ALLOCATION={"bin_size": 100, "counts": [45, 143, 176, 173, 154, 126, 94, 59, 26, 4]},
        TIMESTEP_LOSS_WEIGHT_CURVE={"preset": "bell"}, TIMESTEP_FORCE_IMAGE_BIN_SPREAD=True, NUM_WORKERS=0)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def _base_checkpoint(path, cfg_model):
    from safetensors.torch import save_file
    from aozora_sdxl_training_amd import checkpoint as C
    from aozora_sdxl_training_amd.unet_spec import param_table
    g = torch.Generator().manual_seed(3)
    km = C.unet_key_mapping([n for n, _ in param_table(cfg_model)])
    t = {km[n]: ((torch.ones(s) if n.endswith("weight") else torch.zeros(s)) if "norm" in n else torch.randn(*s, generator=g) * 0.05).to(torch.bfloat16)
         for n, s in param_table(cfg_model)}
    t["first_stage_model.post_quant_conv.bias"] = torch.zeros(4)
    save_file(t, str(path))


def _model():
    from aozora_sdxl_training_amd.unet_spec import mini_config
    return mini_config(ctx_dim=64, pooled=32)


def _train(cfg, model_path):
    from aozora_sdxl_training_amd import checkpoint as C
    from aozora_sdxl_training_amd.trainer import train
    from aozora_sdxl_training_amd.telemetry import Reporter
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        unet = C.load_unet(model_path, DEV, _model())
        h = train(cfg, unet=unet, device=DEV, reporter=Reporter(cfg.MAX_TRAIN_STEPS, asynchronous=False))
    torch.cuda.synchronize()
    return unet, h, buf.getvalue()


@pytest.fixture(scope="module")
def full_run(tmp_path_factory):
    """The uninterrupted run with RAVEN_PARAMS["ema_decay"] = 0.99, shared (read only) by the tests below."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tmp = str(tmp_path_factory.mktemp("ema_trainer"))
    cfg = _config(tmp, MODE)
    _base_checkpoint(cfg.SINGLE_FILE_CHECKPOINT_PATH, _model())
    unet, h, out = _train(cfg, cfg.SINGLE_FILE_CHECKPOINT_PATH)
    return types.SimpleNamespace(tmp=tmp, cfg=cfg, unet=unet, h=h, out=out, pflat=unet.pflat.clone())


def _state(path):
    return torch.load(path, map_location="cpu", weights_only=False)


def test_ema_files_are_written_and_listed(full_run):
    r = full_run
    od = r.cfg.OUTPUT_DIR
    assert r.h["saved"] == [("mini_run_step_2.safetensors", "mini_run_training_state_step_2.pt"),
                            ("mini_run_step_4.safetensors", "mini_run_training_state_step_4.pt")]        # keeps its shape
    assert r.h["saved_ema"] == ["mini_run_step_2_ema.safetensors", "mini_run_step_4_ema.safetensors"]
    assert r.h["final_ema_model"] == os.path.join(od, "mini_run_ema.safetensors")
    # two checkpoints at SAVE_EVERY_N_STEPS = 2 over four optimizer steps: their two _ema model files and the two training states that
    # carry "ema_state" are the four files of the option, plus the final one
    for f in r.h["saved_ema"] + ["mini_run_ema.safetensors"]:
        assert os.path.getsize(os.path.join(od, f)) > 0, f
    for step in (2, 4):
        st = _state(os.path.join(od, f"mini_run_training_state_step_{step}.pt"))
        es = st["ema_state"]
        assert es["k"] == step and es["decay"] == 0.99 and es["warmup"] is True and es["world"] == 1 and es["rank"] == 0
        assert es["ema"].dtype == torch.float32 and es["ema"].numel() == sum(b - a for a, b in es["ranges"])
        assert {"global_step", "micro_step", "optimizer_state", "sampler_seed"} <= set(st)              # the reference's keys are all still there
    assert r.out.count("INFO: EMA of the trainable weights is ON") == 1 and "an option outside the reference" in r.out
    assert "decay 0.99" in r.out and "warm-up on" in r.out and f"{4 * es['ema'].numel()} bytes" in r.out


def test_final_ema_file_is_the_merged_cast_ema(full_run):
    from safetensors.torch import load_file
    from aozora_sdxl_training_amd import checkpoint as C
    from aozora_sdxl_training_amd.ema import logical_views
    r = full_run
    u = r.unet
    names = [n for n, _ in u.named_parameters()]
    km = C.unet_key_mapping(names)
    model, ema_f = load_file(r.h["final_model"]), load_file(r.h["final_ema_model"])
    assert set(model) == set(ema_f)
    unet_keys = set(km.values())
    frozen = {km[n] for n, p in u.named_parameters() if not p.requires_grad}
    assert frozen and "first_stage_model.post_quant_conv.bias" in set(model) - unet_keys
    for k in set(model) - unet_keys | frozen:
        assert ema_f[k].dtype == model[k].dtype and torch.equal(ema_f[k], model[k]), k
    assert any(not torch.equal(ema_f[k], model[k]) for k in unet_keys - frozen)
    # every UNet key = bf16 of the fp32 EMA state of the last checkpoint (optimizer step 4 = the end of this run) laid over the parameters
    es = _state(os.path.join(r.cfg.OUTPUT_DIR, "mini_run_training_state_step_4.pt"))["ema_state"]
    flat = r.pflat.float().cpu()
    o = 0
    for a, b in es["ranges"]:
        flat[a:b] = es["ema"][o:o + (b - a)]
        o += b - a
    assert o == es["ema"].numel() == sum(b - a for a, b in u.trainable_ranges())       # (the trainable ranges, cut at the region bounds)
    for n, v in logical_views(u, flat).items():
        assert torch.equal(ema_f[km[n]], v.bfloat16().contiguous()), n
    assert all(bool(torch.isfinite(t.float()).all()) for t in ema_f.values())


def test_resumed_run_ends_bitwise_like_the_uninterrupted_one(full_run):
    from safetensors.torch import load_file
    r = full_run
    od = r.cfg.OUTPUT_DIR
    out2 = os.path.join(r.tmp, "out_resumed")
    cfg2 = _config(r.tmp, MODE, RESUME_TRAINING=True, OUTPUT_DIR=out2,
                   RESUME_MODEL_PATH=os.path.join(od, "mini_run_step_2.safetensors"),
                   RESUME_STATE_PATH=os.path.join(od, "mini_run_training_state_step_2.pt"))
    unet2, h2, _ = _train(cfg2, cfg2.RESUME_MODEL_PATH)
    assert h2["micro_step"] == 8 and h2["optimizer_step"] == 4 and h2["losses"] == r.h["losses"][4:]
    assert torch.equal(unet2.pflat, r.pflat)
    assert h2["saved_ema"] == ["mini_run_step_4_ema.safetensors"]
    a = _state(os.path.join(od, "mini_run_training_state_step_4.pt"))["ema_state"]
    b = _state(os.path.join(out2, "mini_run_training_state_step_4.pt"))["ema_state"]
    assert a["k"] == b["k"] == 4 and a["ranges"] == b["ranges"]
    assert torch.equal(a["ema"].view(torch.int32), b["ema"].view(torch.int32))
    fa, fb = load_file(r.h["final_ema_model"]), load_file(h2["final_ema_model"])
    assert h2["final_ema_model"] == os.path.join(out2, "mini_run_ema.safetensors") and set(fa) == set(fb)
    for k in fa:
        assert fa[k].dtype == fb[k].dtype and torch.equal(fa[k].view(torch.int16) if fa[k].dtype == torch.bfloat16 else fa[k],
                                                          fb[k].view(torch.int16) if fb[k].dtype == torch.bfloat16 else fb[k]), k


def test_resume_without_an_ema_state_starts_from_the_parameters_and_with_an_unused_one_ignores_it(full_run, tmp_path):
    r = full_run
    od = r.cfg.OUTPUT_DIR
    # option off, file with the key: ignored, with a line saying so
    cfg_off = _config(r.tmp, MODE, RESUME_TRAINING=True, OUTPUT_DIR=str(tmp_path / "off"), RAVEN_PARAMS=dict(RAVEN), SAVE_EVERY_N_STEPS=0,
                      RESUME_MODEL_PATH=os.path.join(od, "mini_run_step_2.safetensors"),
                      RESUME_STATE_PATH=os.path.join(od, "mini_run_training_state_step_2.pt"))
    u_off, h_off, out_off = _train(cfg_off, cfg_off.RESUME_MODEL_PATH)
    assert "holds an EMA" in out_off and "ignored" in out_off and "saved_ema" not in h_off and "final_ema_model" not in h_off
    assert torch.equal(u_off.pflat, r.pflat)                            # and the parameters are what they are with the option on
    assert not glob.glob(str(tmp_path / "off" / "*_ema.safetensors"))
    # option on, file without the key: k = 0 from the loaded parameters, with a line saying so
    st = _state(os.path.join(od, "mini_run_training_state_step_2.pt"))
    st.pop("ema_state")
    bare = str(tmp_path / "bare_state.pt")
    torch.save(st, bare)
    cfg_on = _config(r.tmp, MODE, RESUME_TRAINING=True, OUTPUT_DIR=str(tmp_path / "on"), RESUME_STATE_PATH=bare,
                     RESUME_MODEL_PATH=os.path.join(od, "mini_run_step_2.safetensors"))
    u_on, h_on, out_on = _train(cfg_on, cfg_on.RESUME_MODEL_PATH)
    assert "holds no EMA" in out_on and "k = 0" in out_on
    assert _state(str(tmp_path / "on" / "mini_run_training_state_step_4.pt"))["ema_state"]["k"] == 2
    assert torch.equal(u_on.pflat, r.pflat)


@pytest.mark.parametrize("optimizer", ["paged_adamw_8bit"])
def test_module_optimizer_branch(tmp_path, optimizer):
    from safetensors.torch import load_file
    from aozora_sdxl_training_amd import checkpoint as C
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tmp = str(tmp_path)
    cfg = _config(tmp, MODE, OPTIMIZER_TYPE=optimizer, RAVEN_PARAMS=dict(RAVEN),
                  PAGED_ADAMW_8BIT_PARAMS=dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, ema_decay=0.99, ema_warmup="false"))
    _base_checkpoint(cfg.SINGLE_FILE_CHECKPOINT_PATH, _model())
    unet, h, out = _train(cfg, cfg.SINGLE_FILE_CHECKPOINT_PATH)
    assert h["optimizer_step"] == 4 and h["saved_ema"] == ["mini_run_step_2_ema.safetensors", "mini_run_step_4_ema.safetensors"]
    for f in h["saved_ema"]:
        assert os.path.getsize(os.path.join(cfg.OUTPUT_DIR, f)) > 0
    assert "warm-up off" in out
    model, ema_f = load_file(h["final_model"]), load_file(h["final_ema_model"])
    km = C.unet_key_mapping([n for n, _ in unet.named_parameters()])
    assert all(bool(torch.isfinite(t.float()).all()) for t in ema_f.values())
    frozen = [km[n] for n, p in unet.named_parameters() if not p.requires_grad]
    assert frozen and all(torch.equal(ema_f[k], model[k]) for k in frozen)
    assert any(not torch.equal(ema_f[km[n]], model[km[n]]) for n, p in unet.named_parameters() if p.requires_grad)
    es = _state(os.path.join(cfg.OUTPUT_DIR, "mini_run_training_state_step_4.pt"))["ema_state"]
    assert es["k"] == 4 and es["warmup"] is False


def test_key_absent_leaves_no_trace(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tmp = str(tmp_path)
    cfg = _config(tmp, MODE, RAVEN_PARAMS=dict(RAVEN), MAX_TRAIN_STEPS=4)
    _base_checkpoint(cfg.SINGLE_FILE_CHECKPOINT_PATH, _model())
    _, h, out = _train(cfg, cfg.SINGLE_FILE_CHECKPOINT_PATH)
    assert h["optimizer_step"] == 2 and len(h["saved"]) == 1
    assert "saved_ema" not in h and "final_ema_model" not in h and "EMA of the trainable weights" not in out
    assert not glob.glob(os.path.join(cfg.OUTPUT_DIR, "*_ema*"))
    assert "ema_state" not in _state(os.path.join(cfg.OUTPUT_DIR, "mini_run_training_state_step_2.pt"))


def test_invalid_value_is_refused_before_anything_is_allocated(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd.trainer import train
    cfg = _config(str(tmp_path), MODE, RAVEN_PARAMS=dict(RAVEN, ema_decay=1.0))
    with pytest.raises(ValueError, match="0 < decay < 1"):
        train(cfg, unet=None, device=DEV)              # (no base checkpoint exists: the refusal comes before the model is read)
