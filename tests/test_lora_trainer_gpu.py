"""trainer.train with LORA_PARAMS over the mini UNet (tests/test_trainer_gpu._config / _base_checkpoint, four optimizer steps): the base
stays bit-unchanged and the adapters move under raven and prodigy, every model file is the kohya-ss adapter file (keys, shapes,
metadata) and loads back bit for bit, a resumed run equals the uninterrupted one, `save_merged` writes a full model, every refusal
fires before a UNet is loaded, and a run without LORA_PARAMS is today's run."""
import contextlib
import io
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
DEV = "cuda:0"
LORA = dict(rank=8, alpha=4)
PRODIGY = dict(OPTIMIZER_TYPE="prodigy", PRODIGY_PARAMS=dict(d0=1e-5, weight_decay=0.01, safeguard_warmup=True), LR_CUSTOM_CURVE=[[0.0, 1.0], [1.0, 0.5]])


def _model():
    from aozora_sdxl_training_amd.unet_spec import mini_config
    return mini_config(ctx_dim=64, pooled=32)


def _run(tmp, **over):
    """One trainer.train over the mini UNet -> (hist, unet, printed text, config)."""
    from test_trainer_gpu import _base_checkpoint, _config
    from aozora_sdxl_training_amd import checkpoint as C, lora
    from aozora_sdxl_training_amd.telemetry import Reporter
    from aozora_sdxl_training_amd.trainer import train
    model = _model()
    cfg = _config(tmp, "v_prediction", **over)
    if not os.path.exists(cfg.SINGLE_FILE_CHECKPOINT_PATH):
        _base_checkpoint(cfg.SINGLE_FILE_CHECKPOINT_PATH, model)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        spec = lora.options(cfg, cfg=model)[0]
        if spec is None:
            unet = C.load_unet(cfg.SINGLE_FILE_CHECKPOINT_PATH, DEV, model)
        else:
            unet = lora.load_unet(cfg.SINGLE_FILE_CHECKPOINT_PATH, DEV, model, spec, cfg.SEED, cfg.RESUME_MODEL_PATH if over.get("RESUME_TRAINING") else None)
        base0 = unet.pflat.clone()
        h = train(cfg, unet=unet, device=DEV, reporter=Reporter(cfg.MAX_TRAIN_STEPS, asynchronous=False))
    torch.cuda.synchronize()
    return h, unet, buf.getvalue(), cfg, base0


def _predict(unet):
    from aozora_sdxl_training_amd.train_step import TrainStep
    from test_model_gpu import _inputs
    lat, noise, ctx, pooled, tid, ts, jit = _inputs(2, 8, 8, unet.cfg, seed=3)
    unet.zero_grad()
    step = TrainStep(unet, mode="epsilon", grad_accum=1, use_graph=False)
    step.micro_step(lat.to(DEV), noise.to(DEV), ts, ctx.to(DEV), pooled.to(DEV), tid.to(DEV), jit)
    step.synchronize()
    return step.last_pred_nhwc.clone()


@pytest.fixture(scope="module")
def raven_run(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("lora_raven"))
    h, unet, out, cfg, base0 = _run(tmp, LORA_PARAMS=dict(LORA, save_merged=True), SAVE_EVERY_N_STEPS=1)
    return dict(tmp=tmp, h=h, unet=unet, out=out, cfg=cfg, base0=base0)


def _check_run(h, unet, out, cfg, base0):
    from safetensors import safe_open
    from aozora_sdxl_training_amd import lora
    from aozora_sdxl_training_amd.unet import AozoraUNet
    assert h["optimizer_step"] == 4 and all(l == l and 0.0 < l < 10.0 for l in h["losses"]) and all(g > 0 for g in h["grad_norms"])
    assert "LoRA is ON" in out and "UNET_EXCLUDE_TARGETS is not applied" in out
    lo = unet._slots["conv_out.bias"][0] + 64
    assert torch.equal(unet.pflat[:lo], base0[:lo]), "a frozen base parameter changed"
    names = [n for n, p in unet.named_parameters() if p.requires_grad]
    assert names and all(".lora_" in n for n in names) and len(unet.trainable_ranges()) == 1
    lsd = unet.lora_state_dict()
    assert all(bool(t.any()) for n, t in lsd.items() if n.endswith(".lora_B.weight")), "an up matrix did not move"
    # the file: exactly the expected keys, shapes, dtype and metadata
    spec = unet.lora
    want = {}
    for n, t in lsd.items():
        module, _, leaf = n.rpartition(".lora_")
        key = lora.file_key(module)
        assert key.startswith("lora_unet_") and "." not in key
        want[key + (".lora_down.weight" if leaf == "A.weight" else ".lora_up.weight")] = tuple(t.shape)
        want[key + ".alpha"] = ()
    assert "lora_unet_input_blocks_4_1_transformer_blocks_0_attn1_to_q.lora_down.weight" in want
    with safe_open(h["final_model"], framework="pt", device="cpu") as f:
        assert set(f.keys()) == set(want)
        for k in f.keys():
            t = f.get_tensor(k)
            assert tuple(t.shape) == want[k] and t.dtype == torch.bfloat16, k
            if k.endswith(".lora_down.weight"):
                assert t.shape[0] == spec.rank
            if k.endswith(".alpha"):
                assert float(t) == spec.alpha
        meta = f.metadata()
        for k, v in {"ss_network_module": "networks.lora", "ss_network_dim": str(spec.rank), "ss_network_alpha": f"{spec.alpha:g}",
                     "ss_base_model_version": "sdxl_base_v1-0"}.items():
            assert meta.get(k) == v, (k, meta)
    # loaded into a fresh UNet it reproduces the prediction bit for bit
    fresh = lora.load_unet(cfg.SINGLE_FILE_CHECKPOINT_PATH, DEV, unet.cfg, spec, 0, h["final_model"])
    assert torch.equal(fresh.pflat, unet.pflat)
    assert torch.equal(_predict(fresh), _predict(unet))


def test_raven_trains_the_adapters_alone(raven_run):
    r = raven_run
    _check_run(r["h"], r["unet"], r["out"], r["cfg"], r["base0"])


def test_prodigy_trains_the_adapters_alone(tmp_path):
    _check_run(*_run(str(tmp_path), LORA_PARAMS=dict(LORA), SAVE_EVERY_N_STEPS=0, **PRODIGY))


def test_resume_equals_the_uninterrupted_run(raven_run):
    r = raven_run
    out = r["cfg"].OUTPUT_DIR
    h2, unet2, _, _, _ = _run(r["tmp"], LORA_PARAMS=dict(LORA), SAVE_EVERY_N_STEPS=0, RESUME_TRAINING=True,
                              RESUME_MODEL_PATH=os.path.join(out, "mini_run_step_1.safetensors"),
                              RESUME_STATE_PATH=os.path.join(out, "mini_run_training_state_step_1.pt"))
    assert h2["optimizer_step"] == 4 and h2["losses"] == r["h"]["losses"][2:]
    assert torch.equal(unet2.pflat, r["unet"].pflat)


def test_save_merged_writes_a_full_model(raven_run):
    from safetensors.torch import load_file
    from aozora_sdxl_training_amd import checkpoint as C
    r = raven_run
    merged = load_file(os.path.join(r["cfg"].OUTPUT_DIR, "mini_run_merged.safetensors"))
    base = load_file(r["cfg"].SINGLE_FILE_CHECKPOINT_PATH)
    assert set(merged) == set(base)
    adapted = {C.PREFIX + C._sd_name(n[:-len(".lora_A.weight")] + ".weight") for n in r["unet"].lora_state_dict() if n.endswith(".lora_A.weight")}
    assert len(adapted) == 8 * 17 and adapted <= set(base)
    for k in base:
        same = torch.equal(merged[k].float(), base[k].to(torch.bfloat16).float())
        assert same != (k in adapted), k
    # W + s B A formed in fp32 on the CPU and rounded once
    u, s = r["unet"], r["unet"].lora.scale
    n = "mid_block.attentions.0.transformer_blocks.1.attn2.to_v"
    sd, ls = u.state_dict(), u.lora_state_dict()
    want = (sd[n + ".weight"].float().cpu() + s * (ls[n + ".lora_B.weight"].float().cpu() @ ls[n + ".lora_A.weight"].float().cpu())).bfloat16()
    assert torch.equal(merged[C.PREFIX + C._sd_name(n + ".weight")], want)


@pytest.mark.parametrize("over, why", [
    (dict(LORA_PARAMS=dict(rank=8, alpha=4, dropout=0.1)), "unknown key"),
    (dict(LORA_PARAMS=dict(rank=5)), "rank 5"),
    (dict(LORA_PARAMS=dict(rank=128)), "rank 128"),
    (dict(LORA_PARAMS=dict(rank=[8, 16])), "one rank"),
    (dict(LORA_PARAMS=dict(rank=8, alpha=0)), "alpha must be > 0"),
    (dict(LORA_PARAMS=dict(rank=8, targets="no_such_layer")), "selects no"),
    (dict(LORA_PARAMS=dict(rank=8, targets="proj_in")), "out of scope"),
    (dict(LORA_PARAMS=dict(rank=8, targets="ff.net.0.proj")), "out of scope"),
    (dict(LORA_PARAMS=dict(rank=8), RAVEN_PARAMS=dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, debias_strength=0.3, ema_decay=0.999)), "ema_decay"),
], ids=lambda v: v if isinstance(v, str) else "")
def test_refusals_fire_before_a_unet_is_loaded(tmp_path, over, why):
    from test_trainer_gpu import _config
    from aozora_sdxl_training_amd.trainer import train
    cfg = _config(str(tmp_path), "v_prediction", **over)
    assert not os.path.exists(cfg.SINGLE_FILE_CHECKPOINT_PATH)          # loading a UNet would fail with another error
    with pytest.raises(ValueError, match=why):
        train(cfg, unet=None, device=DEV)


def test_more_than_one_process_and_a_mismatched_unet_are_refused(tmp_path):
    from test_trainer_gpu import _base_checkpoint, _config
    from aozora_sdxl_training_amd import checkpoint as C, lora
    from aozora_sdxl_training_amd.trainer import train
    with pytest.raises(ValueError, match="more than one rank"):
        lora.options(types.SimpleNamespace(LORA_PARAMS=dict(LORA)), world=2)
    assert lora.options(types.SimpleNamespace(), world=2) == (None, False) and lora.options(types.SimpleNamespace(LORA_PARAMS={})) == (None, False)
    cfg = _config(str(tmp_path), "v_prediction", LORA_PARAMS=dict(LORA))
    _base_checkpoint(cfg.SINGLE_FILE_CHECKPOINT_PATH, _model())
    plain = C.load_unet(cfg.SINGLE_FILE_CHECKPOINT_PATH, DEV, _model())
    with pytest.raises(ValueError, match="matching spec"):
        train(cfg, unet=plain, device=DEV)


def test_without_lora_params_the_run_is_todays(tmp_path):
    """LORA_PARAMS absent, and LORA_PARAMS = {}: the same run bit for bit, with the reference's full model file and freeze mask.
    Both are the off-path of THIS tree, so the test shows that the two spellings of "off" agree and that "off" keeps the full-model
    file and the freeze keywords; it cannot see a change to the LoRA-off arithmetic.  That is pinned by the tests that existed
    before LoRA (tests/test_trainer_gpu.py's bitwise resume, tests/test_model_gpu.py's oracle parity, the reference goldens), which
    run unchanged, and by the alternated benchmark against the parent recorded in profiles/lora_bench_ab.json."""
    from aozora_sdxl_training_amd import checkpoint as C
    os.makedirs(str(tmp_path / "a")); os.makedirs(str(tmp_path / "b"))
    h0, u0, out0, cfg0, _ = _run(str(tmp_path / "a"), MAX_TRAIN_STEPS=4, SAVE_EVERY_N_STEPS=0)
    h1, u1, out1, _, _ = _run(str(tmp_path / "b"), MAX_TRAIN_STEPS=4, SAVE_EVERY_N_STEPS=0, LORA_PARAMS={})
    assert u0.lora is None and "LoRA" not in out0 + out1
    assert h0["losses"] == h1["losses"] and torch.equal(u0.pflat, u1.pflat) and u0.flat_numel == u1.flat_numel
    frozen = [n for n, p in u0.named_parameters() if not p.requires_grad]
    assert frozen and all(("conv1" in n or "conv2" in n) for n in frozen)
    saved = C.read_unet_state(h0["final_model"], [n for n, _ in u0.named_parameters()])
    assert all(torch.equal(saved[n], p.detach().cpu()) for n, p in u0.named_parameters())
