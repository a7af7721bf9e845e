"""stochastic_rounding=True through the optimizer classes and the trainer: the random bits are keyed by the offset in the owner's flat
buffer, so dist.ShardedRaven with one region, with three regions and optimizers.RavenAdamW leave the same parameters bit for bit;
with the flag off every class issues the calls it always issued; a trainer run with RAVEN_PARAMS["stochastic_rounding"] repeats and
resumes bitwise."""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
DEV = "cuda:0"
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, debias_strength=0.3, momentum_dtype=torch.bfloat16)
STEPS = 3


@pytest.fixture(scope="module")
def model():
    """Mini UNet, its initial flat parameters, three synthetic gradients (zero on the channel padding of 4-D weights, as a backward
    leaves it) and the mask of real elements."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import mini_config
    u = AozoraUNet(mini_config(), DEV)
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for n, p in u.named_parameters():
            if "norm" in n:
                p.fill_(1.0 if n.endswith("weight") else 0.0)
            else:
                p.copy_((torch.randn(p.shape, generator=g) * 0.05).bfloat16())
    real = torch.zeros(u.flat_numel, dtype=torch.bfloat16, device=DEV)
    for name, (o, st, shape) in u._slots.items():
        k = 1
        for d in st:
            k *= d
        v = real[o:o + k].view(st)
        (v.permute(0, 3, 1, 2)[:, :shape[1]] if len(st) == 4 else v).fill_(1.0)
    grads = [(torch.randn(u.flat_numel, generator=g) * 1e-2).to(torch.bfloat16).to(DEV) * real for _ in range(STEPS)]
    torch.cuda.synchronize()
    return u, u.pflat.clone(), grads, real


def _reset(u, start):
    u.wait_tail_params()
    torch.cuda.synchronize()
    u.pflat.copy_(start)
    u.mark_params_dirty()
    for p in u.parameters():
        p.requires_grad = True


def _sharded_raven(model, **kw):
    from aozora_sdxl_training_amd.dist import ShardedRaven
    u, start, grads, _ = model
    _reset(u, start)
    opt = ShardedRaven(u, clip_grad_norm=0, force_local=True, **HP, **kw)
    for g in grads:
        opt.zero_grad()
        u.wait_tail_params(); torch.cuda.synchronize()      # the clear may run on the background stream
        u.gflat.copy_(g)
        opt.step()
    u.wait_tail_params(); torch.cuda.synchronize()
    assert opt.step_count == STEPS
    return u.pflat.clone()


def _raven(model, **kw):
    from aozora_sdxl_training_amd.optimizers import RavenAdamW
    u, start, grads, _ = model
    _reset(u, start)
    opt = RavenAdamW([{"params": list(u.parameters()), "lr_scale": 1.0}], **HP, **kw)
    for g in grads:
        opt.zero_grad(set_to_none=True)
        u.gflat.copy_(g)
        u.expose_grads()
        opt.step()
    torch.cuda.synchronize()
    return u.pflat.clone()


def _sharded_titan(model, **kw):
    from aozora_sdxl_training_amd.dist import ShardedTitan
    u, start, grads, _ = model
    _reset(u, start)
    opt = ShardedTitan(u, clip_grad_norm=0, force_local=True, **HP, **kw)
    for g in grads:
        opt.zero_grad()
        u.wait_tail_params(); torch.cuda.synchronize()
        u.gflat.copy_(g)
        opt.accumulate()
        opt.step()
    u.wait_tail_params(); torch.cuda.synchronize()
    return u.pflat.clone()


def _titan(model, **kw):
    from aozora_sdxl_training_amd.optimizers import TitanAdamW
    u, start, grads, _ = model
    _reset(u, start)
    opt = TitanAdamW([{"params": list(u.parameters()), "lr_scale": 1.0}], **HP, **kw)
    try:
        for g in grads:
            opt.zero_grad(set_to_none=True)
            u.gflat.copy_(g)
            opt.offload_flat(u)
            opt.step()
        torch.cuda.synchronize()
        return u.pflat.clone()
    finally:
        opt.close()


SR = dict(stochastic_rounding=True, sr_seed=42)


@pytest.fixture(scope="module")
def raven_runs(model):
    """Every Raven form once, flag off (constructed WITHOUT the new arguments) and on."""
    return dict(off_1=_sharded_raven(model, regions=1), off_3=_sharded_raven(model, regions=3), off_dropin=_raven(model, state_on_device=True),
                on_1=_sharded_raven(model, regions=1, **SR), on_3=_sharded_raven(model, regions=3, **SR),
                on_dropin=_raven(model, state_on_device=True, **SR))


def test_raven_forms_agree_bitwise_with_stochastic_rounding(model, raven_runs):
    r = raven_runs
    assert torch.equal(r["off_1"], r["off_3"]) and torch.equal(r["off_1"], r["off_dropin"])          # the identity as it stands today
    assert torch.equal(r["on_1"], r["on_3"]), "three regions draw other bits than one"
    assert torch.equal(r["on_1"], r["on_dropin"]), "RavenAdamW draws other bits than ShardedRaven"
    moved = float((r["on_1"] != r["off_1"]).float().mean())
    assert 0.2 < moved < 0.8, moved                                                                    # the option selects results
    _, start, _, real = model
    pad = real == 0
    assert bool((r["on_1"][pad] == 0).all()) and bool((start[pad] == 0).all())                        # padding stays zero


def test_raven_host_state_pipeline_agrees(model, raven_runs):
    """RavenAdamW's default residency (pinned host moments through az_raven_step_sr) against the resident form."""
    assert torch.equal(_raven(model, **SR), raven_runs["on_dropin"])
    assert torch.equal(_raven(model), raven_runs["off_dropin"])


def test_flag_off_is_the_default_and_seed_matters(model, raven_runs):
    assert torch.equal(_sharded_raven(model, regions=1, stochastic_rounding=False, sr_seed=42), raven_runs["off_1"])
    assert torch.equal(_raven(model, state_on_device=True, stochastic_rounding=False, sr_seed=7), raven_runs["off_dropin"])
    assert torch.equal(_sharded_raven(model, regions=1, **SR), raven_runs["on_1"])                   # repeats
    other = _sharded_raven(model, regions=1, stochastic_rounding=True, sr_seed=43)
    assert not torch.equal(other, raven_runs["on_1"])


def test_titan_forms_agree_bitwise(model):
    """dist.ShardedTitan (fp32 accumulator in HBM) against optimizers.TitanAdamW (fp32 gradients in pinned host memory) without a
    clip: one micro-step per window, so both hold float(g); flag off as the control, then flag on."""
    off_s, off_h = _sharded_titan(model), _titan(model)
    assert torch.equal(off_s, off_h)
    on_s, on_h = _sharded_titan(model, **SR), _titan(model, **SR)
    assert torch.equal(on_s, on_h)
    assert not torch.equal(on_s, off_s)
    assert torch.equal(_sharded_titan(model, stochastic_rounding=False), off_s)


def test_foreign_tensors_take_their_own_domain():
    """Two equal contiguous tensors with equal gradients: domain = 1 + position keeps their bits apart; the flag off keeps them
    equal; a repeat draws the same bits."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd.optimizers import RavenAdamW

    def run(**kw):
        g = torch.Generator().manual_seed(3)
        w = (torch.randn(4099, generator=g) * 0.05).bfloat16()
        gr = (torch.randn(4099, generator=g) * 1e-2).bfloat16()
        a, b = (torch.nn.Parameter(w.clone().to(DEV)) for _ in range(2))
        opt = RavenAdamW([{"params": [a, b], "lr_scale": 1.0}], state_on_device=True, **HP, **kw)
        for _ in range(2):
            a.grad, b.grad = gr.to(DEV), gr.to(DEV)
            opt.step()
        torch.cuda.synchronize()
        return a.detach().clone(), b.detach().clone()
    a0, b0 = run()
    assert torch.equal(a0, b0)
    a1, b1 = run(**SR)
    assert not torch.equal(a1, b1) and not torch.equal(a1, a0)
    a2, b2 = run(**SR)
    assert torch.equal(a1, a2) and torch.equal(b1, b2)


# ---------------- the trainer ------------------------------------------------------------------------------------------------------------
def _config(tmp, **over):
    import synth_cache
    synth_cache.build(os.path.join(tmp, "set0"), n_items=23, json_mode=False, seed=0, rf=False)
    cfg = types.SimpleNamespace(
        INSTANCE_DATASETS=[{"path": os.path.join(tmp, "set0"), "repeats": 1}], CAPTION_SOURCE_TYPE="txt", SEED=42,
        MAX_TRAIN_STEPS=8, BATCH_SIZE=2, GRADIENT_ACCUMULATION_STEPS=2, PREDICTION_TYPE="v_prediction", CLIP_GRAD_NORM=1.0,
        LR_CUSTOM_CURVE=[[0.0, 0.0], [0.2, 1e-4], [1.0, 2e-5]], LEARNING_RATE=1e-4, OPTIMIZER_TYPE="raven",
        RAVEN_PARAMS=dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, debias_strength=0.3, momentum_dtype="bfloat16"),
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


def test_trainer_with_stochastic_rounding_repeats_and_resumes_bitwise(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd import checkpoint as C
    from aozora_sdxl_training_amd.trainer import train
    from aozora_sdxl_training_amd.telemetry import Reporter
    from aozora_sdxl_training_amd.unet_spec import mini_config
    model = mini_config(ctx_dim=64, pooled=32)
    SRP = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, debias_strength=0.3, momentum_dtype="bfloat16", stochastic_rounding=True)

    def run(tag, path=None, **over):
        tmp = str(tmp_path / tag)
        os.makedirs(tmp)
        cfg = _config(tmp, **over)
        _base_checkpoint(cfg.SINGLE_FILE_CHECKPOINT_PATH, model)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            unet = C.load_unet(path(cfg) if path else cfg.SINGLE_FILE_CHECKPOINT_PATH, DEV, model)
            h = train(cfg, unet=unet, device=DEV, reporter=Reporter(cfg.MAX_TRAIN_STEPS, asynchronous=False))
        torch.cuda.synchronize()
        assert h["micro_step"] == 8 and h["optimizer_step"] == 4
        return cfg, h, unet.pflat.clone(), buf.getvalue()

    cfg_a, h_a, p_a, out_a = run("a", RAVEN_PARAMS=SRP)
    assert all(l == l and 0.0 < l < 10.0 for l in h_a["losses"]) and len(h_a["grad_norms"]) == 4
    assert out_a.count("stochastic rounding of the bf16 parameter update is ON") == 1
    _, h_off, p_off, out_off = run("off")
    assert "stochastic rounding" not in out_off
    assert not torch.equal(p_a, p_off)                                     # the option selects results
    _, h_b, p_b, _ = run("b", RAVEN_PARAMS=SRP)
    assert torch.equal(p_a, p_b) and h_a["losses"] == h_b["losses"]       # repeats bitwise
    # resumed from the checkpoint written after optimizer step 2: the same seed and the restored step count draw the same bits
    _, h_r, p_r, _ = run("r", RAVEN_PARAMS=SRP, RESUME_TRAINING=True, SAVE_EVERY_N_STEPS=0,
                         RESUME_MODEL_PATH=os.path.join(cfg_a.OUTPUT_DIR, "mini_run_step_2.safetensors"),
                         RESUME_STATE_PATH=os.path.join(cfg_a.OUTPUT_DIR, "mini_run_training_state_step_2.pt"),
                         path=lambda c: c.RESUME_MODEL_PATH)
    assert h_r["losses"] == h_a["losses"][4:] and h_r["grad_norms"] == h_a["grad_norms"][2:]
    assert torch.equal(p_r, p_a)
