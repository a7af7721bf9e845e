"""Whole-step parity and executor checks on latent sizes whose sides are not multiples of 4 (mini SDXL-topology UNet, B = 2):
the up path returns to the geometry of every level on the way down through size-targeted nearest upsamples, as diffusers'
UNet2DConditionModel.forward does (tests/oddsize_ref.py restates that rule on top of the oracle).

Gates: prediction <= 1.5e-2; gradient vector <= max(1.5e-2, 1.5x the bf16 oracle's deviation); EVERY parameter <= max(5e-2, 2x
the bf16 oracle's deviation for that tensor); loss and gradient norm each within max(3e-3, 2x the bf16 oracle's own relative
deviation from the fp32 oracle on the same inputs) -- at these shapes the reference dataflow alone sits at 2.6e-3 ... 2.7e-3 in
v-prediction loss, so a fixed 3e-3 would test the rounding, not the code."""
import contextlib
import io
import json
import math
import os
import types
from pathlib import Path

import pytest
import torch

from tests.oddsize_ref import OddSizeRefUNet
from tests.test_arena_gpu import check_bound, run_order, same
from tests.test_model_gpu import OUT, _inputs, _mini, _rel      # OUT: where the existing parity test writes its measured values

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ODD = (18, 10)


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from oracle.unet_ref import init_params, param_table
    pc, oc = _mini()
    params = {k: v.bfloat16().float() for k, v in init_params(oc, seed=1234).items()}
    g = torch.Generator().manual_seed(99)       # norms / biases non-trivial so their gradients are exercised (as tests/test_model_gpu.py)
    for k in params:
        if "norm" in k and k.endswith(".weight"):
            params[k] = (1 + 0.1 * torch.randn(params[k].shape, generator=g)).bfloat16().float()
        if "norm" in k and k.endswith(".bias"):
            params[k] = (0.1 * torch.randn(params[k].shape, generator=g)).bfloat16().float()
    unet = AozoraUNet(pc, DEV)
    assert [n for n, _ in unet._table] == [n for n, _ in param_table(oc)]
    unet.load_state_dict(params)
    return pc, oc, params, unet


def _oracle(oc, params, mode, bf16, args):
    from oracle.step_ref import RefTrainer
    t = RefTrainer(oc, params, mode=mode, bf16=bf16, ga=1, clip=1.0)
    t.net = OddSizeRefUNet(oc, t.params)
    loss = t.micro_step(*args)
    return t, loss


@pytest.mark.parametrize("mode", ["epsilon", "v_prediction", "rectified_flow"])
@pytest.mark.parametrize("h,w", [(26, 22), (21, 19), (18, 10)])
def test_micro_step_matches_oddsize_oracle(setup, h, w, mode):
    from aozora_sdxl_training_amd.train_step import TrainStep
    pc, oc, params, unet = setup
    B = 2
    lat, noise, ctx, pooled, tid, ts, jit = _inputs(B, h, w, pc)
    args = (lat, noise, ts, ctx, pooled, tid, jit)
    ref, l_ref = _oracle(oc, params, mode, False, args)
    refb, l_refb = _oracle(oc, params, mode, True, args)
    g_ref, g_b = ref.grads(), refb.grads()

    unet.zero_grad()
    step = TrainStep(unet, mode=mode, grad_accum=1, use_graph=False)
    loss = step.micro_step(lat.to(DEV), noise.to(DEV), ts, ctx.to(DEV), pooled.to(DEV), tid.to(DEV), jit)
    step.synchronize()
    l_hip = loss.item()
    unet.expose_grads()
    pred = step.last_pred_nhwc.view(B, h, w, 4).permute(0, 3, 1, 2).float().cpu()
    rows = []
    sq_h = sq_r = sq_d = sq_db = sq_b = 0.0
    for name, p in unet.named_parameters():
        gh, gr, gb = p.grad.float().cpu(), g_ref[name].float(), g_b[name].float()
        rows.append((name, _rel(gh, gr), gr.norm().item(), _rel(gb, gr)))
        sq_h += gh.double().pow(2).sum().item(); sq_r += gr.double().pow(2).sum().item(); sq_b += gb.double().pow(2).sum().item()
        sq_d += (gh - gr).double().pow(2).sum().item()
        sq_db += (gb - gr).double().pow(2).sum().item()
    gn_h, gn_r, gn_b = math.sqrt(sq_h), math.sqrt(sq_r), math.sqrt(sq_b)
    worst = max(rows, key=lambda r: r[1])
    rep = dict(shape=[h, w], mode=mode, loss_hip=l_hip, loss_fp32=l_ref, loss_bf16_oracle=l_refb, pred_rel=_rel(pred, ref.last_pred),
               pred_rel_bf16_oracle_vs_fp32=_rel(refb.last_pred, ref.last_pred), gradnorm_hip=gn_h, gradnorm_fp32=gn_r,
               gradnorm_bf16_oracle=gn_b, worst_param=worst[0], worst_rel=worst[1],
               grad_vector_rel=math.sqrt(sq_d / sq_r), grad_vector_rel_bf16_oracle=math.sqrt(sq_db / sq_r),
               loss_rel=abs(l_hip - l_ref) / abs(l_ref), loss_rel_bf16_oracle=abs(l_refb - l_ref) / abs(l_ref),
               gradnorm_rel=abs(gn_h - gn_r) / gn_r, gradnorm_rel_bf16_oracle=abs(gn_b - gn_r) / gn_r)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, f"oddsize_parity_{h}x{w}_{mode}.json"), "w") as f:
        json.dump(dict(summary=rep, per_param=sorted(rows, key=lambda r: -r[1])[:40]), f, indent=1)
    print(rep)
    assert math.isfinite(l_hip) and pred.shape == ref.last_pred.shape
    assert rep["pred_rel"] <= 1.5e-2, rep
    assert rep["loss_rel"] <= max(3e-3, 2 * rep["loss_rel_bf16_oracle"]), rep
    assert rep["gradnorm_rel"] <= max(3e-3, 2 * rep["gradnorm_rel_bf16_oracle"]), rep
    assert rep["grad_vector_rel"] <= max(1.5e-2, 1.5 * rep["grad_vector_rel_bf16_oracle"]), rep
    assert len(rows) == len(params) and all(nr > 1e-6 for _, _, nr, _ in rows), "every parameter takes part in the per-parameter gate"
    bad = [(n, e, eb) for n, e, nr, eb in rows if e > max(5e-2, 2 * eb)]
    assert not bad, bad[:10]


def test_every_executor_gives_the_same_bits_on_an_odd_size(setup):
    """Eager issue, the launch tape replayed from Python, the native tape and the hipGraph: bit-identical loss and flat gradient;
    so is the copying form of the skip concatenations (ExecPolicy.cat_inplace = False)."""
    from aozora_sdxl_training_amd.train_step import TrainStep
    from aozora_sdxl_training_amd.unet import AozoraUNet, ExecPolicy
    pc, oc, params, _ = setup
    lat, noise, ctx, pooled, tid, ts, jit = _inputs(2, *ODD, pc, seed=11)
    args = (lat.to(DEV), noise.to(DEV), ts, ctx.to(DEV), pooled.to(DEV), tid.to(DEV), jit)
    results = {}
    for tag, policy, graph in [("eager", ExecPolicy(host_tape=False), False), ("python replay", ExecPolicy(native_tape=False), False),
                               ("native tape", ExecPolicy(), False), ("graph", ExecPolicy(), True),
                               ("copying concat", ExecPolicy(cat_inplace=False, host_tape=False), False)]:
        unet = AozoraUNet(pc, DEV, policy=policy).load_state_dict(params)
        step = TrainStep(unet, mode="v_prediction", grad_accum=1, use_graph=graph)
        runs = []
        for i in range(4):          # run 0 allocates, run 1 records / captures, runs 2 and 3 replay
            unet.zero_grad()
            l = step.micro_step(*args).item()
            step.synchronize()
            runs.append((l, unet.gflat.clone()))
        bk = step.last_bucket
        if tag in ("eager", "copying concat"):
            assert bk.tape is None and bk.graph is None
        elif tag == "graph":
            assert bk.graph is not None
        else:
            assert bk.tape is not None and (bk.ntape is not None) == (tag == "native tape")
        results[tag] = runs
    first = results["eager"][0]
    assert math.isfinite(first[0]) and float(first[1].float().abs().max()) > 0
    for tag, runs in results.items():
        for i, (l, g) in enumerate(runs):
            assert l == first[0] and torch.equal(g, first[1]), (tag, i)


def test_interleaving_an_odd_size_with_other_buckets_changes_no_bit():
    a, b, c = ODD, (16, 16), (24, 16)
    order = [a, b, a, c, b, a, c, b, a, c]
    unet, mixed, _ = run_order(order)
    ab = check_bound(unet)
    assert ab["generation"] <= 3 and len(ab["arena"]) == 1 and len(ab["need"]) == 3
    for bucket in (a, b, c):
        idx = [i for i, s in enumerate(order) if s == bucket]
        _, alone, _ = run_order([bucket] * len(idx), seeds=idx)
        same([mixed[i] for i in idx], alone)


@pytest.mark.parametrize("up_to", [None, (9, 6), (10, 5), (9, 5)])
def test_standalone_upsample_layer_takes_a_target(setup, up_to):
    """unet.upsample (the stand-alone layer beside the gather form of unet.conv) and its tape entry, against autograd."""
    import torch.nn.functional as F
    from aozora_sdxl_training_amd.unet import Act, AozoraUNet
    from tests.oddsize_ref import cropped_fold
    unet = AozoraUNet(setup[0], DEV)
    B, H, W, C = 2, 5, 3, 16
    g = torch.Generator().manual_seed(5)
    xh = torch.randn(B, H, W, C, generator=g).bfloat16()
    unet.begin_step((B, H, W, 77, "call"))
    x = Act(xh.to(DEV).view(B * H * W, C))
    y, geom = unet.upsample(x, (B, H, W), up_to=up_to)
    Ho, Wo = up_to if up_to is not None else (2 * H, 2 * W)
    assert geom == (B, Ho, Wo)
    ref = F.interpolate(xh.float().permute(0, 3, 1, 2), size=(Ho, Wo), mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(y.t.view(B, Ho, Wo, C).cpu().float(), ref)
    dy = torch.randn(B, Ho, Wo, C, generator=g).bfloat16()
    y.g = dy.to(DEV).view(B * Ho * Wo, C)
    unet._tape[-1]()
    torch.cuda.synchronize()
    assert torch.equal(x.g.view(B, H, W, C).cpu(), cropped_fold(dy.permute(0, 3, 1, 2), H, W).permute(0, 2, 3, 1).bfloat16())


@pytest.mark.parametrize("h,w", [(3, 16), (16, 3), (2, 2)])
def test_a_side_below_4_raises_before_any_launch(setup, h, w):
    from aozora_sdxl_training_amd._lib import AozoraError, lib
    from aozora_sdxl_training_amd.train_step import TrainStep
    pc, oc, params, unet = setup
    lat, noise, ctx, pooled, tid, ts, jit = _inputs(2, h, w, pc)
    step = TrainStep(unet, mode="epsilon", grad_accum=1, use_graph=False)
    pools = set(unet._pools)
    L = lib()
    L.recorder = []
    try:
        with pytest.raises(AozoraError, match=f"{h}x{w}"):
            step.micro_step(lat.to(DEV), noise.to(DEV), ts, ctx.to(DEV), pooled.to(DEV), tid.to(DEV), jit)
        assert L.recorder == []          # no entry point was called
    finally:
        L.recorder = None
    assert not step._buckets and set(unet._pools) == pools
    with pytest.raises(AozoraError, match=f"{h}x{w}"):
        unet(lat.to(DEV), ts, ctx.to(DEV), added_cond_kwargs={"text_embeds": pooled.to(DEV), "time_ids": tid.to(DEV)})
    assert set(unet._pools) == pools


# ---- through the trainer: a cache in the reference's format (layout of tests/golden/synth_cache.py) with two 9:5 buckets ---------
TRAINER_BUCKETS = [(144, 80), (80, 144), (128, 128)]         # (w, h) in pixels = 8 x latent: latents 10x18, 18x10, 16x16
CACHE_DIR = ".precomputed_embeddings_cache_standard_sdxl"


def _build_cache(root, n_items=18, seed=0):
    cache = Path(root) / CACHE_DIR
    cache.mkdir(parents=True, exist_ok=True)
    g = torch.Generator().manual_seed(1000 + seed)
    files = []
    for k in range(n_items):
        w, h = TRAINER_BUCKETS[k % len(TRAINER_BUCKETS)]
        rel = os.path.join(f"sub{k % 3}", f"Img_{k:03d}.png")
        stem = rel[:-4].replace(os.sep, "_")
        meta = dict(relative_path=rel, original_size=(w * 2 + k, h * 2 + 3), scaled_size=(w + (k % 5), h + (k % 3)), target_size=(w, h),
                    crop_coords=(k % 4, (k * 3) % 7), bucket_variant_index=0)
        lat = cache / f"{stem}_lat.pt"
        torch.save({"latents": torch.randn(4, h // 8, w // 8, generator=g).to(torch.bfloat16), "cache_options": {"cache_schema_version": 13}}, lat)
        te = cache / f"{stem}_te.pt"
        torch.save(dict(meta, original_stem=Path(rel).stem, caption_type="txt", caption=f"caption {k}",
                        embeds=torch.randn(77, 64, generator=g).to(torch.bfloat16), pooled=torch.randn(32, generator=g).to(torch.bfloat16),
                        cache_options={"cache_schema_version": 13}), te)
        files.append(dict(meta, te_path=str(te), lat_path=str(lat), image_file_signature=None, caption_file_signature=None, caption_signature=None))
    torch.save({"version": 13, "cache_options": {"cache_schema_version": 13}, "files": files[::-1]}, cache / "dataset_index.pt")
    torch.save({"embeds": torch.randn(1, 77, 64, generator=g).to(torch.bfloat16), "pooled": torch.randn(1, 32, generator=g).to(torch.bfloat16)},
               cache / "null_embeds.pt")


def test_trainer_runs_a_cache_with_odd_size_buckets(tmp_path):
    from safetensors.torch import save_file
    from aozora_sdxl_training_amd import checkpoint as C
    from aozora_sdxl_training_amd.telemetry import Reporter
    from aozora_sdxl_training_amd.trainer import train
    from aozora_sdxl_training_amd.unet_spec import mini_config, param_table
    model = mini_config(ctx_dim=64, pooled=32)
    tmp = str(tmp_path)
    _build_cache(os.path.join(tmp, "set0"))
    g = torch.Generator().manual_seed(3)
    km = C.unet_key_mapping([n for n, _ in param_table(model)])
    t = {km[n]: ((torch.ones(s) if n.endswith("weight") else torch.zeros(s)) if "norm" in n else torch.randn(*s, generator=g) * 0.05).to(torch.bfloat16)
         for n, s in param_table(model)}
    t["first_stage_model.post_quant_conv.bias"] = torch.zeros(4)
    base = os.path.join(tmp, "base.safetensors")
    save_file(t, base)

    def run(tag):
        cfg = types.SimpleNamespace(
            INSTANCE_DATASETS=[{"path": os.path.join(tmp, "set0"), "repeats": 1}], CAPTION_SOURCE_TYPE="txt", SEED=42,
            MAX_TRAIN_STEPS=8, BATCH_SIZE=2, GRADIENT_ACCUMULATION_STEPS=2, PREDICTION_TYPE="v_prediction", CLIP_GRAD_NORM=1.0,
            LR_CUSTOM_CURVE=[[0.0, 0.0], [0.2, 1e-4], [1.0, 2e-5]], LEARNING_RATE=1e-4, OPTIMIZER_TYPE="raven",
            RAVEN_PARAMS=dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, debias_strength=0.3, momentum_dtype="bfloat16"),
            UNET_EXCLUDE_TARGETS="conv1, conv2", SAVE_EVERY_N_STEPS=0, OUTPUT_DIR=os.path.join(tmp, "out" + tag), OUTPUT_NAME="mini_run",
            SINGLE_FILE_CHECKPOINT_PATH=base, RESUME_TRAINING=False,
            TIMESTEP_ALLOCATION={"bin_size": 100, "counts": [45, 143, 176, 173, 154, 126, 94, 59, 26, 4]},
            TIMESTEP_LOSS_WEIGHT_CURVE={"preset": "bell"}, TIMESTEP_FORCE_IMAGE_BIN_SPREAD=True, NUM_WORKERS=0)
        with contextlib.redirect_stdout(io.StringIO()):
            unet = C.load_unet(base, DEV, model)
            h = train(cfg, unet=unet, device=DEV, reporter=Reporter(cfg.MAX_TRAIN_STEPS, asynchronous=False))
        torch.cuda.synchronize()
        return unet, h
    u1, h1 = run("1")
    assert h1["micro_step"] == 8 and len(h1["losses"]) == 8 and len(h1["grad_norms"]) == 4
    assert all(math.isfinite(l) and 0.0 < l < 10.0 for l in h1["losses"]) and all(0.0 < n < float("inf") for n in h1["grad_norms"])
    ab = check_bound(u1)                 # one arena, no larger than the largest bucket needs
    geoms = {(k[1], k[2]) for k in ab["need"]}
    print(f"buckets {sorted(ab['need'])} arena {ab['arena']} generation {ab['generation']}")
    assert geoms & {(10, 18), (18, 10)}, geoms        # latent sides that are not multiples of 4 went through it
    u2, h2 = run("2")
    assert h2["losses"] == h1["losses"] and h2["grad_norms"] == h1["grad_norms"]
    assert torch.equal(u1.pflat, u2.pflat)
