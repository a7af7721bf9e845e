"""trainer.train with LORA_PARAMS "dora" over the mini UNet (the method of tests/test_lora_trainer_gpu.py, four optimizer steps) with
raven and once with prodigy (always an fp32 master): finite losses, magnitudes that move, the norm pass once per optimizer step and
never per micro-step, the `dora_scale` keys of the saved file, a resumed run bitwise the uninterrupted one, `save_merged` against the
float64 merged weight within one bf16 rounding, and the refusals that fire before a UNet is loaded."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import dora_ref as D                                              # noqa: E402
import elem_ref as R                                              # noqa: E402
from test_lora_trainer_gpu import _predict, _run                  # noqa: E402

DEV = "cuda:0"
LORA = dict(rank=8, alpha=4, scope="transformer", dora=True)
MODULES = 192
# A magnitude is a bf16 number near 1 (spacing 2^-8 to 2^-7): the step must be of that size for it to move in four optimizer steps, under
# raven's bf16-only update as well as through prodigy's fp32 master (whose step is d0 x the curve at first)
RAVEN = dict(LR_CUSTOM_CURVE=[[0.0, 2e-2], [1.0, 1e-2]], LEARNING_RATE=2e-2)
PRODIGY = dict(OPTIMIZER_TYPE="prodigy", PRODIGY_PARAMS=dict(d0=2e-2, weight_decay=0.01, safeguard_warmup=True), LR_CUSTOM_CURVE=[[0.0, 1.0], [1.0, 0.5]])


def _counted_run(tmp, **over):
    """_run with every az_dora_norm_bf16 launch counted (ops.dora_norm is the only way to it)."""
    from aozora_sdxl_training_amd import ops
    calls, real = [], ops.dora_norm

    def counting(table, tiles, init=False, stream=None):
        calls.append(bool(init))
        return real(table, tiles, init, stream)
    ops.dora_norm = counting
    try:
        return _run(tmp, **over) + (calls,)
    finally:
        ops.dora_norm = real


@pytest.fixture(scope="module")
def raven_run(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("dora_raven"))
    h, unet, out, cfg, base0, calls = _counted_run(tmp, LORA_PARAMS=dict(LORA, save_merged=True), SAVE_EVERY_N_STEPS=1, **RAVEN)
    return dict(tmp=tmp, h=h, unet=unet, out=out, cfg=cfg, base0=base0, calls=calls)


def _check_run(h, unet, out, cfg, base0, calls):
    from safetensors import safe_open
    from aozora_sdxl_training_amd import lora
    assert h["optimizer_step"] == 4 and len(h["losses"]) == 8 and all(l == l and 0.0 < l < 10.0 for l in h["losses"]) and all(g > 0 for g in h["grad_norms"])
    assert "LoRA is ON" in out and f"DoRA is ON ({MODULES} magnitude vectors" in out
    # one pass with init when the adapters were drawn (none behind the load of the base before it), then exactly one per optimizer
    # step: none per micro-step (8 of them)
    assert calls == [True] + [False] * 4, calls
    lo = unet._slots["conv_out.bias"][0] + 64
    assert torch.equal(unet.pflat[:lo], base0[:lo]), "a frozen base parameter changed"
    names = [n for n, p in unet.named_parameters() if p.requires_grad]
    lsd = unet.lora_state_dict()
    assert set(names) == set(lsd) and len(unet.trainable_ranges()) == 1 and sum(n.endswith(".dora_scale") for n in names) == MODULES
    moved = 0
    for n, t in lsd.items():
        if n.endswith(".dora_scale"):
            o = unet._slots[n][0]
            moved += int(not torch.equal(t.flatten(), base0[o:o + t.numel()]))
    assert moved == MODULES, f"{MODULES - moved} magnitude vectors did not move"
    # the gains on the device are those of the final parameters (the pass behind the last step)
    g_dev, inv_dev = unet.dora.g.clone(), unet.dora.inv.clone()
    unet.dora.refresh()
    torch.cuda.synchronize()
    assert torch.equal(unet.dora.g, g_dev) and torch.equal(unet.dora.inv, inv_dev)
    with safe_open(h["final_model"], framework="pt", device="cpu") as f:
        keys = set(f.keys())
        assert len(keys) == 4 * MODULES and sum(k.endswith(".dora_scale") for k in keys) == MODULES
        k = "lora_unet_input_blocks_4_1_transformer_blocks_0_attn1_to_q.dora_scale"
        assert k in keys and tuple(f.get_tensor(k).shape) == (128, 1) and f.get_tensor(k).dtype == torch.bfloat16
        assert '"dora_wd": "True"' in f.metadata()["ss_network_args"]
    fresh = lora.load_unet(cfg.SINGLE_FILE_CHECKPOINT_PATH, DEV, unet.cfg, unet.lora, 0, h["final_model"])
    assert torch.equal(fresh.pflat, unet.pflat) and torch.equal(fresh.dora.g, unet.dora.g)
    assert torch.equal(_predict(fresh), _predict(unet))


def test_raven_trains_adapters_and_magnitudes(raven_run):
    r = raven_run
    _check_run(r["h"], r["unet"], r["out"], r["cfg"], r["base0"], r["calls"])


def test_prodigy_trains_adapters_and_magnitudes(tmp_path):
    h, unet, out, cfg, base0, calls = _counted_run(str(tmp_path), LORA_PARAMS=dict(LORA), SAVE_EVERY_N_STEPS=1, **PRODIGY)
    _check_run(h, unet, out, cfg, base0, calls)
    # the fp32 master saw the initial magnitudes: every adapter element is bf16_rn of it
    st = torch.load(os.path.join(cfg.OUTPUT_DIR, "mini_run_training_state_step_4.pt"), map_location="cpu", weights_only=False)
    (a, b), = unet.trainable_ranges()
    w = st["optimizer_state"]["w"]
    assert w.numel() == b - a and torch.equal(unet.pflat[a:b].cpu(), R.f32_to_bf16_bits(w.float()))


def test_resume_is_bitwise_the_uninterrupted_run(raven_run):
    r = raven_run
    out = r["cfg"].OUTPUT_DIR
    h2, unet2, _, _, _, calls = _counted_run(r["tmp"], LORA_PARAMS=dict(LORA), SAVE_EVERY_N_STEPS=0, RESUME_TRAINING=True, **RAVEN,
                                             RESUME_MODEL_PATH=os.path.join(out, "mini_run_step_2.safetensors"),
                                             RESUME_STATE_PATH=os.path.join(out, "mini_run_training_state_step_2.pt"))
    assert h2["optimizer_step"] == 4 and h2["losses"] == r["h"]["losses"][4:] and h2["grad_norms"] == r["h"]["grad_norms"][2:]
    assert calls == [False] * 3, calls                    # the load of the adapters, then one per optimizer step (3 and 4)
    assert torch.equal(unet2.pflat, r["unet"].pflat) and torch.equal(unet2.dora.g, r["unet"].dora.g)


def test_save_merged_is_the_float64_merged_weight_rounded_once(raven_run):
    from safetensors.torch import load_file
    from aozora_sdxl_training_amd import checkpoint as C
    r = raven_run
    merged = load_file(os.path.join(r["cfg"].OUTPUT_DIR, "mini_run_merged.safetensors"))
    base = load_file(r["cfg"].SINGLE_FILE_CHECKPOINT_PATH)
    assert set(merged) == set(base)
    u = r["unet"]
    sd, ls = u.state_dict(), u.lora_state_dict()
    mods = [n[:-len(".dora_scale")] for n in ls if n.endswith(".dora_scale")]
    assert len(mods) == MODULES
    for n in mods:
        want = D.merged_weight(sd[n + ".weight"].cpu(), ls[n + ".lora_A.weight"].cpu(), ls[n + ".lora_B.weight"].cpu(), ls[n + ".dora_scale"].cpu(),
                               u.lora.scale_of(n))
        got = merged[C.PREFIX + C._sd_name(n + ".weight")].double()
        # one bf16 rounding of the fp32 value.  That value (lora.merge_into: B A, W + s B A, the row norm over K terms, m / n, the product,
        # all in fp32) is within (K + 2 r + 8) 2^-24 (m / n) V of the float64 one, V = |W| + |s| |B||A| >= |W + s B A|: r roundings in an
        # element of the sum, at most K / 2 + r relative in the norm, three more for quotient, product and the sum itself
        Wd, Ad, Bd = sd[n + ".weight"].cpu().double(), ls[n + ".lora_A.weight"].cpu().double(), ls[n + ".lora_B.weight"].cpu().double()
        V = Wd.abs() + abs(u.lora.scale_of(n)) * (Bd.abs() @ Ad.abs())
        gain = (ls[n + ".dora_scale"].cpu().double().abs() / D.LR.merged_weight(Wd, Ad, Bd, u.lora.scale_of(n)).norm(dim=1))[:, None]
        tol = R.half_ulp_bf16(want) + (Wd.shape[1] + 2 * Ad.shape[0] + 8) * D.U * gain * V
        assert bool(((got - want).abs() <= tol).all()), n
    adapted = {C.PREFIX + C._sd_name(n + ".weight") for n in mods}
    for k in base:
        if k not in adapted:
            assert torch.equal(merged[k].float(), base[k].to(torch.bfloat16).float()), k


@pytest.mark.parametrize("over, why", [
    (dict(rank=8, dora=True, scope="unet"), "convolutions"),
    (dict(rank=8, dora=True, network_dropout=0.1), "dropout"),
    (dict(rank=8, dora=True, rank_dropout=0.1), "dropout"),
    (dict(rank=8, dora=True, module_dropout=0.1), "dropout"),
    (dict(rank=8, dora=True, scale_weight_norms=1.0), "max-norm"),
], ids=["scope-unet", "network_dropout", "rank_dropout", "module_dropout", "scale_weight_norms"])
def test_refusals_fire_before_a_unet_is_loaded(tmp_path, over, why):
    from test_trainer_gpu import _config
    from aozora_sdxl_training_amd.trainer import train
    cfg = _config(str(tmp_path), "v_prediction", LORA_PARAMS=over)
    assert not os.path.exists(cfg.SINGLE_FILE_CHECKPOINT_PATH)          # loading a UNet would fail with another error
    with pytest.raises(ValueError, match="follow-up") as e:
        train(cfg, unet=None, device=DEV)
    assert why in str(e.value)
