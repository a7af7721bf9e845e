"""trainer.train with LORA_PARAMS = {rank: 4, scope: "unet", conv_rank: 8} over the mini UNet (by the method of
tests/test_lora_ff_trainer_gpu.py, two optimizer steps): every up matrix moves -- those of conv1, conv2 and conv_shortcut included --
the model file holds exactly the 3 x 237 keys of the kohya-ss layout with the convolutions' 4-D shapes, a resumed run loads it and is
bitwise the uninterrupted one, `save_merged` writes W + s B (*) A rounded once for a 3x3 convolution and a shortcut, and the
refusals fire before a UNet is loaded."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from test_lora_trainer_gpu import _predict, _run        # noqa: E402

DEV = "cuda:0"
LORA = dict(rank=4, scope="unet", conv_rank=8)
MODULES = 192 + 2 * 17 + 11
NEW_KEYS = ("lora_unet_input_blocks_1_0_in_layers_2", "lora_unet_input_blocks_4_0_skip_connection", "lora_unet_middle_block_2_out_layers_3",
            "lora_unet_output_blocks_8_0_in_layers_2")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("lora_conv"))
    h, unet, out, cfg, base0 = _run(tmp, LORA_PARAMS=dict(LORA, save_merged=True), SAVE_EVERY_N_STEPS=1, MAX_TRAIN_STEPS=4)
    return dict(tmp=tmp, h=h, unet=unet, out=out, cfg=cfg, base0=base0)


def test_every_adapter_trains_and_the_file_holds_them_all(run):
    from safetensors import safe_open
    from aozora_sdxl_training_amd import lora
    h, unet, out, cfg, base0 = (run[k] for k in ("h", "unet", "out", "cfg", "base0"))
    assert h["optimizer_step"] == 2 and all(l == l and 0.0 < l < 10.0 for l in h["losses"]) and all(g > 0 for g in h["grad_norms"])
    assert "LoRA is ON" in out and "scope unet" in out and "203 adapted linears" in out and "34 adapted 3x3 convolutions at conv_rank 8" in out
    lo = unet._slots["conv_out.bias"][0] + 64
    assert torch.equal(unet.pflat[:lo], base0[:lo]), "a frozen base parameter changed"
    assert len(unet.trainable_ranges()) == 1
    lsd = unet.lora_state_dict()
    assert len(lsd) == 2 * MODULES
    still = [n for n, t in lsd.items() if n.endswith(".lora_B.weight") and not bool(t.any())]
    assert not still, f"up matrices that did not move: {still[:4]}"
    want = {}
    for n, t in lsd.items():
        module, _, leaf = n.rpartition(".lora_")
        shape = tuple(t.shape)
        if ".resnets." in module and len(shape) == 2:        # a convolution's up matrix, and both matrices of the 1x1 shortcut
            shape += (1, 1)
        want[lora.file_key(module) + (".lora_down.weight" if leaf == "A.weight" else ".lora_up.weight")] = shape
        want[lora.file_key(module) + ".alpha"] = ()
    with safe_open(h["final_model"], framework="pt", device="cpu") as f:
        keys = set(f.keys())
        assert keys == set(want) and len(keys) == 3 * MODULES
        for k in keys:
            t = f.get_tensor(k)
            assert tuple(t.shape) == want[k] and t.dtype == torch.bfloat16, k
        for k in NEW_KEYS:
            assert {k + ".lora_down.weight", k + ".lora_up.weight", k + ".alpha"} <= keys, k
        assert tuple(f.get_tensor(NEW_KEYS[0] + ".lora_down.weight").shape) == (8, 64, 3, 3) and float(f.get_tensor(NEW_KEYS[0] + ".alpha")) == 4.0
        assert tuple(f.get_tensor(NEW_KEYS[1] + ".lora_down.weight").shape) == (4, 64, 1, 1) and tuple(f.get_tensor(NEW_KEYS[1] + ".lora_up.weight").shape) == (128, 4, 1, 1)
        meta = f.metadata()
        assert meta["ss_network_module"] == "networks.lora" and meta["ss_network_dim"] == "4"
        assert json.loads(meta["ss_network_args"]) == {"conv_dim": "8", "conv_alpha": "4"}
    fresh = lora.load_unet(cfg.SINGLE_FILE_CHECKPOINT_PATH, DEV, unet.cfg, unet.lora, 0, h["final_model"])
    assert torch.equal(fresh.pflat, unet.pflat) and torch.equal(_predict(fresh), _predict(unet))


def test_resume_is_bitwise_the_uninterrupted_run(run):
    out = run["cfg"].OUTPUT_DIR
    h2, unet2, _, _, _ = _run(run["tmp"], LORA_PARAMS=dict(LORA), SAVE_EVERY_N_STEPS=0, MAX_TRAIN_STEPS=4, RESUME_TRAINING=True,
                              RESUME_MODEL_PATH=os.path.join(out, "mini_run_step_1.safetensors"),
                              RESUME_STATE_PATH=os.path.join(out, "mini_run_training_state_step_1.pt"))
    assert h2["optimizer_step"] == 2 and h2["losses"] == run["h"]["losses"][2:]
    assert torch.equal(unet2.pflat, run["unet"].pflat)


def test_save_merged_folds_the_convolution_adapters(run):
    from safetensors.torch import load_file
    from aozora_sdxl_training_amd import checkpoint as C
    merged = load_file(os.path.join(run["cfg"].OUTPUT_DIR, "mini_run_merged.safetensors"))
    base = load_file(run["cfg"].SINGLE_FILE_CHECKPOINT_PATH)
    u, spec = run["unet"], run["unet"].lora
    sd, ls = u.state_dict(), u.lora_state_dict()
    adapted = {C.PREFIX + C._sd_name(n[:-len(".lora_A.weight")] + ".weight") for n in ls if n.endswith(".lora_A.weight")}
    assert set(merged) == set(base) and len(adapted) == MODULES and adapted <= set(base)
    for n in ("mid_block.resnets.0.conv1", "up_blocks.1.resnets.2.conv2", "down_blocks.1.resnets.0.conv_shortcut"):
        W, A, Bm = (t.double().cpu() for t in (sd[n + ".weight"], ls[n + ".lora_A.weight"], ls[n + ".lora_B.weight"]))
        s = spec.scale_of(n)
        assert (s, A.shape[0]) == ((1.0, 4) if n.endswith("_shortcut") else (0.5, 8))        # alpha defaults to rank; conv_alpha to alpha
        ref = W + s * (Bm @ A.reshape(A.shape[0], -1)).reshape(W.shape)              # float64; the file holds the fp32 merge rounded once
        k = C.PREFIX + C._sd_name(n + ".weight")
        got = merged[k].double()
        assert tuple(got.shape) == tuple(W.shape)
        assert bool(((got - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-6).all()), n         # one bf16 rounding of a sum formed in fp32
        assert float((got - W).abs().max()) > 0 and not torch.equal(merged[k].float(), base[k].to(torch.bfloat16).float()), n


@pytest.mark.parametrize("hp, why", [
    (dict(rank=8, scope="unet", conv_rank=5), "conv_rank 5"),
    (dict(rank=8, scope="unet", conv_alpha=0), "conv_alpha"),
    (dict(rank=8, conv_rank=8), "scope"),
    (dict(rank=8, scope="unet", conv_dim=8), "unknown key"),
    (dict(rank=8, scope="unet", targets="time_emb_proj"), "out of scope"),
    (dict(rank=8, scope="unet", targets="downsamplers.0.conv"), "out of scope"),
    (dict(rank=8, scope="unet", targets="upsamplers"), "out of scope"),
    (dict(rank=8, scope="unet", targets="conv_in"), "out of scope"),
    (dict(rank=8, scope="unet", targets="conv_out"), "out of scope"),
], ids=lambda v: v if isinstance(v, str) else "")
def test_refusals_fire_before_a_unet_is_loaded(tmp_path, hp, why):
    from test_trainer_gpu import _config
    from aozora_sdxl_training_amd.trainer import train
    cfg = _config(str(tmp_path), "v_prediction", LORA_PARAMS=hp)
    assert not os.path.exists(cfg.SINGLE_FILE_CHECKPOINT_PATH)          # loading a UNet would fail with another error
    with pytest.raises(ValueError, match=why):
        train(cfg, unet=None, device=DEV)
