"""trainer.train with LORA_PARAMS = {rank: 8, scope: "transformer"} over the mini UNet (by the method of tests/test_lora_trainer_gpu.py,
two optimizer steps): every up matrix moves -- the feed-forward, proj_in and proj_out ones included -- the model file holds the
3 x 192 keys of the kohya-ss layout, a resumed run loads it and equals the uninterrupted one, `save_merged` writes W + s B A rounded
once for a feed-forward weight, and scope "attention" writes the file keys of a run without the key."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from test_lora_trainer_gpu import _model, _predict, _run        # noqa: E402

DEV = "cuda:0"
LORA = dict(rank=8, scope="transformer")
NEW_KEYS = ("lora_unet_input_blocks_4_1_proj_in", "lora_unet_input_blocks_4_1_transformer_blocks_0_ff_net_0_proj",
            "lora_unet_middle_block_1_transformer_blocks_0_ff_net_2", "lora_unet_output_blocks_0_1_proj_out")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("lora_ff"))
    h, unet, out, cfg, base0 = _run(tmp, LORA_PARAMS=dict(LORA, save_merged=True), SAVE_EVERY_N_STEPS=1, MAX_TRAIN_STEPS=4)
    return dict(tmp=tmp, h=h, unet=unet, out=out, cfg=cfg, base0=base0)


def test_every_adapter_trains_and_the_file_holds_them_all(run):
    from safetensors import safe_open
    from aozora_sdxl_training_amd import lora
    h, unet, out, cfg, base0 = (run[k] for k in ("h", "unet", "out", "cfg", "base0"))
    assert h["optimizer_step"] == 2 and all(l == l and 0.0 < l < 10.0 for l in h["losses"]) and all(g > 0 for g in h["grad_norms"])
    assert "LoRA is ON" in out and "scope transformer" in out and "192 adapted linears" in out
    lo = unet._slots["conv_out.bias"][0] + 64
    assert torch.equal(unet.pflat[:lo], base0[:lo]), "a frozen base parameter changed"
    assert len(unet.trainable_ranges()) == 1
    lsd = unet.lora_state_dict()
    assert len(lsd) == 384
    still = [n for n, t in lsd.items() if n.endswith(".lora_B.weight") and not bool(t.any())]
    assert not still, f"up matrices that did not move: {still[:4]}"
    want = {}
    for n, t in lsd.items():
        module, _, leaf = n.rpartition(".lora_")
        want[lora.file_key(module) + (".lora_down.weight" if leaf == "A.weight" else ".lora_up.weight")] = tuple(t.shape)
        want[lora.file_key(module) + ".alpha"] = ()
    with safe_open(h["final_model"], framework="pt", device="cpu") as f:
        keys = set(f.keys())
        assert keys == set(want) and len(keys) == 3 * 192
        for k in keys:
            t = f.get_tensor(k)
            assert tuple(t.shape) == want[k] and t.dtype == torch.bfloat16, k
        for k in NEW_KEYS:
            assert {k + ".lora_down.weight", k + ".lora_up.weight", k + ".alpha"} <= keys, k
        assert f.get_tensor(NEW_KEYS[1] + ".lora_up.weight").shape[1] == 8 and f.get_tensor(NEW_KEYS[2] + ".lora_down.weight").shape[0] == 8
        assert f.metadata()["ss_network_module"] == "networks.lora" and f.metadata()["ss_network_dim"] == "8"
    fresh = lora.load_unet(cfg.SINGLE_FILE_CHECKPOINT_PATH, DEV, unet.cfg, unet.lora, 0, h["final_model"])
    assert torch.equal(fresh.pflat, unet.pflat) and torch.equal(_predict(fresh), _predict(unet))


def test_resume_loads_the_file(run):
    out = run["cfg"].OUTPUT_DIR
    h2, unet2, _, _, _ = _run(run["tmp"], LORA_PARAMS=dict(LORA), SAVE_EVERY_N_STEPS=0, MAX_TRAIN_STEPS=4, RESUME_TRAINING=True,
                              RESUME_MODEL_PATH=os.path.join(out, "mini_run_step_1.safetensors"),
                              RESUME_STATE_PATH=os.path.join(out, "mini_run_training_state_step_1.pt"))
    assert h2["optimizer_step"] == 2 and h2["losses"] == run["h"]["losses"][2:]
    assert torch.equal(unet2.pflat, run["unet"].pflat)


def test_save_merged_folds_a_feed_forward_adapter(run):
    from safetensors.torch import load_file
    from aozora_sdxl_training_amd import checkpoint as C
    merged = load_file(os.path.join(run["cfg"].OUTPUT_DIR, "mini_run_merged.safetensors"))
    base = load_file(run["cfg"].SINGLE_FILE_CHECKPOINT_PATH)
    u, s = run["unet"], run["unet"].lora.scale
    sd, ls = u.state_dict(), u.lora_state_dict()
    adapted = {C.PREFIX + C._sd_name(n[:-len(".lora_A.weight")] + ".weight") for n in ls if n.endswith(".lora_A.weight")}
    assert set(merged) == set(base) and len(adapted) == 192 and adapted <= set(base)
    for n in ("mid_block.attentions.0.transformer_blocks.1.ff.net.0.proj", "down_blocks.1.attentions.0.transformer_blocks.0.ff.net.2"):
        want = (sd[n + ".weight"].float().cpu() + s * (ls[n + ".lora_B.weight"].float().cpu() @ ls[n + ".lora_A.weight"].float().cpu())).bfloat16()
        k = C.PREFIX + C._sd_name(n + ".weight")
        assert torch.equal(merged[k], want) and not torch.equal(merged[k].float(), base[k].to(torch.bfloat16).float()), n


def test_scope_attention_writes_the_default_file_keys(run, tmp_path):
    import types
    from safetensors import safe_open
    from aozora_sdxl_training_amd import lora
    keys = []
    for i, hp in enumerate((dict(rank=8), dict(rank=8, scope="attention"))):
        spec = lora.options(types.SimpleNamespace(LORA_PARAMS=hp), cfg=_model())[0]
        unet = lora.load_unet(run["cfg"].SINGLE_FILE_CHECKPOINT_PATH, DEV, _model(), spec, 0)
        path = lora.save_lora_file(tmp_path / f"{i}.safetensors", unet)
        with safe_open(str(path), framework="pt", device="cpu") as f:
            keys.append(sorted(f.keys()))
    assert keys[0] == keys[1] and len(keys[0]) == 3 * 136 and not any("_ff_net_" in k or "_proj_in" in k or "_proj_out" in k for k in keys[0])
