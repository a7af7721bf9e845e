"""trainer.train with the three LoRA dropout keys over the mini UNet (tests/test_lora_trainer_gpu._run): four micro-steps at GA 2, the
"LoRA is ON" line names the dropouts, the adapter file carries their metadata beside unchanged tensors, the run is reproducible, and a
run stopped after the first optimizer step and resumed equals the uninterrupted one bit for bit -- the masks depend on SEED and the
global micro-step alone, nothing of them is in a training state."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_lora_trainer_gpu import _run, DEV      # noqa: E402

LORA = dict(rank=8, alpha=4, network_dropout=0.1, rank_dropout=0.25, module_dropout=0.5)
RUN = dict(MAX_TRAIN_STEPS=4, GRADIENT_ACCUMULATION_STEPS=2, LR_CUSTOM_CURVE=[[0.0, 1e-4], [1.0, 2e-5]])       # no warm-up from 0: the first optimizer step moves the up matrices


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("lora_dropout"))
    h, unet, out, cfg, base0 = _run(tmp, LORA_PARAMS=dict(LORA), SAVE_EVERY_N_STEPS=1, **RUN)
    return dict(tmp=tmp, h=h, unet=unet, out=out, cfg=cfg, base0=base0)


def test_trains_with_the_three_keys_and_writes_their_metadata(run):
    from safetensors import safe_open
    from aozora_sdxl_training_amd import lora
    h, unet, out, cfg = run["h"], run["unet"], run["out"], run["cfg"]
    spec = unet.lora
    assert (spec.dropout, spec.rank_dropout, spec.module_dropout) == (0.1, 0.25, 0.5) and unet.adapters.seed == cfg.SEED
    assert h["optimizer_step"] == 2 and len(h["losses"]) == 4 and all(l == l and 0.0 < l < 10.0 for l in h["losses"]) and all(g > 0 for g in h["grad_norms"])
    line = [l for l in out.splitlines() if "LoRA is ON" in l]
    assert len(line) == 1 and "dropout 0.1 / rank_dropout 0.25 / module_dropout 0.5" in line[0]
    lo = unet._slots["conv_out.bias"][0] + 64
    assert torch.equal(unet.pflat[:lo], run["base0"][:lo]), "a frozen base parameter changed"
    lsd = unet.lora_state_dict()
    with safe_open(h["final_model"], framework="pt", device="cpu") as f:
        meta = f.metadata()
        assert meta["ss_network_dropout"] == "0.1" and json.loads(meta["ss_network_args"]) == {"rank_dropout": "0.25", "module_dropout": "0.5"}
        assert meta["ss_network_dim"] == "8" and meta["ss_network_alpha"] == "4"
        assert len(list(f.keys())) == 3 * (len(lsd) // 2)          # the tensors of the file do not change: down, up, alpha per module
    fresh = lora.load_unet(cfg.SINGLE_FILE_CHECKPOINT_PATH, DEV, unet.cfg, spec, cfg.SEED, h["final_model"])      # read_lora_file ignores the new metadata
    assert torch.equal(fresh.pflat, unet.pflat)


def test_dropout_changes_the_run_and_the_run_is_reproducible(run, tmp_path):
    os.makedirs(str(tmp_path / "again")); os.makedirs(str(tmp_path / "plain"))
    h1, u1, _, _, _ = _run(str(tmp_path / "again"), LORA_PARAMS=dict(LORA), SAVE_EVERY_N_STEPS=0, **RUN)
    assert h1["losses"] == run["h"]["losses"] and torch.equal(u1.pflat, run["unet"].pflat)
    h0, u0, out0, _, _ = _run(str(tmp_path / "plain"), LORA_PARAMS=dict(rank=8, alpha=4), SAVE_EVERY_N_STEPS=0, **RUN)
    assert "rank_dropout" not in out0 and not torch.equal(u0.pflat, run["unet"].pflat)
    assert h0["losses"][0] == run["h"]["losses"][0]          # the up matrices start at zero: the first prediction has no adapter term to mask
    assert h0["losses"][2:] != run["h"]["losses"][2:]


def test_resume_equals_the_uninterrupted_run(run):
    out = run["cfg"].OUTPUT_DIR
    h2, unet2, _, _, _ = _run(run["tmp"], LORA_PARAMS=dict(LORA), SAVE_EVERY_N_STEPS=0, RESUME_TRAINING=True,
                              RESUME_MODEL_PATH=os.path.join(out, "mini_run_step_1.safetensors"),
                              RESUME_STATE_PATH=os.path.join(out, "mini_run_training_state_step_1.pt"), **RUN)
    assert h2["optimizer_step"] == 2 and h2["losses"] == run["h"]["losses"][2:]
    assert torch.equal(unet2.pflat, run["unet"].pflat)
