"""trainer.train with LORA_PARAMS "scale_weight_norms" over the mini UNet (scope "unet", rank 4, conv_rank 8; the method of
tests/test_lora_trainer_gpu.py): the limit is taken from a run WITHOUT the key (the median module norm after two optimizer
steps), so a four-step run with it scales some modules and leaves others alone at every step.  The three history lists, the limit on the reported and on the saved adapters, the
file's metadata, the checkpoint line, a resumed run bitwise the uninterrupted one, the key absent / None = today's history keys and
bits, and under "master_weights" and prodigy every adapter element is bf16_rn of its master."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import elem_ref as R                                              # noqa: E402
import lora_maxnorm_ref as N                                      # noqa: E402
from test_lora_trainer_gpu import PRODIGY, _run                   # noqa: E402

DEV = "cuda:0"
LORA = dict(rank=4, scope="unet", conv_rank=8)
MODULES = 192 + 2 * 17 + 11
RAVEN_MASTER = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, debias_strength=0.3, momentum_dtype="bfloat16", master_weights=True)


def _mats(lsd, spec):
    out = {}
    for n, t in lsd.items():
        if n.endswith(".lora_A.weight"):
            m = n[:-len(".lora_A.weight")]
            A = t.double().cpu().numpy()
            out[m] = (A.reshape(A.shape[0], -1), lsd[m + ".lora_B.weight"].double().cpu().numpy().reshape(-1, A.shape[0]), spec.scale_of(m))
    return out


def _norms(lsd, spec):
    return {m: float(np.sqrt(N.n2_gram(A, B, s))) for m, (A, B, s) in _mats(lsd, spec).items()}


def _slack(lsd, spec):
    """2^-8 + the largest bound_q over the modules (tests/test_lora_maxnorm_model_gpu.py derives the sum)."""
    return 2.0 ** -8 + max(N.q_bound(A, B, s) for A, B, s in _mats(lsd, spec).values() if B.any())


@pytest.fixture(scope="module")
def off_run(tmp_path_factory):
    """Two optimizer steps without the key: the module norms the limit is taken from."""
    tmp = str(tmp_path_factory.mktemp("maxnorm_off"))
    h, unet, out, cfg, _ = _run(tmp, LORA_PARAMS=dict(LORA), SAVE_EVERY_N_STEPS=0, MAX_TRAIN_STEPS=4)
    norms = np.array(sorted(_norms(unet.lora_state_dict(), unet.lora).values()))
    assert len(norms) == MODULES and norms[0] > 0
    return dict(h=h, unet=unet, out=out, limit=float(np.float32(np.median(norms))))


@pytest.fixture(scope="module")
def on_run(tmp_path_factory, off_run):
    tmp = str(tmp_path_factory.mktemp("maxnorm_on"))
    hp = dict(LORA, scale_weight_norms=off_run["limit"])
    h, unet, out, cfg, base0 = _run(tmp, LORA_PARAMS=hp, SAVE_EVERY_N_STEPS=1)
    return dict(tmp=tmp, h=h, unet=unet, out=out, cfg=cfg, base0=base0, hp=hp, limit=off_run["limit"])


def test_history_and_the_limit(on_run):
    h, unet, out, limit = on_run["h"], on_run["unet"], on_run["out"], on_run["limit"]
    assert h["optimizer_step"] == 4 and all(l == l and 0.0 < l < 10.0 for l in h["losses"])
    ks, avg, mx = h["lora_keys_scaled"], h["lora_avg_key_norm"], h["lora_max_key_norm"]
    print("keys scaled", ks, "avg", avg, "max", mx, "limit", limit)
    assert len(ks) == len(avg) == len(mx) == 4 == len(h["grad_norms"])
    assert all(isinstance(k, int) and 0 <= k <= MODULES for k in ks) and ks[-1] > 0 and sum(ks[1:]) > 0
    lsd = unet.lora_state_dict()
    slack = _slack(lsd, unet.lora)
    assert all(0.0 <= a <= m <= limit for a, m in zip(avg, mx))          # the reported norm is min(norm, limit)
    assert mx[-1] == limit                                                # ... and some module was at it
    norms = _norms(lsd, unet.lora)
    assert max(norms.values()) <= limit * (1.0 + slack), (max(norms.values()), limit)
    assert f"LoRA max-norm is ON (scale_weight_norms {limit:g}, {MODULES} modules" in out
    assert out.count("lora max-norm: ") == 4 and f"(lora max-norm: {ks[-1]} keys scaled" in out
    lo = unet._slots["conv_out.bias"][0] + 64
    assert torch.equal(unet.pflat[:lo], on_run["base0"][:lo]), "a frozen base parameter changed"


def test_saved_adapters_satisfy_the_limit_and_carry_the_key(on_run):
    from safetensors import safe_open
    from aozora_sdxl_training_amd import lora
    unet, limit, h = on_run["unet"], on_run["limit"], on_run["h"]
    with safe_open(h["final_model"], framework="pt", device="cpu") as f:
        assert float(f.metadata()["ss_scale_weight_norms"]) == limit
    fresh = lora.load_unet(on_run["cfg"].SINGLE_FILE_CHECKPOINT_PATH, DEV, unet.cfg, unet.lora, 0, h["final_model"])
    assert torch.equal(fresh.pflat, unet.pflat)
    lsd = fresh.lora_state_dict()
    assert max(_norms(lsd, unet.lora).values()) <= limit * (1.0 + _slack(lsd, unet.lora))


def test_resume_is_bitwise_the_uninterrupted_run(on_run):
    out = on_run["cfg"].OUTPUT_DIR
    h2, unet2, _, _, _ = _run(on_run["tmp"], LORA_PARAMS=dict(on_run["hp"]), SAVE_EVERY_N_STEPS=0, RESUME_TRAINING=True,
                              RESUME_MODEL_PATH=os.path.join(out, "mini_run_step_2.safetensors"),
                              RESUME_STATE_PATH=os.path.join(out, "mini_run_training_state_step_2.pt"))
    h = on_run["h"]
    assert h2["optimizer_step"] == 4 and h2["losses"] == h["losses"][4:] and h2["grad_norms"] == h["grad_norms"][2:]
    for k in ("lora_keys_scaled", "lora_avg_key_norm", "lora_max_key_norm"):
        assert h2[k] == h[k][2:], k
    assert torch.equal(unet2.pflat, on_run["unet"].pflat)


def test_without_the_key_the_run_is_todays(off_run, tmp_path):
    """The key absent and the key None: the same history keys -- none of the three lists -- and the same bits (both are the off-path of
    this tree; the tests that existed before pin its arithmetic)."""
    h1, u1, out1, _, _ = _run(str(tmp_path), LORA_PARAMS=dict(LORA, scale_weight_norms=None), SAVE_EVERY_N_STEPS=0, MAX_TRAIN_STEPS=4)
    h0, u0 = off_run["h"], off_run["unet"]
    assert set(h0) == set(h1) and not any(k.startswith("lora_") for k in h0)
    assert "max-norm" not in off_run["out"] + out1 and u0.lora == u1.lora and u0.lora.max_norm is None
    assert h0["losses"] == h1["losses"] and h0["grad_norms"] == h1["grad_norms"] and torch.equal(u0.pflat, u1.pflat)
    from safetensors import safe_open
    with safe_open(h1["final_model"], framework="pt", device="cpu") as f:
        assert "ss_scale_weight_norms" not in f.metadata()


def _adapter_range(unet):
    (a, b), = unet.trainable_ranges()
    return a, b


def test_raven_master_weights_are_scaled_with_the_adapters(off_run, tmp_path):
    hp = dict(LORA, scale_weight_norms=off_run["limit"] * 0.5)
    h, unet, out, cfg, _ = _run(str(tmp_path), LORA_PARAMS=hp, SAVE_EVERY_N_STEPS=1, MAX_TRAIN_STEPS=4, RAVEN_PARAMS=dict(RAVEN_MASTER))
    assert h["optimizer_step"] == 2 and sum(h["lora_keys_scaled"]) > 0 and "fp32 masters scaled with them" in out
    st = torch.load(os.path.join(cfg.OUTPUT_DIR, "mini_run_training_state_step_2.pt"), map_location="cpu", weights_only=False)
    ms = st["master_state"]
    a, b = _adapter_range(unet)
    assert [tuple(r) for rs in ms["ranges"] for r in rs] == [(a, b)] and ms["master"].numel() == b - a
    want = R.f32_to_bf16_bits(ms["master"].float())
    assert torch.equal(unet.pflat[a:b].cpu(), want), "an adapter element is not bf16_rn of its master"
    assert bool((ms["master"] != unet.pflat[a:b].cpu().float()).any())          # the master keeps bits below the bf16 grid
    lsd = unet.lora_state_dict()
    assert max(_norms(lsd, unet.lora).values()) <= hp["scale_weight_norms"] * (1.0 + _slack(lsd, unet.lora))


def test_prodigy_master_is_scaled_with_the_adapters(off_run, tmp_path):
    # prodigy moves the adapters at its own pace: the limit is a fraction of what ITS first two steps reach
    hp = dict(LORA, scale_weight_norms=5e-5)
    h, unet, out, cfg, _ = _run(str(tmp_path), LORA_PARAMS=hp, SAVE_EVERY_N_STEPS=1, MAX_TRAIN_STEPS=4, **PRODIGY)
    assert h["optimizer_step"] == 2 and "fp32 masters scaled with them" in out
    print("prodigy keys scaled", h["lora_keys_scaled"], "max", h["lora_max_key_norm"])
    st = torch.load(os.path.join(cfg.OUTPUT_DIR, "mini_run_training_state_step_2.pt"), map_location="cpu", weights_only=False)
    os_ = st["optimizer_state"]
    a, b = _adapter_range(unet)
    assert [tuple(r) for r in os_["ranges"]] == [("flat", a, b)] and os_["w"].numel() == b - a
    assert torch.equal(unet.pflat[a:b].cpu(), R.f32_to_bf16_bits(os_["w"].float())), "an adapter element is not bf16_rn of prodigy's master"
    lsd = unet.lora_state_dict()
    assert max(_norms(lsd, unet.lora).values()) <= 5e-5 * (1.0 + _slack(lsd, unet.lora))
    assert sum(h["lora_keys_scaled"]) > 0
