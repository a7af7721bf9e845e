"""tests/lora_ref.py without a GPU: the backward formulas of the LoRA contract agree with torch.autograd in float64, the B = 0
identity, the merged weight, the oracle UNet with adapters, the exactness condition and the share of outputs that need rounding for
every case tests/test_lora_gpu.py runs, and the argument checks of the az_lora_* entry points (they return before any HIP call)."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import gemm_ref as R                # noqa: E402
import lora_ref as LR               # noqa: E402
import test_lora_gpu as T           # noqa: E402


def _layer(M=37, K=24, N=40, r=8, seed=7):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(x=mk(M, K), W=mk(N, K), A=mk(r, K), B=mk(N, r), dy=mk(M, N))


def test_backward_formulas_agree_with_autograd():
    d, s = _layer(), 0.75
    x, A, B = (d[k].clone().requires_grad_(True) for k in ("x", "A", "B"))
    y = x @ d["W"].t() + s * ((x @ A.t()) @ B.t())
    y.backward(d["dy"])
    y_base, dx_base = d["x"] @ d["W"].t(), d["dy"] @ d["W"]
    u, y_ref = LR.lora_forward(d["x"], y_base, d["A"], d["B"], s, rounded=False)
    du, dx, dA, dB = LR.lora_backward(d["x"], u, d["dy"], dx_base, d["A"], d["B"], s, rounded=False)
    for got, want in ((y_ref, y.detach()), (dx, x.grad), (dA, A.grad), (dB, B.grad)):
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    # accumulation over micro-steps: the previous gradient is added, not overwritten
    _, _, dA2, dB2 = LR.lora_backward(d["x"], u, d["dy"], dx_base, d["A"], d["B"], s, dA_prev=dA, dB_prev=dB, rounded=False)
    assert torch.allclose(dA2, 2 * dA, rtol=1e-12) and torch.allclose(dB2, 2 * dB, rtol=1e-12)


def test_zero_up_matrix_is_the_identity():
    d = _layer()
    x, W, A, dy = (d[k].bfloat16() for k in ("x", "W", "A", "dy"))
    B = torch.zeros(40, 8, dtype=torch.bfloat16)
    y_base = LR.bf(x.double() @ W.double().t())
    u, y = LR.lora_forward(x, y_base, A, B, 2.0)
    assert torch.equal(y, y_base)
    dx_base = LR.bf(dy.double() @ W.double())
    du, dx, dA, dB = LR.lora_backward(x, u, dy, dx_base, A, B, 2.0)
    assert torch.equal(dx, dx_base) and not bool(du.any()) and not bool(dA.any()) and bool(dB.any())


def test_merged_weight_gives_the_adapted_forward():
    d, s = _layer(), 16.0 / 8
    y = d["x"] @ d["W"].t() + s * ((d["x"] @ d["A"].t()) @ d["B"].t())
    ym = d["x"] @ LR.merged_weight(d["W"], d["A"], d["B"], s).t()
    assert float((y - ym).abs().max()) <= 1e-12 * float(y.abs().max())


def test_ref_unet_with_adapters():
    from oracle.unet_ref import RefUNet, init_params, mini_config
    cfg = mini_config()
    p = {k: v.double() for k, v in init_params(cfg, seed=3).items()}
    g = torch.Generator().manual_seed(1)
    targets = [n[:-7] for n in p if n.endswith(".weight") and (".attn1.to_" in n or ".attn2.to_" in n)]
    assert targets and len(targets) % 8 == 0
    r = 4
    for n in targets:
        N, K = p[n + ".weight"].shape
        p[n + ".lora_A.weight"] = (torch.rand(r, K, generator=g, dtype=torch.float64) * 2 - 1) / K ** 0.5
        p[n + ".lora_B.weight"] = torch.zeros(N, r, dtype=torch.float64)
    args = (torch.randn(1, 4, 8, 8, generator=g, dtype=torch.float64), torch.tensor([500]),
            torch.randn(1, 7, cfg.cross_attention_dim, generator=g, dtype=torch.float64),
            torch.randn(1, cfg.pooled_dim, generator=g, dtype=torch.float64), torch.tensor([[64., 64, 0, 0, 64, 64]], dtype=torch.float64))
    base = {k: v for k, v in p.items() if ".lora_" not in k}
    y0 = RefUNet(cfg, base).forward(*args)
    assert torch.equal(LR.LoraRefUNet(cfg, p, 2.0).forward(*args), y0)              # B = 0
    for n in targets:
        p[n + ".lora_B.weight"] = 0.05 * torch.randn(p[n + ".lora_B.weight"].shape, generator=g, dtype=torch.float64)
    y1 = LR.LoraRefUNet(cfg, p, 2.0).forward(*args)
    assert not torch.equal(y1, y0)
    merged = dict(base)
    for n in targets:
        merged[n + ".weight"] = LR.merged_weight(p[n + ".weight"], p[n + ".lora_A.weight"], p[n + ".lora_B.weight"], 2.0)
    ym = RefUNet(cfg, merged).forward(*args)
    assert float((ym - y1).abs().max()) <= 1e-12 * max(1.0, float(y1.abs().max()))


# ---------------- the GPU test's case tables ---------------------------------------------------------------------------------------
def _covers(values, seen, what):
    assert set(values) <= set(seen), f"{what}: {sorted(set(values) - set(seen))} not covered"


def test_tables_cross_every_edge():
    for name, cases, rows, widths, ranks in (("down", T.DOWN_CASES, "M", ("K",), "r"), ("up", T.UP_CASES, "M", ("N",), "r"),
                                             ("wgrad", T.WGRAD_CASES, "M", ("nb",), "ns")):
        _covers((1, 63, 64, 65, 154, 257), [getattr(c, rows) for c in cases], name + " M")
        _covers((64, 72, 320), [getattr(c, w) for c in cases for w in widths], name + " width")
        _covers((4, 8, 16, 64), [getattr(c, ranks) for c in cases], name + " rank")
        _covers((1, 2, 3), [c.parts for c in cases], name + " parts")
        _covers(LR.EXACT_SCALES, [c.s for c in cases], name + " s")
    _covers((True, False), [c.acc for c in T.WGRAD_CASES], "wgrad accumulate")
    _covers((True, False), [c.small_major for c in T.WGRAD_CASES], "wgrad layout")


@pytest.mark.parametrize("c", T.DOWN_CASES, ids=T.cid)
def test_down_cases_are_exact_and_need_rounding(c):
    d = T.make_down(c)               # lora_ref.down asserts exact_ok_scaled
    assert LR.exact_ok_scaled(d["S"] / c.s, c.s) and R.inexact_share(d["ref"]) > 0


@pytest.mark.parametrize("c", T.UP_CASES, ids=T.cid)
def test_up_cases_are_exact_and_need_rounding(c):
    d = T.make_up(c)
    assert R.inexact_share(d["ref"]) > 0


@pytest.mark.parametrize("c", T.WGRAD_CASES, ids=T.cid)
def test_wgrad_cases_are_exact_and_need_rounding(c):
    d = T.make_wgrad(c)
    assert R.inexact_share(d["ref"]) > 0


def test_exactness_condition_refuses_other_scales_and_large_sums():
    S = torch.full((2, 2), 100.0, dtype=torch.float64)
    assert LR.exact_ok_scaled(S, 0.5)
    with pytest.raises(AssertionError):
        LR.exact_ok_scaled(S, 1.0 / 3.0)
    with pytest.raises(AssertionError):
        LR.exact_ok_scaled(S * 2.0 ** 20, 1.0)
    with pytest.raises(AssertionError):
        LR.exact_ok_scaled(S * 2.0 ** 17, 2.0, prev=torch.full((2, 2), 8.0))      # 16 S < 2^24 but 32 (2 S + 8) is not


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Host-only: every call below fails its argument check, so no HIP call is made."""
    from aozora_sdxl_training_amd._lib import lib
    fn = lib()._fn
    p = ctypes.c_void_p(1 << 20)            # aligned, never dereferenced
    down = lambda M=16, K=64, r=8, parts=1, ldo=8: fn["az_lora_down_bf16"](M, K, r, parts, 1.0, p, K, 0, p, K, r * K, p, ldo, None)
    assert down(K=60) == -1110 and down(r=6) == -1110 and down(r=2) == -1110 and down(r=68, parts=3, ldo=204) == -1110
    assert down(parts=4, ldo=32) == -1110 and down(ldo=6) == -1112
    assert fn["az_lora_down_bf16"](16, 64, 8, 1, 1.0, ctypes.c_void_p((1 << 20) + 8), 64, 0, p, 64, 512, p, 8, None) == -1111
    up = lambda N=64, r=8, ldy=64: fn["az_lora_up_bf16"](16, N, r, 1, 1.0, p, r, r, p, r, N * r, p, ldy, N, None)
    assert up(N=66) == -1113 and up(r=196) == -1113 and up(ldy=60) == -1115
    wg = lambda ns=8, nb=64, ws=1 << 20: fn["az_lora_wgrad_bf16"](16, ns, nb, 1, 1.0, p, ns, ns, p, nb, nb, p, nb, 1, ns * nb, 0, p, ws, None)
    assert wg(ns=6) == -1116 and wg(nb=60) == -1116 and wg(ws=64) == -1119


# ---------------- LORA_PARAMS, the preset key and the adapter file (host-side code of aozora_sdxl_training_amd/lora.py) ------------------
def _cfg(**hp):
    import types
    return types.SimpleNamespace(LORA_PARAMS=hp)


def test_lora_params_are_parsed_and_refused_as_specified():
    import types
    from aozora_sdxl_training_amd import lora
    from aozora_sdxl_training_amd.unet_spec import LoraSpec, SDXL_BASE, lora_modules, lora_table
    assert lora.options(types.SimpleNamespace()) == (None, False) and lora.options(_cfg()) == (None, False)
    spec, merged = lora.options(_cfg(rank=16, alpha=16, targets="to_q, to_v", save_merged=False))
    assert spec == LoraSpec(16, 16.0, "to_q, to_v") and merged is False and spec.scale == 1.0
    assert lora.options(_cfg(rank="32", alpha="8", save_merged="true")) == (LoraSpec(32, 8.0, ""), True)
    assert lora.options(_cfg(rank=4))[0].alpha == 4.0
    assert len(lora_modules(SDXL_BASE, LoraSpec(16, 16.0))) == 560 and len(lora_table(SDXL_BASE, LoraSpec(16, 16.0))) == 1120
    assert len(lora_modules(SDXL_BASE, LoraSpec(16, 16.0, "attn2.to_k"))) == 70
    for hp, why in ((dict(rank=16, dropout=0.1), "unknown key"), (dict(rank=5), "rank 5"), (dict(rank=3.5), "numbers"), (dict(rank=128), "rank 128"),
                    (dict(rank=[4, 8]), "one rank"), (dict(rank=8, alpha=0), "alpha must be > 0"), (dict(rank=8, alpha=-2), "alpha must be > 0"),
                    (dict(rank=8, targets="nothing_here"), "selects no"), (dict(rank=8, targets="proj_out"), "out of scope"),
                    (dict(rank=8, targets="to_q, ff.net.2"), "out of scope")):
        with pytest.raises(ValueError, match=why):
            lora.options(_cfg(**hp))
    with pytest.raises(ValueError, match="more than one rank"):
        lora.options(_cfg(rank=8), world=2)
    with pytest.raises(ValueError, match="ema_decay"):
        lora.options(_cfg(rank=8), ema_decay=0.999)


def test_preset_key_is_read_beside_the_optimizer_dictionaries(tmp_path):
    import json
    from aozora_sdxl_training_amd.config import TrainingConfig, flat_defaults
    path = tmp_path / "preset.json"
    path.write_text(json.dumps({"config_version": 1, "active_mode": "sdxl",
                                "sdxl": {"sdxl_lora_params": {"rank": 16, "alpha": 16, "targets": "attn1", "save_merged": False}}}))
    cfg = TrainingConfig(config_path=str(path))
    assert cfg.LORA_PARAMS == {"rank": 16, "alpha": 16, "targets": "attn1", "save_merged": False}
    assert "LORA_PARAMS" not in cfg.as_dict() and "LORA_PARAMS" not in flat_defaults()        # kept out of the reference's key table
    path.write_text(json.dumps({"config_version": 1, "active_mode": "sdxl", "sdxl": {}}))
    assert TrainingConfig(config_path=str(path)).LORA_PARAMS == {}


def test_adapter_file_keys_shapes_and_metadata(tmp_path):
    from safetensors import safe_open
    from safetensors.torch import save_file
    from aozora_sdxl_training_amd import lora
    from aozora_sdxl_training_amd.unet_spec import LoraSpec, SDXL_BASE, lora_table
    spec = LoraSpec(4, 2.0, "transformer_blocks.0.attn")
    table = lora_table(SDXL_BASE, spec)
    assert table[0] == ("down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q.lora_A.weight", (4, 640))
    assert [n.split(".attn1.")[1] for n, _ in table[:8]] == [p + s for s in (".lora_A.weight", ".lora_B.weight") for p in ("to_q", "to_k", "to_v")] + \
        ["to_out.0.lora_A.weight", "to_out.0.lora_B.weight"]                                   # the A's of a fused group side by side
    assert table[9][0].endswith("attn2.to_q.lora_B.weight") and table[10] == (table[10][0], (4, 2048)) and table[13][1] == (640, 4)
    state = {n: torch.full(s, 0.5) for n, s in table}
    tensors = lora.file_tensors(state, spec)
    assert len(tensors) == 3 * len(table) // 2
    k = "lora_unet_input_blocks_4_1_transformer_blocks_0_attn1_to_q"
    assert tensors[k + ".lora_down.weight"].shape == (4, 640) and tensors[k + ".lora_up.weight"].shape == (640, 4)
    assert tensors[k + ".alpha"].dim() == 0 and float(tensors[k + ".alpha"]) == 2.0 and all(t.dtype == torch.bfloat16 for t in tensors.values())
    assert "lora_unet_middle_block_1_transformer_blocks_0_attn2_to_out_0.lora_up.weight" in tensors
    assert "lora_unet_output_blocks_0_1_transformer_blocks_0_attn2_to_k.lora_down.weight" in tensors
    save_file(tensors, str(tmp_path / "a.safetensors"), metadata=lora.file_metadata(spec))
    with safe_open(str(tmp_path / "a.safetensors"), framework="pt", device="cpu") as f:
        meta = f.metadata()
    assert meta["ss_network_module"] == "networks.lora" and meta["ss_network_dim"] == "4" and meta["ss_network_alpha"] == "2"
    assert meta["ss_base_model_version"] == "sdxl_base_v1-0"
