"""LoRA on the ResnetBlock2D convolutions, without a GPU: tests/lora_conv_ref.py against F.conv2d and its autograd, the case table of
tests/test_lora_conv_gpu.py (exactness, the cap 16 S < 2^24, rounding, that every batch case would change under a tap that crosses
into the next image), scope "unet" (module order, shapes, the counts derived from the parameter table, that the other scopes' tables
are what they were), every refusal of the spec, the options and the reader, the adapter file's keys, shapes and metadata, and the
merged weights against a float64 merge."""
import hashlib
import json
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import gemm_ref as R                # noqa: E402
import lora_ref as LR               # noqa: E402
import lora_conv_ref as CR          # noqa: E402
import test_lora_conv_gpu as T      # noqa: E402

from aozora_sdxl_training_amd import lora                                                                                   # noqa: E402
from aozora_sdxl_training_amd.unet_spec import LORA_SCOPES, LoraSpec, SDXL_BASE, lora_modules, lora_table, mini_config, param_table  # noqa: E402

A_, B_ = ".lora_A.weight", ".lora_B.weight"


# ---------------- the restatements against torch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(1, 1, 1), (2, 3, 5), (1, 7, 1), (3, 4, 4)], ids=str)
def test_restatements_agree_with_conv2d_and_its_autograd(geom):
    g = torch.Generator().manual_seed(sum(geom))
    Bn, H, W = geom
    C, r, s = 6, 3, 0.75
    x = torch.randn(Bn * H * W, C, generator=g, dtype=torch.float64, requires_grad=True)
    a = torch.randn(r, 3, 3, C, generator=g, dtype=torch.float64, requires_grad=True)
    u = s * F.conv2d(CR.to_nchw(x, geom), CR.to_oihw(a), padding=1)
    ref, S = CR.down(x.detach(), a.detach(), geom, s, exact=False)
    assert torch.allclose(ref, u.permute(0, 2, 3, 1).reshape(-1, r), rtol=1e-12, atol=1e-12) and bool((S >= ref.abs() - 1e-12).all())
    du = torch.randn(Bn * H * W, r, generator=g, dtype=torch.float64)
    dx, da = torch.autograd.grad(u, (x, a), CR.to_nchw(du, geom))
    prev_x, prev_a = torch.randn(Bn * H * W, C, generator=g, dtype=torch.float64), torch.randn(r, 3, 3, C, generator=g, dtype=torch.float64)
    assert torch.allclose(CR.dgrad(du, a.detach(), prev_x, geom, s, exact=False)[0], prev_x + dx, rtol=1e-12, atol=1e-12)
    assert torch.allclose(CR.wgrad(du, x.detach(), prev_a, geom, s, exact=False)[0], prev_a + da, rtol=1e-12, atol=1e-12)
    assert torch.allclose(CR.wgrad(du, x.detach(), None, geom, s, exact=False)[0], da, rtol=1e-12, atol=1e-12)


def test_merged_convolution_is_the_adapted_one():
    g = torch.Generator().manual_seed(5)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, W, A, Bm, s = mk(2, 6, 5, 4), mk(10, 6, 3, 3), mk(3, 6, 3, 3), mk(10, 3), 0.5
    y = F.conv2d(x, W, padding=1) + s * F.conv2d(F.conv2d(x, A, padding=1), Bm[:, :, None, None])
    assert torch.allclose(F.conv2d(x, CR.merged_conv_weight(W, A, Bm, s), padding=1), y, rtol=1e-11, atol=1e-11)
    W1, A1 = mk(10, 6, 1, 1), mk(3, 6)
    y1 = F.conv2d(x, W1) + s * F.conv2d(F.conv2d(x, A1[:, :, None, None]), Bm[:, :, None, None])
    assert torch.allclose(F.conv2d(x, CR.merged_conv_weight(W1, A1, Bm, s)), y1, rtol=1e-11, atol=1e-11)


# ---------------- the GPU test's case table -------------------------------------------------------------------------------------------
def test_table_crosses_geometry_channels_and_every_rank():
    assert set(LR.RANKS) == {4, 8, 16, 32, 64} and len(T.CASES) == len(T.GEOMS) * len(T.CINS) * len(LR.RANKS) == len(set(T.CASES))
    assert T.GEOMS == [(1, 1, 1), (1, 1, 9), (1, 7, 1), (2, 3, 5), (3, 4, 4), (2, 5, 13), (1, 8, 8), (2, 16, 9)] and T.CINS == [8, 24, 40, 64, 136]
    assert {(c.B, c.H, c.W, c.Cin, c.r) for c in T.CASES} == {(*g, cin, r) for g in T.GEOMS for cin in T.CINS for r in LR.RANKS}
    assert {c.s for c in T.CASES} == set(LR.EXACT_SCALES)
    for cin in T.CINS:          # every scale meets every channel count and every rank
        assert {c.s for c in T.CASES if c.Cin == cin} == set(LR.EXACT_SCALES)
    pixels = sorted({g[0] * g[1] * g[2] for g in T.GEOMS})
    assert pixels[0] == 1 and any(p < 16 for p in pixels[1:]) and any(16 < p < 64 for p in pixels) and 64 in pixels and pixels[-1] > 4 * 64
    assert 9 * min(T.CINS) < 4 * 32 and any(9 * c % 32 for c in T.CINS) and 9 * max(T.CINS) > 4 * 4 * 32
    assert T.GAUSS == (2, 9, 7, 136, 16, 1.0 / 3.0)


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["down", "dgrad", "wgrad"])
def test_cases_are_exact_and_need_rounding(kind):
    """make() runs lora_ref.exact_ok_scaled on every case (16 S < 2^24 and the scaled sum + previous contents exact)."""
    shares = []
    for c in T.CASES:
        d = T.make(kind, c)
        S = d["S"]
        assert 16.0 * float(S.max()) < 2.0 ** 24
        if kind == 0:
            assert float(S.max()) <= c.s * 144.0 * c.Cin         # operands in [-4, 4]: at most 16 per product, 9 Cin products
        shares.append(R.inexact_share(d["ref"]))
        M = c.B * c.H * c.W
        assert tuple(d["ref"].shape) == ((M, c.r), (M, c.Cin), (c.r, 3, 3, c.Cin))[kind]
    assert max(shares) > 0.05, "no case exercises the rounding of the store"
    accs = {T.make(2, c)["acc"] for c in T.CASES}
    assert accs == {True, False}


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["down", "dgrad", "wgrad"])
def test_a_tap_that_crosses_into_the_next_image_changes_every_batch_case(kind):
    n = 0
    for c in T.CASES:
        if c.B == 1:
            continue
        d, geom, merged = T.make(kind, c), (c.B, c.H, c.W), (1, c.B * c.H, c.W)       # the batch as ONE tall image: taps cross the seams
        if kind == 0:
            wrong = CR.down(d["x"], d["a"], merged, c.s, exact=False)[0]
        elif kind == 1:
            wrong = CR.dgrad(d["du"], d["a"], d["prev"], merged, c.s, exact=False)[0]
        else:
            wrong = CR.wgrad(d["du"], d["x"], d["prev"] if d["acc"] else None, merged, c.s, exact=False)[0]
        assert not torch.equal(R.expected_bits(wrong), R.expected_bits(d["ref"])), c
        n += 1
    assert n == 4 * len(T.CINS) * len(LR.RANKS)


# ---------------- scope "unet" ----------------------------------------------------------------------------------------------------------
def _resnet_counts(cfg):
    names = [n for n, _ in param_table(cfg)]
    return sum(n.endswith(".conv1.weight") and ".resnets." in n for n in names), sum(n.endswith(".conv_shortcut.weight") for n in names)


@pytest.mark.parametrize("cfg", [SDXL_BASE, mini_config()], ids=["sdxl", "mini"])
def test_module_counts_are_derived_from_the_parameter_table(cfg):
    n_res, n_sc = _resnet_counts(cfg)
    n_tr = len(lora_modules(cfg, LoraSpec(16, 16.0, "", "transformer")))
    mods = lora_modules(cfg, LoraSpec(16, 16.0, "", "unet", 16))
    assert len(mods) == n_tr + 2 * n_res + n_sc and len(set(mods)) == len(mods)
    assert [m for m in mods if ".attentions." in m] == lora_modules(cfg, LoraSpec(16, 16.0, "", "transformer"))
    convs = [m for m in mods if ".resnets." in m]
    assert sum(m.endswith(".conv1") for m in convs) == sum(m.endswith(".conv2") for m in convs) == n_res
    assert sum(m.endswith(".conv_shortcut") for m in convs) == n_sc and len(convs) == 2 * n_res + n_sc
    order = {n[:-7]: i for i, (n, _) in enumerate(param_table(cfg)) if n.endswith(".weight")}
    assert [order[m] for m in mods] == sorted(order[m] for m in mods)                  # parameter-table order
    assert not any(k in m for m in mods for k in ("time_emb_proj", "downsamplers", "upsamplers", "conv_in", "conv_out", "time_embedding", "add_embedding"))
    assert len(lora_table(cfg, LoraSpec(16, 16.0, "", "unet", 16))) == 2 * len(mods)
    assert len(lora_modules(cfg, LoraSpec(16, 16.0, "resnets", "unet", 16))) == 2 * n_res + n_sc
    assert len(lora_modules(cfg, LoraSpec(16, 16.0, "conv1, conv_shortcut", "unet", 16))) == n_res + n_sc


def test_sdxl_size_has_the_counted_modules():
    assert _resnet_counts(SDXL_BASE) == _resnet_counts(mini_config()) == (17, 11)
    assert len(lora_modules(SDXL_BASE, LoraSpec(16, 16.0, "", "unet", 16))) == 722 + 45


def test_table_entries_of_the_convolutions():
    spec = LoraSpec(16, 8.0, "", "unet", 4, 2.0)
    assert (spec.rank_of("down_blocks.1.resnets.0.conv1"), spec.alpha_of("down_blocks.1.resnets.0.conv2")) == (4, 2.0)
    assert (spec.rank_of("down_blocks.1.resnets.0.conv_shortcut"), spec.alpha_of("down_blocks.1.resnets.0.conv_shortcut")) == (16, 8.0)
    assert spec.scale_of("mid_block.resnets.0.conv1") == 0.5 and spec.scale_of("mid_block.attentions.0.proj_in") == 0.5 == spec.scale
    assert LoraSpec(16, 8.0, "", "unet", 16).rank_of("mid_block.resnets.0.conv1") == 16 and LoraSpec(16, 8.0, "", "unet", 16, 4.0).scale_of("mid_block.resnets.0.conv2") == 0.25
    table = lora_table(SDXL_BASE, spec)
    names = [n for n, _ in table]
    shapes = dict(table)
    p = "down_blocks.1.resnets.0."
    i = names.index(p + "conv1" + A_)
    assert names[i:i + 6] == [p + "conv1" + A_, p + "conv1" + B_, p + "conv2" + A_, p + "conv2" + B_, p + "conv_shortcut" + A_, p + "conv_shortcut" + B_]
    assert [shapes[n] for n in names[i:i + 6]] == [(4, 320, 3, 3), (640, 4), (4, 640, 3, 3), (640, 4), (16, 320), (640, 16)]
    assert shapes["up_blocks.0.resnets.0.conv1" + A_] == (4, 2560, 3, 3) and shapes["up_blocks.2.resnets.2.conv_shortcut" + A_] == (16, 640)
    assert "down_blocks.0.resnets.0.conv_shortcut" + A_ not in shapes and "mid_block.resnets.1.conv2" + B_ in shapes
    # down_blocks.1 lists its attentions in front of its resnets (the parameter table's order); the linears keep rank / alpha
    assert names.index("down_blocks.1.attentions.1.proj_out" + B_) < i and shapes["down_blocks.1.attentions.1.proj_out" + B_] == (640, 16)
    assert names[0] == "down_blocks.0.resnets.0.conv1" + A_ and names[-1] == "mid_block.resnets.1.conv2" + B_
    for n, s in table:          # A directly in front of its B for every module outside the fused attention groups
        if n.endswith(A_) and ".attn" not in n:
            assert names[names.index(n) + 1] == n[:-len(A_)] + B_


def test_other_scopes_give_the_tables_they_gave():
    """sha256 of repr(lora_table(...)) as the tables stood before scope "unet" existed."""
    want = {("sdxl", "attention", 4): (1120, "1618c2d46f478bb4"), ("sdxl", "attention", 16): (1120, "575da905786d1bf8"),
            ("sdxl", "transformer", 4): (1444, "383dbbbbe92a7085"), ("sdxl", "transformer", 16): (1444, "e4a9dbf94a0b79a9"),
            ("mini", "attention", 4): (272, "0bac97f4d8653a54"), ("mini", "attention", 16): (272, "a063691664b9689e"),
            ("mini", "transformer", 4): (384, "75eda7c8d4890e02"), ("mini", "transformer", 16): (384, "68a6b13890e9ed73")}
    for (name, scope, r), (n, digest) in want.items():
        t = lora_table(SDXL_BASE if name == "sdxl" else mini_config(), LoraSpec(r, 8.0, "", scope))
        assert len(t) == n and hashlib.sha256(repr(t).encode()).hexdigest()[:16] == digest, (name, scope, r)
    t_un = lora_table(SDXL_BASE, LoraSpec(16, 8.0, "", "unet", 16))
    assert [e for e in t_un if ".attentions." in e[0]] == lora_table(SDXL_BASE, LoraSpec(16, 8.0, "", "transformer"))


def test_shipped_kernel_rules_follow_the_measured_table():
    """lora_exec.LoraRoutes.CONV_*_GEMM issue the general convolution exactly where profiles/lora_conv_time.json has it winning beyond the
    repeat spread, at every measured shape and rank; rank 4 (Cout % 8) never goes there."""
    from aozora_sdxl_training_amd.lora_exec import LoraRoutes as U
    prof = json.load(open(os.path.join(ROOT, "profiles", "lora_conv_time.json")))["kernels"]
    rules = {"down": U.CONV_DOWN_GEMM, "dgrad": U.CONV_DGRAD_GEMM, "wgrad": U.CONV_WGRAD_GEMM}
    assert len(prof) == 8
    for label, res in prof.items():
        side, r = int(label.split("x")[0]), int(label.rsplit("r=", 1)[1])
        for product, rule in rules.items():
            m = res[product]
            assert m["general_wins_beyond_spread"] == (m["adapter"]["median_us"] - m["general"]["median_us"] > max(m["adapter"]["spread_us"], m["general"]["spread_us"]))
            assert U.conv_general(rule, 4 * side * side, r) == m["general_wins_beyond_spread"], (label, product)
    for rule in rules.values():
        assert not U.conv_general(rule, 1 << 20, 4) and not U.conv_general(rule, 128, 64)


# ---------------- refusals ----------------------------------------------------------------------------------------------------------------
def _cfg(**hp):
    return types.SimpleNamespace(LORA_PARAMS=hp)


def test_spec_refusals():
    assert LORA_SCOPES == ("attention", "transformer", "unet")
    assert LoraSpec(8, 8.0, "", "unet", 8) == LoraSpec(8, 8.0, "", "unet", 8, None)
    with pytest.raises(ValueError, match="scope \"unet\" needs"):          # a spec of scope "unet" names its conv_rank; lora.options fills it from rank
        LoraSpec(8, 8.0, "", "unet")
    for r in (0, 3, 5, 128, 2.5):
        with pytest.raises(ValueError, match="conv_rank"):
            LoraSpec(8, 8.0, "", "unet", r)
    for a in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="conv_alpha"):
            LoraSpec(8, 8.0, "", "unet", 8, a)
    for scope in ("attention", "transformer"):
        with pytest.raises(ValueError, match="scope \"unet\""):
            LoraSpec(8, 8.0, "", scope, 8)
    for kw, why in (("time_emb_proj", "parameter-gradient branch"), ("downsamplers", "stride-2"), ("downsamplers.0.conv", "stride-2"),
                    ("upsamplers", "nearest-2x gather"), ("conv_in", "input convolution"), ("conv_out", "output convolution")):
        with pytest.raises(ValueError, match="out of scope \"unet\"") as e:
            lora_modules(SDXL_BASE, LoraSpec(8, 8.0, "to_q, " + kw, "unet", 8))
        assert why in str(e.value) and repr(kw) in str(e.value)
    for kw in ("time_embedding", "add_embedding", "no_such_layer", "conv_norm_out"):
        with pytest.raises(ValueError, match="selects no"):
            lora_modules(SDXL_BASE, LoraSpec(8, 8.0, kw, "unet", 8))
    # a keyword that selects modules of the scope may also match names outside it (`resnets` matches time_emb_proj): it selects the scope's
    assert len(lora_modules(SDXL_BASE, LoraSpec(8, 8.0, "resnets.0", "unet", 8))) > 0
    # the narrower scopes still refuse a convolution
    for scope in ("attention", "transformer"):
        with pytest.raises(ValueError):
            lora_modules(SDXL_BASE, LoraSpec(8, 8.0, "conv1", scope))


def test_options_are_parsed_and_refused():
    assert set(lora._CONV_KEYS) == {"conv_rank", "conv_alpha"}
    assert lora.options(_cfg(rank=8, scope="unet"))[0] == LoraSpec(8, 8.0, "", "unet", 8)
    assert lora.options(_cfg(rank=8, scope=" UNet ", conv_rank=4, conv_alpha="2"))[0] == LoraSpec(8, 8.0, "", "unet", 4, 2.0)
    assert lora.options(_cfg(rank=8, alpha=4, scope="unet", conv_rank=16.0, targets=["conv1", "to_q"]))[0] == LoraSpec(8, 4.0, "conv1, to_q", "unet", 16, None)
    assert lora.options(_cfg(rank=8, scope="unet", conv_alpha=1))[0].scale_of("mid_block.resnets.0.conv1") == 1.0 / 8.0
    for hp, why in ((dict(rank=8, scope="unet", conv_rank=5), "conv_rank 5"), (dict(rank=8, scope="unet", conv_rank=3.5), "conv_rank"),
                    (dict(rank=8, scope="unet", conv_rank=[4, 8]), "conv_rank"), (dict(rank=8, scope="unet", conv_rank="many"), "conv_rank"),
                    (dict(rank=8, scope="unet", conv_rank=128), "conv_rank 128"), (dict(rank=8, scope="unet", conv_alpha=0), "conv_alpha"),
                    (dict(rank=8, scope="unet", conv_alpha=-2), "conv_alpha"), (dict(rank=8, scope="unet", conv_alpha="x"), "conv_alpha"),
                    (dict(rank=8, conv_rank=4), "scope"), (dict(rank=8, scope="transformer", conv_alpha=1.0), "scope"),
                    (dict(rank=8, scope="unet", conv_dim=4), "unknown key"), (dict(rank=8, scope="unet", targets="time_emb_proj"), "out of scope"),
                    (dict(rank=8, scope="unet", targets="upsamplers"), "out of scope"), (dict(rank=8, scope="unet", targets="nothing_here"), "selects no"),
                    (dict(rank=8, scope="everything"), "scope")):
        with pytest.raises(ValueError, match=why):
            lora.options(_cfg(**hp))
    with pytest.raises(ValueError, match="data parallel"):
        lora.options(_cfg(rank=8, scope="unet"), world=2)


def test_trainer_main_refuses_before_a_unet_is_loaded(tmp_path, capsys, monkeypatch):
    """trainer.main prints ERROR: ... and returns 2 with nothing loaded (lora.load_unet and checkpoint.load_unet would be reached only
    behind the refusal; both are made to fail loudly here)."""
    from aozora_sdxl_training_amd import checkpoint, trainer

    def loaded(*a, **k):
        raise AssertionError("a UNet was loaded")
    monkeypatch.setattr(lora, "load_unet", loaded)
    monkeypatch.setattr(checkpoint, "load_unet", loaded)
    for i, (hp, why) in enumerate(((dict(rank=8, scope="unet", conv_rank=5), "conv_rank 5"), (dict(rank=8, scope="unet", targets="downsamplers"), "out of scope"),
                                   (dict(rank=8, conv_alpha=2.0), "scope"), (dict(rank=8, scope="unet", conv_alpha=0), "conv_alpha"))):
        preset = tmp_path / f"p{i}.json"
        preset.write_text(json.dumps({"config_version": 1, "active_mode": "sdxl", "sdxl": {"sdxl_lora_params": hp}}))
        rc = trainer.main(["--config", str(preset)])
        out = capsys.readouterr().out
        assert rc == 2 and "ERROR: " in out and why in out, (hp, rc, out)


# ---------------- the adapter file --------------------------------------------------------------------------------------------------------
def _state(cfg, spec, seed=1):
    g = torch.Generator().manual_seed(seed)
    return {n: torch.randn(shape, generator=g).bfloat16() for n, shape in lora_table(cfg, spec)}


def test_file_keys_shapes_and_metadata():
    assert lora.file_key("down_blocks.0.resnets.0.conv1") == "lora_unet_input_blocks_1_0_in_layers_2"
    assert lora.file_key("down_blocks.0.resnets.0.conv2") == "lora_unet_input_blocks_1_0_out_layers_3"
    assert lora.file_key("down_blocks.1.resnets.0.conv_shortcut") == "lora_unet_input_blocks_4_0_skip_connection"
    assert lora.file_key("mid_block.resnets.1.conv1") == "lora_unet_middle_block_2_in_layers_2"
    cfg, spec = mini_config(), LoraSpec(8, 4.0, "", "unet", 4, 1.0)
    st = _state(cfg, spec)
    # the device keeps A as [r][3][3][Cin] and exposes the logical (r, Cin, 3, 3) with channels-last strides: hand file_tensors that view
    name = "down_blocks.1.resnets.0.conv1" + A_
    st[name] = st[name].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not st[name].is_contiguous()
    ft = lora.file_tensors(st, spec)
    mods = lora_modules(cfg, spec)
    assert set(ft) == {lora.file_key(m) + sfx for m in mods for sfx in (".lora_down.weight", ".lora_up.weight", ".alpha")} and len(ft) == 3 * len(mods)
    k = lora.file_key("down_blocks.1.resnets.0.conv1")
    assert tuple(ft[k + ".lora_down.weight"].shape) == (4, 64, 3, 3) and ft[k + ".lora_down.weight"].is_contiguous()
    assert torch.equal(ft[k + ".lora_down.weight"], st[name]) and tuple(ft[k + ".lora_up.weight"].shape) == (128, 4, 1, 1)
    assert float(ft[k + ".alpha"]) == 1.0 and ft[k + ".alpha"].dim() == 0
    k = lora.file_key("down_blocks.1.resnets.0.conv_shortcut")
    assert tuple(ft[k + ".lora_down.weight"].shape) == (8, 64, 1, 1) and tuple(ft[k + ".lora_up.weight"].shape) == (128, 8, 1, 1) and float(ft[k + ".alpha"]) == 4.0
    k = lora.file_key("down_blocks.1.attentions.0.proj_in")
    assert tuple(ft[k + ".lora_down.weight"].shape) == (8, 128) and float(ft[k + ".alpha"]) == 4.0
    assert all(t.dtype == torch.bfloat16 for t in ft.values())
    meta = lora.file_metadata(spec)
    assert meta["ss_network_dim"] == "8" and meta["ss_network_alpha"] == "4" and json.loads(meta["ss_network_args"]) == {"conv_dim": "4", "conv_alpha": "1"}
    assert json.loads(lora.file_metadata(LoraSpec(8, 4.0, "", "unet", 8))["ss_network_args"]) == {"conv_dim": "8", "conv_alpha": "4"}
    assert "ss_network_args" not in lora.file_metadata(LoraSpec(8, 4.0, "", "transformer"))


class _FakeUNet:
    """What read_lora_file and merged_state ask of a UNet."""

    def __init__(self, cfg, spec, seed=1):
        self.lora, self._ls = spec, _state(cfg, spec, seed)
        g = torch.Generator().manual_seed(seed + 100)
        self._sd = {n: torch.randn(shape, generator=g).bfloat16() for n, shape in param_table(cfg)}

    def lora_state_dict(self):
        return dict(self._ls)

    def state_dict(self):
        return dict(self._sd)


def test_reader_round_trip_and_refusals(tmp_path):
    from safetensors.torch import save_file
    cfg, spec = mini_config(), LoraSpec(8, 4.0, "resnets.0, proj_in", "unet", 4, 1.0)
    u = _FakeUNet(cfg, spec)
    ft = lora.file_tensors(u.lora_state_dict(), spec)
    path = tmp_path / "a.safetensors"
    save_file(ft, str(path), metadata=lora.file_metadata(spec))
    got = lora.read_lora_file(path, u)
    assert set(got) == set(u._ls) and all(torch.equal(got[n], u._ls[n]) and got[n].shape == u._ls[n].shape for n in got)
    for extra in ("lora_unet_input_blocks_1_0_emb_layers_1", "lora_unet_input_blocks_3_0_op", "lora_unet_output_blocks_2_1_conv", "lora_unet_zzz"):
        more = dict(ft)
        more[extra + ".lora_down.weight"] = torch.zeros(4, 8, dtype=torch.bfloat16)
        more["lora_unet_zzzz_later.alpha"] = torch.tensor(1.0, dtype=torch.bfloat16)
        save_file(more, str(tmp_path / "b.safetensors"))
        with pytest.raises(KeyError) as e:
            lora.read_lora_file(tmp_path / "b.safetensors", u)
        assert extra + ".lora_down.weight" in str(e.value) and "zzzz_later" not in str(e.value)       # the FIRST such key is named
    less = {k: v for k, v in ft.items() if "in_layers_2.lora_up" not in k}
    save_file(less, str(tmp_path / "c.safetensors"))
    with pytest.raises(KeyError, match="missing"):
        lora.read_lora_file(tmp_path / "c.safetensors", u)
    save_file(ft, str(tmp_path / "d.safetensors"))
    with pytest.raises(ValueError, match="alpha"):
        lora.read_lora_file(tmp_path / "d.safetensors", _FakeUNet(cfg, LoraSpec(8, 4.0, "resnets.0, proj_in", "unet", 4, 2.0)))
    with pytest.raises(ValueError, match="shape"):
        lora.read_lora_file(tmp_path / "d.safetensors", _FakeUNet(cfg, LoraSpec(8, 4.0, "resnets.0, proj_in", "unet", 8, 1.0)))


def test_merged_state_against_a_float64_merge():
    cfg, spec = mini_config(), LoraSpec(8, 4.0, "", "unet", 4, 3.0)
    u = _FakeUNet(cfg, spec, seed=3)
    merged = lora.merged_state(u)
    assert set(merged) == set(u._sd)
    adapted = {n[:-len(A_)] for n in u._ls if n.endswith(A_)}
    seen = set()
    for name, W in u._sd.items():
        m = name[:-len(".weight")] if name.endswith(".weight") else None
        if m not in adapted:
            assert torch.equal(merged[name], W), name
            continue
        A, Bm, s = u._ls[m + A_], u._ls[m + B_], spec.scale_of(m)
        ref = CR.merged_conv_weight(W, A, Bm, s) if W.dim() == 4 else LR.merged_weight(W, A, Bm, s)
        A4 = A.double() if A.dim() == 4 else A.double()[:, :, None, None]
        S = W.double().abs().reshape(ref.shape) + s * torch.einsum("oj,jchw->ochw", Bm.double().abs(), A4.abs()).reshape(ref.shape)
        got = merged[name]
        assert got.dtype == torch.float32 and got.shape == W.shape
        assert bool(((got.double() - ref).abs() <= (A.shape[0] + 2) * 2.0 ** -24 * S).all()), name       # r products, the scale, the sum: fp32
        assert not torch.equal(got, W.float())
        seen.add(m.rsplit(".", 1)[-1])
    assert {"conv1", "conv2", "conv_shortcut", "proj_in", "to_q"} <= seen
    assert spec.scale_of("mid_block.resnets.0.conv1") == 0.75 and spec.scale_of("mid_block.resnets.0.conv_shortcut") == 0.5
