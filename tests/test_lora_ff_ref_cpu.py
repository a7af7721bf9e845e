"""LoRA on the feed-forward and proj_in / proj_out linears, without a GPU: the case table of tests/test_lora_ff_gpu.py (exactness,
rounding, coverage), tests/lora_ff_ref.py against torch, LoraSpec.scope and what it selects (counts, table order, file keys,
refusals), the merged weight of an ff.net.0.proj-shaped adapter, and the argument checks of az_lora_up_geglu_bf16 (they return before
any HIP call)."""
import ctypes
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import gemm_ref as R                # noqa: E402
import lora_ref as LR               # noqa: E402
import lora_ff_ref as FR            # noqa: E402
import test_lora_ff_gpu as T        # noqa: E402

from aozora_sdxl_training_amd import lora                                                                     # noqa: E402
from aozora_sdxl_training_amd.unet_spec import LoraSpec, SDXL_BASE, lora_modules, lora_table, mini_config       # noqa: E402


# ---------------- the GPU test's case table -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.CASES, ids=T.cid)
def test_cases_are_exact_and_need_rounding(c):
    d = T.make(c)                    # lora_ref.up asserts exact_ok_scaled
    P = d["u"].double().abs() @ d["w"].double().abs().t()
    assert LR.exact_ok_scaled(P, c.s, d["y"]) and R.inexact_share(d["ref"]) > 0
    assert d["ref"].shape == (c.M, 2 * c.H) and d["out_ref"].shape == (c.M, c.H)


def test_table_crosses_every_edge():
    for values, seen, what in (((1, 15, 16, 17, 63, 65, 154, 257), [c.M for c in T.CASES], "M"), ((8, 24, 64, 72, 136, 320), [c.H for c in T.CASES], "H"),
                               ((4, 8, 12, 16, 32, 64), [c.r for c in T.CASES], "r"), (LR.EXACT_SCALES, [c.s for c in T.CASES], "s")):
        assert set(values) <= set(seen), f"{what}: {sorted(set(values) - set(seen))} not covered"
    assert T.GAUSS == (154, 320, 16, 1.0 / 3.0)


def test_reference_geglu_is_the_erf_gelu():
    g = torch.Generator().manual_seed(3)
    p = torch.randn(9, 48, generator=g, dtype=torch.float64) * 3
    want = p[:, :24] * torch.nn.functional.gelu(p[:, 24:])
    assert torch.allclose(FR.geglu(p), want, rtol=1e-13, atol=1e-13)
    u, w, y = R.quarters((5, 8), 1), R.quarters((32, 8), 2), R.quarters((5, 32), 3, 8)
    ref, S, out = FR.up_geglu(u, w, y, 0.5)
    assert torch.equal(ref, y.double() + 0.5 * (u.double() @ w.double().t()))
    assert torch.equal(out, FR.geglu(R.expected_bits(ref)))          # of the STORED proj, not of the exact one


# ---------------- LoraSpec.scope ------------------------------------------------------------------------------------------------------
def test_module_counts_per_scope():
    for cfg, n_attn, n_all in ((SDXL_BASE, 560, 722), (mini_config(), 136, 192)):
        assert len(lora_modules(cfg, LoraSpec(16, 16.0))) == n_attn
        assert len(lora_modules(cfg, LoraSpec(16, 16.0, "", "attention"))) == n_attn
        assert len(lora_modules(cfg, LoraSpec(16, 16.0, "", "transformer"))) == n_all
        assert len(lora_modules(cfg, LoraSpec(16, 16.0, "*", "transformer"))) == n_all
        assert len(lora_table(cfg, LoraSpec(16, 16.0, "", "transformer"))) == 2 * n_all
    blocks = 70
    assert len(lora_modules(SDXL_BASE, LoraSpec(8, 8.0, "ff.net", "transformer"))) == 2 * blocks
    assert len(lora_modules(SDXL_BASE, LoraSpec(8, 8.0, "proj_in, proj_out", "transformer"))) == 2 * 11
    assert len(lora_modules(SDXL_BASE, LoraSpec(8, 8.0, "attn1, attn2", "transformer"))) == 560


def test_default_scope_table_is_unchanged():
    spec = LoraSpec(16, 16.0)
    assert spec == LoraSpec(16, 16.0, "", "attention") and spec.scope == "attention"
    table = lora_table(SDXL_BASE, spec)
    assert table == lora_table(SDXL_BASE, LoraSpec(16, 16.0, "", "attention")) and len(table) == 1120
    b = "down_blocks.1.attentions.0.transformer_blocks.0."
    assert [n for n, _ in table[:8]] == [b + "attn1." + p + s for s in (".lora_A.weight", ".lora_B.weight") for p in ("to_q", "to_k", "to_v")] + \
        [b + "attn1.to_out.0.lora_A.weight", b + "attn1.to_out.0.lora_B.weight"]
    assert table[0][1] == (16, 640) and table[3][1] == (640, 16)
    e = "mid_block.attentions.0.transformer_blocks.9.attn2."
    assert [n for n, _ in table[-8:]] == [e + x for x in ("to_q.lora_A.weight", "to_q.lora_B.weight", "to_k.lora_A.weight", "to_v.lora_A.weight",
                                                         "to_k.lora_B.weight", "to_v.lora_B.weight", "to_out.0.lora_A.weight", "to_out.0.lora_B.weight")]
    assert table[-4][1] == (1280, 16) and table[-6][1] == (16, 2048)
    assert all("ff.net" not in n and "proj_in" not in n and "proj_out" not in n for n, _ in table)


def test_transformer_scope_order_within_one_transformer():
    r = 8
    table = lora_table(SDXL_BASE, LoraSpec(r, 8.0, "", "transformer"))
    pre = "down_blocks.1.attentions.0."
    assert table[0] == (pre + "proj_in.lora_A.weight", (r, 640)) and table[1] == (pre + "proj_in.lora_B.weight", (640, r))
    mine = [(n[len(pre):], s) for n, s in table if n.startswith(pre)]
    assert len(mine) == 2 * (2 + 2 * 10) and table[:len(mine)] == [(pre + n, s) for n, s in mine]        # contiguous: one transformer after another
    A, Bm = ".lora_A.weight", ".lora_B.weight"
    per_block = ["attn1.to_q" + A, "attn1.to_k" + A, "attn1.to_v" + A, "attn1.to_q" + Bm, "attn1.to_k" + Bm, "attn1.to_v" + Bm,
                 "attn1.to_out.0" + A, "attn1.to_out.0" + Bm, "attn2.to_q" + A, "attn2.to_q" + Bm, "attn2.to_k" + A, "attn2.to_v" + A,
                 "attn2.to_k" + Bm, "attn2.to_v" + Bm, "attn2.to_out.0" + A, "attn2.to_out.0" + Bm,
                 "ff.net.0.proj" + A, "ff.net.0.proj" + Bm, "ff.net.2" + A, "ff.net.2" + Bm]
    want = ["proj_in" + A, "proj_in" + Bm] + [f"transformer_blocks.{i}." + x for i in range(2) for x in per_block] + ["proj_out" + A, "proj_out" + Bm]
    assert [n for n, _ in mine] == want
    shapes = dict(mine)
    assert shapes["transformer_blocks.1.ff.net.0.proj" + A] == (r, 640) and shapes["transformer_blocks.1.ff.net.0.proj" + Bm] == (5120, r)
    assert shapes["transformer_blocks.1.ff.net.2" + A] == (r, 2560) and shapes["transformer_blocks.1.ff.net.2" + Bm] == (640, r)
    assert shapes["proj_out" + A] == (r, 640) and shapes["proj_out" + Bm] == (640, r)
    # the modules follow the parameter-table order, and a narrowed list keeps it
    narrowed = lora_table(SDXL_BASE, LoraSpec(r, 8.0, "ff.net.2, proj_out", "transformer"))
    assert [n[len(pre):] for n, _ in narrowed[:6]] == ["transformer_blocks.0.ff.net.2" + A, "transformer_blocks.0.ff.net.2" + Bm,
                                                       "transformer_blocks.1.ff.net.2" + A, "transformer_blocks.1.ff.net.2" + Bm,
                                                       "proj_out" + A, "proj_out" + Bm]


def test_file_keys_of_the_new_modules():
    assert lora.file_key("down_blocks.1.attentions.0.proj_in") == "lora_unet_input_blocks_4_1_proj_in"
    assert lora.file_key("down_blocks.1.attentions.0.transformer_blocks.0.ff.net.0.proj") == "lora_unet_input_blocks_4_1_transformer_blocks_0_ff_net_0_proj"
    assert lora.file_key("mid_block.attentions.0.transformer_blocks.9.ff.net.2") == "lora_unet_middle_block_1_transformer_blocks_9_ff_net_2"
    spec = LoraSpec(4, 2.0, "", "transformer")
    keys = {lora.file_key(m) for m in lora_modules(SDXL_BASE, spec)}
    assert len(keys) == 722 and "lora_unet_output_blocks_5_1_proj_out" in keys
    assert lora.file_metadata(spec)["ss_network_module"] == "networks.lora"


def _cfg(**hp):
    return types.SimpleNamespace(LORA_PARAMS=hp)


def test_scope_is_parsed_and_refused():
    assert lora.options(_cfg(rank=8))[0] == LoraSpec(8, 8.0, "", "attention")
    assert lora.options(_cfg(rank=8, scope="attention"))[0] == lora.options(_cfg(rank=8))[0]
    assert lora.options(_cfg(rank=8, scope="transformer", targets="ff.net.0.proj"))[0] == LoraSpec(8, 8.0, "ff.net.0.proj", "transformer")
    assert "scope" in lora._KEYS and len(lora._KEYS) == 5
    with pytest.raises(ValueError, match="scope"):
        LoraSpec(8, 8.0, "", "unet")
    for bad in ("everything", 3, None, ["transformer"]):
        with pytest.raises(ValueError, match="scope"):
            lora.options(_cfg(rank=8, scope=bad))
    for kw in ("conv1", "time_emb_proj", "time_embedding"):
        with pytest.raises(ValueError, match="transformer"):
            lora_modules(SDXL_BASE, LoraSpec(8, 8.0, kw, "transformer"))
    with pytest.raises(ValueError, match="scope \"transformer\""):
        lora.options(_cfg(rank=8, scope="transformer", targets="to_q, conv1"))
    # the default scope keeps its refusals and their wording
    for targets, why in (("proj_in", "out of scope"), ("ff.net.2", "out of scope"), ("no_such_layer", "selects no attention projection")):
        with pytest.raises(ValueError, match=why):
            lora.options(_cfg(rank=8, targets=targets))
        with pytest.raises(ValueError, match=why):
            lora_modules(SDXL_BASE, LoraSpec(8, 8.0, targets, "attention"))


def test_merged_weight_of_a_geglu_projection_adapter():
    g = torch.Generator().manual_seed(11)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    c, r, s = 16, 4, 2.0
    x, W, A, Bm = mk(7, c), mk(8 * c, c), mk(r, c), mk(8 * c, r)
    proj = x @ W.t() + s * ((x @ A.t()) @ Bm.t())
    pm = x @ LR.merged_weight(W, A, Bm, s).t()
    assert float((proj - pm).abs().max()) <= 1e-12 * float(proj.abs().max())
    assert torch.allclose(FR.geglu(proj), FR.geglu(pm), rtol=1e-11, atol=1e-11)


# ---------------- the entry point's argument checks -------------------------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Host-only: every call below fails its argument check, so no HIP call is made.  One error number per rule."""
    from aozora_sdxl_training_amd._lib import lib
    fn = lib()._fn["az_lora_up_geglu_bf16"]
    a = 1 << 20                              # aligned, never dereferenced
    P = ctypes.c_void_p

    def call(M=16, H=64, r=8, U=a, ldu=None, W=a + (1 << 16), ldw=None, proj=a + (2 << 16), ldp=None, out=a + (3 << 16), ldo=None):
        return fn(M, H, r, 1.0, P(U), r if ldu is None else ldu, P(W), r if ldw is None else ldw, P(proj), 2 * H if ldp is None else ldp,
                  P(out), H if ldo is None else ldo, None)
    assert call(M=0) == -1120
    assert call(H=60) == -1121 and call(H=0) == -1121
    assert call(r=6) == -1122 and call(r=68) == -1122 and call(r=0) == -1122
    assert call(U=0) == -1123 and call(out=0) == -1123 and call(proj=a + (2 << 16) + 4) == -1123
    assert call(ldp=120) == -1124 and call(ldo=60) == -1124 and call(ldu=4) == -1124 and call(ldw=10) == -1124
    assert call(out=a + (2 << 16) + 128) == -1125 and call(U=a + (2 << 16) + 16 * 128 * 2 - 8) == -1125
    assert call(M=64 * 65535 + 1, U=a, W=a + (1 << 16), proj=1 << 40, out=1 << 41) == -1126
