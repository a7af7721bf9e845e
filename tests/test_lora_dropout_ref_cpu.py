"""LoRA dropout on the CPU (INTEGRATION.md "LoRA dropout"): the LORA_PARAMS keys and their refusals, the adapter file's metadata, the
statistics and the independence of the masks of tests/lora_dropout_ref.py, the module ids a LoraGroup carries, the masked forward /
backward formulas against torch autograd in float64, and the argument checks of az_lora_dropout_bf16 (they return before any launch)."""
import ctypes
import json
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import lora_dropout_ref as D        # noqa: E402

from aozora_sdxl_training_amd import lora                                                                         # noqa: E402
from aozora_sdxl_training_amd.unet_spec import LoraSpec, lora_dropout_threshold, lora_table, mini_config, param_table  # noqa: E402

SEED = 42
PS = (0.1, 0.25, 0.5)


def _cfg(**hp):
    return types.SimpleNamespace(LORA_PARAMS=hp)


def test_options_accept_the_three_keys_and_defaults_equal_todays_spec():
    spec, _ = lora.options(_cfg(rank=16, alpha=16, network_dropout=0.1, rank_dropout="0.25", module_dropout=0.5))
    assert (spec.dropout, spec.rank_dropout, spec.module_dropout) == (0.1, 0.25, 0.5) and spec.has_dropout
    assert spec.dropout_thresholds == (6554, 16384, 32768) and spec.dropout_inv == 1.0 / (0.9 * 0.75)
    plain, _ = lora.options(_cfg(rank=16, alpha=16))
    assert plain == LoraSpec(16, 16.0) and not plain.has_dropout and plain.dropout_thresholds == (0, 0, 0) and plain.dropout_inv == 1.0
    assert lora.options(_cfg(rank=16, alpha=16, network_dropout=0, rank_dropout=0.0, module_dropout="0"))[0] == LoraSpec(16, 16.0)
    assert lora.options(_cfg(rank=8, scope="unet", conv_rank=4, module_dropout=0.5))[0] == LoraSpec(8, 8.0, "", "unet", 4, None, 0.0, 0.0, 0.5)
    assert LoraSpec(16, 16.0, dropout=0.1) != LoraSpec(16, 16.0)
    # the key of network dropout is kohya-ss's own, "network_dropout" (LoraSpec.dropout); a bare "dropout" stays the unknown key it was
    with pytest.raises(ValueError, match="unknown key.*network_dropout"):
        lora.options(_cfg(rank=16, dropout=0.1))


@pytest.mark.parametrize("key", ["network_dropout", "rank_dropout", "module_dropout"])
@pytest.mark.parametrize("bad", [True, False, [0.1], {"p": 0.1}, "a tenth", -0.1, 1, 1.0, 1.5, "1", float("nan")],
                         ids=["true", "false", "list", "dict", "text", "negative", "one", "one-float", "above", "one-text", "nan"])
def test_options_refuse_what_is_no_probability_and_name_the_key(key, bad):
    with pytest.raises(ValueError, match=rf"\b{key}\b"):
        lora.options(_cfg(rank=8, **{key: bad}))


def test_spec_validates_its_dropouts():
    for key in ("dropout", "rank_dropout", "module_dropout"):
        for bad in (True, "0.1", -0.5, 1.0, None):
            with pytest.raises(ValueError, match=key):
                LoraSpec(8, 8.0, **{key: bad})
    assert [lora_dropout_threshold(p) for p in (0.0, 1e-9, 0.1, 0.5, 0.999999)] == [0, 1, 6554, 32768, 65535]
    assert [D.threshold(p) for p in (0.0, 1e-9, 0.1, 0.5, 0.999999)] == [0, 1, 6554, 32768, 65535]


def test_metadata_is_written_as_specified():
    base = lora.file_metadata(LoraSpec(8, 4.0))
    assert "ss_network_dropout" not in base and "ss_network_args" not in base
    m = lora.file_metadata(LoraSpec(8, 4.0, dropout=0.1, rank_dropout=0.25, module_dropout=0.5))
    assert m["ss_network_dropout"] == "0.1" and json.loads(m["ss_network_args"]) == {"rank_dropout": "0.25", "module_dropout": "0.5"}
    assert {k: v for k, v in m.items() if k not in ("ss_network_dropout", "ss_network_args")} == base
    m = lora.file_metadata(LoraSpec(8, 4.0, rank_dropout=0.25))
    assert "ss_network_dropout" not in m and json.loads(m["ss_network_args"]) == {"rank_dropout": "0.25"}
    m = lora.file_metadata(LoraSpec(8, 4.0, "", "unet", 4, 1.0, 0.0, 0.0, 0.5))
    assert json.loads(m["ss_network_args"]) == {"conv_dim": "4", "conv_alpha": "1", "module_dropout": "0.5"}
    assert json.loads(lora.file_metadata(LoraSpec(8, 4.0, "", "unet", 4, 1.0))["ss_network_args"]) == {"conv_dim": "4", "conv_alpha": "1"}


@pytest.mark.parametrize("p", PS)
def test_keep_counts_lie_within_four_standard_deviations(p):
    t = D.threshold(p)
    counts = {
        "element": (int(D.keep_net(SEED, 3, 17, 154, 48, t).sum()), 154 * 48),                                    # 7392 draws
        "rank": (int(D.keep_rank(SEED, 3, 17, 64, 64, t).sum()), 4096),
        "module": (sum(D.keep_mod(SEED, step, mid, t) for step in range(1, 17) for mid in range(560)), 8960),
    }
    for kind, (kept, n) in counts.items():
        sd = math.sqrt(n * p * (1 - p))
        print(kind, p, kept, n * (1 - p), (kept - n * (1 - p)) / sd)
        assert abs(kept - n * (1 - p)) <= 4 * sd, (kind, p, kept, n)


def test_masks_differ_between_steps_and_between_modules():
    ts = D.thresholds(0.5, 0.5, 0.0)
    a = D.mask(SEED, 1, 17, 154, 77, 16, ts)
    assert a.shape == (154, 16) and 0 < a.sum() < a.size
    assert not np.array_equal(a, D.mask(SEED, 2, 17, 154, 77, 16, ts))
    assert not np.array_equal(a, D.mask(SEED, 1, 18, 154, 77, 16, ts))
    assert not np.array_equal(a, D.mask(7, 1, 17, 154, 77, 16, ts))
    assert np.array_equal(a, D.mask(SEED, 1, 17, 154, 77, 16, ts))
    # the three kinds draw in domains of their own; rank dropout is constant over a sample's rows, element dropout is not
    kr = D.mask(SEED, 1, 17, 154, 77, 16, (0, 32768, 0))
    assert np.array_equal(kr[:77], np.repeat(kr[:1], 77, 0)) and np.array_equal(kr[77:], np.repeat(kr[77:78], 77, 0)) and not np.array_equal(kr[0], kr[77])
    kn = D.mask(SEED, 1, 17, 154, 77, 16, (32768, 0, 0))
    assert not np.array_equal(kn[:77], np.repeat(kn[:1], 77, 0)) and not np.array_equal(kn[:2], kr[:2])
    mods = [D.keep_mod(SEED, 1, mid, 32768) for mid in range(64)]
    assert 0 < sum(mods) < 64 and mods != [D.keep_mod(SEED, 2, mid, 32768) for mid in range(64)]
    assert D.mask(SEED, 1, 17, 4, 2, 8, (0, 0, 0)).all()                                     # every kind off: nothing drawn


def _adapters(cfg, spec):
    """lora_exec.LoraAdapters over CPU buffers laid out by AozoraUNet's rule (whole ALIGN-element slots in table order)."""
    from aozora_sdxl_training_amd.lora_exec import LoraAdapters
    from aozora_sdxl_training_amd.param_groups import ALIGN
    slots, off = {}, 0
    for name, shape in lora_table(cfg, spec):
        st = (shape[0], shape[2], shape[3], shape[1]) if len(shape) == 4 else tuple(shape)
        slots[name] = (off, st, tuple(shape))
        off += (math.prod(st) + ALIGN - 1) // ALIGN * ALIGN
    flat = [torch.zeros(off, dtype=torch.bfloat16) for _ in range(3)]
    mids = D.module_ids(cfg)
    return LoraAdapters(slots, *flat, spec.scale_of, lambda n: True, spec, mids.__getitem__), mids


def test_a_modules_mask_does_not_depend_on_its_neighbours():
    cfg = mini_config()
    pre = "down_blocks.1.attentions.0.transformer_blocks.0.attn1"
    names = [f"{pre}.to_q", f"{pre}.to_k", f"{pre}.to_v"]
    table = [n for n, _ in param_table(cfg)]
    full, mids = _adapters(cfg, LoraSpec(8, 8.0, dropout=0.5, rank_dropout=0.5, module_dropout=0.5))
    assert full.drop == ((32768, 32768, 32768), 4.0) and full.step_word is None
    g = full.group(names)
    assert g.full and g.mids == [table.index(n + ".weight") for n in names] == [mids[n] for n in names]
    some, _ = _adapters(cfg, LoraSpec(8, 8.0, "attn1.to_q, attn1.to_v", dropout=0.5, rank_dropout=0.5, module_dropout=0.5))
    g2 = some.group(names)
    assert not g2.full and g2.parts == [0, 2] and g2.mids == [g.mids[0], g.mids[2]]
    wide, _ = _adapters(cfg, LoraSpec(8, 8.0, "", "unet", 4, None, 0.5, 0.5, 0.5))
    assert wide.group(names).mids == g.mids
    gc = wide.group(["down_blocks.1.resnets.0.conv1"], conv3=True)
    assert gc.conv3 and gc.r == 4 and gc.mids == [table.index("down_blocks.1.resnets.0.conv1.weight")]
    ts = full.drop[0]
    m3 = D.group_mask(SEED, 5, g.mids, 128, 64, 8, ts)
    m2 = D.group_mask(SEED, 5, g2.mids, 128, 64, 8, ts)
    assert np.array_equal(m3[:, :8], m2[:, :8]) and np.array_equal(m3[:, 16:], m2[:, 8:])
    assert not _adapters(cfg, LoraSpec(8, 8.0))[0].drop


def test_masked_formulas_agree_with_autograd_in_float64():
    g = torch.Generator().manual_seed(3)
    rows, rps, K, N, r, s, mid, step = 12, 6, 10, 7, 4, 0.5, 321, 9
    ts, inv = D.thresholds(0.1, 0.25, 0.0), float(D.inv_of(0.1, 0.25))
    m = torch.from_numpy(D.mask(SEED, step, mid, rows, rps, r, D.thresholds(0.5, 0.5, 0.0))).double()
    assert 0 < m.sum() < m.numel() and ts == (6554, 16384, 0)
    x, A, Bm, dy = (torch.randn(sh, generator=g, dtype=torch.float64) for sh in ((rows, K), (r, K), (N, r), (rows, N)))
    x.requires_grad_(True); A.requires_grad_(True); Bm.requires_grad_(True)
    y = s * (((x @ A.T) * m * inv) @ Bm.T)
    y.backward(dy)
    with torch.no_grad():
        u1 = torch.where(m > 0, (x @ A.T) * inv, torch.zeros(()).double())
        du1 = torch.where(m > 0, (s * dy @ Bm) * inv, torch.zeros(()).double())
        assert torch.allclose(y, s * u1 @ Bm.T, rtol=1e-13, atol=1e-13)
        assert torch.allclose(A.grad, du1.T @ x, rtol=1e-12, atol=1e-13)
        assert torch.allclose(Bm.grad, s * dy.T @ u1, rtol=1e-12, atol=1e-13)
        assert torch.allclose(x.grad, du1 @ A, rtol=1e-12, atol=1e-13)
    # a dropped module: exact zeros everywhere
    z = torch.zeros_like(m)
    assert not bool((torch.where(z > 0, (x @ A.T) * inv, torch.zeros(()).double())).any())


def test_reference_selects_zero_and_rescales_in_bf16():
    u = np.array([[0x7F80, 0xFF80, 0x7FC0, 0x3F80, 0xBF80, 0x8000, 0x0001, 0x4049]] * 4, dtype=np.uint16)      # inf, -inf, NaN, 1, -1, -0, tiny, pi
    ts = D.thresholds(0.5, 0.0, 0.0)
    out = D.apply_bits(u, 8, 2, [5], ts, D.inv_of(0.5, 0.0), SEED, 1)
    m = D.mask(SEED, 1, 5, 4, 2, 8, ts)
    assert 0 < m.sum() < m.size
    assert (out[~m] == 0).all()
    want = np.array([0x7F80, 0xFF80, 0x7FC0, 0x4000, 0xC000, 0x8000, 0x0002, 0x40C9], dtype=np.uint16)          # x 2: exact
    assert (out[m] == np.broadcast_to(want, u.shape)[m]).all()
    assert np.array_equal(D.apply_bits(u, 8, 2, [5], (0, 0, 0), 1.0, SEED, 1), u)
    only_mod = D.apply_bits(u, 8, 2, [5], (0, 0, 32768), 1.0, SEED, 1)
    assert np.array_equal(only_mod, u) or not only_mod.any()


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Every refusal returns its own nonzero code before anything touches a device (the pointers are never dereferenced)."""
    from aozora_sdxl_training_amd._lib import lib
    fn = lib()._fn["az_lora_dropout_bf16"]
    P = ctypes.c_void_p
    u, w = P(0x1000), P(0x2000)

    def call(rows=8, r=8, parts=1, rps=4, U=u, ldu=8, mids=(1, 2, 3), t=(32768, 0, 0), word=w):
        return fn(rows, r, parts, rps, U, ldu, *mids, *t, 2.0, SEED, word, None)
    for parts in (0, 4, -1):
        assert call(parts=parts, ldu=64) == -1140
    for r in (0, 2, 12, 24, 128):
        assert call(r=r, ldu=256) == -1141
    assert call(rows=9, rps=4, ldu=8) == -1142 and call(rows=0) == -1142 and call(rps=0) == -1142
    assert call(parts=3, ldu=23) == -1143 and call(ldu=7) == -1143
    for t in ((-1, 0, 0), (0, 65536, 0), (0, 0, 70000)):
        assert call(t=t) == -1144
    assert call(word=P(0)) == -1145 and call(word=None) == -1145 and call(U=P(0)) == -1145 and call(word=P(0x2002)) == -1145
    assert call(mids=(-1, 0, 0)) == -1146 and call(parts=2, ldu=16, mids=(1, 1 << 27, 0)) == -1146
    assert call(t=(0, 0, 0)) == 0          # every kind off: nothing to do, no launch
