"""DoRA without a GPU (tests/dora_ref.py, unet_spec.LoraSpec(dora=...), lora.options, the adapter file): the reference's hand-written
backward against float64 autograd with the norm held fixed, the merged weight against the forward, the B = 0 / m = n identity, the bound
on n2 against an fp32 restatement with another summation order, the table's order and shapes, a spec without DoRA equal to today's,
every refusal of lora.options, and the file's keys, shapes and metadata with the mismatches of read_lora_file in both directions."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import dora_ref as D                # noqa: E402

from aozora_sdxl_training_amd import lora                                                           # noqa: E402
from aozora_sdxl_training_amd.params import ParamStore                                              # noqa: E402
from aozora_sdxl_training_amd.unet_spec import LoraSpec, lora_table, mini_config, param_table       # noqa: E402


def _layer(seed=0, M=24, K=40, N=16, r=4, s=2.0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape, k=1.0: (k * torch.randn(*shape, generator=g)).bfloat16().double()
    x, W, A, B = rn(M, K), rn(N, K, k=K ** -0.5), rn(r, K, k=K ** -0.5), rn(N, r, k=0.3)
    m = (1.0 + 0.2 * torch.randn(N, generator=g)).bfloat16().double()
    return x, W, A, B, m, rn(N), rn(M, N), rn(M, N), s


def test_hand_written_backward_equals_autograd_with_the_norm_held_fixed():
    x, W, A, B, m, bias, res, dy, s = _layer()
    leaves = [t.clone().requires_grad_(True) for t in (x, A, B, m, bias, res)]
    xl, Al, Bl, ml, bl, rl = leaves
    n = (W + s * (B @ A)).norm(dim=1)                   # a constant: the paper's section 4.3
    y = (ml / n) * (xl @ W.t() + s * ((xl @ Al.t()) @ Bl.t())) + bl + rl
    y.backward(dy)
    u, v, y_ref, n_ref = D.forward(x, W, A, B, m, s, bias, res, rounded=False)
    assert torch.allclose(y_ref, y.detach(), rtol=1e-12, atol=1e-12) and torch.allclose(n_ref, n, rtol=1e-13)
    got = D.backward(x, u, v, dy, W, A, B, m, s, n_ref, rounded=False)
    for key, leaf in (("dx", xl), ("dA", Al), ("dB", Bl), ("dm", ml), ("dbias", bl), ("dres", rl)):
        assert torch.allclose(got[key], leaf.grad, rtol=1e-11, atol=1e-11), key


def test_rounded_steps_stay_near_float64():
    x, W, A, B, m, bias, res, dy, s = _layer(seed=3)
    u, v, y, n = D.forward(x, W, A, B, m, s, bias, res, rounded=True)
    _, v64, y64, _ = D.forward(x, W, A, B, m, s, bias, res, rounded=False)
    assert (y - y64).abs().max() <= 2.0 ** -7 * y64.abs().max()
    got, want = D.backward(x, u, v, dy, W, A, B, m, s, n), D.backward(x, u, v64, dy, W, A, B, m, s, n, rounded=False)
    for key in ("dv", "dm", "dx", "dA", "dB"):
        assert (got[key] - want[key]).abs().max() <= 2.0 ** -6 * want[key].abs().max(), key


def test_merged_weight_reproduces_the_forward_and_b_zero_is_the_base():
    x, W, A, B, m, bias, _, _, s = _layer(seed=5)
    _, _, y, n = D.forward(x, W, A, B, m, s, bias, rounded=False)
    assert torch.allclose(x @ D.merged_weight(W, A, B, m, s).t() + bias, y, rtol=1e-12, atol=1e-12)
    _, _, y0, n0 = D.forward(x, W, A, torch.zeros_like(B), W.norm(dim=1), s, bias, rounded=False)
    assert torch.allclose(y0, x @ W.t() + bias, rtol=1e-12, atol=1e-12)
    # lora.merge_into (fp32 on the CPU) against the float64 rule
    spec = LoraSpec(4, 8.0, dora=True)
    sd = lora.merge_into({"l.weight": W.float()}, {"l.lora_A.weight": A.float(), "l.lora_B.weight": B.float(), "l.dora_scale": m.float()}, spec)
    want = D.merged_weight(W, A, B, m, spec.scale_of("l"))
    assert (sd["l.weight"].double() - want).abs().max() <= 2.0 ** -20 * want.abs().max()
    plain = lora.merge_into({"l.weight": W.float()}, {"l.lora_A.weight": A.float(), "l.lora_B.weight": B.float()}, LoraSpec(4, 8.0))
    assert torch.allclose(plain["l.weight"].double(), W + 2.0 * (B @ A), rtol=1e-6)


def test_n2_bound_holds_for_an_fp32_restatement_with_another_order():
    for mods in (D.gauss_inputs(), D.exact_inputs()):
        for i, (W, A, B, s) in enumerate(mods):
            n2, nb = D.n2_64(W, A, B, s), D.n2_bound(W, A, B, s)
            err = np.abs(D.n2_f32(W, A, B, s).astype(np.float64) - n2)
            assert (err <= nb).all(), (i, float((err / nb).max()))
            assert (n2 > 0).all()
    for W, A, B, s in D.exact_inputs():                 # exactly summable: fp32 gives the float64 value
        assert np.array_equal(D.n2_f32(W, A, B, s).astype(np.float64), D.n2_64(W, A, B, s))
    inv, g, mb = D.gains32(np.asarray([4.0, 2.0, 9.0], np.float32))
    assert inv.tolist() == [0.5, float(np.float32(1.0) / np.sqrt(np.float32(2.0))), float(np.float32(1.0) / np.float32(3.0))]
    assert D.from_bits(mb).tolist() == [2.0, 1.4140625, 3.0] and g[0] == 1.0 and abs(g[1] - 1.0) <= 2.0 ** -8


def test_table_order_and_shapes():
    cfg = mini_config()
    shapes = dict(param_table(cfg))
    for scope, targets in (("attention", ""), ("transformer", ""), ("attention", "to_q, to_v")):
        plain, tab = lora_table(cfg, LoraSpec(4, 8.0, targets, scope)), lora_table(cfg, LoraSpec(4, 8.0, targets, scope, dora=True))
        assert [e for e in tab if not e[0].endswith(".dora_scale")] == plain
        scales = [e for e in tab if e[0].endswith(".dora_scale")]
        assert len(scales) == len(plain) // 2
        names = [n for n, _ in tab]
        for name, shape in scales:
            assert shape == (shapes[name[:-len(".dora_scale")] + ".weight"][0],)
        # behind the up matrices of its group, in the group's part order
        i = 0
        while i < len(names):
            k = 0
            while names[i + k].endswith(".lora_A.weight"):
                k += 1
            mods = [n[:-len(".lora_A.weight")] for n in names[i:i + k]]
            assert names[i + k:i + 3 * k] == [m + ".lora_B.weight" for m in mods] + [m + ".dora_scale" for m in mods], names[i:i + 3 * k]
            i += 3 * k
    tab = lora_table(cfg, LoraSpec(4, 8.0, "", "attention", dora=True))
    assert [n.rsplit(".", 2)[-2] + "." + n.rsplit(".", 1)[-1] for n, _ in tab[6:9]] == ["to_q.dora_scale", "to_k.dora_scale", "to_v.dora_scale"]


def test_a_spec_without_dora_equals_todays():
    assert LoraSpec(4, 8.0) == LoraSpec(4, 8.0, dora=False) and hash(LoraSpec(4, 8.0)) == hash(LoraSpec(4, 8.0, dora=False))
    assert LoraSpec(4, 8.0) != LoraSpec(4, 8.0, dora=True) and LoraSpec().dora is False
    cfg = mini_config()
    assert lora_table(cfg, LoraSpec(4, 8.0, dora=False)) == lora_table(cfg, LoraSpec(4, 8.0))
    assert all(".dora_scale" not in n for n, _ in lora_table(cfg, LoraSpec(4, 8.0, "", "transformer")))
    assert "dora_wd" not in json.dumps(lora.file_metadata(LoraSpec(4, 8.0)))
    for bad in (dict(scope="unet", conv_rank=4), dict(dropout=0.1), dict(rank_dropout=0.1), dict(module_dropout=0.1), dict(max_norm=1.0)):
        with pytest.raises(ValueError, match="follow-up"):
            LoraSpec(4, 8.0, dora=True, **bad)
    with pytest.raises(ValueError):
        LoraSpec(4, 8.0, dora=1)


def _options(hp):
    return lora.options(SimpleNamespace(LORA_PARAMS=hp), cfg=mini_config())


def test_options_read_dora_and_refuse_what_is_a_follow_up():
    assert _options({"rank": 4})[0] == LoraSpec(4, 4.0) and _options({"rank": 4, "dora": False})[0] == LoraSpec(4, 4.0)
    assert _options({"rank": 4, "dora": "false"})[0].dora is False
    for v in (True, "true", "1", 1):
        spec = _options({"rank": 4, "alpha": 8, "scope": "transformer", "dora": v})[0]
        assert spec == LoraSpec(4, 8.0, "", "transformer", dora=True)
    for hp, word in (({"scope": "unet"}, "convolutions"), ({"network_dropout": 0.1}, "dropout"), ({"rank_dropout": 0.2}, "dropout"),
                     ({"module_dropout": 0.3}, "dropout"), ({"scale_weight_norms": 1.0}, "max-norm")):
        with pytest.raises(ValueError, match="follow-up") as e:
            _options({"rank": 4, "dora": True, **hp})
        assert word in str(e.value) and "dora" in str(e.value)
        _options({"rank": 4, **hp})                      # the same options without DoRA are read
    _options({"rank": 4, "dora": True, "network_dropout": 0.0})
    with pytest.raises(ValueError, match="unknown"):
        _options({"rank": 4, "dora_wd": True})


def _store(spec, seed=1):
    cfg = mini_config()
    base = param_table(cfg)
    ps = ParamStore(cfg, base + lora_table(cfg, spec), len(base), "cpu")
    ps.init_lora(seed)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in ps.named_parameters():
            if n.endswith(".dora_scale") or n.endswith(".lora_B.weight"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
    return SimpleNamespace(lora=spec, lora_state_dict=ps.lora_state_dict, load_lora_state_dict=ps.load_lora_state_dict, params=ps)


def test_file_keys_shapes_metadata_and_mismatches(tmp_path):
    from safetensors import safe_open
    spec, plain_spec = LoraSpec(4, 8.0, "to_q, to_out", dora=True), LoraSpec(4, 8.0, "to_q, to_out")
    dora_unet, plain_unet = _store(spec), _store(plain_spec)
    p_dora, p_plain = lora.save_lora_file(tmp_path / "d.safetensors", dora_unet), lora.save_lora_file(tmp_path / "p.safetensors", plain_unet)
    with safe_open(str(p_dora), framework="pt", device="cpu") as f:
        keys, meta = set(f.keys()), f.metadata()
        scales = sorted(k for k in keys if k.endswith(".dora_scale"))
        state = dora_unet.lora_state_dict()
        assert len(scales) == len(state) // 3 == 68 and len(keys) == 4 * 68      # 17 blocks x 2 attentions x (to_q, to_out.0)
        for k in scales:
            t = f.get_tensor(k)
            up = f.get_tensor(k[:-len(".dora_scale")] + ".lora_up.weight")
            assert t.dtype == torch.bfloat16 and tuple(t.shape) == (up.shape[0], 1) and k.startswith("lora_unet_")
    assert json.loads(meta["ss_network_args"]) == {"dora_wd": "True"}
    with safe_open(str(p_plain), framework="pt", device="cpu") as f:
        assert not any(k.endswith(".dora_scale") for k in f.keys()) and "ss_network_args" not in (f.metadata() or {})
    # the round trip, bit for bit
    fresh = _store(spec, seed=2)
    fresh.load_lora_state_dict(lora.read_lora_file(p_dora, fresh))
    a, b = dora_unet.lora_state_dict(), fresh.lora_state_dict()
    assert set(a) == set(b) and all(torch.equal(a[n], b[n]) for n in a)
    # a DoRA file under a plain spec: its magnitudes are named as extra; a plain file under a DoRA spec: the missing key
    with pytest.raises(KeyError, match="dora_scale"):
        lora.read_lora_file(p_dora, plain_unet)
    with pytest.raises(KeyError, match="dora_scale.* is missing"):
        lora.read_lora_file(p_plain, dora_unet)
