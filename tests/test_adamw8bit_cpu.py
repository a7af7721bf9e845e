"""paged_adamw_8bit without a GPU: the quantisation maps, the encode / decode rules of the restatement (tests/adamw8bit_ref.py),
how closely the restatement tracks an fp64 AdamW, and the trainer's refusal of the optimizer under data parallel."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adamw8bit_ref as R        # noqa: E402


@pytest.mark.parametrize("signed", [True, False])
def test_maps(signed):
    q = R.dynamic_map(signed)
    assert q.dtype == np.float32 and q.shape == (256,)
    assert np.all(np.diff(q) > 0) and q.max() == 1.0 and int((q == 0).sum()) == 1
    if signed:
        assert q.min() > -1.0 and q[127] == 0.0 and int((q < 0).sum()) == 127
    else:
        assert q[0] == 0.0 and q.min() == 0.0
    # the product builds the same map (and the kernel relies on where its zero is)
    from aozora_sdxl_training_amd.optimizers.adamw8bit import create_dynamic_map
    assert np.array_equal(create_dynamic_map(signed).numpy(), q)


def test_encode_nearest_ties_to_lo():
    q = R.dynamic_map(True)
    x = np.array([q[200], q[200] * np.float32(1.0000001), -0.99999, 1.0, 0.0], dtype=np.float32)
    assert list(R.encode(x, q)) == [200, 200, 0, 255, 127]
    # a value between two entries goes to the nearer one; an exact fp32 tie goes to the lower index
    for lo in (10, 140, 250):
        mid = np.float32((np.float64(q[lo]) + np.float64(q[lo + 1])) / 2)
        a, b = np.float32(q[lo + 1] - mid), np.float32(mid - q[lo])
        want = lo + 1 if a < b else lo
        assert R.encode(np.array([mid]), q)[0] == want
        if a == b:
            assert want == lo
        assert R.encode(np.array([np.nextafter(mid, np.float32(2))]), q)[0] == lo + 1
        assert R.encode(np.array([np.nextafter(mid, np.float32(-2))]), q)[0] == lo
    # at least one exact tie exists among these
    ties = [lo for lo in range(255) if np.float32(q[lo + 1] - np.float32((np.float64(q[lo]) + np.float64(q[lo + 1])) / 2))
            == np.float32(np.float32((np.float64(q[lo]) + np.float64(q[lo + 1])) / 2) - q[lo])]
    assert ties
    lo = ties[0]
    mid = np.float32((np.float64(q[lo]) + np.float64(q[lo + 1])) / 2)
    assert R.encode(np.array([mid]), q)[0] == lo


def test_sign_rule_and_zero_absmax():
    q1, q2 = R.dynamic_map(True), R.dynamic_map(False)
    A = np.float32(1.0)
    # a tiny negative m is nearest to 0.0 (a non-negative code): bitsandbytes moves it one step down, to the smallest negative
    vals = np.array([1.0, -1e-12, 1e-12, 0.0, -0.0], dtype=np.float32)
    c = R.quantize(vals, A, q1, True)
    assert list(c) == [255, 126, 127, 127, 127]
    assert q1[126] < 0
    # decode of every code keeps m's sign (or zero)
    rng = np.random.default_rng(0)
    m = (rng.standard_normal(4096) * np.exp(rng.uniform(-20, 0, 4096))).astype(np.float32)
    c = R.quantize(m, np.abs(m).max(), q1, True)
    dec = q1[c]
    assert np.all((dec == 0) | (np.sign(dec) == np.sign(m))) and np.all(dec[m < 0] < 0)
    # absmax 0: the code of 0.0 in either map
    z = np.zeros(7, np.float32)
    assert np.all(R.quantize(z, np.float32(0), q1, True) == 127) and np.all(R.quantize(z, np.float32(0), q2, False) == 0)


def test_restatement_tracks_fp64_adamw():
    """Bound: every step re-encodes m (v) to the nearest map entry, an error of at most d1 * A1_t (d2 * A2_t), where d = half the
    largest gap between adjacent map entries and A_t the block's new absmax; near zero the sign rule may move a code one step
    further, which adds at most the magnitude of the smallest negative entry.  The decoded error of step t-1 enters step t
    multiplied by beta, so E_t <= beta * E_{t-1} + e_t; fp32 rounding adds a few ulps per step (1e-6 relative slack)."""
    rng = np.random.default_rng(1)
    n, T = 10_000, 20
    betas, lr, eps, wd = (0.9, 0.999), 1e-3, 1e-8, 1e-2
    q1, q2 = R.dynamic_map(True), R.dynamic_map(False)
    d1 = float(np.diff(q1.astype(np.float64)).max()) / 2 + float(abs(q1[126]))
    d2 = float(np.diff(q2.astype(np.float64)).max()) / 2
    p = R.f32_to_bf16_bits(rng.standard_normal(n).astype(np.float32) * 0.05)
    opt = R.RefAdamW8bit([n], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    m64, v64 = np.zeros(n), np.zeros(n)
    E1, E2 = np.zeros(n), np.zeros(n)
    nb = (n + 255) // 256
    blk = np.arange(n) // 256
    for t in range(1, T + 1):
        g = R.bf16_round((rng.standard_normal(n) * np.exp(rng.uniform(-6, 0, n))).astype(np.float32))
        (p,) = opt.step([p], [g])
        m64 = betas[0] * m64 + (1 - betas[0]) * g.astype(np.float64)
        v64 = betas[1] * v64 + (1 - betas[1]) * g.astype(np.float64) ** 2
        st = opt.state[0]
        mh = q1[st["c1"]].astype(np.float64) * st["a1"][blk]
        vh = q2[st["c2"]].astype(np.float64) * st["a2"][blk]
        a1 = np.array([np.abs(m64[blk == b]).max() for b in range(nb)])[blk]
        a2 = np.array([np.abs(v64[blk == b]).max() for b in range(nb)])[blk]
        E1 = betas[0] * E1 + d1 * (a1 + E1) * (1 + 1e-6) + 1e-6 * np.abs(m64)
        E2 = betas[1] * E2 + d2 * (a2 + E2) * (1 + 1e-6) + 1e-6 * np.abs(v64)
        assert np.all(np.abs(mh - m64) <= E1), (t, float(np.max(np.abs(mh - m64) / E1)))
        assert np.all(np.abs(vh - v64) <= E2), (t, float(np.max(np.abs(vh - v64) / E2)))
    # and the bound is not vacuous: the decoded moments carry the signal (relative error of the block-scaled moments)
    assert np.max(np.abs(mh - m64)) < 0.05 * np.max(np.abs(m64))
    assert np.max(np.abs(vh - v64)) < 0.05 * np.max(np.abs(v64))


def test_main_refuses_8bit_under_data_parallel(tmp_path, monkeypatch, capsys):
    import torch
    from aozora_sdxl_training_amd import trainer
    preset = {"config_version": 2, "active_mode": "sdxl", "sdxl": {"sdxl_optimizer_type": "paged_adamw_8bit"}}
    path = tmp_path / "preset.json"
    path.write_text(json.dumps(preset))
    monkeypatch.setenv("WORLD_SIZE", "2")

    def no_device(*a, **k):
        raise AssertionError("the refusal must come before any device is touched")
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    assert trainer.main(["--config", str(path)]) == 2
    out = capsys.readouterr().out
    assert "paged_adamw_8bit" in out and "one rank" in out


def test_train_refuses_8bit_under_data_parallel(monkeypatch):
    """trainer.train: ValueError before anything is allocated (no unet is loaded: the config has no model path at all)."""
    import types
    import torch.distributed as tdist
    from aozora_sdxl_training_amd import trainer
    monkeypatch.setattr(tdist, "is_initialized", lambda: True)
    monkeypatch.setattr(tdist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(tdist, "get_rank", lambda *a: 0)
    cfg = types.SimpleNamespace(OPTIMIZER_TYPE="paged_adamw_8bit")
    with pytest.raises(ValueError, match="one rank"):
        trainer.train(cfg)
