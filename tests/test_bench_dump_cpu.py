"""bench.py --dump-outputs: which elements the sample takes and where their optimizer state sits, on a stand-in model on the CPU;
and the argument checks a plain run makes before it touches the GPU."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _standin():
    # three parameter slots of a flat buffer (padding between them, as unet._layout aligns them), their trainable ranges in three
    # regions, and the moments of the owned elements back to back (dist.ShardedRaven)
    slots = {"a": (0, (3, 5), (3, 5)), "b": (32, (7,), (7,)), "c": (64, (2, 2, 2, 4), (2, 4, 2, 2))}
    unet = types.SimpleNamespace(_slots=slots, pflat=torch.arange(128, dtype=torch.float32).bfloat16(), device=torch.device("cpu"),
                                 wait_tail_params=lambda: None)
    m = torch.arange(56, dtype=torch.float32).bfloat16()
    opt = types.SimpleNamespace(ranges=[[(0, 16)], [(32, 40)], [(64, 96)]], range_off=[[0], [16], [24]], state_on_host=False,
                                m_dev=m, v_dev=m + 100, synchronize_state=lambda: None)
    return unet, opt


def _dump(tmp_path, monkeypatch, sample):
    import bench
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", sample)
    unet, opt = _standin()
    bench.dump_outputs(str(tmp_path), unet, opt, torch.tensor(1.5), torch.tensor(3.0), 1)
    return {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}


def test_dump_maps_samples_to_parameters_and_moments(tmp_path, monkeypatch):
    out = _dump(tmp_path, monkeypatch, 12)
    assert sorted(out) == ["exp_avg_sample", "exp_avg_sq_sample", "grad_norm", "loss", "params_sample"]
    assert all(v.dtype == np.float32 for v in out.values())
    assert out["loss"].tolist() == [1.5] and out["grad_norm"].tolist() == [3.0]
    pos = out["params_sample"]                          # pflat holds its own offsets: the sample IS the positions it took
    real = set(range(0, 15)) | set(range(32, 39)) | set(range(64, 96))
    assert len(pos) == 12 and all(int(p) in real for p in pos) and list(pos) == sorted(pos)
    moff = np.where(pos < 32, pos, np.where(pos < 64, pos - 32 + 16, pos - 64 + 24))
    assert np.array_equal(out["exp_avg_sample"], moff) and np.array_equal(out["exp_avg_sq_sample"], moff + 100)


def test_dump_is_the_same_sample_every_run_and_everything_when_small(tmp_path, monkeypatch):
    a = _dump(tmp_path / "a", monkeypatch, 12)
    b = _dump(tmp_path / "b", monkeypatch, 12)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    every = _dump(tmp_path / "c", monkeypatch, 1000)["params_sample"]
    assert every.tolist() == list(range(0, 15)) + list(range(32, 39)) + list(range(64, 96))


def test_dump_stays_within_64_mb():
    import bench
    assert 3 * 4 * bench.DUMP_SAMPLE <= 64 * 2 ** 20


def test_plain_run_refuses_what_only_full_runs():
    for args, msg in ((["--steps", "0"], "--steps must be at least 1"),
                      (["--profile-out", "x.json"], "--profile-out is written by the per-kernel profile of --full")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and msg in r.stderr, r.stderr[-1000:]
