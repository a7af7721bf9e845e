"""What round-to-nearest and stochastic rounding of the bf16 write-back keep of a Raven update at the reference's default learning
rate, on the CPU with the numpy restatements of the kernels (tests/elem_ref.py, tests/sr_ref.py): 2^20 weights drawn like a
default-initialised 1280-input linear layer, a persistent fp32 gradient of scale 1e-3, the reference's default hyper-parameters.
Prints, after 1 and 100 steps, the share of weights left bit for bit unchanged, the projection of the applied update onto the update
of an fp32 master copy, and the mean |delta p|.  The figures of INTEGRATION.md "Stochastic rounding" come from here.
    python tools/sr_projection.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import elem_ref as R        # noqa: E402
import sr_ref as S          # noqa: E402

n = 1 << 20
g0 = torch.Generator().manual_seed(0)
bound = 1.0 / np.sqrt(1280.0)
p0 = ((torch.rand(n, generator=g0) * 2 - 1) * bound).bfloat16()
grad = (torch.randn(n, generator=g0) * 1e-3)          # persistent fp32 gradient
hp = lambda s: R.adamw_hyper(8e-7, (0.9, 0.999), 0.01, 1e-8, 0.3, s)
def master(steps):
    f = np.float32
    p, m, v = p0.float().numpy().copy(), np.zeros(n, f), np.zeros(n, f)
    g = grad.numpy()
    for s in range(1, steps + 1):
        _, b1, b2, eps, wdf, step, sbc2, _ = (f(x) for x in hp(s))
        m = R.fma32(g, np.full_like(g, f(1) - b1), m * b1)
        v = v * b2 + (((f(1) - b2) * g) * g)
        p = p * wdf
        p = p + ((-step * m) / (np.sqrt(v) / sbc2 + eps))
    return p
def run(steps, sr):
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    for s in range(1, steps + 1):
        p, m, v = (S.adamw_sr_bits(p, grad, m, v, hp(s), None, 42, s, 0, 0) if sr else R.adamw_bits(p, grad, m, v, hp(s)))
    return p.float().numpy()
for steps in (1, 100):
    dm = master(steps).astype(np.float64) - p0.float().numpy()
    for sr in (False, True):
        d = run(steps, sr).astype(np.float64) - p0.float().numpy()
        print(f"steps {steps:3d} sr={sr}: unchanged {np.mean(d == 0) * 100:.1f} %  projection {np.dot(d, dm) / np.dot(dm, dm):.3f}  mean|dp| {np.abs(d).mean():.3e} (master {np.abs(dm).mean():.3e})")
