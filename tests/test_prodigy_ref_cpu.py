"""tests/prodigy_ref.py, the CPU restatement of the Prodigy optimizer (INTEGRATION.md "The Prodigy optimizer"), against a plain float64
transcription of the published pseudo-code, hand-computed values and the properties the contract states.  No GPU, no library."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import prodigy_ref as PR        # noqa: E402


def published_f64(p, grads, lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0, use_bias_correction=False,
                  safeguard_warmup=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf")):
    """Prodigy as published (Algorithm 1 of arXiv 2306.06101 in the Adam form of the authors' implementation), float64 numpy, one
    tensor: -> (p after the last step, [d after every step])."""
    b1, b2 = betas
    b3 = math.sqrt(b2) if beta3 is None else beta3
    p = p.astype(np.float64).copy()
    p0, m, v, s = p.copy(), np.zeros_like(p), np.zeros_like(p), np.zeros_like(p)
    d, d_max, d_num, k, ds = d0, d0, 0.0, 0, []
    for g in grads:
        g = g.astype(np.float64)
        bc = math.sqrt(1 - b2 ** (k + 1)) / (1 - b1 ** (k + 1)) if use_bias_correction else 1.0
        dlr = d * lr * bc
        d_num = d_num * b3 + (d / d0) * dlr * float(np.dot(g, p0 - p))
        m = m * b1 + d * (1 - b1) * g
        v = v * b2 + d * d * (1 - b2) * g * g
        s = s * b3 + (d / d0) * (d if safeguard_warmup else dlr) * g
        d_den = float(np.abs(s).sum())
        if d_den == 0:
            ds.append(d)
            continue
        d_hat = d_coef * d_num / d_den
        if d == d0:
            d = max(d, d_hat)
        d_max = max(d_max, d_hat)
        d = min(d_max, d * growth_rate)
        if weight_decay != 0:
            p = p * (1 - weight_decay * dlr)
        p = p - dlr * m / (np.sqrt(v) + d * eps)
        k += 1
        ds.append(d)
    return p, ds


def test_restatement_agrees_with_the_published_pseudo_code_in_float64():
    """n = 64, 30 steps, parameters starting at 0 and gradients whose sign is fixed per element, so that every quantity of the run (m, s,
    the updates, w, the numerator terms) is a sum of same-signed terms: nothing cancels and float32 errors stay RELATIVE.  Tolerance:
    one step adds at most 16 float32 roundings (2^-24 each) along its longest chain d -> c_m, c_v -> m, v -> sqrt, +, *, / -> w ->
    numerator -> d_hat, and the error of d re-enters the next d_hat through at most four factors (numerator and denominator are each of
    degree <= 2 in d): 30 steps x 16 roundings x 4 x 2^-24 = 1.2e-4 relative, on d and on every element of w.  Any structural
    difference (a missing factor, beta3, the OLD / NEW d) is O(1)."""
    n, steps = 64, 30
    rtol = steps * 16 * 4 * 2.0 ** -24
    g = torch.Generator().manual_seed(11)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    grads = [(sign * (0.05 + torch.rand(n, generator=g))).float() for _ in range(steps)]
    for kw in (dict(), dict(use_bias_correction=True, weight_decay=0.01), dict(safeguard_warmup=True, d_coef=2.0, growth_rate=1.5, betas=(0.8, 0.99))):
        ref = PR.ProdigyRef([torch.zeros(n)], **kw)
        got = []
        for gr in grads:
            ref.step([gr])
            got.append(ref.sc["d"])
        want_p, want_d = published_f64(np.zeros(n), [x.numpy() for x in grads], **kw)
        assert want_d[-1] > 10 * want_d[0], "the run must leave d0 behind, or the comparison shows nothing"
        for a, b in zip(got, want_d):
            assert abs(a - b) <= rtol * abs(b), (kw, a, b)
        err = np.abs(ref.w[0].astype(np.float64) - want_p)
        assert np.all(err <= rtol * np.abs(want_p)), (kw, float((err / np.abs(want_p)).max()))
        assert ref.sc["k"] == steps


def test_first_update_is_d0_lr_sign_g():
    """With bias correction bc = sqrt(1 - b2) / (1 - b1) at k = 0 and the first update is -d0 lr sign(g) where |g| sqrt(1 - b2) >> eps;
    without it the factor (1 - b1) / sqrt(1 - b2) remains.  A handful of float32 roundings: 1e-6 relative."""
    g = torch.tensor([0.5, -2.0, 3.0, -0.25, 1.0])
    p = torch.tensor([0.1, -0.2, 0.3, 0.4, -0.5]).bfloat16()
    for bias, factor in ((True, 1.0), (False, 0.1 / math.sqrt(0.001))):
        ref = PR.ProdigyRef([p], lr=0.5, d0=1e-3, use_bias_correction=bias)
        assert ref.step([g])
        upd = ref.w[0].astype(np.float64) - p.float().numpy().astype(np.float64)
        want = -1e-3 * 0.5 * factor * np.sign(g.numpy())
        assert np.all(np.abs(upd - want) <= 1e-6 * np.abs(want) + 2.0 ** -24 * 0.5), (bias, upd, want)
        assert ref.sc["d"] == 1e-3 and ref.sc["k"] == 1.0      # p0 - w was 0: d_hat = 0, d stays d0


def test_hand_computed_two_element_d_hat():
    """betas (0, 0) (beta3 = 0), d_coef 2, d0 = 2^-20, g = (1, -2) every step, p = 0, eps negligible: every value is a power of two times
    a small integer.  Step 1: numerator 0, d stays d0, w = -d0 sign g.  Step 2: numerator d0 (d0 + 2 d0) = 3 d0^2, denominator |s| = d0 (1 + 2)
    -> d_hat = 2 d0 = d.  Step 3 (d = 2 d0, dlr = 2 d0, w = -2 d0 sign g): numerator 2 * 2 d0 * (2 d0 + 4 d0) = 24 d0^2, denominator
    4 d0 * 3 -> d_hat = 4 d0 = d_max = d."""
    d0 = 2.0 ** -20
    ref = PR.ProdigyRef([torch.zeros(2)], betas=(0.0, 0.0), d_coef=2.0, d0=d0, eps=1e-30)
    g = torch.tensor([1.0, -2.0])
    seen = []
    for _ in range(3):
        ref.step([g])
        seen.append((ref.sc["d"], ref.sc["d_hat"], ref.sc["d_numerator"], ref.sc["d_denom"]))
    assert seen[0] == (d0, 0.0, 0.0, 3 * d0)
    assert seen[1] == (2 * d0, 2 * d0, 3 * d0 * d0, 3 * d0)
    assert seen[2] == (4 * d0, 4 * d0, 24 * d0 * d0, 12 * d0)
    assert ref.w[0].tolist() == [-(1 + 1 + 2) * d0, (1 + 1 + 2) * d0] and ref.sc["d_max"] == 4 * d0 and ref.sc["k"] == 3.0


def _random_run(steps, seed=3, n=96, **kw):
    g = torch.Generator().manual_seed(seed)
    p = (0.02 * torch.randn(n, generator=g)).bfloat16()
    grads = [(0.01 * torch.randn(n, generator=g)).bfloat16() for _ in range(steps)]
    return p, grads, PR.ProdigyRef([p[:40], p[40:]], **kw)


def test_d_never_decreases():
    p, grads, ref = _random_run(40, growth_rate=2.0)
    last = ref.sc["d"]
    for gr in grads:
        ref.step([gr[:40], gr[40:]], coef=0.37)
        assert ref.sc["d"] >= last and ref.sc["d_max"] >= ref.sc["d"]
        last = ref.sc["d"]
    assert last > ref.sc["d0"]


def _snapshot(ref):
    return [x.copy() for k in ("w", "p0", "m", "v", "s") for x in getattr(ref, k)], dict(ref.sc)


def _same(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a[0], b[0])) and a[1] == b[1]


def test_lr_zero_changes_nothing():
    p, grads, ref = _random_run(4)
    ref.step([grads[0][:40], grads[0][40:]])
    before = _snapshot(ref)
    assert ref.step([grads[1][:40], grads[1][40:]], lr=0.0) is False
    assert _same(before, _snapshot(ref))


def test_all_zero_gradients_leave_parameters_and_k_alone():
    p, grads, ref = _random_run(2)
    z = [torch.zeros(40, dtype=torch.bfloat16), torch.zeros(56, dtype=torch.bfloat16)]
    assert ref.step(z) is False                         # from the initial state: s stays 0, d_denom == 0
    assert ref.sc["k"] == 0.0 and ref.sc["d"] == ref.sc["d0"] and ref.sc["d_denom"] == 0.0
    assert np.array_equal(np.concatenate(ref.w), p.float().numpy()) and torch.equal(torch.cat(ref.p), p)


def test_state_round_trip():
    p, grads, a = _random_run(5, weight_decay=0.01)
    for gr in grads[:3]:
        a.step([gr[:40], gr[40:]])
    st = a.save()
    assert set(st) == {"options", "scalars", "ranges", "w", "p0", "m", "v", "s"} and st["ranges"] == [40, 56]
    _, _, b = _random_run(5, weight_decay=0.01)
    b.load(st)
    for gr in grads[3:]:
        a.step([gr[:40], gr[40:]])
        b.step([gr[:40], gr[40:]])
    assert _same(_snapshot(a), _snapshot(b)) and all(torch.equal(x, y) for x, y in zip(a.p, b.p))


def toy_problem(step_fn, p):
    """The 256-element quadratic of the contract's motivation: target = p + 0.1 randn (fixed seed), gradient bf16(w - target), lr 1.
    step_fn(gradient bf16 tensor) -> the new master as a float32 torch tensor.  -> (initial loss, final loss)."""
    g = torch.Generator().manual_seed(2306)
    target = p.float() + 0.1 * torch.randn(p.numel(), generator=g)
    w = p.float()
    first = float(((w - target) ** 2).mean())
    for _ in range(80):
        w = step_fn((w - target).bfloat16())
    return first, float(((w - target) ** 2).mean())


def toy_parameters(n=256):
    return (0.02 * torch.randn(n, generator=torch.Generator().manual_seed(6101))).bfloat16()


def test_toy_problem_finds_its_step_size():
    p = toy_parameters()
    ref = PR.ProdigyRef([p])

    def step(gr):
        ref.step([gr])
        return torch.from_numpy(ref.w[0].copy())

    first, last = toy_problem(step, p)
    print(f"toy problem: d / d0 = {ref.sc['d'] / ref.sc['d0']:.3e}, loss ratio = {last / first:.3e}")
    assert ref.sc["d"] >= 1e3 * ref.sc["d0"]
    assert last <= 1e-2 * first
