"""tests/sr_ref.py on its own (no GPU): Philox4x32-10 known answers, exact unbiasedness of the rounding rule over all 65 536 values of
r, and the drift experiment that motivates the option -- at the reference's default learning rate round-to-nearest leaves a bf16
weight where it was, stochastic rounding follows the fp32 master copy."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import elem_ref as R        # noqa: E402
import sr_ref as S          # noqa: E402


def _philox_independent(ctr, key):
    """A second implementation in Python integers (one counter at a time), as the algorithm is usually written."""
    c, k = [int(x) for x in ctr], [int(x) for x in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert tuple(int(x) for x in S.philox4x32_10(ctr, key)) == want
    assert tuple(_philox_independent(ctr, key)) == want


def test_philox_vectorised_equals_scalar():
    g = np.random.default_rng(5)
    ctr = g.integers(0, 2 ** 32, size=(4, 257), dtype=np.uint64)
    key = (0x12345678, 0x9ABCDEF0)
    out = S.philox4x32_10(tuple(ctr), key)
    for j in (0, 1, 100, 256):
        assert [int(o[j]) for o in out] == _philox_independent(ctr[:, j], key)


def test_bits16_lane_layout():
    """Eight neighbouring elements share one Philox evaluation: word (e & 7) >> 1, low half for even e; the group index crosses into
    the counter's second word at e = 2^35."""
    seed, step, dom = 123456789012, 9, 3
    for base in (0, 8 * 77, 2 ** 35 - 8, 2 ** 35):
        grp = base >> 3
        w = _philox_independent((grp & 0xFFFFFFFF, grp >> 32, step, dom), (seed & 0xFFFFFFFF, seed >> 32))
        want = [(w[l >> 1] >> (16 * (l & 1))) & 0xFFFF for l in range(8)]
        assert [int(x) for x in S.sr_bits16(seed, step, dom, base + np.arange(8))] == want
    assert not np.array_equal(S.sr_bits16(1, 1, 0, np.arange(64)), S.sr_bits16(1, 1, 1, np.arange(64)))
    assert not np.array_equal(S.sr_bits16(1, 1, 0, np.arange(64)), S.sr_bits16(1, 2, 0, np.arange(64)))
    assert not np.array_equal(S.sr_bits16(1, 1, 0, np.arange(64)), S.sr_bits16(1 << 32, 1, 0, np.arange(64)))


ALL_R = np.arange(65536, dtype=np.uint32)
# both signs, ordinary values, a denormal, the smallest low half, one just below the bf16 maximum 0x7F7F0000 (+ its low half)
UNBIASED = [0x3C123456, 0xBC123456, 0x3F800001, 0xBF80FFFF, 0x00012345, 0x80400001, 0x7F7F8000, 0xFF7FFFFF, 0x3DC08000]


@pytest.mark.parametrize("u", UNBIASED, ids=[f"{u:08x}" for u in UNBIASED])
def test_rounding_is_exactly_unbiased(u):
    x = np.full(65536, u, dtype=np.uint32).view(np.float32)
    o = S.sr_round(x, ALL_R)
    lo, low = np.uint16(u >> 16), u & 0xFFFF
    assert set(np.unique(o)) <= {int(lo), int(lo) + 1}                     # never leaves the two neighbours
    away = int((o != lo).sum())
    if ((int(lo) + 1) & 0x7F80) == 0x7F80:                                 # the upper neighbour is inf: stays finite, i.e. truncates
        assert away == 0
    else:
        assert away == low                                                 # exactly L of the 65 536 values of r round away from zero
        up = (o.astype(np.uint32) << 16).view(np.float32)
        assert bool((np.abs(up) > np.abs(x))[o != lo].all()) and bool((np.abs(up) <= np.abs(x))[o == lo].all())
    assert bool(np.isfinite((o.astype(np.uint32) << 16).view(np.float32)).all())


def test_representable_and_nonfinite_values_never_change():
    u = np.array([0x00000000, 0x80000000, 0x3F800000, 0xBF810000, 0x00010000, 0x7F7F0000, 0xFF7F0000, 0x7F800000, 0xFF800000,
                  0x7FC00000, 0x7F800001, 0xFFC12345, 0x7FFFFFFF], dtype=np.uint32)
    x = u.view(np.float32)
    want = R.bf16_bits_np(x)
    for r in (0, 1, 0x7FFF, 0x8000, 0xFFFF):
        assert np.array_equal(S.sr_round(x, np.full(u.shape, r, dtype=np.uint32)), want), hex(r)
    for i in range(7):                                                      # the finite ones are their own upper 16 bits
        assert int(want[i]) == int(u[i] >> 16)


def test_update_shares_adamw_bits_arithmetic():
    """m and v are adamw_bits' own; p lies on one of the two bf16 neighbours of the fp32 value and equals adamw_bits where that value
    is representable or not finite."""
    n = 4099
    for mdtype, f32g in ((0, False), (1, True), (2, False)):
        p = R.gauss_bf16((n,), seed=3, scale=0.1)
        g = R.adamw_grads(n, 4, f32g)
        m = (1e-3 * torch.randn(n, generator=R.gen(5))).to(R.moment_dtype(mdtype))
        v = (1e-4 * torch.rand(n, generator=R.gen(6))).to(R.moment_dtype(mdtype))
        h = R.adamw_hyper(1e-3, (0.9, 0.999), 0.01, 1e-8, 0.3, 2)
        p1, m1, v1 = R.adamw_bits(p, g, m, v, h, 0.37)
        p2, m2, v2 = S.adamw_sr_bits(p, g, m, v, h, 0.37, seed=42, step=2, domain=0, elem0=3)
        bits = lambda t: t.view(torch.int16 if t.element_size() == 2 else torch.int32)
        assert torch.equal(bits(m1), bits(m2)) and torch.equal(bits(v1), bits(v2))
        pp, _, _ = S.adamw_pp(p, g, m, v, h, 0.37)
        fin = np.isfinite(pp)
        trunc = (pp.view(np.uint32) >> 16).astype(np.int64)
        got = p2.view(torch.int16).numpy().astype(np.uint16).astype(np.int64)
        assert bool(((got == trunc) | (got == trunc + 1))[fin].all())
        assert np.array_equal(got[~fin], p1.view(torch.int16).numpy().astype(np.uint16).astype(np.int64)[~fin])
        assert 0.2 < float((got != trunc)[fin].mean()) < 0.8                 # both neighbours occur


@pytest.fixture(scope="module")
def master():
    return S.drift_master()


def test_drift_master_and_round_to_nearest(master):
    d = S.DRIFT
    moved = (master - d["p0"]) / S.DRIFT_ULP
    assert abs(moved - (-1.955)) < 0.002, moved                            # the fp32 master moves -1.955 bf16 ulp in 64 steps
    n = d["n"]
    p = torch.full((n,), d["p0"]).bfloat16()
    g = torch.full((n,), d["g"])
    m, v = torch.zeros(n), torch.zeros(n)
    for s in range(1, d["steps"] + 1):
        p, m, v = R.adamw_bits(p, g, m, v, S.drift_hyper(s))
    assert int((p.float() != d["p0"]).sum()) == 0                          # round-to-nearest: no element ever moves


@pytest.mark.parametrize("seed", S.DRIFT["seeds"])
def test_drift_stochastic_rounding_follows_the_master(master, seed):
    d = S.DRIFT
    n = d["n"]
    p = torch.full((n,), d["p0"]).bfloat16()
    g = torch.full((n,), d["g"])
    m, v = torch.zeros(n), torch.zeros(n)
    for s in range(1, d["steps"] + 1):
        p, m, v = S.adamw_sr_bits(p, g, m, v, S.drift_hyper(s), None, seed, s, 0, 0)
    err = (float(p.double().mean()) - master) / S.DRIFT_ULP
    print(f"seed {seed}: mean(p_sr) - master = {err:+.4f} ulp (bound {S.DRIFT_BOUND_ULP:.4f})")
    assert abs(err) <= S.DRIFT_BOUND_ULP, err
