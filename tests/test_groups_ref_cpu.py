"""tests/groups_ref.py against the single-group restatements it generalises: elem_ref.adamw_bits, master_ref.adamw_master_bits and
sr_ref.adamw_sr_bits called ONCE PER SEGMENT with that segment's hyper vector must give the bits of the per-element form; the lookup
(first segment whose end lies past the element, the last segment beyond the table, clamped ids) is checked on its own.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import elem_ref as R        # noqa: E402
import groups_ref as G      # noqa: E402
import master_ref as M      # noqa: E402
import sr_ref as S          # noqa: E402

HYPER = dict(lr=1e-3, betas=(0.9, 0.999), wd=0.01, eps=1e-8, debias=0.3)
GROUPS = [(1.0, 0.01), (1.0, 0.0), (0.25, 0.01), (0.0, 0.0)]


def eq(a, b):
    a, b = a.float().numpy(), b.float().numpy()
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def inputs(n, mdtype, f32, seed):
    g = R.gen(seed)
    p = (0.1 * torch.randn(n, generator=g)).bfloat16()
    w = 0.1 * torch.randn(n, generator=g)
    m = (1e-3 * torch.randn(n, generator=g)).to(R.moment_dtype(mdtype))
    v = (1e-4 * torch.rand(n, generator=g)).to(R.moment_dtype(mdtype))
    return p, w, R.adamw_grads(n, seed + 1, f32), m, v


def test_lookup():
    ends, gids = [3, 8, 13, 40], [0, 5, -2, 1]
    assert list(G.segment_of(ends, 0, 14)) == [0] * 3 + [1] * 5 + [2] * 5 + [3]
    assert list(G.segment_of(ends, 38, 4)) == [3, 3, 3, 3]                       # past the last end: the last segment
    assert list(G.group_ids(ends, gids, 3, 2, 12)) == [0] + [2] * 5 + [0] * 5 + [1]      # ids clamped to [0, 3)
    assert G.segments_in(ends, 2, 12) == [(0, 1, 0), (1, 6, 1), (6, 11, 2), (11, 12, 3)]
    assert G.segments_in([100], 7, 5) == [(0, 5, 0)]


def test_group_hyper_is_the_single_group_vector_per_group():
    for step in (1, 2, 50):
        gh = G.ghyper(GROUPS, HYPER["lr"], HYPER["betas"], HYPER["debias"], step)
        for (scale, wd), row in zip(GROUPS, gh):
            h = R.adamw_hyper(lr=HYPER["lr"] * scale, betas=HYPER["betas"], wd=wd, eps=HYPER["eps"], debias=HYPER["debias"], step=step)
            assert row[0] == h[4] and row[1] == h[5]
        assert gh[3][0] == 1.0 and gh[3][1] == 0.0


@pytest.mark.parametrize("mdtype,f32", [(0, False), (1, False), (2, False), (0, True), (1, True), (2, True)])
@pytest.mark.parametrize("coef", [None, 0.37])
def test_per_element_form_equals_one_call_per_segment(mdtype, f32, coef):
    n, elem0 = 301, 5
    ends, gids = G.random_table(elem0 + n + 40, 37, len(GROUPS), seed=3 + mdtype)
    p, w, g, m, v = inputs(n, mdtype, f32, 11 + mdtype)
    hyper = R.adamw_hyper(step=2, **HYPER)
    gh = G.ghyper(GROUPS, HYPER["lr"], HYPER["betas"], HYPER["debias"], 2)
    gid = G.group_ids(ends, gids, len(GROUPS), elem0, n)
    p1, m1, v1 = G.adamw_seg_bits(p, g, m, v, hyper, gh, gid, coef)
    pm, wm, mm, vm = G.adamw_seg_master_bits(w, g, m, v, hyper, gh, gid, coef)
    ps, ms, vs = G.adamw_seg_sr_bits(p, g, m, v, hyper, gh, gid, coef, 42, 2, 0, elem0)
    pieces = G.segments_in(ends, elem0, n)
    assert len(pieces) > 20
    for a, b, s in pieces:
        h = G.segment_hyper(hyper, gh, gids[s])
        sl = slice(a, b)
        p2, m2, v2 = R.adamw_bits(p[sl], g[sl], m[sl], v[sl], h, coef)
        assert eq(p1[sl], p2) and eq(m1[sl], m2) and eq(v1[sl], v2)
        p3, w3, m3, v3 = M.adamw_master_bits(w[sl], g[sl], m[sl], v[sl], h, coef)
        assert eq(pm[sl], p3) and eq(wm[sl], w3) and eq(mm[sl], m3) and eq(vm[sl], v3)
        p4, m4, v4 = S.adamw_sr_bits(p[sl], g[sl], m[sl], v[sl], h, coef, 42, 2, 0, elem0 + a)
        assert eq(ps[sl], p4) and eq(ms[sl], m4) and eq(vs[sl], v4)


def test_frozen_group_leaves_the_parameter_alone():
    """lr_scale 0 and weight_decay 0: wd_factor 1, step_size 0 -- p + (-0 * m) / denom = p bit for bit (finite moments)."""
    n = 64
    p, w, g, m, v = inputs(n, 0, False, 5)
    g = (1e-2 * torch.randn(n, generator=R.gen(6))).bfloat16()           # finite gradients
    hyper = R.adamw_hyper(step=1, **HYPER)
    gh = G.ghyper(GROUPS, HYPER["lr"], HYPER["betas"], HYPER["debias"], 1)
    p1, m1, v1 = G.adamw_seg_bits(p, g, m, v, hyper, gh, np.full(n, 3), None)
    assert eq(p1, p) and not eq(m1, m)
