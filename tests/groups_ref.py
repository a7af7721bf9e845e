"""Numpy restatement of az_adamw_flat_seg (csrc/az_optim.hip): the group of every element from the segment table, then elem_ref.adamw_bits'
/ master_ref's / sr_ref's arithmetic with wd_factor and step_size PER ELEMENT -- nothing else differs from those restatements."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import elem_ref as R        # noqa: E402
import sr_ref as S          # noqa: E402


def ghyper(groups, lr, betas, debias, step):
    """fp32 [G][2] = [wd_factor, step_size] of every (lr_scale, weight_decay) group, formed like elem_ref.adamw_hyper's entries 4 and 5:
    in Python doubles, rounded once."""
    b1 = betas[0]
    bc1 = 1.0 - b1 ** step
    if debias < 1.0:
        bc1 = 1.0 - (1.0 - bc1) * debias
    rows = []
    for scale, wd in groups:
        lr_g = lr * scale
        rows.append([1.0 - lr_g * wd if wd != 0 else 1.0, lr_g / bc1])
    return np.array(rows, dtype=np.float32)


def segment_of(seg_end, elem0, n):
    """Index of the first segment with end > e for e = elem0 .. elem0 + n - 1; past the last end: the last segment."""
    ends = np.asarray(seg_end, dtype=np.int64)
    e = np.int64(elem0) + np.arange(n, dtype=np.int64)
    return np.minimum(np.searchsorted(ends, e, side="right"), len(ends) - 1)


def group_ids(seg_end, seg_gid, ngroups, elem0, n):
    gid = np.asarray(seg_gid, dtype=np.int64)[segment_of(seg_end, elem0, n)]
    return np.clip(gid, 0, ngroups - 1)            # the kernel's clamp


def segments_in(seg_end, elem0, n):
    """[(a, b, segment index)] -- the pieces [a, b) of the call's range [0, n) that lie in one segment each."""
    s = segment_of(seg_end, elem0, n)
    cuts = [0] + [int(i) + 1 for i in np.nonzero(s[1:] != s[:-1])[0]] + [n]
    return [(a, b, int(s[a])) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def _pp(param_f32, g, m, v, hyper, gh, gid, coef):
    """elem_ref.adamw_bits up to the fp32 parameter value with per-element wdf / step -> (pp float32, m, v as stored)."""
    mdtype = {torch.bfloat16: 0, torch.float32: 1, torch.float16: 2}[m.dtype]
    f = np.float32
    b1, b2, eps, sbc2 = f(hyper[1]), f(hyper[2]), f(hyper[3]), f(hyper[6])
    gh = np.asarray(gh, dtype=np.float32)
    wdf, step = gh[gid, 0], gh[gid, 1]
    omb1, omb2 = f(1.0) - b1, f(1.0) - b2
    with np.errstate(all="ignore"):
        gr = g.float().numpy() * (f(coef) if coef is not None else f(1.0))
        if g.dtype == torch.bfloat16:
            gr = R.bf16_round_np(gr)
        mm = R.fma32(gr, np.full_like(gr, omb1), m.float().numpy() * b1)
        vv = v.float().numpy() * b2
        vv = vv + ((omb2 * gr) * gr)
        pp = param_f32 * wdf
        denom = np.sqrt(vv) / sbc2 + eps
        pp = pp + ((-step * mm) / denom)
    return np.ascontiguousarray(pp, dtype=np.float32), R._store(mm, mdtype), R._store(vv, mdtype)


def adamw_seg_bits(p, g, m, v, hyper, gh, gid, coef=None):
    """Round to nearest: p bf16 -> (p, m, v)."""
    pp, m2, v2 = _pp(R.bf16_to_np(p), g, m, v, hyper, gh, gid, coef)
    return R.bits_to_bf16(R.bf16_bits_np(pp)), m2, v2


def adamw_seg_master_bits(w, g, m, v, hyper, gh, gid, coef=None):
    """fp32 master: -> (p bf16, w fp32, m, v)."""
    pp, m2, v2 = _pp(w.numpy().astype(np.float32), g, m, v, hyper, gh, gid, coef)
    return R.bits_to_bf16(R.bf16_bits_np(pp)), torch.from_numpy(pp.copy()), m2, v2


def adamw_seg_sr_bits(p, g, m, v, hyper, gh, gid, coef, seed, step, domain, elem0):
    """Stochastic rounding with the bits of global index elem0 + i: -> (p, m, v)."""
    pp, m2, v2 = _pp(R.bf16_to_np(p), g, m, v, hyper, gh, gid, coef)
    e = np.int64(elem0) + np.arange(pp.shape[0], dtype=np.int64)
    return R.bits_to_bf16(S.sr_round(pp, S.sr_bits16(seed, step, domain, e))), m2, v2


def segment_hyper(hyper, gh, g):
    """The 8-float hyper vector a single-group kernel needs for group g: the base vector with entries 4 and 5 from the group table."""
    h = np.array(hyper, dtype=np.float32).copy()
    h[4], h[5] = np.float32(gh[g][0]), np.float32(gh[g][1])
    return h


def random_table(total, nseg, ngroups, seed):
    """nseg pseudo-random segment lengths covering [0, total), group ids cycling with a random start."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, total), size=nseg - 1, replace=False))
    ends = [int(c) for c in cuts] + [int(total)]
    gids = [int(x) for x in rng.integers(0, ngroups, size=nseg)]
    return ends, gids

