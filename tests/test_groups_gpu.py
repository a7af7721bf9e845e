"""az_adamw_flat_seg (csrc/az_optim.hip) bit for bit, in p, w where present, m and v (a NaN equals a NaN), against two yardsticks: the
numpy restatement tests/groups_ref.py, and the single-group kernels az_adamw_flat_ex / _sr / _master launched ONCE PER SEGMENT with that
segment's hyper vector.  Sizes around the 8-wide group and the block, segments of one element, segment ends inside aligned groups of 8 and
exactly on the head / body / tail transitions, pointers and elem0 shifted by 0-7, a table far longer than the range, one segment (= the
single launch), a range cut in two calls, a range whose group loop wraps the capped grid under a thousand random segments, every moment /
gradient type, with and without a clip coefficient, gradients holding NaN, +-inf and 0, group ids outside the table (clamped), the argument
checks.  Every buffer sits between sentinel borders that must come back unchanged."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import elem_ref as R                # noqa: E402
import groups_ref as G              # noqa: E402
import test_master_gpu as T         # noqa: E402   (framed buffers, bit equality, WRAP_N)

pytestmark = pytest.mark.gpu

DEV, BF16, F32 = T.DEV, T.BF16, T.F32
HYPER = T.HYPER
GROUPS = [(1.0, 0.01), (1.0, 0.0), (0.25, 0.01), (0.0, 0.0), (3.0, 0.5)]
STEP = 2
SEED = 0x1234567890AB
MODES = ("plain", "sr", "master")
E0 = 4000                           # multiple of 8: elem0 = E0 + k puts the call's first element k past a Philox group


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd import ops as _ops
    return _ops


def vp(x):
    return ctypes.c_void_p(int(x))


def hyper_and_groups(step=STEP):
    return R.adamw_hyper(step=step, **HYPER), G.ghyper(GROUPS, HYPER["lr"], HYPER["betas"], HYPER["debias"], step)


class Table:
    """A segment table and the group values on the device."""
    def __init__(self, ends, gids, gh, ngroups=None):
        self.ends, self.gids, self.gh = list(ends), list(gids), gh
        self.ngroups = len(gh) if ngroups is None else ngroups
        self.end_dev = torch.tensor(self.ends, dtype=torch.int64, device=DEV)
        self.gid_dev = torch.tensor(self.gids, dtype=torch.int32, device=DEV)
        self.gh_dev = torch.from_numpy(np.ascontiguousarray(gh, dtype=np.float32)).to(DEV)

    def args(self, elem0):
        return (vp(self.end_dev.data_ptr()), vp(self.gid_dev.data_ptr()), len(self.ends), vp(self.gh_dev.data_ptr()), self.ngroups, int(elem0))


def seg(ops, mode, n, p, w, g, gdtype, m, v, mdtype, h, c, tab, elem0, step=STEP):
    T.call("az_adamw_flat_seg", n, ops._ptr(p), ops._ptr(w if mode == "master" else None), ops._ptr(g), gdtype, ops._ptr(m), ops._ptr(v), mdtype,
           ops._ptr(h), ops._ptr(c), *tab.args(elem0), int(mode == "sr"), SEED, step, 0, ops._stream())


def parent(ops, mode, n, p, w, g, gdtype, m, v, mdtype, h, c, elem0, step=STEP):
    """The single-group entry points of the parent commit."""
    rest = (ops._ptr(g), gdtype, ops._ptr(m), ops._ptr(v), mdtype, ops._ptr(h), ops._ptr(c))
    if mode == "master":
        T.call("az_adamw_flat_master", n, ops._ptr(p), ops._ptr(w), *rest, ops._stream())
    elif mode == "sr":
        T.call("az_adamw_flat_sr", n, ops._ptr(p), *rest, SEED, step, 0, int(elem0), ops._stream())
    else:
        T.call("az_adamw_flat_ex", n, ops._ptr(p), *rest, ops._stream())


def state(n, mdtype, f32_grads, seed):
    """p bf16, w fp32 (not bf16-representable), gradients with a 0, a NaN, an inf (elem_ref.adamw_grads) and a -inf, moments."""
    g = R.gen(seed + 9)
    p = (0.1 * torch.randn(n, generator=g)).bfloat16()
    w = 0.1 * torch.randn(n, generator=g)
    grad = R.adamw_grads(n, seed + 1, f32_grads)
    if n > 6:
        grad[5] = float("-inf")
    m = (1e-3 * torch.randn(n, generator=g)).to(R.moment_dtype(mdtype))
    v = (1e-4 * torch.rand(n, generator=g)).to(R.moment_dtype(mdtype))
    return p, w, grad, m, v


def restate(mode, p, w, g, m, v, hyper, gh, gid, coef, elem0, step=STEP):
    """-> dict of the expected tensors."""
    if mode == "master":
        p1, w1, m1, v1 = G.adamw_seg_master_bits(w, g, m, v, hyper, gh, gid, coef)
        return dict(p=p1, w=w1, m=m1, v=v1)
    if mode == "sr":
        p1, m1, v1 = G.adamw_seg_sr_bits(p, g, m, v, hyper, gh, gid, coef, SEED, step, 0, elem0)
    else:
        p1, m1, v1 = G.adamw_seg_bits(p, g, m, v, hyper, gh, gid, coef)
    return dict(p=p1, m=m1, v=v1)


def run_case(ops, mode, n, mdtype, gdtype, coef, offs, elem0, ends, gids, seed, with_parent=True, ngroups=None):
    """One update on framed device buffers by the segmented kernel, and by the parent's kernels once per segment on a second set of
    buffers; both against the restatement.  offs: element offsets of (p, w, g, m, v) from a 16-byte boundary."""
    hyper, gh = hyper_and_groups()
    tab = Table(ends, gids, gh, ngroups)
    p, w, g, m, v = state(n, mdtype, gdtype == 1, seed)
    gid = G.group_ids(ends, gids, tab.ngroups, elem0, n)
    want = restate(mode, p, w, g, m, v, hyper, gh, gid, coef, elem0)
    hd = torch.from_numpy(hyper).to(DEV)
    cd = torch.tensor([coef], dtype=F32, device=DEV) if coef is not None else None
    po, wo, go, mo, vo = offs
    what = f"{mode} n={n} mdtype={mdtype} gdtype={gdtype} coef={coef} offsets={offs} elem0={elem0} segments={len(ends)}"

    def buffers():
        # master: p is never read, its old contents must not matter
        pf = T.framed(n, BF16, torch.full((n,), 7.0, dtype=BF16) if mode == "master" else p, po)
        return dict(p=pf, w=T.framed(n, F32, w, wo), g=T.framed(n, g.dtype, g, go), m=T.framed(n, m.dtype, m, mo), v=T.framed(n, v.dtype, v, vo))

    def check(b, who):
        for k, t in want.items():
            T.same(b[k][1], t, f"{k} {who} {what}")
        T.same(b["g"][1], g, f"g is read only {who} {what}")
        if mode != "master":
            T.same(b["w"][1], w, f"w untouched {who} {what}")
        for k, (buf, view) in b.items():
            T.frame_ok(buf, view, f"{k} {who} {what}")

    b = buffers()
    seg(ops, mode, n, b["p"][1], b["w"][1], b["g"][1], gdtype, b["m"][1], b["v"][1], mdtype, hd, cd, tab, elem0)
    check(b, "segmented")
    if not with_parent:
        return
    b2 = buffers()
    pieces = G.segments_in(ends, elem0, n)
    hs = torch.from_numpy(np.stack([G.segment_hyper(hyper, gh, k) for k in range(len(gh))])).to(DEV)
    for a, e, s in pieces:
        k = int(np.clip(gids[s], 0, tab.ngroups - 1))
        parent(ops, mode, e - a, b2["p"][1][a:e], b2["w"][1][a:e], b2["g"][1][a:e], gdtype, b2["m"][1][a:e], b2["v"][1][a:e], mdtype, hs[k], cd,
               elem0 + a)
    check(b2, f"parent x {len(pieces)}")
    for k in want:
        T.same(b[k][1], b2[k][1], f"{k} segmented against the parent's launches {what}")


# ---------------- tables -------------------------------------------------------------------------------------------------------------------
def cycle(n):
    return [k % len(GROUPS) for k in range(n)]


def table_alternating(elem0, n):
    """Segments of one element, groups alternating, from 0 to past the range."""
    ends = list(range(1, elem0 + n + 9))
    return ends, cycle(len(ends))


def table_inside_groups(elem0, n):
    """Ends at elem0 + 3, 8, 13, 24, ...: inside aligned groups of 8 wherever the range starts."""
    ends, e, k, lens = [], elem0, 0, (3, 5, 5, 11, 8, 1, 7, 16, 2)
    while e < elem0 + n:
        e += lens[k % len(lens)]
        k += 1
        ends.append(e)
    return ends, cycle(len(ends))


def table_on_transitions(elem0, n, head):
    """Ends exactly where the head meets the body and the body meets the tail (head: scalar elements in front of the first group)."""
    head = min(head, n)
    body = head + ((n - head) // 8) * 8
    ends = sorted({elem0 + x for x in (head, body) if 0 < x < n} | {elem0 + n + 64})
    return ends, [(k + 1) % len(GROUPS) for k in range(len(ends))]


def table_wide(elem0, n):
    """Far more table than range, in front of it and behind; elem0 lies in the middle of a segment."""
    ends = [10, 200, 1024, elem0 - 7, elem0 + (n + 1) // 2, elem0 + n + 100, elem0 + n + 5000, elem0 + n + 5001, 2 ** 40]
    return ends, [4, 3, 2, 1, 2, 3, 0, 1, 2]


def head_of(shift):
    return (8 - shift) % 8


def elem0_for(mode, shift):
    """sr: a group of 8 needs (elem0 + i) % 8 == 0 where the pointers are 16-byte aligned -- elem0 = shift (mod 8) keeps the wide form;
    the other two modes take any elem0: shifted independently of the pointers."""
    return E0 + (shift if mode == "sr" else (3 * shift + 1) % 8)


# ---------------- (a) the table shapes, every size, every shift ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["alternating", "inside_groups", "on_transitions", "wide", "one"])
def test_tables_sizes_and_shifts(ops, mode, kind):
    for n in T.SIZES:
        for shift in range(8):
            elem0 = elem0_for(mode, shift)
            if kind == "alternating":
                ends, gids = table_alternating(elem0, n)
            elif kind == "inside_groups":
                ends, gids = table_inside_groups(elem0, n)
            elif kind == "on_transitions":
                ends, gids = table_on_transitions(elem0, n, head_of(shift))
            elif kind == "wide":
                ends, gids = table_wide(elem0, n)
            else:
                ends, gids = [elem0 + n], [2]
            # the parent's kernels once per segment: everywhere but the thousands of launches of the largest size (two shifts there)
            with_parent = n < 4096 or kind in ("on_transitions", "wide", "one") or shift in (0, 3)
            run_case(ops, mode, n, 0, 0, 0.37, (shift,) * 5, elem0, ends, gids, seed=n + shift, with_parent=with_parent)


@pytest.mark.parametrize("mode", MODES)
def test_one_segment_equals_the_single_launch(ops, mode):
    """One segment over everything, its group the base: the parent's ONE launch with the plain hyper vector."""
    n, elem0 = 4096 + 5, E0
    hyper, gh = hyper_and_groups()
    p, w, g, m, v = state(n, 0, False, 77)
    hd, cd = torch.from_numpy(hyper).to(DEV), torch.tensor([0.37], dtype=F32, device=DEV)
    tab = Table([elem0 + n], [0], gh)
    assert gh[0][0] == hyper[4] and gh[0][1] == hyper[5]
    outs = []
    for which in ("segmented", "parent"):
        pd, wd, gd, md, vd = p.to(DEV), w.to(DEV), g.to(DEV), m.to(DEV), v.to(DEV)
        if which == "segmented":
            seg(ops, mode, n, pd, wd, gd, 0, md, vd, 0, hd, cd, tab, elem0)
        else:
            parent(ops, mode, n, pd, wd, gd, 0, md, vd, 0, hd, cd, elem0)
        outs.append((pd, wd, md, vd))
    for x, y, nm in zip(outs[0], outs[1], "pwmv"):
        T.same(x, y, f"{nm} {mode}")


# ---------------- (b) every type pair, with and without the clip coefficient ----------------------------------------------------------------
@pytest.mark.parametrize("mdtype,gdtype", T.COMBOS)
@pytest.mark.parametrize("coef", [None, 0.37])
@pytest.mark.parametrize("mode", MODES)
def test_every_type_pair(ops, mode, mdtype, gdtype, coef):
    n = 1000 + 5
    for shift in (0, 5):
        elem0 = elem0_for(mode, shift)
        ends, gids = table_inside_groups(elem0, n)
        run_case(ops, mode, n, mdtype, gdtype, coef, (shift,) * 5, elem0, ends, gids, seed=17 + mdtype + 3 * gdtype)


@pytest.mark.parametrize("mode", MODES)
def test_elementwise_when_nothing_coaligns(ops, mode):
    """g one element further from its 16-byte boundary than the rest (and, sr, elem0 off the pointers' phase): every element scalar."""
    n = 4096 + 5
    for shift in (0, 6):
        elem0 = E0 + shift + (1 if mode == "sr" else 0)
        ends, gids = table_inside_groups(elem0, n)
        offs = (shift,) * 5 if mode == "sr" else (shift, shift, shift + 1, shift, shift)
        run_case(ops, mode, n, 0, 0, 0.37, offs, elem0, ends, gids, seed=23, with_parent=shift == 0)


# ---------------- (c) cut invariance, the wrapped grid ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("a", [5, 1001])
def test_two_calls_equal_one(ops, mode, a):
    n, elem0 = 4096 + 5, E0
    hyper, gh = hyper_and_groups()
    ends, gids = table_inside_groups(elem0, n)
    tab = Table(ends, gids, gh)
    p, w, g, m, v = state(n, 0, False, 21)
    hd = torch.from_numpy(hyper).to(DEV)
    outs = []
    for cut in (None, a):
        pd, wd, gd, md, vd = p.to(DEV), w.to(DEV), g.to(DEV), m.to(DEV), v.to(DEV)
        if cut is None:
            seg(ops, mode, n, pd, wd, gd, 0, md, vd, 0, hd, None, tab, elem0)
        else:
            seg(ops, mode, cut, pd, wd, gd, 0, md, vd, 0, hd, None, tab, elem0)
            seg(ops, mode, n - cut, pd[cut:], wd[cut:], gd[cut:], 0, md[cut:], vd[cut:], 0, hd, None, tab, elem0 + cut)
        outs.append(dict(p=pd, w=wd, m=md, v=vd))
    want = restate(mode, p, w, g, m, v, hyper, gh, G.group_ids(ends, gids, len(gh), elem0, n), None, elem0)
    for k, t in want.items():
        T.same(outs[0][k], t, f"{k} one call")
        T.same(outs[1][k], outs[0][k], f"{k} cut at {a}")


def test_group_loop_wraps_the_capped_grid_under_a_thousand_segments(ops):
    """8 388 637 elements = 1 048 579 groups for 4096 x 256 threads: threads 0-2 take a second group, whose segments lie at the far end
    of the table.  Start shift 3: a 5-element head, no tail.  A thousand pseudo-random segment lengths; the restatement is computed once,
    the parent's kernel runs once per segment on a second set of buffers."""
    n, shift, elem0 = T.WRAP_N, 3, E0 + 1
    assert (n - 5) // 8 > 4096 * 256
    hyper, gh = hyper_and_groups(3)
    ends, gids = G.random_table(elem0 + n, 1000, len(GROUPS), seed=5)
    tab = Table(ends, gids, gh)
    rng = np.random.default_rng(77)
    p = torch.from_numpy((0.1 * rng.standard_normal(n)).astype(np.float32)).bfloat16()
    g = torch.from_numpy((1e-2 * rng.standard_normal(n)).astype(np.float32)).bfloat16()
    m = torch.from_numpy((1e-3 * rng.standard_normal(n)).astype(np.float32)).bfloat16()
    v = torch.from_numpy((1e-4 * rng.random(n)).astype(np.float32)).bfloat16()
    g[n - 1], g[n - 9], g[4096 * 256 * 8 + 3] = float("nan"), float("inf"), 0.0
    p1, m1, v1 = G.adamw_seg_bits(p, g, m, v, hyper, gh, G.group_ids(ends, gids, len(gh), elem0, n), 0.37)
    cd, hd = torch.tensor([0.37], dtype=F32, device=DEV), torch.from_numpy(hyper).to(DEV)
    hs = torch.from_numpy(np.stack([G.segment_hyper(hyper, gh, k) for k in range(len(gh))])).to(DEV)
    outs = []
    for which in ("segmented", "parent"):
        fr = [T.framed(n, BF16, x, shift) for x in (p, g, m, v)]
        (pb, pd), (gb, gd), (mb, md), (vb, vd) = fr
        if which == "segmented":
            seg(ops, "plain", n, pd, None, gd, 0, md, vd, 0, hd, cd, tab, elem0, step=3)
        else:
            for a, e, s in G.segments_in(ends, elem0, n):
                parent(ops, "plain", e - a, pd[a:e], None, gd[a:e], 0, md[a:e], vd[a:e], 0, hs[gids[s]], cd, elem0 + a, step=3)
        T.same(pd, p1, f"p {which}"); T.same(md, m1, f"m {which}"); T.same(vd, v1, f"v {which}")
        for (b, x), nm in zip(fr, "pgmv"):
            T.frame_ok(b, x, nm)
        outs.append((pd, md, vd))
    for x, y, nm in zip(outs[0], outs[1], "pmv"):
        T.same(x, y, nm)


# ---------------- (d) what the tables may hold, empty ranges, argument errors ----------------------------------------------------------------
def test_ids_outside_the_group_table_are_clamped_and_the_last_segment_never_ends(ops):
    """The documented clamp (include/aozora_hip.h): ids below 0 read group 0, ids past the table its last group; an element past the
    last end takes the last segment."""
    n, elem0 = 255, E0 + 2
    ends = [elem0 + 10, elem0 + 50, elem0 + 100]                # the range goes on for 155 elements past the last end
    for mode in MODES:
        run_case(ops, mode, n, 0, 0, None, (2,) * 5, elem0, ends, [-5, 300, 2 ** 31 - 1], seed=9, with_parent=True)
        run_case(ops, mode, n, 0, 0, None, (2,) * 5, elem0, ends, [1, 2, 7], seed=9, with_parent=True, ngroups=3)


def test_empty_range_launches_nothing_and_bad_arguments_are_refused(ops):
    from aozora_sdxl_training_amd._lib import AozoraError, lib
    n = 8
    p, g, m, v = (torch.full((n,), T.SENT, dtype=BF16, device=DEV) for _ in range(4))
    w = torch.full((n,), T.SENT, dtype=F32, device=DEV)
    hyper, gh = hyper_and_groups()
    h = torch.from_numpy(hyper).to(DEV)
    tab = Table([100], [0], gh)
    st = ops._stream()
    P, W, Gp, Mm, V, H, SE, SG, GH = (x.data_ptr() for x in (p, w, g, m, v, h, tab.end_dev, tab.gid_dev, tab.gh_dev))

    def args(n=n, P=P, W=0, Gp=Gp, gdt=0, Mm=Mm, V=V, mdt=0, H=H, SE=SE, SG=SG, nseg=1, GH=GH, ng=len(GROUPS), elem0=0, rounding=0):
        return (ctypes.c_long(n), vp(P), vp(W), vp(Gp), gdt, vp(Mm), vp(V), mdt, vp(H), vp(0), vp(SE), vp(SG), ctypes.c_long(nseg), vp(GH), ng,
                ctypes.c_long(elem0), rounding, ctypes.c_long(1), ctypes.c_long(1), ctypes.c_long(0), st)

    raw = lib().raw("az_adamw_flat_seg")
    assert raw(*args(n=0)) == 0                                             # empty: nothing happens
    bad = [dict(n=-1), dict(P=0), dict(Gp=0), dict(Mm=0), dict(V=0), dict(H=0), dict(SE=0), dict(SG=0), dict(GH=0),       # null operands / tables
           dict(nseg=0), dict(nseg=-3), dict(ng=0), dict(ng=256), dict(ng=-1), dict(elem0=-1),
           dict(mdt=3), dict(mdt=-1), dict(gdt=2), dict(gdt=-1), dict(rounding=2), dict(rounding=-1),
           dict(W=W, rounding=1),                                                                                          # master with stochastic rounding
           dict(P=P + 1), dict(W=W + 2), dict(Gp=Gp + 1), dict(Mm=Mm + 1), dict(V=V + 1),                                   # not aligned to the element
           dict(Gp=Gp + 2, gdt=1), dict(Mm=Mm + 2, V=V + 2, mdt=1), dict(SE=SE + 4), dict(SG=SG + 2), dict(GH=GH + 2),
           dict(n=0, P=0)]                                                                                                 # the checks come before the n == 0 return
    for kw in bad:
        with pytest.raises(AozoraError, match="argument error"):
            T.call("az_adamw_flat_seg", *args(**kw))
    torch.cuda.synchronize()
    for x in (p, w, g, m, v):
        assert bool((x == T.SENT).all())


def test_ops_wrapper_routes_and_refuses(ops):
    """ops.adamw_range(groups=) is the one caller: it reaches the segmented kernel in all three modes, refuses the pinned-host pipeline and
    a stochastic-rounding index that differs from the lookup's; ops.check_group_tables refuses malformed host tables."""
    from aozora_sdxl_training_amd._lib import AozoraError
    n, elem0 = 1000 + 5, E0
    hyper, gh = hyper_and_groups()
    ends, gids = table_inside_groups(elem0, n)
    tab = Table(ends, gids, gh)
    hd = torch.from_numpy(hyper).to(DEV)
    gid = G.group_ids(ends, gids, len(gh), elem0, n)
    groups = (tab.end_dev.data_ptr(), tab.gid_dev.data_ptr(), len(ends), tab.gh_dev.data_ptr(), len(gh), elem0)
    stream = torch.cuda.current_stream().cuda_stream
    for mode in MODES:
        p, w, g, m, v = state(n, 0, False, 41)
        pd, wd, gd, md, vd = p.to(DEV), w.to(DEV), g.to(DEV), m.to(DEV), v.to(DEV)
        ops.adamw_range(n, pd.data_ptr(), gd.data_ptr(), 0, md.data_ptr(), vd.data_ptr(), BF16, hd.data_ptr(), None, stream,
                        master=wd.data_ptr() if mode == "master" else None, sr=(SEED, STEP, 0, elem0) if mode == "sr" else None, groups=groups)
        want = restate(mode, p, w, g, m, v, hyper, gh, gid, None, elem0)
        got = dict(p=pd, w=wd, m=md, v=vd)
        for k, t in want.items():
            T.same(got[k], t, f"{k} {mode}")
    with pytest.raises(AozoraError, match="pinned-host"):
        ops.adamw_range(n, 0, 0, 0, 0, 0, BF16, 0, None, stream, groups=groups, host_pipeline=(0, 1, 0, 0))
    with pytest.raises(AozoraError, match="same global element"):
        ops.adamw_range(n, 0, 0, 0, 0, 0, BF16, 0, None, stream, groups=groups, sr=(SEED, STEP, 0, elem0 + 8))
    ok = ([64, 128, 4096], [0, 1, 0], 2, [(0, 128), (256, 4096)])
    assert ops.check_group_tables(*ok) == ([64, 128, 4096], [0, 1, 0])
    for bad in (([64, 64, 4096], [0, 1, 0], 2, []), ([128, 64, 4096], [0, 1, 0], 2, []), ([64, 128], [0, 1, 0], 2, []), ([], [], 1, []),
                ([64, 128, 4096], [0, 2, 0], 2, []), ([64, 128, 4096], [0, -1, 0], 2, []), ([64, 128, 4096], [0, 1, 0], 256, []),
                ([64, 128, 4096], [0, 1, 0], 0, []), ([64, 128, 4096], [0, 1, 0], 2, [(0, 4097)]), ([0, 128], [0, 1], 2, [])):
        with pytest.raises(AozoraError):
            ops.check_group_tables(*bad)
