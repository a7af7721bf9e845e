"""az_adamw_flat_master (csrc/az_optim.hip) against tests/master_ref.py, bit for bit in p, w, m and v (a NaN equals a NaN): sizes around
the 8-wide group and the block, a range whose group loop wraps the capped grid, starts shifted by 0-7 elements with the five pointers
co-aligned (head, groups, tail) and with w shifted against the rest (everything element-wise), every moment / gradient type with and
without a clip coefficient, gradients holding NaN, +-inf and 0, a range cut in two calls, the drift experiment, the argument checks.
Every buffer sits between sentinel borders that must come back unchanged."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import elem_ref as R        # noqa: E402
import master_ref as M      # noqa: E402
import sr_ref as S          # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -1232.0            # exact in bf16, fp16 and fp32
PAD = 64
BF16, F32 = torch.bfloat16, torch.float32
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), wd=0.01, eps=1e-8, debias=0.3)
SIZES = (1, 7, 8, 9, 255, 4096 + 5)
WRAP_N = 8 * 1048576 + 8 * 3 + 5          # more than 8 x 4096 x 256 elements: the group loop of the capped grid runs a second time
COMBOS = [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd import ops as _ops
    return _ops


def vp(x):
    return ctypes.c_void_p(x)


def call(name, *args):
    from aozora_sdxl_training_amd._lib import lib
    return lib().call(name, *args)


def refused(*args):
    from aozora_sdxl_training_amd._lib import AozoraError
    with pytest.raises(AozoraError, match="argument error"):
        call("az_adamw_flat_master", *args)


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b, what):
    """Bit equality; a NaN counts as equal to a NaN whatever its payload."""
    a, b = a.to(DEV), b.to(DEV)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, tuple(a.shape), tuple(b.shape), a.dtype, b.dtype)
    eq = (bits(a) == bits(b)) | (a.isnan() & b.isnan())
    if not bool(eq.all()):
        i = int((~eq).reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int((~eq).sum())} of {eq.numel()} elements differ; first at {i}: {float(a[i])!r} vs {float(b[i])!r}")


def framed(n, dtype, fill, off):
    """PAD + off sentinels, n elements (from a CPU tensor), PAD sentinels -> (buffer, view).  Allocations are 256-byte aligned, so off
    is the view's distance in elements from a 16-byte boundary (mod 8 for 2-byte types, mod 4 for 4-byte ones)."""
    buf = torch.full((PAD + off + n + PAD,), SENT, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 256 == 0
    view = buf[PAD + off:PAD + off + n]
    view.copy_(fill.to(DEV))
    return buf, view


def frame_ok(buf, view, what):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    n = view.numel()
    assert bool((buf[:lo] == SENT).all()) and bool((buf[lo + n:] == SENT).all()), f"{what}: wrote outside its {n} elements"


def hyper_dev(hyper):
    return torch.from_numpy(np.stack(hyper)).to(DEV)


def state(n, mdtype, f32_grads, seed, steps=2):
    """Inputs of `steps` updates on the CPU: w fp32 (NOT bf16-representable: the master's low bits are live from the start), gradients
    with a 0, a NaN, an inf (elem_ref.adamw_grads) and a -inf, moments, hyper vectors."""
    g = R.gen(seed + 9)
    w = 0.1 * torch.randn(n, generator=g)
    grads = [R.adamw_grads(n, seed + 1 + s, f32_grads) for s in range(steps)]
    if n > 6:
        grads[0][5] = float("-inf")
    m = (1e-3 * torch.randn(n, generator=g)).to(R.moment_dtype(mdtype))
    v = (1e-4 * torch.rand(n, generator=g)).to(R.moment_dtype(mdtype))
    return w, grads, m, v, [R.adamw_hyper(step=s + 1, **HYPER) for s in range(steps)]


def master(ops, n, p, w, g, gdtype, m, v, mdtype, h, c):
    call("az_adamw_flat_master", n, ops._ptr(p), ops._ptr(w), ops._ptr(g), gdtype, ops._ptr(m), ops._ptr(v), mdtype, ops._ptr(h), ops._ptr(c),
         ops._stream())


def run_case(ops, n, mdtype, gdtype, coef, offs, seed, steps=2):
    """offs: element offsets of (p, w, g, m, v) from a 16-byte boundary.  Two updates on framed device buffers against the restatement."""
    w, grads, m, v, hyper = state(n, mdtype, gdtype == 1, seed, steps)
    po, wo, go, mo, vo = offs
    pb, pd = framed(n, BF16, torch.full((n,), 7.0, dtype=BF16), po)       # p is never read: its old contents must not matter
    wb, wd = framed(n, F32, w, wo)
    mb, md = framed(n, m.dtype, m, mo)
    vb, vd = framed(n, v.dtype, v, vo)
    hd = hyper_dev(hyper)
    cd = torch.tensor([coef], dtype=F32, device=DEV) if coef is not None else None
    for s in range(steps):
        gb, gd = framed(n, grads[s].dtype, grads[s], go)
        master(ops, n, pd, wd, gd, gdtype, md, vd, mdtype, hd[s], cd)
        p, w, m, v = M.adamw_master_bits(w, grads[s], m, v, hyper[s], coef)
        what = f"n={n} mdtype={mdtype} gdtype={gdtype} coef={coef} offsets={offs} step {s + 1}"
        same(pd, p, "p " + what); same(wd, w, "w " + what); same(md, m, "m " + what); same(vd, v, "v " + what)
        frame_ok(gb, gd, "g " + what)
        same(gd, grads[s], "g is read only " + what)
    frame_ok(pb, pd, "p"); frame_ok(wb, wd, "w"); frame_ok(mb, md, "m"); frame_ok(vb, vd, "v")


def test_the_offsets_select_the_two_forms():
    """All five pointers `shift` ELEMENTS past a 16-byte boundary (2-byte types shift * 2 bytes, 4-byte types shift * 4): element
    (8 - shift) % 8 aligns every one of them -- 16 or 32 bytes per 8 elements.  w one element further: p needs h = -shift (mod 8), w
    needs h = -(shift + 1) (mod 4): no element aligns both."""
    for s in range(8):
        h = (8 - s) % 8
        assert (2 * (s + h)) % 16 == 0 and (4 * (s + h)) % 16 == 0
        assert not [k for k in range(8) if (2 * (s + k)) % 16 == 0 and (4 * (s + 1 + k)) % 16 == 0]


# ---------------- (a) bit-exact against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mdtype,gdtype", COMBOS)
@pytest.mark.parametrize("coef", [None, 0.37])
def test_master_two_steps_bit_for_bit(ops, mdtype, gdtype, coef):
    """n = 1, 7: scalar only; 8, 9: one group (+ tail); 255: one block, ragged; 4101: several blocks.  Every start shift 0-7 with the five
    pointers co-aligned: head of (8 - shift) % 8 elements, groups, tail."""
    for n in SIZES:
        for shift in range(8):
            run_case(ops, n, mdtype, gdtype, coef, (shift,) * 5, seed=n + mdtype)


@pytest.mark.parametrize("mdtype,gdtype", COMBOS)
def test_master_elementwise_when_the_pointers_cannot_be_coaligned(ops, mdtype, gdtype):
    """w one element further from its 16-byte boundary than p, g, m, v from theirs, at every start shift 0-7: no element aligns all five,
    every element takes the scalar form -- same bits."""
    for n in (9, 4096 + 5):
        for shift in range(8):
            run_case(ops, n, mdtype, gdtype, 0.37, (shift, shift + 1, shift, shift, shift), seed=3 * n + mdtype)


def test_master_group_loop_wraps_the_capped_grid(ops):
    """8 388 637 elements = 1 048 579 groups for 4096 x 256 threads: threads 0-2 take a second group.  Start shift 0: no head, a
    5-element tail; shift 3: a 5-element head, the same groups, no tail.  bf16 moments and gradients, the production types; the
    restatement is computed once."""
    n = WRAP_N
    assert (n - 5) // 8 > 4096 * 256
    rng = np.random.default_rng(77)
    w = torch.from_numpy((0.1 * rng.standard_normal(n)).astype(np.float32))
    g = torch.from_numpy((1e-2 * rng.standard_normal(n)).astype(np.float32)).bfloat16()
    m = torch.from_numpy((1e-3 * rng.standard_normal(n)).astype(np.float32)).bfloat16()
    v = torch.from_numpy((1e-4 * rng.random(n)).astype(np.float32)).bfloat16()
    g[n - 1], g[n - 9], g[4096 * 256 * 8 + 3] = float("nan"), float("inf"), 0.0
    hyper = R.adamw_hyper(step=3, **HYPER)
    p1, w1, m1, v1 = M.adamw_master_bits(w, g, m, v, hyper, 0.37)
    cd, hd = torch.tensor([0.37], dtype=F32, device=DEV), hyper_dev([hyper])[0]
    for shift in (0, 3):
        pb, pd = framed(n, BF16, torch.zeros(1, dtype=BF16).expand(n), shift)
        wb, wd = framed(n, F32, w, shift)
        gb, gd = framed(n, BF16, g, shift)
        mb, md = framed(n, BF16, m, shift)
        vb, vd = framed(n, BF16, v, shift)
        master(ops, n, pd, wd, gd, 0, md, vd, 0, hd, cd)
        same(pd, p1, f"p shift {shift}"); same(wd, w1, f"w shift {shift}"); same(md, m1, f"m shift {shift}"); same(vd, v1, f"v shift {shift}")
        for b, x, nm in ((pb, pd, "p"), (wb, wd, "w"), (gb, gd, "g"), (mb, md, "m"), (vb, vd, "v")):
            frame_ok(b, x, nm)


# ---------------- (b) cut invariance -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [5, 1001])
def test_two_calls_equal_one(ops, a):
    n = 4096 + 5
    w, grads, m, v, hyper = state(n, 0, False, seed=21)
    hd = hyper_dev(hyper)[0]
    outs = []
    for cut in (None, a):
        pd, wd, gd, md, vd = torch.zeros(n, dtype=BF16, device=DEV), w.to(DEV), grads[0].to(DEV), m.to(DEV), v.to(DEV)
        if cut is None:
            master(ops, n, pd, wd, gd, 0, md, vd, 0, hd, None)
        else:
            master(ops, cut, pd, wd, gd, 0, md, vd, 0, hd, None)
            master(ops, n - cut, pd[cut:], wd[cut:], gd[cut:], 0, md[cut:], vd[cut:], 0, hd, None)
        outs.append((pd, wd, md, vd))
    for x, y, nm in zip(outs[0], outs[1], "pwmv"):
        same(y, x, f"{nm} cut at {a}")
    p1, w1, m1, v1 = M.adamw_master_bits(w, grads[0], m, v, hyper[0], None)
    same(outs[0][0], p1, "p"); same(outs[0][1], w1, "w")


# ---------------- (c) the drift experiment -------------------------------------------------------------------------------------------------
def test_drift_master_moves_where_round_to_nearest_stays(ops):
    d = S.DRIFT
    n = d["n"]
    hd = hyper_dev([S.drift_hyper(s) for s in range(1, d["steps"] + 1)])
    g = torch.full((n,), d["g"], dtype=F32, device=DEV)
    p = torch.full((n,), d["p0"], dtype=BF16, device=DEV)
    w = torch.full((n,), d["p0"], dtype=F32, device=DEV)
    m, v = torch.zeros(n, dtype=F32, device=DEV), torch.zeros(n, dtype=F32, device=DEV)
    for s in range(d["steps"]):
        master(ops, n, p, w, g, 1, m, v, 1, hd[s], None)
    want = torch.full((n,), S.drift_master(), dtype=torch.float64).float()
    same(w, want, "w against drift_master()")
    same(p, R.f32_to_bf16_bits(want), "p == bf16(w)")
    assert bool((p.float() == d["p0"] - 2 * S.DRIFT_ULP).all())


# ---------------- (d) the wrapper, empty ranges, argument errors ---------------------------------------------------------------------------
def test_ops_wrapper_runs_on_the_given_stream_and_checks_operands(ops):
    from aozora_sdxl_training_amd._lib import AozoraError
    n = 4096 + 5
    w, grads, m, v, hyper = state(n, 0, False, seed=31)
    pd, wd, gd, md, vd = torch.zeros(n, dtype=BF16, device=DEV), w.to(DEV), grads[0].to(DEV), m.to(DEV), v.to(DEV)
    hd, cd = hyper_dev(hyper)[0], torch.tensor([0.37], dtype=F32, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    ops.adamw_flat_master(pd, wd, gd, md, vd, hd, cd, side)
    side.synchronize()
    p1, w1, m1, v1 = M.adamw_master_bits(w, grads[0], m, v, hyper[0], 0.37)
    same(pd, p1, "p"); same(wd, w1, "w"); same(md, m1, "m"); same(vd, v1, "v")
    ops.adamw_flat_master(pd[:0], wd[:0], gd[:0], md[:0], vd[:0], hd)          # empty: nothing happens
    for bad in ((pd.float(), wd, gd, md, vd), (pd, wd.bfloat16(), gd, md, vd), (pd[:-1], wd, gd, md, vd), (pd, wd, gd, md, vd.float()),
                (pd.cpu(), wd, gd, md, vd), (pd, wd[::2], gd, md, vd), (pd, wd, gd.half(), md, vd)):
        with pytest.raises(AozoraError):
            ops.adamw_flat_master(*bad, hd)
    with pytest.raises(AozoraError):
        ops.adamw_flat_master(pd, wd, gd, md, vd, hd[:3])


def test_empty_range_launches_nothing_and_bad_arguments_are_refused(ops):
    from aozora_sdxl_training_amd._lib import lib
    n = 8
    p, g, m, v = (torch.full((n,), SENT, dtype=BF16, device=DEV) for _ in range(4))
    w = torch.full((n,), SENT, dtype=F32, device=DEV)
    h = hyper_dev([R.adamw_hyper(step=1, **HYPER)])[0]
    st = ops._stream()
    P, W, G, Mm, V, H = (x.data_ptr() for x in (p, w, g, m, v, h))
    assert lib().raw("az_adamw_flat_master")(ctypes.c_long(0), vp(P), vp(W), vp(G), 0, vp(Mm), vp(V), 0, vp(H), vp(0), st) == 0
    refused(-1, vp(P), vp(W), vp(G), 0, vp(Mm), vp(V), 0, vp(H), vp(0), st)
    for k in range(6):                                                       # a null p / w / g / m / v / hyper
        a = [P, W, G, Mm, V, H]
        a[k] = 0
        refused(n, vp(a[0]), vp(a[1]), vp(a[2]), 0, vp(a[3]), vp(a[4]), 0, vp(a[5]), vp(0), st)
    for mdt, gdt in ((3, 0), (-1, 0), (0, 2), (0, -1)):
        refused(n, vp(P), vp(W), vp(G), gdt, vp(Mm), vp(V), mdt, vp(H), vp(0), st)
    refused(n - 1, vp(P + 1), vp(W), vp(G), 0, vp(Mm), vp(V), 0, vp(H), vp(0), st)      # p not 2-byte aligned
    refused(n - 1, vp(P), vp(W + 2), vp(G), 0, vp(Mm), vp(V), 0, vp(H), vp(0), st)      # w not 4-byte aligned
    refused(n - 1, vp(P), vp(W + 1), vp(G), 0, vp(Mm), vp(V), 0, vp(H), vp(0), st)
    refused(0, vp(0), vp(W), vp(G), 0, vp(Mm), vp(V), 0, vp(H), vp(0), st)              # the checks come before the n == 0 return
    torch.cuda.synchronize()
    for x in (p, w, g, m, v):
        assert bool((x == SENT).all())
