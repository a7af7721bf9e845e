"""az_adamw_flat_sr / az_raven_step_sr (csrc/az_optim.hip) against tests/sr_ref.py, bit for bit: every moment / gradient type, ranges
whose head and tail leave the 8-wide body, a global index past 2^35 (the counter's second word), the element-wise fallback, cut
invariance, the chunked host-state pipeline, and the drift experiment that motivates the option."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import elem_ref as R        # noqa: E402
import sr_ref as S          # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -1232.0            # exact in bf16, fp16 and fp32
PAD = 64
BF16, F32 = torch.bfloat16, torch.float32
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), wd=0.01, eps=1e-8, debias=0.3)
SEED = 123456789012       # needs the key's second word


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


def refused(name, *args):
    from aozora_sdxl_training_amd._lib import AozoraError
    with pytest.raises(AozoraError, match="argument error"):
        call(name, *args)


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
    """off elements of sentinel, n elements (from a CPU tensor), a sentinel tail -> (buffer, view).  off moves the view off the
    allocation's 16-byte alignment the way a range that starts at global index off (mod 8) of an aligned flat buffer is."""
    buf = torch.full((PAD + n + PAD,), SENT, dtype=dtype, device=DEV)
    view = buf[off:off + n]
    view.copy_(fill.to(DEV))
    return buf, view, off


def frame_ok(buf, view, off, what):
    n = view.numel()
    assert bool((buf[:off] == SENT).all()) and bool((buf[off + n:] == SENT).all()), f"{what}: wrote outside its {n} elements"


def hyper_dev(hyper):
    return torch.from_numpy(np.stack(hyper)).to(DEV)


def state(n, mdtype, f32_grads, seed):
    p = R.gauss_bf16((n,), seed=seed, scale=0.1)
    grads = [R.adamw_grads(n, seed + 1 + s, f32_grads) for s in range(2)]
    g = R.gen(seed + 9)
    m = (1e-3 * torch.randn(n, generator=g)).to(R.moment_dtype(mdtype))
    v = (1e-4 * torch.rand(n, generator=g)).to(R.moment_dtype(mdtype))
    hyper = [R.adamw_hyper(step=s + 1, **HYPER) for s in range(2)]
    return p, grads, m, v, hyper


def flat_sr(ops, n, p, g, gdtype, m, v, mdtype, h, c, seed, step, domain, elem0):
    call("az_adamw_flat_sr", n, ops._ptr(p), ops._ptr(g), gdtype, ops._ptr(m), ops._ptr(v), mdtype, ops._ptr(h), ops._ptr(c), seed, step, domain, elem0,
         ops._stream())


# ---------------- (a) bit-exact against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("mdtype,gdtype", [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)])
def test_flat_sr_two_steps_bit_for_bit(ops, mdtype, gdtype):
    """n = 1, 7: head only; 8, 9: one whole group (+ tail); 4099, 65 541: several blocks, ragged.  elem0 = 3 and 2^35 - 5 start the
    range 3 elements into a group (the buffers are offset alike, as a range of a flat buffer is); 2^35 - 5 crosses into the counter's
    second word inside the range."""
    for n in (1, 7, 8, 9, 4099, 65541):
        for elem0 in (0, 3, 2 ** 35 - 5):
            for coef in (None, 0.37):
                p, grads, m, v, hyper = state(n, mdtype, gdtype == 1, seed=n + mdtype)
                off = elem0 & 7
                pb, pd, _ = framed(n, BF16, p, off)
                mb, md, _ = framed(n, m.dtype, m, off)
                vb, vd, _ = framed(n, v.dtype, v, off)
                hd = hyper_dev(hyper)
                cd = torch.tensor([coef], dtype=F32, device=DEV) if coef is not None else None
                for s in range(2):
                    gb, gd, _ = framed(n, grads[s].dtype, grads[s], off)
                    flat_sr(ops, n, pd, gd, gdtype, md, vd, mdtype, hd[s], cd, SEED, s + 1, 0, elem0)
                    m_rn, v_rn = R.adamw_bits(p, grads[s], m, v, hyper[s], coef)[1:]
                    p, m, v = S.adamw_sr_bits(p, grads[s], m, v, hyper[s], coef, SEED, s + 1, 0, elem0)
                    what = f"n={n} elem0={elem0} coef={coef} step {s + 1}"
                    same(md, m, "m " + what); same(vd, v, "v " + what); same(pd, p, "p " + what)
                    same(md, m_rn, "m against adamw_bits " + what); same(vd, v_rn, "v against adamw_bits " + what)
                frame_ok(pb, pd, off, "p"); frame_ok(mb, md, off, "m"); frame_ok(vb, vd, off, "v")


@pytest.mark.parametrize("mdtype,gdtype", [(0, 0), (1, 1)])
def test_flat_sr_elementwise_fallback(ops, mdtype, gdtype):
    """Pointers whose 16-byte alignment does not coincide with the group boundary of the global index (here: aligned + 1 element at
    elem0 = 0, and one buffer only) take the element-wise path: same bits."""
    n = 4099
    for which in ("all", "m"):
        p, grads, m, v, hyper = state(n, mdtype, gdtype == 1, seed=11)
        o = {k: (1 if which in ("all", k) else 0) for k in "pgmv"}
        pb, pd, _ = framed(n, BF16, p, o["p"])
        gb, gd, _ = framed(n, grads[0].dtype, grads[0], o["g"])
        mb, md, _ = framed(n, m.dtype, m, o["m"])
        vb, vd, _ = framed(n, v.dtype, v, o["v"])
        flat_sr(ops, n, pd, gd, gdtype, md, vd, mdtype, hyper_dev(hyper)[0], None, 42, 1, 0, 0)
        p1, m1, v1 = S.adamw_sr_bits(p, grads[0], m, v, hyper[0], None, 42, 1, 0, 0)
        same(pd, p1, "p " + which); same(md, m1, "m " + which); same(vd, v1, "v " + which)
        frame_ok(pb, pd, o["p"], "p"); frame_ok(mb, md, o["m"], "m"); frame_ok(vb, vd, o["v"], "v")


# ---------------- (b) cut invariance ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole(ops):
    """One call over [0, n): inputs (CPU) and the device result, shared by the cut tests."""
    n, mdtype, gdtype = 4099, 0, 0
    p, grads, m, v, hyper = state(n, mdtype, False, seed=21)
    pd, md, vd, gd = p.to(DEV), m.to(DEV), v.to(DEV), grads[0].to(DEV)
    hd = hyper_dev(hyper)
    flat_sr(ops, n, pd, gd, gdtype, md, vd, mdtype, hd[0], None, 42, 1, 0, 0)
    torch.cuda.synchronize()
    return dict(n=n, p=p, g=grads, m=m, v=v, hyper=hyper, hd=hd, out=(pd, md, vd))


@pytest.mark.parametrize("a", [1, 5, 8, 1001])
def test_two_calls_equal_one(ops, whole, a):
    n = whole["n"]
    pd, md, vd, gd = [whole[k].to(DEV) for k in ("p", "m", "v")] + [whole["g"][0].to(DEV)]
    flat_sr(ops, a, pd, gd, 0, md, vd, 0, whole["hd"][0], None, 42, 1, 0, 0)
    flat_sr(ops, n - a, pd[a:], gd[a:], 0, md[a:], vd[a:], 0, whole["hd"][0], None, 42, 1, 0, a)
    for x, y, nm in zip((pd, md, vd), whole["out"], "pmv"):
        same(x, y, f"{nm} cut at {a}")


class HostBuf:
    """Memory from az_host_alloc as a numpy byte array."""

    def __init__(self, nbytes):
        p = ctypes.c_void_p()
        call("az_host_alloc", ctypes.byref(p), nbytes)
        assert p.value
        self.ptr = p.value
        self.bytes = np.frombuffer((ctypes.c_uint8 * nbytes).from_address(p.value), dtype=np.uint8)

    def tensor(self, dtype):
        return torch.from_numpy(self.bytes).view(dtype)

    def free(self):
        self.bytes = None
        call("az_host_free", vp(self.ptr))


@pytest.mark.parametrize("mdtype,gdtype", [(0, 0), (1, 1), (2, 0)])
@pytest.mark.parametrize("chunk", [1001, 1024], ids=["chunk_not_multiple_of_8", "chunk_1024"])
def test_raven_step_sr_equals_flat_sr(ops, mdtype, gdtype, chunk):
    """Two az_raven_step_sr calls back to back, moments in az_host_alloc memory, five ragged chunks: p, m, v equal two az_adamw_flat_sr
    steps at the same elem0 (a chunk length that is no multiple of 8 sends the later chunks down the element-wise path: same bits)."""
    n, elem0 = 4 * chunk + 77, 8 * 5
    mdt = R.moment_dtype(mdtype)
    esz = 4 if mdtype == 1 else 2
    p0, grads, m0, v0, hyper = state(n, mdtype, gdtype == 1, seed=n)
    hd = hyper_dev(hyper)
    cd = torch.tensor([0.37], dtype=F32, device=DEV)
    gds = [torch.cat([x, torch.zeros(chunk, dtype=x.dtype)]).to(DEV) for x in grads]
    pf, mf, vf = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    for s in range(2):
        flat_sr(ops, n, pf, gds[s], gdtype, mf, vf, mdtype, hd[s], cd, SEED, s + 1, 2, elem0)
    sc, sh, sd = (torch.cuda.Stream(DEV) for _ in range(3))
    hm, hv = HostBuf((n + chunk) * esz), HostBuf((n + chunk) * esz)
    try:
        mh, vh = hm.tensor(mdt), hv.tensor(mdt)
        mh[:n], vh[:n], mh[n:], vh[n:] = m0, v0, SENT, SENT
        used = 2 * 2 * chunk * esz
        staging = torch.full((used + 1024,), 0xA5, dtype=torch.uint8, device=DEV)
        pbuf = torch.full((n + chunk,), SENT, dtype=BF16, device=DEV)
        pr = pbuf[:n]
        pr.copy_(p0)
        torch.cuda.synchronize()
        for s in range(2):
            call("az_raven_step_sr", n, ops._ptr(pr), ops._ptr(gds[s]), gdtype, vp(hm.ptr), vp(hv.ptr), mdtype, ops._ptr(hd[s]), ops._ptr(cd),
                 ops._ptr(staging), chunk, vp(sc.cuda_stream), vp(sh.cuda_stream), vp(sd.cuda_stream), SEED, s + 1, 2, elem0)
        sc.synchronize()
        torch.cuda.synchronize()
        same(pr, pf, "p")
        same(mh[:n].clone(), mf, "m"); same(vh[:n].clone(), vf, "v")
        assert bool((mh[n:] == SENT).all()) and bool((vh[n:] == SENT).all()), "host moments beyond n written"
        assert bool((pbuf[n:] == SENT).all()), "parameters beyond n written"
        assert bool((staging[used:] == 0xA5).all()), "staging beyond 2 x 2 x chunk elements written"
        p_ref, m_ref, v_ref = p0, m0, v0
        for s in range(2):
            p_ref, m_ref, v_ref = S.adamw_sr_bits(p_ref, grads[s], m_ref, v_ref, hyper[s], 0.37, SEED, s + 1, 2, elem0)
        same(pr, p_ref, "p against the reference")
    finally:
        mh = vh = None
        hm.free(); hv.free()


# ---------------- (c) seed, step, domain -------------------------------------------------------------------------------------------------
def test_seed_step_domain_select_the_bits(ops, whole):
    n = whole["n"]

    def run(seed, step, domain):
        pd, md, vd, gd = [whole[k].to(DEV) for k in ("p", "m", "v")] + [whole["g"][0].to(DEV)]
        flat_sr(ops, n, pd, gd, 0, md, vd, 0, whole["hd"][0], None, seed, step, domain, 0)
        same(md, whole["out"][1], "m"); same(vd, whole["out"][2], "v")          # the moments never depend on the random bits
        return pd
    base = whole["out"][0]
    same(run(42, 1, 0), base, "same seed and step")
    for seed, step, domain in ((43, 1, 0), (42 + (1 << 32), 1, 0), (42, 2, 0), (42, 1, 1)):
        got = run(seed, step, domain)
        frac = float((bits(got) != bits(base)).float().mean())
        assert 0.2 < frac < 0.8, (seed, step, domain, frac)                      # two independent draws differ on about half the elements
        same(got, S.adamw_sr_bits(whole["p"], whole["g"][0], whole["m"], whole["v"], whole["hyper"][0], None, seed, step, domain, 0)[0],
             f"seed {seed} step {step} domain {domain}")


# ---------------- (d) the drift experiment ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drift(ops):
    d = S.DRIFT
    hd = hyper_dev([S.drift_hyper(s) for s in range(1, d["steps"] + 1)])
    g = torch.full((d["n"],), d["g"], dtype=F32, device=DEV)
    return d, hd, g, S.drift_master()


def test_drift_round_to_nearest_never_moves(ops, drift):
    d, hd, g, master = drift
    n = d["n"]
    p = torch.full((n,), d["p0"], dtype=BF16, device=DEV)
    m, v = torch.zeros(n, dtype=F32, device=DEV), torch.zeros(n, dtype=F32, device=DEV)
    for s in range(d["steps"]):
        call("az_adamw_flat_ex", n, ops._ptr(p), ops._ptr(g), 1, ops._ptr(m), ops._ptr(v), 1, ops._ptr(hd[s]), vp(0), ops._stream())
    assert int((p.float() != d["p0"]).sum()) == 0
    assert abs((master - d["p0"]) / S.DRIFT_ULP - (-1.955)) < 0.002


@pytest.mark.parametrize("seed", S.DRIFT["seeds"])
def test_drift_stochastic_rounding_follows_the_master(ops, drift, seed):
    d, hd, g, master = drift
    n = d["n"]
    p = torch.full((n,), d["p0"], dtype=BF16, device=DEV)
    m, v = torch.zeros(n, dtype=F32, device=DEV), torch.zeros(n, dtype=F32, device=DEV)
    for s in range(d["steps"]):
        flat_sr(ops, n, p, g, 1, m, v, 1, hd[s], None, seed, s + 1, 0, 0)
    err = (float(p.double().mean()) - master) / S.DRIFT_ULP
    print(f"seed {seed}: mean(p_sr) - master = {err:+.4f} ulp (bound {S.DRIFT_BOUND_ULP:.4f})")
    assert abs(err) <= S.DRIFT_BOUND_ULP, err


# ---------------- (e) argument errors ----------------------------------------------------------------------------------------------------
def test_sr_entry_points_refuse_bad_arguments(ops):
    n = 8
    p, g, m = (torch.zeros(n, dtype=BF16, device=DEV) for _ in range(3))
    h = hyper_dev([R.adamw_hyper(step=1, **HYPER)])
    for nn, gdt, mdt, e0 in ((0, 0, 0, 0), (-3, 0, 0, 0), (n, 2, 0, 0), (n, -1, 0, 0), (n, 0, 3, 0), (n, 0, -1, 0), (n, 0, 0, -8)):
        refused("az_adamw_flat_sr", nn, ops._ptr(p), ops._ptr(g), gdt, ops._ptr(m), ops._ptr(m), mdt, ops._ptr(h), vp(0), 1, 1, 0, e0, ops._stream())
    st = torch.zeros(256, dtype=torch.uint8, device=DEV)
    s3 = [vp(torch.cuda.current_stream().cuda_stream)] * 3
    hb = HostBuf(64)
    try:
        for nn, gdt, mdt, chunk, e0 in ((0, 0, 0, 8, 0), (n, 0, 0, 0, 0), (n, 0, 0, -4, 0), (n, 0, 3, 8, 0), (n, 2, 0, 8, 0), (n, 0, 0, 8, -1)):
            refused("az_raven_step_sr", nn, ops._ptr(p), ops._ptr(g), gdt, vp(hb.ptr), vp(hb.ptr + 32), mdt, ops._ptr(h), vp(0), ops._ptr(st), chunk,
                    *s3, 1, 1, 0, e0)
    finally:
        hb.free()
    torch.cuda.synchronize()
    assert bool((p == 0).all()) and bool((m == 0).all())
