"""ops.adamw_range against the direct C ABI call it stands for, on cloned inputs, bit for bit in p, m, v (and w); the direct calls are
pinned to the numpy restatements by test_elem_gpu.py, test_sr_gpu.py and test_master_gpu.py.  Ranges of 1, 7, 29 and 77 elements that
start 0 and 3 elements into 16-byte-aligned buffers: n = 1, 7 are all scalar; at start 0, n = 29 / 77 have 3 / 9 groups and a 5-element
tail; at start 3 a 5-element head, then 3 / 9 groups.  Plain (bf16 moments), stochastic rounding (fp32 moments) and master weights (fp16
moments), each with bf16 and fp32 gradients; the pinned-host pipeline in five chunks, the last ragged; the two refusals; n = 0."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import elem_ref as R        # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32, F16 = torch.bfloat16, torch.float32, torch.float16
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), wd=0.01, eps=1e-8, debias=0.3)
SIZES = (1, 7, 29, 77)
STARTS = (0, 3)
MOMENTS = {"plain": BF16, "sr": F32, "master": F16}      # one moment type per form, each type once
SEED, DOMAIN = 0x1234567890, 2


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


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b, what):
    """Bit equality; a NaN counts as equal to a NaN whatever its payload."""
    assert a.shape == b.shape and a.dtype == b.dtype, what
    eq = (bits(a) == bits(b)) | (a.isnan() & b.isnan())
    assert bool(eq.all()), f"{what}: {int((~eq).sum())} of {eq.numel()} elements differ"


def inputs(total, mdt, f32_grads, seed):
    """p, g, m, v, w of `total` elements on the device (256-byte-aligned allocations); the gradients hold a 0, a NaN and an inf."""
    g = R.gen(seed)
    w = 0.1 * torch.randn(total, generator=g)
    t = dict(p=w.bfloat16(), g=R.adamw_grads(total, seed + 1, f32_grads), m=(1e-3 * torch.randn(total, generator=g)).to(mdt),
             v=(1e-4 * torch.rand(total, generator=g)).to(mdt), w=w)
    t = {k: x.to(DEV) for k, x in t.items()}
    assert all(x.data_ptr() % 256 == 0 for x in t.values())
    return t


def clone(t):
    return {k: x.clone() for k, x in t.items()}


def hyper(step):
    return torch.from_numpy(R.adamw_hyper(step=step, **HYPER)).to(DEV)


def addr(t, key, start):
    return t[key].data_ptr() + start * t[key].element_size()


def direct(ops, form, n, t, start, gdtype, h, c, step=1, elem0=None):
    """The entry point of `form` itself, resident moments, on the current stream."""
    md = ops.MOMENT_CODE[t["m"].dtype]
    a = lambda k: vp(addr(t, k, start))
    if form == "master":
        call("az_adamw_flat_master", n, a("p"), a("w"), a("g"), gdtype, a("m"), a("v"), md, vp(h.data_ptr()), vp(c.data_ptr()), ops._stream())
    elif form == "sr":
        call("az_adamw_flat_sr", n, a("p"), a("g"), gdtype, a("m"), a("v"), md, vp(h.data_ptr()), vp(c.data_ptr()), SEED, step, DOMAIN,
             start if elem0 is None else elem0, ops._stream())
    else:
        call("az_adamw_flat_ex", n, a("p"), a("g"), gdtype, a("m"), a("v"), md, vp(h.data_ptr()), vp(c.data_ptr()), ops._stream())


def ranged(ops, form, n, t, start, gdtype, h, c, step=1, **kw):
    elem0 = kw.pop("elem0", start)
    if form == "master":
        kw["master"] = addr(t, "w", start)
    if form == "sr":
        kw["sr"] = (SEED, step, DOMAIN, elem0)
    ops.adamw_range(n, addr(t, "p", start), addr(t, "g", start), gdtype, addr(t, "m", start), addr(t, "v", start), t["m"].dtype, h.data_ptr(),
                    c.data_ptr(), torch.cuda.current_stream().cuda_stream, **kw)


def all_same(x, y, what):
    for k in "pgmvw":
        same(x[k], y[k], f"{k} {what}")


@pytest.mark.parametrize("gdtype", [0, 1])
@pytest.mark.parametrize("form", ["plain", "sr", "master"])
def test_range_equals_the_entry_point(ops, form, gdtype):
    c = torch.tensor([0.37], dtype=F32, device=DEV)
    h = hyper(1)
    for n in SIZES:
        for start in STARTS:
            x = inputs(start + n + 8, MOMENTS[form], gdtype == 1, seed=10 * n + start)
            y, before = clone(x), clone(x)
            ranged(ops, form, n, x, start, gdtype, h, c)
            direct(ops, form, n, y, start, gdtype, h, c)
            what = f"{form} gdtype={gdtype} n={n} start={start}"
            all_same(x, y, what)
            assert not torch.equal(bits(x["m"])[start:start + n], bits(before["m"])[start:start + n]), what + ": nothing was updated"
            for k in "pmvw":                                    # nothing outside the range
                same(x[k][:start], before[k][:start], f"{k} in front of the range, " + what)
                same(x[k][start + n:], before[k][start + n:], f"{k} behind the range, " + what)


@pytest.mark.parametrize("form", ["plain", "sr"])
def test_pinned_host_pipeline_equals_two_resident_calls(ops, form):
    """n = 77 in chunks of 16: five chunks, the last of 13; two updates back to back on the same three streams.  The range starts at
    global element 24 for the random bits: every chunk starts a group, as every resident group does."""
    n, chunk, gdtype = 77, 16, 1 if form == "sr" else 0
    mdt = MOMENTS[form]
    c = torch.tensor([0.37], dtype=F32, device=DEV)
    x = inputs(n, mdt, gdtype == 1, seed=5)
    y = clone(x)
    mh, vh = x["m"].cpu().pin_memory(), x["v"].cpu().pin_memory()
    staging = torch.empty(4 * chunk * mh.element_size(), dtype=torch.uint8, device=DEV)
    h2d, d2h = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    xs = dict(x, m=mh, v=vh)
    for step in (1, 2):
        ranged(ops, form, n, xs, 0, gdtype, hyper(step), c, step=step, elem0=24,
               host_pipeline=(staging.data_ptr(), chunk, h2d.cuda_stream, d2h.cuda_stream))
    for step in (1, 2):
        direct(ops, form, n, y, 0, gdtype, hyper(step), c, step=step, elem0=24)
    torch.cuda.synchronize()
    same(x["p"], y["p"], "p"); same(mh.to(DEV), y["m"], "m"); same(vh.to(DEV), y["v"], "v")


def test_master_combines_with_neither(ops):
    from aozora_sdxl_training_amd._lib import AozoraError
    n = 29
    x = inputs(n, BF16, False, seed=7)
    before = clone(x)
    h, c = hyper(1), torch.tensor([0.37], dtype=F32, device=DEV)
    staging = torch.empty(4 * 16 * 2, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    for kw in (dict(sr=(SEED, 1, DOMAIN, 0)), dict(host_pipeline=(staging.data_ptr(), 16, s, s))):
        with pytest.raises(AozoraError, match="master"):
            ranged(ops, "master", n, x, 0, 0, h, c, **kw)
    torch.cuda.synchronize()
    all_same(x, before, "after a refusal")


def test_empty_range(ops):
    """n = 0 as each entry point answers it: the master form launches nothing and succeeds, the others refuse (argument error)."""
    from aozora_sdxl_training_amd._lib import AozoraError
    x = inputs(8, BF16, False, seed=9)
    before = clone(x)
    h, c = hyper(1), torch.tensor([0.37], dtype=F32, device=DEV)
    staging = torch.empty(4 * 16 * 2, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    ranged(ops, "master", 0, x, 0, 0, h, c)
    for form, kw in (("plain", {}), ("sr", {}), ("plain", dict(host_pipeline=(staging.data_ptr(), 16, s, s))),
                     ("sr", dict(host_pipeline=(staging.data_ptr(), 16, s, s)))):
        with pytest.raises(AozoraError, match="argument error"):
            ranged(ops, form, 0, x, 0, 0, h, c, **kw)
    torch.cuda.synchronize()
    all_same(x, before, "after n = 0")
