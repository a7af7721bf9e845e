"""az_ema_flat (csrc/az_optim.hip) against tests/ema_ref.py, bit for bit (NaN positions compared as positions): sizes around the
8-wide group and the block, every pairing of pointer offsets (scalar head, tail, co-aligned 16-byte body, the element-wise form
when p and e cannot be co-aligned), five successive updates, special values, guard elements, and the argument checks."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ema_ref as E        # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64                    # guard elements in front of and behind every buffer
P_SENT, E_SENT = 0xC49A, -1232.0          # bf16 bits of -1232.0, and the same value in fp32
STEPS = 5
SIZES = [1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 2 ** 22 + 3]
P_OFFS, E_OFFS = (0, 1, 3, 5), (0, 1, 2, 3)
OMD_BITS = [0x3f800000, 0x3f51745d, 0x3a83126f, 0x38d1b717]
# bf16 bit patterns: +-0, smallest / largest subnormal (both signs), +-3.0e38 (rounded to bf16), +-inf, NaN (quiet, signalling payload, negative)
P_SPECIAL = [0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x807F, 0x7F62, 0xFF62, 0x7F80, 0xFF80, 0x7FC0, 0x7FA5, 0xFFC1]
E_SPECIAL = [np.inf, -np.inf, np.nan, 3.0e38, -3.0e38, 0.0, -0.0, 1e-45, -1.1754942e-38]


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
        call("az_ema_flat", *args)


def omd_of(bits):
    return float(np.array([bits], dtype=np.uint32).view(np.float32)[0])


@functools.lru_cache(maxsize=None)
def inputs(n):
    """(e0 fp32, [p bf16 bits] * STEPS) for a range of n elements: normals, with the special values at spread-out positions (as many
    as fit), the specials of e away from those of the first p where n allows."""
    rng = np.random.default_rng(1000 + n)
    e0 = rng.standard_normal(n).astype(np.float32)
    ps = []
    for s in range(STEPS):
        p = (rng.standard_normal(n).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        for j, b in enumerate(P_SPECIAL):
            p[(j * 5 + s) % n if n < 128 else (j * 149 + 11 * s) % n] = b
        ps.append(p)
    for j, v in enumerate(E_SPECIAL):
        if n >= 128:
            e0[(j * 211 + 70) % n] = v
        elif n >= 16 and j < 3:
            e0[n - 1 - j] = v
    return e0, ps


def same_bits(got, want, what):
    g, w = got.view(np.uint32), want.view(np.uint32)
    ok = (g == w) | (np.isnan(got) & np.isnan(want))
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} elements differ; first at {i}: {got[i]!r} ({g[i]:#010x}) vs {want[i]!r} ({w[i]:#010x})")


@pytest.mark.parametrize("omd_bits", OMD_BITS)
@pytest.mark.parametrize("n", SIZES)
def test_ema_flat_bit_for_bit(ops, n, omd_bits):
    omd = omd_of(omd_bits)
    e0, ps = inputs(n)
    want = [e0]
    for s in range(STEPS):
        want.append(E.ema_update(want[-1], E.bf16_bits_to_f32(ps[s]), np.float32(omd)))
    assert np.isnan(want[-1]).any() or n < 16
    st = ops._stream()
    p_dev = [torch.from_numpy(p.view(np.int16)).to(DEV) for p in ps]
    e_dev = torch.from_numpy(e0).to(DEV)
    for po in P_OFFS:
        for eo in E_OFFS:
            pbuf = torch.full((PAD + po + n + PAD,), P_SENT - 65536, dtype=torch.int16, device=DEV)        # (allocations are 256-byte aligned)
            ebuf = torch.full((PAD + eo + n + PAD,), E_SENT, dtype=torch.float32, device=DEV)
            assert pbuf.data_ptr() % 256 == 0 and ebuf.data_ptr() % 256 == 0
            pv, ev = pbuf[PAD + po:PAD + po + n], ebuf[PAD + eo:PAD + eo + n]
            ev.copy_(e_dev)
            for s in range(STEPS):
                pv.copy_(p_dev[s])
                call("az_ema_flat", n, vp(pv.data_ptr()), vp(ev.data_ptr()), omd, st)
                if s in (0, STEPS - 1) or n <= 4096:
                    same_bits(ev.cpu().numpy(), want[s + 1], f"n={n} p+{po} e+{eo} omd={omd_bits:#x} update {s + 1}")
            pb, eb = pbuf.cpu().numpy().view(np.uint16), ebuf.cpu().numpy()
            assert (pb[:PAD + po] == P_SENT).all() and (pb[PAD + po + n:] == P_SENT).all(), "the guards of p changed"
            assert (pb[PAD + po:PAD + po + n] == ps[-1]).all(), "p is read only"
            assert (eb[:PAD + eo] == E_SENT).all() and (eb[PAD + eo + n:] == E_SENT).all(), f"n={n} p+{po} e+{eo}: wrote outside its {n} elements"


def test_ops_wrapper_runs_on_the_given_stream_and_checks_operands(ops):
    from aozora_sdxl_training_amd._lib import AozoraError
    n = 4099
    e0, ps = inputs(2049)
    p = torch.from_numpy(np.tile(ps[0], 3)[:n].view(np.int16)).to(DEV).view(torch.bfloat16)
    e = torch.from_numpy(np.tile(e0, 3)[:n].copy()).to(DEV)
    want = E.ema_update(e.cpu().numpy(), E.bf16_bits_to_f32(p.cpu().view(torch.int16).numpy().view(np.uint16)), np.float32(0.25))
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    ops.ema_flat(p, e, 0.25, side)
    side.synchronize()
    same_bits(e.cpu().numpy(), want, "ops.ema_flat on a side stream")
    ops.ema_flat(p[:0], e[:0], 0.25)                                   # empty: nothing happens
    for bad_p, bad_e in ((p.float(), e), (p, e.bfloat16()), (p[:-1], e), (p.cpu(), e), (p[::2], e[:p[::2].numel()])):
        with pytest.raises(AozoraError):
            ops.ema_flat(bad_p, bad_e, 0.25)


def test_empty_range_launches_nothing_and_bad_arguments_are_refused(ops):
    from aozora_sdxl_training_amd._lib import lib
    e = torch.full((64,), E_SENT, dtype=torch.float32, device=DEV)
    p = torch.zeros(64, dtype=torch.bfloat16, device=DEV)
    st = ops._stream()
    assert lib().raw("az_ema_flat")(ctypes.c_long(0), vp(p.data_ptr()), vp(e.data_ptr()), ctypes.c_float(1.0), st) == 0
    torch.cuda.synchronize()
    assert bool((e == E_SENT).all())
    refused(-1, vp(p.data_ptr()), vp(e.data_ptr()), 0.5, st)
    refused(8, vp(0), vp(e.data_ptr()), 0.5, st)
    refused(8, vp(p.data_ptr()), vp(0), 0.5, st)
    refused(0, vp(0), vp(e.data_ptr()), 0.5, st)                       # the checks come before the n == 0 return
    refused(8, vp(p.data_ptr() + 1), vp(e.data_ptr()), 0.5, st)        # p not 2-byte aligned
    refused(8, vp(p.data_ptr()), vp(e.data_ptr() + 2), 0.5, st)        # e not 4-byte aligned
    refused(8, vp(p.data_ptr()), vp(e.data_ptr() + 1), 0.5, st)
    torch.cuda.synchronize()
    assert bool((e == E_SENT).all())
