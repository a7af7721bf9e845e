"""The strip-staged 3x3 convolution weight gradient (csrc/az_gemm_strip.inc, option CONVWG_STRIP) against tests/gemm_ref.py.

Exactly summable inputs: the output with CONVWG_STRIP = 1 equals the output with 0 bit for bit, and both equal the float64
reference's bf16 bits, for forced split_k 1 and 3, accumulate on and off, with and without the fused bias / per-sample sums.  X and dY
sit inside larger poisoned allocations (lead and tail rows, a row stride of C + 64, a column offset), so a halo read across a row end,
a sample end or a buffer end multiplies the poison 3 * 2^40 into the result.  Gaussian inputs over K = 4096 pixels must stay within
the round-to-nearest worst case (excess <= 1.0 of gemm_ref's bound, which allows 2.0).  Shapes the strip form does not cover must give
the same bits with the option on and off."""
import contextlib
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gemm_ref as R        # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16

# (B, H, W, Cin, Cout)
STRIP_SHAPES = [
    (2, 8, 8, 32, 64),        # a k-tile is one whole sample; both sample borders
    (1, 16, 32, 64, 64),      # two rows per k-tile
    (1, 64, 64, 32, 64),      # one row per k-tile
    (1, 2, 128, 32, 64),      # half a row per k-tile; both vertical halos outside the image
    (1, 16, 16, 320, 320),    # the model's channel count: five row blocks, ten channel chunks
    (1, 16, 16, 64, 80),      # Cout not a multiple of the block
]
# (B, H, W, Cin, Cout, ks, stride, upsample): x is stored at H x W; with upsample the conv sees 2H x 2W
FALLBACK_CASES = [
    (1, 16, 16, 48, 64, 3, 1, False),      # Cin % 32 != 0
    (1, 12, 20, 32, 64, 3, 1, False),      # W neither divides 64 nor is a multiple of it
    (1, 16, 16, 32, 64, 3, 2, False),      # stride 2
    (1, 8, 8, 32, 64, 3, 1, True),         # fused nearest-2x upsample
    (1, 16, 16, 32, 64, 1, 1, False),      # 1x1
]
GAUSS_SHAPE = (1, 64, 64, 32, 64)          # K = 4096 pixels


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def option(name, value):
    from aozora_sdxl_training_amd._lib import get_option, set_option
    old = get_option(name)
    set_option(name, value)
    try:
        yield
    finally:
        set_option(name, old)


def ibits(t):
    return t.contiguous().view(torch.int16)


def dev_nhwc(t, lead, tail, off=8, pad=64):
    """(B, H, W, C) operand inside a poisoned [lead + pixels + tail][off + C + pad - off] allocation -> the NHWC device view."""
    B, H, W, C = t.shape
    e = R.embed(t.reshape(-1, C), C + pad, lead, tail, off)
    v = e.view(e.buf.to(DEV))
    ld = v.stride(0)
    return v.as_strided((B, H, W, C), (H * W * ld, W * ld, ld, 1))


class FlatOut:
    """A contiguous output with 64 sentinels in front and behind; prev = None fills it with the poison (accumulate off must overwrite)."""

    def __init__(self, shape, prev=None):
        n = 1
        for s in shape:
            n *= s
        self.shape, self.n = tuple(shape), n
        self.init = torch.full((n + 128,), R.POISON, dtype=BF16)
        if prev is not None:
            self.init[64:64 + n] = prev.reshape(-1)
        self.init = self.init.to(DEV)
        self.buf = self.init.clone()

    def reset(self):
        self.buf.copy_(self.init)
        return self

    def view(self):
        return self.buf[64:64 + self.n].view(self.shape)

    def check(self, want, name):
        full = self.init.clone()
        full[64:64 + self.n] = want.reshape(-1).to(DEV)
        if torch.equal(ibits(self.buf), ibits(full)):
            return
        msg = R.first_mismatch(self.view(), want.reshape(self.shape))
        raise AssertionError(f"{name}: {msg if msg is not None else 'a sentinel around the output was overwritten'}")


@functools.lru_cache(maxsize=None)
def make_case(B, H, W, Cin, Cout, ks=3, stride=1, ups=False, gaussian=False):
    """Inputs and float64 references of one weight gradient, computed once and left unchanged."""
    seed = 7 + 1000003 * (B * 131 + H * 17 + W) + 101 * Cin + Cout + 13 * ks + 5 * stride + int(ups)
    mk = (lambda shape, i, lim=4: R.gauss(shape, seed + i)) if gaussian else (lambda shape, i, lim=4: R.quarters(shape, seed + i, lim))
    Hc, Wc = (2 * H, 2 * W) if ups else (H, W)
    Ho, Wo = R.conv_out(Hc, ks, stride), R.conv_out(Wc, ks, stride)
    d = dict(Ho=Ho, Wo=Wo)
    d["x"], d["dy"] = mk((B, H, W, Cin), 1), mk((B, Ho, Wo, Cout), 2)
    d["prev"], d["bold"] = mk((Cout, ks, ks, Cin), 3, lim=8), mk(Cout, 4, lim=8)
    out_hw = (Hc, Wc) if ups else None
    ex = not gaussian
    d["dw"], d["dwS"] = R.conv_wgrad(d["dy"], d["x"], ks, stride, Cout, out_hw=out_hw, exact=ex)
    d["dw_acc"], d["dw_accS"] = R.conv_wgrad(d["dy"], d["x"], ks, stride, Cout, prev=d["prev"], out_hw=out_hw, exact=ex)
    d["seg"], _, d["bg"], _ = R.conv_sums(d["dy"], Cout, d["bold"], exact=ex)
    return d


@functools.lru_cache(maxsize=None)
def dev_case(key):
    d = make_case(*key)
    B, H, W = key[0], key[1], key[2]
    # lead / tail rows: more than one image row + 1, so that the halo rows above the first and below the last sample lie in the poison
    return dict(x=dev_nhwc(d["x"], W + 3, W + 5), dy=dev_nhwc(d["dy"], 2, 3))


def run_both(ops, key, name, splits=(1, 3)):
    """Every (split, accumulate, sums) combination with the option off and on: equal bits, equal to the reference's."""
    d, g = make_case(*key), dev_case(key)
    B, Cin, Cout = key[0], key[3], key[4]
    ks, stride, ups = (key[5], key[6], key[7]) if len(key) > 5 else (3, 1, False)
    with_seg = (d["Ho"] * d["Wo"]) % 64 == 0
    dw = {acc: FlatOut((Cout, ks, ks, Cin), prev=d["prev"] if acc else None) for acc in (False, True)}
    bg, seg = FlatOut((Cout,), prev=d["bold"]), FlatOut((B, Cout))
    want = {False: R.expected_bits(d["dw"]), True: R.expected_bits(d["dw_acc"])}
    for split in splits:
        for acc in (False, True):
            for sums in (False, True):
                got = {}
                for strip in (0, 1):
                    what = f"{name} split={split} accumulate={acc} sums={sums} CONVWG_STRIP={strip}"
                    o = dw[acc].reset(); bg.reset(); seg.reset()
                    kw = dict(bias_grad=bg.view(), seg_grad=seg.view().view(-1) if with_seg else None) if sums else {}
                    with option("CONVWG_STRIP", strip):
                        ops.conv_wgrad(g["dy"], g["x"], o.view(), stride=stride, cout_real=Cout, accumulate=acc, split_k=split, upsample=ups, **kw)
                    o.check(want[acc], what)
                    if sums:
                        bg.check(R.expected_bits(d["bg"]), what + " bias gradient")
                        if with_seg:
                            seg.check(R.expected_bits(d["seg"]), what + " per-sample sums")
                    got[strip] = o.buf.clone()
                assert torch.equal(ibits(got[0]), ibits(got[1])), f"{name} split={split} accumulate={acc} sums={sums}: the option changed the bits"


@pytest.mark.parametrize("shape", STRIP_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_strip_exact(ops, shape):
    run_both(ops, shape, f"strip wgrad {shape}")


@pytest.mark.parametrize("shape", STRIP_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_strip_auto_split(ops, shape):
    """split_k = 0: the heuristic's split count; two launches give equal bits (and, on exact inputs, the reference's)."""
    d, g = make_case(*shape), dev_case(shape)
    B, H, W, Cin, Cout = shape
    o = FlatOut((Cout, 3, 3, Cin), prev=d["prev"])
    runs = []
    with option("CONVWG_STRIP", 1):
        for _ in range(2):
            o.reset()
            ops.conv_wgrad(g["dy"], g["x"], o.view(), cout_real=Cout, accumulate=True, split_k=0)
            o.check(R.expected_bits(d["dw_acc"]), f"strip wgrad {shape} automatic split")
            runs.append(o.buf.clone())
    assert torch.equal(ibits(runs[0]), ibits(runs[1])), f"strip wgrad {shape}: two launches with the automatic split differ"


@pytest.mark.parametrize("case", FALLBACK_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_fallback_shapes(ops, case):
    run_both(ops, case, f"fall-back wgrad {case}")


def test_strip_gaussian(ops):
    """K = 4096 pixels of Gaussian inputs: within the round-to-nearest worst case of n fp32 additions (excess <= 1.0)."""
    B, H, W, Cin, Cout = GAUSS_SHAPE
    key = GAUSS_SHAPE + (3, 1, False, True)
    d, g = make_case(*key), dev_case(key)
    for strip in (0, 1):
        for split in (1, 3):
            dw = d["prev"].to(DEV).clone()
            with option("CONVWG_STRIP", strip):
                ops.conv_wgrad(g["dy"], g["x"], dw, cout_real=Cout, accumulate=True, split_k=split)
            got = dw.cpu().double().reshape(-1)
            assert torch.isfinite(got).all(), "non-finite output"
            n = B * H * W + 1 + split
            x = R.excess(got, d["dw_acc"].reshape(-1), d["dw_accS"].reshape(-1), n)
            print(f"gaussian strip wgrad CONVWG_STRIP={strip} split={split}: excess {x:.4f} x n 2^-24 S (n = {n})")
            assert x <= 1.0, f"CONVWG_STRIP={strip} split={split}: needed {x:.3f} n 2^-24 S, more than the round-to-nearest worst case"
