"""The three adapter kernels for 3x3 convolutions (csrc/az_lora.hip: az_lora_conv_down_bf16, az_lora_conv_dgrad_bf16,
az_lora_conv_wgrad_bf16) bit for bit on exactly summable inputs, and under the derived bound on Gaussian inputs, by the method of
tests/test_lora_gpu.py.

Inputs are multiples of 2^-2 in [-4, 4], previous contents lie in [-8, 8], s is one of {1, 1/2, 2} (dealt over the cases);
tests/lora_conv_ref.py restates the products in float64 and tests/lora_ref.exact_ok_scaled asserts that every partial sum is exact, so
the expected output is one bf16 bit pattern per element and EVERY element is compared.  Activations sit in larger allocations (row
stride above the width, a poison row in front and two behind) whose other elements are the finite poison 3 * 2^40; the contiguous
weight operands sit in a poison row of their own.  A tap that leaves the image at its first or last row therefore reads poison if it
is loaded at all, and one that crosses into the next image of the batch reads that image's values (tests/test_lora_conv_ref_cpu.py
checks that this would change the result of every batch case).

The table crosses the geometries (a lone pixel with all eight neighbours outside, a single row, a single column, pixel counts around
a 16-row tile and a 64-row block, several blocks), Cin (below one 32-deep k-step, no multiple of it, past one round of the four
waves: 9 Cin = 72 .. 1224) and every allowed rank.

Gaussian layer: B = 2, 9x7, Cin = 136, r = 16, s = 1/3 and |out - ref| <= 2^-8 |ref| + 2 n 2^-24 S with n = the number of summed
products + 1 for the scale + 1 for the previous contents where there are any."""
import functools
import os
import sys
from collections import namedtuple

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gemm_ref as R             # noqa: E402
import lora_ref as LR            # noqa: E402
import lora_conv_ref as CR       # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEOMS = [(1, 1, 1), (1, 1, 9), (1, 7, 1), (2, 3, 5), (3, 4, 4), (2, 5, 13), (1, 8, 8), (2, 16, 9)]
CINS = [8, 24, 40, 64, 136]
Case = namedtuple("Case", "B H W Cin r s")
CASES = [Case(*g, cin, r, LR.EXACT_SCALES[(i + j + k) % 3]) for i, g in enumerate(GEOMS) for j, cin in enumerate(CINS) for k, r in enumerate(LR.RANKS)]
GAUSS = Case(2, 9, 7, 136, 16, 1.0 / 3.0)


def cid(c):
    return f"{c.B}x{c.H}x{c.W}-c{c.Cin}-r{c.r}-s{c.s:g}"


def seed_of(kind, c):
    s = 97531 + kind
    for v in (c.B, c.H, c.W, c.Cin, c.r):
        s = (s * 1000003 + v + 17) % 2147483647
    return s


def _mk(gaussian, seed):
    if gaussian:
        return lambda shape, i, lim=4: R.gauss(shape, seed + i)
    return lambda shape, i, lim=4: R.quarters(shape, seed + i, lim)


@functools.lru_cache(maxsize=None)
def make(kind, c, gaussian=False):
    """kind 0 down, 1 dgrad, 2 wgrad (accumulating on odd ranks' cases: r in (8, 32), and the Gaussian one) -> operands, ref, S."""
    mk = _mk(gaussian, seed_of(kind, c))
    geom, M = (c.B, c.H, c.W), c.B * c.H * c.W
    a = mk((c.r, 3, 3, c.Cin), 1)
    if kind == 0:
        x = mk((M, c.Cin), 2)
        ref, S = CR.down(x, a, geom, c.s, exact=not gaussian)
        return dict(x=x, a=a, ref=ref, S=S)
    if kind == 1:
        du, prev = mk((M, c.r), 2), mk((M, c.Cin), 3, 8)
        ref, S = CR.dgrad(du, a, prev, geom, c.s, exact=not gaussian)
        return dict(du=du, a=a, at=a.permute(3, 1, 2, 0).contiguous(), prev=prev, ref=ref, S=S)
    du, x, prev = mk((M, c.r), 2), mk((M, c.Cin), 3), mk((c.r, 3, 3, c.Cin), 4, 8)
    acc = gaussian or c.r in (8, 32)
    ref, S = CR.wgrad(du, x, prev if acc else None, geom, c.s, exact=not gaussian)
    return dict(du=du, x=x, prev=prev, acc=acc, ref=ref, S=S)


# ---------------- device side ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    from aozora_sdxl_training_amd import ops as _ops
    return _ops


class Dev:
    """A 2-D operand embedded in poison, on the device."""

    def __init__(self, t, ld, lead, tail, off):
        self.emb = R.embed(t, ld, lead_rows=lead, tail_rows=tail, col_offset=off)
        self.buf = self.emb.buf.to(DEV)

    def view(self):
        return self.emb.view(self.buf)

    def guards_intact(self):
        return self.emb.guards_intact(self.buf)


def wide(t):                 # 16-byte aligned rows: stride and offset multiples of 8 (x of the down product and of the weight gradient)
    return Dev(t, R.up8(t.shape[1]) + 16, 1, 2, 8)


def narrow(t):               # 8-byte aligned rows (u, du, dx)
    return Dev(t, (t.shape[1] + 3) // 4 * 4 + 8, 1, 2, 4)


class Flat(Dev):
    """A contiguous weight operand (4-D) as one row of a poison allocation: view() has its shape, 16-byte aligned."""

    def __init__(self, t):
        self.shape = tuple(t.shape)
        super().__init__(t.reshape(1, -1), t.numel() + 24, 1, 1, 8)

    def view(self):
        return super().view()[0].view(self.shape)


def check_exact(got, d, name, inputs):
    torch.cuda.synchronize()
    bad = R.first_mismatch(got.view().reshape(d["ref"].shape), R.expected_bits(d["ref"]))
    assert bad is None, f"{name}: {bad}"
    assert got.guards_intact(), f"{name}: a sentinel around the output was overwritten"
    for i in inputs:
        assert i.guards_intact(), f"{name}: an input was written"


def poison(*shape):
    return torch.full(shape, R.POISON, dtype=torch.bfloat16)


def run_down(ops, c, gaussian=False):
    d = make(0, c, gaussian)
    x, a, out = wide(d["x"]), Flat(d["a"]), narrow(poison(c.B * c.H * c.W, c.r))
    ops.lora_conv_down(x.view(), (c.B, c.H, c.W), a.view(), out.view(), scale=c.s)
    return d, out, (x, a)


def run_dgrad(ops, c, gaussian=False):
    d = make(1, c, gaussian)
    du, at, dx = narrow(d["du"]), Flat(d["at"]), narrow(d["prev"])
    ops.lora_conv_dgrad(du.view(), (c.B, c.H, c.W), at.view(), dx.view(), scale=c.s)
    return d, dx, (du, at)


def run_wgrad(ops, c, gaussian=False):
    d = make(2, c, gaussian)
    du, x = narrow(d["du"]), wide(d["x"])
    da = Flat(d["prev"] if d["acc"] else poison(*d["prev"].shape))
    ops.lora_conv_wgrad(du.view(), x.view(), (c.B, c.H, c.W), da.view(), scale=c.s, accumulate=d["acc"])
    return d, da, (du, x)


@pytest.mark.parametrize("c", CASES, ids=cid)
def test_down_exact(ops, c):
    d, out, inputs = run_down(ops, c)
    check_exact(out, d, f"lora_conv_down {c}", inputs)


@pytest.mark.parametrize("c", CASES, ids=cid)
def test_dgrad_exact(ops, c):
    d, dx, inputs = run_dgrad(ops, c)
    check_exact(dx, d, f"lora_conv_dgrad {c}", inputs)


@pytest.mark.parametrize("c", CASES, ids=cid)
def test_wgrad_exact(ops, c):
    d, da, inputs = run_wgrad(ops, c)
    check_exact(da, d, f"lora_conv_wgrad {c}", inputs)


@pytest.mark.parametrize("run", [run_down, run_dgrad, run_wgrad], ids=["down", "dgrad", "wgrad"])
def test_two_runs_give_equal_bits(ops, run):
    """No floating-point atomics, one fixed summation order: the same launch twice gives the same bits (Gaussian inputs)."""
    a = run(ops, GAUSS, gaussian=True)[1]
    b = run(ops, GAUSS, gaussian=True)[1]
    torch.cuda.synchronize()
    assert torch.equal(R.bits(a.buf.cpu()), R.bits(b.buf.cpu()))


def test_refusals(ops):
    from aozora_sdxl_training_amd._lib import AozoraError
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=DEV)
    g = (1, 4, 4)
    with pytest.raises(AozoraError):
        ops.lora_conv_down(z(16, 60), g, z(8, 3, 3, 60), z(16, 8))                   # Cin % 8
    with pytest.raises(AozoraError):
        ops.lora_conv_down(z(16, 64), g, z(6, 3, 3, 64), z(16, 6))                   # rank % 4
    with pytest.raises(AozoraError):
        ops.lora_conv_down(z(16, 64), g, z(68, 3, 3, 64), z(16, 68))                 # rank above 64
    with pytest.raises(AozoraError):
        ops.lora_conv_down(z(16, 64), (1, 4, 5), z(8, 3, 3, 64), z(16, 8))           # rows are not the pixels of the geometry
    with pytest.raises(AozoraError):
        ops.lora_conv_down(z(16, 64), g, z(8, 9, 64), z(16, 8))                      # weight layout
    with pytest.raises(AozoraError):
        ops.lora_conv_down(z(16, 72)[:, 4:68], g, z(8, 3, 3, 64), z(16, 8))          # x rows are not 16-byte aligned
    with pytest.raises(AozoraError):
        ops.lora_conv_dgrad(z(16, 8), g, z(64, 3, 3, 16), z(16, 64))                 # rank of the transposed copy
    with pytest.raises(AozoraError):
        ops.lora_conv_dgrad(z(16, 8), g, z(64, 3, 3, 8), z(17, 64))                  # row counts differ
    with pytest.raises(AozoraError):
        ops.lora_conv_dgrad(z(16, 2), g, z(64, 3, 3, 2), z(16, 64))                  # rank below 4
    both = z(16, 72)
    with pytest.raises(AozoraError):
        ops.lora_conv_dgrad(both[:, 64:], g, z(64, 3, 3, 8), both[:, :64])           # du inside dx's extent
    with pytest.raises(AozoraError):
        ops.lora_conv_wgrad(z(16, 8), z(16, 64), g, z(8, 3, 3, 72))                  # channel counts differ
    with pytest.raises(AozoraError):
        ops.lora_conv_wgrad(z(16, 8), z(16, 64), g, z(8, 3, 3, 64).permute(0, 3, 1, 2))   # the gradient must have the device layout
    with pytest.raises(AozoraError):
        ops.lora_conv_wgrad(z(16, 8), z(16, 64).float(), g, z(8, 3, 3, 64))          # dtype


def test_entry_points_return_the_argument_error_for_a_misaligned_pointer():
    """As az_lora_down_bf16 does: the C side checks alignment itself and launches nothing."""
    import ctypes
    from aozora_sdxl_training_amd._lib import lib
    x, a, u = (torch.zeros(n, dtype=torch.bfloat16, device=DEV) for n in (16 * 64 + 8, 8 * 9 * 64 + 8, 16 * 8 + 8))
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    fn, st = lib()._fn, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert fn["az_lora_conv_down_bf16"](1, 4, 4, 64, 8, 1.0, P(x, 2), 64, P(a), P(u), 8, st) == -1131
    assert fn["az_lora_conv_down_bf16"](1, 4, 4, 60, 8, 1.0, P(x), 64, P(a), P(u), 8, st) == -1130
    assert fn["az_lora_conv_dgrad_bf16"](1, 4, 4, 64, 8, 1.0, P(u, 2), 8, P(a), P(x), 64, st) == -1134
    assert fn["az_lora_conv_wgrad_bf16"](1, 4, 4, 64, 8, 1.0, P(u), 8, P(x, 8), 64, P(a), 1, P(x), 1 << 20, st) == -1137
    assert fn["az_lora_conv_wgrad_bf16"](1, 4, 4, 64, 8, 1.0, P(u), 8, P(x), 64, P(a), 1, P(x), 64, st) == -1139
    torch.cuda.synchronize()


# ---------------- Gaussian layer ------------------------------------------------------------------------------------------------------
def within(got, d, n, family):
    torch.cuda.synchronize()
    out, ref, S = got.view().detach().cpu().double().reshape(-1), d["ref"].reshape(-1), d["S"].reshape(-1)
    assert torch.isfinite(out).all(), family + ": non-finite output"
    x = R.excess(out, ref, S, n)
    print(f"{family}: excess {x:.4f} x n 2^-24 S (n = {n})" + (" -- above the round-to-nearest worst case" if x > 1.0 else ""))
    bad = (out - ref).abs() > R.gauss_bound(ref, S, n)
    assert not bool(bad.any()), f"{family}: {int(bad.sum())} of {bad.numel()} outside 2^-8 |ref| + 2 n 2^-24 S; needed {x:.2f} (allowed 2)"
    assert got.guards_intact(), family + ": a sentinel around the output was overwritten"


def test_gaussian_down(ops):
    c = GAUSS
    d, out, _ = run_down(ops, c, gaussian=True)
    within(out, d, 9 * c.Cin + 1, "lora_conv_down")


def test_gaussian_dgrad(ops):
    c = GAUSS
    d, dx, _ = run_dgrad(ops, c, gaussian=True)
    within(dx, d, 9 * c.r + 2, "lora_conv_dgrad")


def test_gaussian_wgrad(ops):
    c = GAUSS
    d, da, _ = run_wgrad(ops, c, gaussian=True)
    within(da, d, c.B * c.H * c.W + 2, "lora_conv_wgrad")
