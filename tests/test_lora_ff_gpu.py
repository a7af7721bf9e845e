"""az_lora_up_geglu_bf16 (csrc/az_lora.hip): the up product of ff.net.0.proj with the GEGLU in its epilogue, by the method of
tests/test_lora_gpu.py.

Exact layer: operands are multiples of 2^-2 in [-4, 4], the previous proj lies in [-8, 8], s in {1, 1/2, 2}; every operand sits in a
larger allocation of the finite poison 3 * 2^40 (row strides above the widths, 8-byte column offsets).  proj must equal the one bf16
bit pattern of the exact result (tests/lora_ff_ref.py on tests/lora_ref.up), and out must equal, bit for bit, what az_geglu_fwd
writes on the GPU from that expected proj.  Every element is compared, every guard and every input is checked.  The table crosses
M in {1, 15, 16, 17, 63, 65, 154, 257} (one row, around a 16-row wave tile, around a 64-row block, several blocks), H in {8, 24, 64,
72, 136, 320} (below a 16-column tile, no multiple of it, exactly / past a wave's 64 columns, several column blocks), every rank the
entry takes in one and two k-steps, and the three exact scales; tests/test_lora_ff_ref_cpu.py checks the table without a GPU.

Gaussian layer (s = 1/3, M = 154, H = 320, r = 16): proj within 2^-8 |ref| + 2 n 2^-24 S with n = r + 2 (the bound test_gaussian_up
derives: r products, the scale, the previous contents), proj bit-equal to az_lora_up_bf16 on the same operands (same operand order,
k-step order and epilogue expression), and out bit for bit az_geglu_fwd of the kernel's own stored proj."""
import functools
import os
import sys
from collections import namedtuple

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gemm_ref as R        # noqa: E402
import lora_ff_ref as FR    # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# M, H (out width; proj and w have 2 H), r, s
UG = namedtuple("UG", "M H r s")
CASES = [UG(1, 8, 4, 1.0), UG(15, 24, 8, 0.5), UG(16, 64, 12, 2.0), UG(17, 72, 16, 1.0), UG(63, 136, 32, 0.5), UG(65, 320, 64, 2.0),
         UG(154, 72, 4, 1.0), UG(257, 64, 16, 0.5), UG(65, 24, 64, 1.0)]
GAUSS = UG(154, 320, 16, 1.0 / 3.0)


def cid(c):
    return "-".join(str(v) for v in c)


def seed_of(*v):
    s = 97531
    for x in v:
        s = (s * 1000003 + int(float(x) * 4) + 17) % 2147483647
    return s


@functools.lru_cache(maxsize=None)
def make(c, gaussian=False):
    seed = seed_of(*c)
    mk = (lambda shape, i, lim=4: R.gauss(shape, seed + i)) if gaussian else (lambda shape, i, lim=4: R.quarters(shape, seed + i, lim))
    u, w, y = mk((c.M, c.r), 1), mk((2 * c.H, c.r), 2), mk((c.M, 2 * c.H), 3, 8)
    ref, S, out_ref = FR.up_geglu(u, w, y, c.s, exact=not gaussian)
    return dict(u=u, w=w, y=y, ref=ref, S=S, out_ref=out_ref)


@pytest.fixture(scope="module")
def ops():
    from aozora_sdxl_training_amd import ops as _ops
    return _ops


class Dev:
    """An operand embedded in poison, on the device: row stride above the width, an 8-byte column offset."""

    def __init__(self, t):
        self.emb = R.embed(t, (t.shape[1] + 3) // 4 * 4 + 8, lead_rows=1, tail_rows=2, col_offset=4)
        self.buf = self.emb.buf.to(DEV)

    def view(self):
        return self.emb.view(self.buf)

    def guards_intact(self):
        return self.emb.guards_intact(self.buf)

    def unwritten(self):
        return torch.equal(R.bits(self.buf.cpu()), R.bits(self.emb.buf))


def run(ops, c, gaussian=False):
    d = make(c, gaussian)
    u, w, proj = Dev(d["u"]), Dev(d["w"]), Dev(d["y"])
    out = Dev(torch.full((c.M, c.H), R.POISON, dtype=torch.bfloat16))
    ops.lora_up_geglu(u.view(), w.view(), proj.view(), out.view(), scale=c.s)
    torch.cuda.synchronize()
    return d, u, w, proj, out


def geglu_of(ops, proj_bf16):
    """What az_geglu_fwd writes from a given stored proj (contiguous, 16-byte aligned rows)."""
    p = proj_bf16.detach().to(DEV).contiguous()
    o = torch.empty(p.shape[0], p.shape[1] // 2, dtype=torch.bfloat16, device=DEV)
    ops.geglu_fwd(p, o)
    torch.cuda.synchronize()
    return o.cpu()


def check_surroundings(name, u, w, proj, out):
    assert proj.guards_intact(), f"{name}: a sentinel around proj was overwritten"
    assert out.guards_intact(), f"{name}: a sentinel around out was overwritten"
    assert u.unwritten() and w.unwritten(), f"{name}: an input was written"


@pytest.mark.parametrize("c", CASES, ids=cid)
def test_up_geglu_exact(ops, c):
    d, u, w, proj, out = run(ops, c)
    name = f"lora_up_geglu {c}"
    want = R.expected_bits(d["ref"])
    bad = R.first_mismatch(proj.view(), want)
    assert bad is None, f"{name} proj: {bad}"
    bad = R.first_mismatch(out.view(), geglu_of(ops, want))
    assert bad is None, f"{name} out: {bad}"
    check_surroundings(name, u, w, proj, out)


def test_up_geglu_gaussian(ops):
    c = GAUSS
    d, u, w, proj, out = run(ops, c, gaussian=True)
    got, ref, S = proj.view().cpu().double().reshape(-1), d["ref"].reshape(-1), d["S"].reshape(-1)
    n = c.r + 2
    assert torch.isfinite(got).all()
    x = R.excess(got, ref, S, n)
    print(f"lora_up_geglu proj: excess {x:.4f} x n 2^-24 S (n = {n})")
    bad = (got - ref).abs() > R.gauss_bound(ref, S, n)
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} outside 2^-8 |ref| + 2 n 2^-24 S; needed {x:.2f} (allowed 2)"
    # the same operands through az_lora_up_bf16: the same bits
    y2 = Dev(d["y"])
    ops.lora_up(u.view(), w.view(), y2.view(), parts=1, scale=c.s)
    torch.cuda.synchronize()
    bad = R.first_mismatch(proj.view(), y2.view())
    assert bad is None, f"proj differs from az_lora_up_bf16: {bad}"
    # out is az_geglu_fwd of the proj the kernel itself stored
    bad = R.first_mismatch(out.view(), geglu_of(ops, proj.view()))
    assert bad is None, f"out differs from az_geglu_fwd of the stored proj: {bad}"
    # ... which approximates the float64 GEGLU of that proj: bf16 rounding + the 4.3e-7 absolute error of gelu_erf (az_common.h) times |value|
    a = proj.view().cpu().double()
    o64 = FR.geglu(a)
    lim = 2.0 ** -8 * o64.abs() + 2.0 * 4.3e-7 * a[:, :c.H].abs() + 1e-30
    assert bool(((out.view().cpu().double() - o64).abs() <= lim).all())
    check_surroundings("gaussian", u, w, proj, out)


def test_refusals(ops):
    from aozora_sdxl_training_amd._lib import AozoraError
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(AozoraError):
        ops.lora_up_geglu(z(16, 8), z(24, 8), z(16, 24), z(16, 12))               # H % 8
    with pytest.raises(AozoraError):
        ops.lora_up_geglu(z(16, 6), z(32, 6), z(16, 32), z(16, 16))               # rank % 4
    with pytest.raises(AozoraError):
        ops.lora_up_geglu(z(16, 68), z(32, 68), z(16, 32), z(16, 16))             # rank above 64
    with pytest.raises(AozoraError):
        ops.lora_up_geglu(z(16, 8), z(32, 8), z(16, 32), z(16, 24))               # out is not half of proj
    with pytest.raises(AozoraError):
        ops.lora_up_geglu(z(16, 8), z(32, 8), z(17, 32), z(16, 16))               # row counts differ
    proj = z(16, 32)
    with pytest.raises(AozoraError):
        ops.lora_up_geglu(z(16, 8), z(32, 8), proj, proj[:, :16])                 # out overlaps proj
    with pytest.raises(AozoraError):
        ops.lora_up_geglu(proj[:, 16:24], z(32, 8), proj, z(16, 16))              # u overlaps proj
