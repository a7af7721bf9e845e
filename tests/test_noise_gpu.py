"""The NOISE_MODE kernels alone (az_noise_shape, az_noise_target_ex; csrc/az_elem.hip) against tests/noise_ref.py: bit for bit against
its fp32 restatement -- u, the partial sums, the noisy NHWC rows with their zero padding channels, the target -- and within
elem_ref.bound of its float64 reference, with K the count of fp32 roundings on the kernel's longest path (noise_ref's docstring and
the kernels' comments: 8 + levels for the shaping, never above 4 + 12 levels; A + 9 for mix and target, A the addition chain of the
partial geometry; (A + 4) 2^-24 relative on r_b).  Shapes: one block and several, sizes that are no multiple of anything, fields that
collapse to 1 x 1 (8 levels on 4 x 4 and 5 x 7), and 90 x 180 where the blocks per sample reach their cap of 64."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import elem_ref as R        # noqa: E402
import noise_ref as N       # noqa: E402
from aozora_sdxl_training_amd import noise as nz      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -1232.0
TAIL = 1024
BF16, F32 = torch.bfloat16, torch.float32
U = 2.0 ** -24
OFFSET, DISCOUNT, PERTURB = 0.05, 0.6, 0.1


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd import ops as _ops
    return _ops


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b, what):
    a, b = a.cpu(), b.cpu()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, tuple(a.shape), tuple(b.shape), a.dtype, b.dtype)
    eq = bits(a) == bits(b)
    if not bool(eq.all()):
        i = int((~eq).reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int((~eq).sum())} of {eq.numel()} elements differ; first at flat {i}: "
                             f"{float(a.reshape(-1)[i])!r} vs {float(b.reshape(-1)[i])!r}")


def within(out, ref, S, k, what, rounding=None):
    out, ref, S = out.cpu().double(), torch.as_tensor(ref), torch.as_tensor(S)
    assert out.shape == ref.shape, (what, tuple(out.shape), tuple(ref.shape))
    assert bool(torch.isfinite(out).all()), f"{what}: non-finite output"
    rounding = R.f32_rounding(ref) if rounding is None else rounding
    need = R.excess(out, ref, S, rounding)
    print(f"{what}: K needed {need:.2f} of {R.K[k]:g}")
    assert bool(((out - ref).abs() <= R.bound(ref, S, k, rounding)).all()), f"{what}: K needed {need:.1f} > {R.K[k]}"


def tailed(n, dtype, fill=None):
    buf = torch.full((n + TAIL,), SENT, dtype=dtype, device=DEV)
    if fill is not None:
        buf[:n] = fill.reshape(-1).to(DEV)
    return buf, buf[:n]


def tail_ok(buf, n, what):
    assert bool((buf[n:] == SENT).all()), f"{what}: written past its end"


class Run:
    """One case on the device: shaping (if the features ask for it) and the three modes' mix and target."""

    def __init__(self, ops, shape, levels, offset, pyramid, perturb, seed, draws=None):
        B, C, H, W = shape
        HW = H * W
        self.shape, self.levels = shape, levels
        eps, o, zs, xi, lat = draws if draws is not None else N.draws(shape, levels, seed)
        self.eps, self.o, self.zs, self.xi, self.lat = eps, (o if offset else None), (zs if pyramid else []), (xi if perturb else None), lat
        spec = nz.NoiseSpec("pyramid" if pyramid else "offset", OFFSET if offset else 0.0, levels if pyramid else 0, DISCOUNT, PERTURB if perturb else 0.0)
        self.rows, total = nz.level_table(B, C, H, W, spec)
        self.weights = [r.weight for r in self.rows]
        assert self.weights == N.weights_of(DISCOUNT, len(self.rows))
        self.ub, self.u = tailed(B * C * HW, F32, eps)
        self.pb = self.part = None
        nblk = ops.noise_partial_blocks(HW)
        assert nblk == N.nblk_of(HW)
        if spec.needs_shape:
            fb = fields = table = None
            if pyramid:
                packed = nz.NoiseAux(None, zs, None).packed()
                assert packed.numel() == total
                fb, fields = tailed(total, F32, packed)
                table = nz.table_tensor(self.rows).to(DEV)
                self.pb, self.part = tailed(B * nblk * 2, F32)
            ops.noise_shape(self.u.view(B, C, H, W), self.o.to(DEV) if offset else None, spec.offset, fields, table, self.rows,
                            self.part.view(B, nblk, 2) if pyramid else None)
            if fb is not None:
                same(fields, packed, "level fields (read only)"); tail_ok(fb, total, "level fields")
        self.out = {}
        xid = self.xi.to(DEV) if perturb else None
        for mode in (0, 1, 2):
            ca, cb = N.coefs(B, mode, HW)
            nb, noisy = tailed(B * HW * 8, BF16)
            tb, tg = tailed(B * C * HW, F32)
            ops.noise_target_ex(mode, lat.to(DEV), self.u.view(B, C, H, W), ca.to(DEV), cb.to(DEV),
                                self.part.view(B, nblk, 2) if pyramid else None, xid, PERTURB, noisy.view(B, H, W, 8), tg.view(B, C, H, W))
            self.out[mode] = (nb, noisy, tb, tg, ca, cb)
        torch.cuda.synchronize()

    def check(self):
        B, C, H, W = self.shape
        HW = H * W
        nblk = N.nblk_of(HW)
        zz = [z.numpy() for z in self.zs]
        want_u = N.shape_bits(self.eps.numpy(), None if self.o is None else self.o.numpy(), OFFSET, zz, self.weights)
        same(self.u.view(B, C, H, W), torch.from_numpy(want_u), "u")
        tail_ok(self.ub, B * C * HW, "u")
        kk = len(zz)
        assert 8 + kk <= 4 + 12 * kk or kk == 0
        u64, S = N.shape64(self.eps.numpy(), None if self.o is None else self.o.numpy(), OFFSET, zz, DISCOUNT)
        within(self.u.view(B, C, H, W), u64, S, N.k_shape(kk), "u against float64")
        want_part = None
        u_cpu = self.u.cpu()
        if self.part is not None:
            want_part = N.partials_bits(want_u)
            same(self.part.view(B, nblk, 2), torch.from_numpy(want_part), "partial sums")
            tail_ok(self.pb, B * nblk * 2, "partial sums")
            p64, S64 = N.partials64(u_cpu.view(B, C, H, W).numpy())
            within(self.part.view(B, nblk, 2), p64, S64, N.k_partial(C, HW), "partial sums against float64")
            r = N.rb_bits(self.part.view(B, nblk, 2).cpu().numpy(), C, HW).astype(np.float64)
            r64 = 1.0 / N.std64(u_cpu.view(B, -1).numpy().reshape(B, C, H, W))
            allowed = (N.rb_chain(C, HW) + 4) * U
            print(f"r_b: relative error {np.abs(r / r64 - 1).max() / U:.2f} x 2^-24 of {allowed / U:g}")
            assert np.all(np.abs(r - r64) <= allowed * r64)
        lat3, u3 = self.lat.view(B, C, HW), u_cpu.view(B, C, HW)
        xi3 = None if self.xi is None else self.xi.view(B, C, HW)
        for mode, (nb, noisy, tb, tg, ca, cb) in self.out.items():
            wn, wt = N.target_ex_bits(mode, lat3, u3, ca, cb, 8, want_part, xi3, PERTURB)
            same(noisy.view(B, HW, 8), wn, f"noisy rows mode {mode}")
            assert bool((bits(noisy.view(B, HW, 8)[..., C:]) == 0).all()), "padding channels of the noisy rows are not +0"
            same(tg.view(B, C, HW), wt, f"target mode {mode}")
            tail_ok(nb, B * HW * 8, "noisy rows"); tail_ok(tb, B * C * HW, "target")
            ref = N.target_ex64(mode, lat3, u3, ca, cb, want_part is not None, xi3, PERTURB)
            k = N.k_target(C, HW, want_part is not None)
            within(noisy.view(B, HW, 8)[..., :C].float(), ref["noisy"], ref["S_noisy"], k, f"noisy rows mode {mode} against float64",
                   rounding=R.half_ulp_bf16(ref["noisy"]))
            within(tg.view(B, C, HW), ref["target"], ref["S_target"], k, f"target mode {mode} against float64")


FEATURES = {"offset": (True, False, False), "pyramid": (False, True, False), "perturb": (False, False, True), "all": (True, True, True)}


# each feature alone and all together; offset and perturb have no level fields, so one run per shape covers them
PARAMS = [(s, l, f) for f in FEATURES for s, l in N.CASES if f in ("pyramid", "all") or (l == 1)]


@pytest.mark.parametrize("shape,levels,feature", PARAMS)
def test_kernels_bit_for_bit_and_within_the_float64_bound(ops, shape, levels, feature):
    Run(ops, shape, levels, *FEATURES[feature], seed=31 * shape[2] * shape[3] + levels).check()


@pytest.mark.parametrize("shape", [(2, 4, 5, 7), (1, 4, 90, 180)])
def test_null_extras_equal_noise_target_bit_for_bit(ops, shape):
    B, C, H, W = shape
    eps, _, _, _, lat = N.draws(shape, 1, seed=5)
    for mode in (0, 1, 2):
        ca, cb = N.coefs(B, mode, H * W)
        outs = []
        for ex in (False, True):
            nb, noisy = tailed(B * H * W * 8, BF16)
            tb, tg = tailed(B * C * H * W, F32)
            if ex:
                ops.noise_target_ex(mode, lat.to(DEV), eps.to(DEV), ca.to(DEV), cb.to(DEV), None, None, 0.0, noisy.view(B, H, W, 8), tg.view(B, C, H, W))
            else:
                ops.noise_target(mode, lat.to(DEV), eps.to(DEV), ca.to(DEV), cb.to(DEV), noisy.view(B, H, W, 8), tg.view(B, C, H, W))
            tail_ok(nb, B * H * W * 8, "noisy rows"); tail_ok(tb, B * C * H * W, "target")
            outs.append((noisy, tg))
        same(outs[1][0], outs[0][0], f"noisy rows mode {mode}"); same(outs[1][1], outs[0][1], f"target mode {mode}")
        assert float(outs[0][1].abs().max()) > 0


def test_a_sample_of_a_batch_equals_the_sample_alone_and_two_runs_agree(ops):
    shape, levels = (3, 4, 9, 6), 3
    d = N.draws(shape, levels, seed=77)
    whole = Run(ops, shape, levels, True, True, True, 0, draws=d)
    again = Run(ops, shape, levels, True, True, True, 0, draws=d)
    same(again.u, whole.u, "u of a second run"); same(again.part, whole.part, "partial sums of a second run")
    for mode in (0, 1, 2):
        same(again.out[mode][1], whole.out[mode][1], "noisy rows of a second run"); same(again.out[mode][3], whole.out[mode][3], "target of a second run")
    B, C, H, W = shape
    HW, nblk = H * W, N.nblk_of(H * W)
    for b in range(B):
        eps, o, zs, xi, lat = d
        one = Run(ops, (1, C, H, W), levels, True, True, True, 0, draws=(eps[b:b + 1], o[b:b + 1], [z[b:b + 1] for z in zs], xi[b:b + 1], lat[b:b + 1]))
        same(one.u, whole.u.view(B, -1)[b], f"u of sample {b} alone")
        same(one.part, whole.part.view(B, -1)[b], f"partial sums of sample {b} alone")
        for mode in (0, 1, 2):
            ca, cb = N.coefs(B, mode, HW)
            ca1, cb1 = N.coefs(1, mode, HW)
            if not (torch.equal(ca[b:b + 1], ca1) and torch.equal(cb[b:b + 1], cb1)):      # the case's coefficients differ per batch size:
                nb, noisy = tailed(HW * 8, BF16)                                            # rerun the sample alone with the batch's own
                tb, tg = tailed(C * HW, F32)
                ops.noise_target_ex(mode, lat[b:b + 1].to(DEV), one.u.view(1, C, H, W), ca[b:b + 1].to(DEV), cb[b:b + 1].to(DEV), one.part.view(1, nblk, 2),
                                    xi[b:b + 1].to(DEV), PERTURB, noisy.view(1, H, W, 8), tg.view(1, C, H, W))
            else:
                noisy, tg = one.out[mode][1], one.out[mode][3]
            same(noisy, whole.out[mode][1].view(B, -1)[b], f"noisy rows of sample {b} alone, mode {mode}")
            same(tg, whole.out[mode][3].view(B, -1)[b], f"target of sample {b} alone, mode {mode}")


def test_a_nan_stays_in_its_sample(ops):
    shape, levels = (3, 4, 9, 6), 1
    eps, o, zs, xi, lat = N.draws(shape, levels, seed=13)
    clean = Run(ops, shape, levels, True, True, True, 0, draws=(eps, o, zs, xi, lat))
    bad = eps.clone()
    bad[1, 2, 4, 3] = float("nan")
    run = Run(ops, shape, levels, True, True, True, 0, draws=(bad, o, zs, xi, lat))
    B = shape[0]
    for mode in (0, 1, 2):
        tg, tg0 = run.out[mode][3].view(B, -1), clean.out[mode][3].view(B, -1)
        nx, nx0 = run.out[mode][1].view(B, -1, 8), clean.out[mode][1].view(B, -1, 8)
        for b in (0, 2):
            same(tg[b], tg0[b], f"target of sample {b}, mode {mode}"); same(nx[b], nx0[b], f"noisy rows of sample {b}, mode {mode}")
            assert bool(torch.isfinite(tg[b]).all())
        assert bool(tg[1].isnan().all()) and bool(nx[1][:, :4].float().isnan().all())      # its own std is NaN: the whole sample says so


def test_operand_refusals_raise_before_launching(ops):
    from aozora_sdxl_training_amd._lib import AozoraError
    B, C, H, W = 2, 4, 5, 7
    eps, o, zs, xi, lat = N.draws((B, C, H, W), 2, seed=3)
    spec = nz.NoiseSpec("pyramid", OFFSET, 2, DISCOUNT, PERTURB)
    rows, total = nz.level_table(B, C, H, W, spec)
    nblk = ops.noise_partial_blocks(H * W)
    ub, u = tailed(B * C * H * W, F32, eps)
    u4 = u.view(B, C, H, W)
    fields, table = nz.NoiseAux(None, zs, None).packed().to(DEV), nz.table_tensor(rows).to(DEV)
    part = torch.full((B, nblk, 2), SENT, dtype=F32, device=DEV)
    od = o.to(DEV)
    bad_rows = [rows[0], rows[1]._replace(offset=rows[1].offset + 1)]
    for args in ((u4.double(), od, OFFSET, fields, table, rows, part), (u4, od[:1], OFFSET, fields, table, rows, part),
                 (u4, od.double(), OFFSET, fields, table, rows, part), (u4, od, -1.0, fields, table, rows, part),
                 (u4, od, OFFSET, fields[:-1], table, rows, part), (u4, od, OFFSET, fields, table[:1], rows, part),
                 (u4, od, OFFSET, fields, table.float(), rows, part), (u4, od, OFFSET, fields, table, bad_rows, part),
                 (u4, od, OFFSET, None, None, rows, part), (u4, od, OFFSET, fields, table, [], part),
                 (u4, od, OFFSET, fields, table, rows, part[:, :, :1]), (u4, od, OFFSET, fields, table, rows, part.view(-1)),
                 (u4, od, OFFSET, fields, table, rows * 5, part), (u4.cpu(), od, OFFSET, fields, table, rows, part)):
        with pytest.raises(AozoraError):
            ops.noise_shape(*args)
    nb, noisy = tailed(B * H * W * 8, BF16)
    tb, tg = tailed(B * C * H * W, F32)
    ld, ca, cb, xd = lat.to(DEV), *[c.to(DEV) for c in N.coefs(B, 0, 1)], xi.to(DEV)
    n4, t4 = noisy.view(B, H, W, 8), tg.view(B, C, H, W)
    for args in ((0, ld, u4, ca, cb, part[:1], xd, PERTURB, n4, t4), (0, ld, u4, ca, cb, part.double(), xd, PERTURB, n4, t4),
                 (0, ld, u4, ca, cb, part, xd[:1], PERTURB, n4, t4), (0, ld, u4, ca, cb, part, xd.double(), PERTURB, n4, t4),
                 (0, ld, u4, ca, cb, part, xd, -0.5, n4, t4), (0, ld.float(), u4, ca, cb, part, xd, PERTURB, n4, t4),
                 (0, ld, u4, ca[:1], cb, part, xd, PERTURB, n4, t4), (0, ld, u4, ca, cb, part, xd, PERTURB, n4[..., :2], t4),
                 (0, ld, u4, ca, cb, part, xd, PERTURB, n4, t4[:1])):
        with pytest.raises(AozoraError):
            ops.noise_target_ex(*args)
    with pytest.raises(AozoraError):
        ops.noise_target_ex(3, ld, u4, ca, cb, None, None, 0.0, n4, t4)        # the library's own refusal: unknown mode
    torch.cuda.synchronize()
    same(u4, eps, "noise after refused calls"); tail_ok(ub, B * C * H * W, "noise")
    assert bool((part == SENT).all()) and bool((noisy == SENT).all()) and bool((tg == SENT).all())
    tail_ok(nb, B * H * W * 8, "noisy rows"); tail_ok(tb, B * C * H * W, "target")
