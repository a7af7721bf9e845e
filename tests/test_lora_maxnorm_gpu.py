"""az_lora_max_norm_bf16 (csrc/az_lora.hip) against tests/lora_maxnorm_ref.py: ONE job table of six modules in one launch -- ranks 4
to 64, a 3x3 convolution's K = 72, out beyond one LDS stage, a fresh adapter with B = 0 -- in a flat buffer with 64 sentinel elements
around every slot.  Exactly summable inputs bit for bit (norm, q, every element); Gaussian inputs within the derived bound on q, the
reference's decision, every element exactly bf16_rn(fl32(x) q_got), untouched modules and sentinels bitwise unchanged; fp32 masters; a
NaN element; two launches alike; every refusal; one recorded call replayed through the native launch tape."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import elem_ref as R                # noqa: E402
import lora_maxnorm_ref as N        # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _bits(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


class Packed:
    """The modules of `mods` in one flat device buffer (lora_maxnorm_ref.layout), their job table, and fp32 masters for `masters`."""

    def __init__(self, mods, masters=(), master_noise=None):
        from aozora_sdxl_training_amd import lora_norm
        self.mods = mods
        self.offs, total = N.layout(mods)
        host = np.full(total, N.SENTINEL, dtype=np.uint16)
        for (A, B, _), (oa, ob) in zip(mods, self.offs):
            host[oa:oa + A.size] = N.to_bits(A).ravel()
            host[ob:ob + B.size] = N.to_bits(B).ravel()
        self.before = host.copy()
        self.buf = R.bits_to_bf16(host).to(DEV)
        # masters: float32(x) plus bits below the bf16 grid (the norm must still come from the bf16 values)
        self.mhost = np.full(total, 777.0, dtype=np.float32)
        for i in masters:
            for m, o in zip(mods[i][:2], self.offs[i]):
                w = np.asarray(m, np.float32).ravel().copy()
                if master_noise is not None:
                    w = (w * (1.0 + master_noise.uniform(-2.0 ** -10, 2.0 ** -10, w.size))).astype(np.float32)
                self.mhost[o:o + m.size] = w
        self.mbuf = torch.from_numpy(self.mhost.copy()).to(DEV)
        p0, m0 = self.buf.data_ptr(), self.mbuf.data_ptr()
        rows = []
        for i, ((A, B, s), (oa, ob)) in enumerate(zip(mods, self.offs)):
            hasm = i in masters
            rows.append([p0 + 2 * oa, p0 + 2 * ob, A.shape[0], A.shape[1], B.shape[0], lora_norm.s_bits(s), m0 + 4 * oa if hasm else 0, m0 + 4 * ob if hasm else 0])
            lora_norm.check_row(rows[-1])
        self.table = torch.tensor(rows, dtype=torch.int64, device=DEV)
        self.stats = torch.full((len(mods), 2), -5.0, dtype=torch.float32, device=DEV)

    def run(self, max_norm=N.MAX_NORM):
        from aozora_sdxl_training_amd import ops
        ops.lora_max_norm(self.table, max_norm, self.stats)
        torch.cuda.synchronize()
        return _bits(self.buf), self.stats.cpu().numpy(), self.mbuf.cpu().numpy()

    def check_untouched_outside(self, got, scaled):
        """Sentinels and every module not in `scaled` are bitwise the input."""
        mask = np.ones(got.size, dtype=bool)
        for i in scaled:
            for m, o in zip(self.mods[i][:2], self.offs[i]):
                mask[o:o + m.size] = False
        assert np.array_equal(got[mask], self.before[mask])
        assert (got[:64] == N.SENTINEL).all() and (got[-64:] == N.SENTINEL).all()


def test_exactly_summable_inputs_bit_for_bit():
    mods = N.exact_inputs()
    pk = Packed(mods)
    got, stats, _ = pk.run()
    scaled = []
    for i, ((A, B, s), (oa, ob)) in enumerate(zip(mods, pk.offs)):
        norm, q, over = N.rule32(N.n2_gram(A, B, s), N.MAX_NORM)
        print(i, A.shape, B.shape, "norm", stats[i, 0], "want", norm, "q", stats[i, 1], "want", q)
        assert stats[i, 0].tobytes() == np.float32(norm).tobytes() and stats[i, 1].tobytes() == np.float32(q).tobytes(), i
        if over:
            scaled.append(i)
            assert np.array_equal(got[oa:oa + A.size], N.scale_bits(pk.before[oa:oa + A.size], q)), i
            assert np.array_equal(got[ob:ob + B.size], N.scale_bits(pk.before[ob:ob + B.size], q)), i
    assert scaled == [0, 2, 4]
    pk.check_untouched_outside(got, scaled)          # the module exactly ON the limit and the B = 0 module among them


def test_gaussian_inputs_within_the_derived_bound():
    mods = N.gauss_inputs()
    pk = Packed(mods)
    got, stats, _ = pk.run()
    scaled = []
    for i, ((A, B, s), (oa, ob)) in enumerate(zip(mods, pk.offs)):
        n2 = N.n2_gram(A, B, s)
        norm, q, over = N.rule64(n2, N.MAX_NORM)
        nb = N.n2_bound(A, B, s)
        n_got, q_got = float(stats[i, 0]), float(stats[i, 1])
        print(i, A.shape, B.shape, "n2 error / bound", abs(n_got ** 2 - n2) / nb if nb else 0.0, "q error / bound",
              abs(q_got / q - 1.0) / N.q_bound(A, B, s) if n2 else 0.0)
        assert (q_got != 1.0) == over, i                                    # the reference's decision
        if n2 == 0.0:
            assert n_got == 0.0 and q_got == 1.0
            continue
        # norm_got = fl32(sqrt(n2_got)): n2's bound plus the rounding of the square root, on the square
        assert abs(n_got ** 2 - n2) <= nb + 2.5 * N.U * n2, i
        if over:
            scaled.append(i)
            assert abs(q_got / q - 1.0) <= N.q_bound(A, B, s), i
            assert np.array_equal(got[oa:oa + A.size], N.scale_bits(pk.before[oa:oa + A.size], stats[i, 1])), i
            assert np.array_equal(got[ob:ob + B.size], N.scale_bits(pk.before[ob:ob + B.size], stats[i, 1])), i
    assert scaled == [0, 2, 4]
    pk.check_untouched_outside(got, scaled)
    # two launches on the same input give identical bits
    pk2 = Packed(mods)
    got2, stats2, _ = pk2.run()
    assert np.array_equal(got, got2) and stats.tobytes() == stats2.tobytes()


def test_masters_are_scaled_and_the_parameter_is_their_rounding():
    """Modules 0 and 4 (above the limit) and 1 (below) carry a master that differs from float32(x) below the bf16 grid; module 2 (above)
    has none, in the same table."""
    mods = N.gauss_inputs()
    plain = Packed(mods)
    _, stats0, _ = plain.run()
    pk = Packed(mods, masters=(0, 1, 4), master_noise=np.random.default_rng(3))
    got, stats, mgot = pk.run()
    assert stats.tobytes() == stats0.tobytes()                          # the norm is taken from the bf16 values, not from the master
    for i in (0, 4):
        for m, o in zip(mods[i][:2], pk.offs[i]):
            wn, xb = N.scale_master(pk.mhost[o:o + m.size], stats[i, 1])
            assert mgot[o:o + m.size].tobytes() == wn.tobytes(), i
            assert np.array_equal(got[o:o + m.size], xb), i
    (oa, ob), (A, B, _) = pk.offs[2], mods[2]
    assert np.array_equal(got[oa:oa + A.size], N.scale_bits(pk.before[oa:oa + A.size], stats[2, 1]))
    assert np.array_equal(got[ob:ob + B.size], N.scale_bits(pk.before[ob:ob + B.size], stats[2, 1]))
    pk.check_untouched_outside(got, [0, 2, 4])
    mask = np.ones(mgot.size, dtype=bool)
    for i in (0, 4):
        for m, o in zip(mods[i][:2], pk.offs[i]):
            mask[o:o + m.size] = False
    assert mgot[mask].tobytes() == pk.mhost[mask].tobytes()             # module 1's master and the fill between the slots


def test_nan_element_leaves_the_module_untouched_and_reports_nan():
    mods = [(A.copy(), B.copy(), s) for A, B, s in N.gauss_inputs()]
    pk = Packed(mods)
    oa = pk.offs[2][0]
    host = pk.before.copy()
    host[oa + 17] = 0x7FC0
    pk.before = host
    pk.buf.copy_(R.bits_to_bf16(host).to(DEV))
    got, stats, _ = pk.run()
    assert np.isnan(stats[2, 0]) and stats[2, 1] == 1.0
    assert [bool(stats[i, 1] != 1.0) for i in range(6)] == [True, False, False, False, True, False]
    pk.check_untouched_outside(got, [0, 4])


def test_refusals_return_their_codes_and_launch_nothing():
    from aozora_sdxl_training_amd import ops
    from aozora_sdxl_training_amd._lib import lib, AozoraError
    fn = lib()._fn["az_lora_max_norm_bf16"]
    pk = Packed(N.gauss_inputs())
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = ctypes.c_float
    codes = [fn(None, 6, f(1.0), P(pk.stats), st), fn(P(pk.table, 4), 6, f(1.0), P(pk.stats), st),
             fn(P(pk.table), 0, f(1.0), P(pk.stats), st), fn(P(pk.table), -3, f(1.0), P(pk.stats), st), fn(P(pk.table), 65536, f(1.0), P(pk.stats), st),
             fn(P(pk.table), 6, f(0.0), P(pk.stats), st), fn(P(pk.table), 6, f(-1.0), P(pk.stats), st), fn(P(pk.table), 6, f(float("inf")), P(pk.stats), st),
             fn(P(pk.table), 6, f(float("nan")), P(pk.stats), st),
             fn(P(pk.table), 6, f(1.0), None, st), fn(P(pk.table), 6, f(1.0), P(pk.stats, 4), st)]
    torch.cuda.synchronize()
    assert codes == [-1150, -1150, -1151, -1151, -1151, -1152, -1152, -1152, -1152, -1153, -1153]
    for bad in (dict(table=pk.table.int()), dict(table=pk.table.cpu()), dict(table=pk.table[:, :7]), dict(table=pk.table.t()), dict(stats=pk.stats.double()),
                dict(stats=pk.stats[:5]), dict(stats=pk.stats.cpu()), dict(max_norm=0.0), dict(max_norm=float("nan")), dict(max_norm=float("inf")),
                dict(max_norm=True), dict(max_norm="1")):
        kw = dict(table=pk.table, max_norm=1.0, stats=pk.stats)
        kw.update(bad)
        with pytest.raises(AozoraError):
            ops.lora_max_norm(kw["table"], kw["max_norm"], kw["stats"])
    torch.cuda.synchronize()
    assert np.array_equal(_bits(pk.buf), pk.before) and bool((pk.stats == -5.0).all())


def test_malformed_rows_are_skipped_by_the_kernel():
    """A row the builder would have refused reaches the kernel: its workgroup touches nothing and reports (NaN, 1); the others run."""
    pk = Packed(N.gauss_inputs())
    tab = pk.table.cpu()
    tab[0, 2] = 12                  # a rank outside LORA_RANKS
    tab[2, 3] = 44                  # K % 8 != 0
    tab[4, 1] += 8                  # B not 16-byte aligned
    pk.table.copy_(tab)
    got, stats, _ = pk.run()
    for i in (0, 2, 4):
        assert np.isnan(stats[i, 0]) and stats[i, 1] == 1.0
    assert np.array_equal(got, pk.before)
    assert stats[1, 1] == 1.0 and stats[1, 0] > 0


def test_recorded_call_replays_through_the_native_tape():
    from aozora_sdxl_training_amd import ops
    from aozora_sdxl_training_amd._lib import lib
    from aozora_sdxl_training_amd.tape import NativeTape
    mods = N.gauss_inputs()
    want_bits, want_stats, _ = Packed(mods).run()
    pk = Packed(mods)
    src = pk.buf.clone()
    L = lib()
    L.recorder = []
    try:
        ops.lora_max_norm(pk.table, N.MAX_NORM, pk.stats)
        recorded = L.recorder
    finally:
        L.recorder = None
    assert [op.name for op in recorded] == ["az_lora_max_norm_bf16"]
    torch.cuda.synchronize()
    assert np.array_equal(_bits(pk.buf), want_bits)
    nt = NativeTape(recorded)
    assert nt.n_calls == 1 and not nt.callbacks
    pk.buf.copy_(src)
    pk.stats.fill_(-5.0)
    nt.play()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(pk.buf), want_bits) and pk.stats.cpu().numpy().tobytes() == want_stats.tobytes()
    nt.play()                       # on the scaled values: every module is now at or below the limit (up to the rounding of the elements)
    torch.cuda.synchronize()
    again = pk.stats.cpu().numpy()
    assert (again[:, 0] <= N.MAX_NORM * (1.0 + 2.0 ** -7)).all()
