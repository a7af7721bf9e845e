"""The four Prodigy entry points (csrc/az_prodigy.hip) against tests/prodigy_ref.py, in lock-step: after az_prodigy_begin and after
az_prodigy_finish the test reads `consts` and `dstate` back, checks every float32 constant against the restatement's own float64 value
(1 ulp) and feeds the DEVICE's float32 constants to the restatement, so that m, v, s, w and p can be compared bit for bit.  The two
sums are compared with math.fsum over the exact terms within the bound of float64 summation in any order, n 2^-53 sum|term|; the scalar
state machine is then followed from the device's own sums (re-added on the host in the kernel's fixed order) at 1e-12 relative --
loose against a dozen float64 operations and a pow (1e-14), tight against any float32 intermediate (6e-8)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"
F32_NAMES = ("c_m", "c_v", "c_s", "beta1", "beta2", "beta3", "dlr", "wd_dlr", "eps_d", "has_wd", "skip")
STATE = ("w", "p0", "m", "v", "s")
# element offsets from a 16-byte base of (the five fp32 state arrays, the gradient, the bf16 parameter)
ALIGNED = dict(state=0, g=0, p=0)
OFFSETS = [ALIGNED, dict(state=1, g=1, p=1), dict(state=3, g=3, p=3),                # co-aligned at elements 0, 7 and 5 (bf16 gradient)
           dict(state=1, g=3, p=3), dict(state=0, g=1, p=1),                         # bf16 operand that can never meet the fp32 ones
           dict(state=0, g=0, p=0, m=1)]                                              # fp32 arrays that can never meet each other


def vp(x):
    return ctypes.c_void_p(x)


def ptr(t):
    """Address of the first element of t (data_ptr() of an EMPTY tensor is null; the n == 0 calls need the real address)."""
    return t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size()


def offset_tensor(src, off):
    """A device copy of the 1-D CPU tensor src that starts `off` elements behind a 16-byte aligned address."""
    buf = torch.zeros(src.numel() + 8, dtype=src.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[off:off + src.numel()]
    out.copy_(src)
    return out


def finish_order_sum(pairs):
    """prodigy_finish_kernel's sum of the partial pairs, addition for addition: thread t adds pairs t, t + 256, ... in order, then a
    tree over the 256 threads."""
    out = []
    for col in (pairs[0::2], pairs[1::2]):
        a = np.zeros(256)
        for t in range(min(256, col.size)):
            acc = 0.0
            for x in col[t::256].tolist():
                acc += x
            a[t] = acc
        o = 128
        while o > 0:
            a[:o] = a[:o] + a[o:2 * o]
            o >>= 1
        out.append(float(a[0]))
    return tuple(out)


class Harness:
    """Device state of one optimizer over `sizes` ranges next to its restatement.  The state starts away from a fresh optimizer's
    (w != p0, non-zero moments) so that the FIRST step already has non-trivial sums."""

    def __init__(self, sizes, off=ALIGNED, gdtype=torch.bfloat16, seed=0, fresh=False, pull=False, **opts):
        import prodigy_ref as PR
        from aozora_sdxl_training_amd._lib import lib
        self.PR, self.L = PR, lib()
        self.sizes, self.off, self.gdtype = list(sizes), off, gdtype
        self.gen = torch.Generator().manual_seed(1000 + seed)
        self.pull = pull
        self.sign = [torch.where(torch.rand(n, generator=self.gen) < 0.5, -1.0, 1.0) for n in sizes]
        ps = [(0.02 * torch.randn(n, generator=self.gen)).bfloat16() for n in sizes]
        self.ref = PR.ProdigyRef(ps, **opts)
        if not fresh:
            for r, n in enumerate(sizes):
                rnd = lambda s: (s * torch.randn(n, generator=self.gen)).float().numpy()
                self.ref.w[r] = (self.ref.p0[r] + rnd(1e-3)).astype(np.float32)
                self.ref.m[r], self.ref.s[r], self.ref.v[r] = rnd(1e-5), rnd(1e-3), rnd(1e-5) ** 2
        self.dev = [{k: offset_tensor(torch.from_numpy(getattr(self.ref, k)[r].copy()), off.get(k, off["state"])) for k in STATE}
                    for r in range(len(sizes))]
        for r, n in enumerate(sizes):
            self.dev[r]["p"] = offset_tensor(torch.full((n,), 7.0).bfloat16(), off["p"])      # never read: any value will do
        d0 = self.ref.o["d0"]
        self.dstate = torch.tensor([d0, d0, 0.0, 0.0, 0.0, 0.0, d0, 0.0], dtype=torch.float64, device=DEV)
        self.consts = torch.zeros(16, dtype=torch.float64, device=DEV)
        self.npairs = [int(self.L._fn["az_prodigy_partials"](n)) for n in sizes]
        assert all(k >= (1 if n else 0) for k, n in zip(self.npairs, sizes))
        self.partials = torch.full((max(1, 2 * sum(self.npairs)),), float("nan"), dtype=torch.float64, device=DEV)
        self.hyper = (ctypes.c_double * 16)()
        self.st = vp(torch.cuda.current_stream().cuda_stream)

    def read_consts(self):
        raw = self.consts.cpu().numpy()
        return dict(zip(F32_NAMES, raw.view(np.float32)[:len(F32_NAMES)].tolist())), raw[8:].copy()

    def read_dstate(self):
        return dict(zip(self.PR.SCALARS, self.dstate.cpu().tolist()))

    def grads(self, scale=0.01, zero=False):
        """Gaussian gradients; pull: with a fixed sign per element, so that the parameters keep moving one way and d grows."""
        out = []
        for n, sg in zip(self.sizes, self.sign):
            g = torch.zeros(n) if zero else scale * torch.randn(n, generator=self.gen)
            out.append((sg * g.abs() if self.pull else g).to(self.gdtype))
        return out

    def launch(self, grads, lr, coef):
        """One step on the device alone (no checks): -> the device gradients (kept alive)."""
        o, h = self.ref.o, self.hyper
        h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7] = lr, o["beta1"], o["beta2"], o["beta3"], o["eps"], o["weight_decay"], o["d_coef"], o["growth_rate"]
        h[8], h[9] = float(o["use_bias_correction"]), float(o["safeguard_warmup"])
        gd = [offset_tensor(g, self.off["g"]) for g in grads]
        cf = torch.tensor([coef], dtype=torch.float32, device=DEV) if coef is not None else None
        self.begin()
        self.moments(gd, cf)
        self.finish()
        self.apply()
        return gd

    def begin(self):
        self.L.call("az_prodigy_begin", vp(self.dstate.data_ptr()), ctypes.cast(self.hyper, ctypes.c_void_p), vp(self.consts.data_ptr()), self.st)

    def moments(self, gd, cf):
        pair = 0
        for r, n in enumerate(self.sizes):
            d = self.dev[r]
            self.L.call("az_prodigy_moments", n, vp(ptr(d["w"])), vp(ptr(d["p0"])), vp(ptr(gd[r])), 0 if self.gdtype == torch.bfloat16 else 1,
                        vp(ptr(d["m"])), vp(ptr(d["v"])), vp(ptr(d["s"])), vp(self.consts.data_ptr()),
                        vp(cf.data_ptr() if cf is not None else 0), vp(self.partials.data_ptr() + 16 * pair), self.st)
            pair += self.npairs[r]

    def finish(self):
        self.L.call("az_prodigy_finish", sum(self.npairs), vp(self.partials.data_ptr()), vp(self.dstate.data_ptr()), vp(self.consts.data_ptr()), self.st)

    def apply(self):
        for r, n in enumerate(self.sizes):
            d = self.dev[r]
            self.L.call("az_prodigy_apply", n, vp(ptr(d["p"])), vp(ptr(d["w"])), vp(ptr(d["m"])), vp(ptr(d["v"])),
                        vp(self.consts.data_ptr()), self.st)

    def same_bits(self, names, what):
        for r in range(len(self.sizes)):
            for k in names:
                got, want = self.dev[r][k].cpu().numpy(), getattr(self.ref, k)[r]
                bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
                assert bad.size == 0, (what, k, r, self.sizes[r], bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())

    def step(self, lr=1.0, coef=None, zero=False):
        """One step in lock-step with the restatement, every check of the module's docstring.  -> whether parameters were updated."""
        ref, PR = self.ref, self.PR
        grads = self.grads(zero=zero)
        o, h = ref.o, self.hyper
        h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7] = lr, o["beta1"], o["beta2"], o["beta3"], o["eps"], o["weight_decay"], o["d_coef"], o["growth_rate"]
        h[8], h[9] = float(o["use_bias_correction"]), float(o["safeguard_warmup"])
        gd = [offset_tensor(g, self.off["g"]) for g in grads]
        cf = torch.tensor([coef], dtype=torch.float32, device=DEV) if coef is not None else None
        before = {"p": [d["p"].clone() for d in self.dev], "w": [d["w"].clone() for d in self.dev]}
        sc0 = dict(ref.sc)
        # begin
        self.begin()
        c32, _ = self.read_consts()
        carried, exact = ref.begin(lr)
        for k in PR.BEGIN_F32:
            assert abs(c32[k] - exact[k]) <= float(np.spacing(np.float32(abs(exact[k])))), ("begin", k, c32[k], exact[k])
        assert c32["skip"] == 1.0 and c32["has_wd"] == (1.0 if o["weight_decay"] != 0 else 0.0)
        # moments
        self.moments(gd, cf)
        fs = ref.moments(grads, c32, coef)
        self.same_bits(("m", "v", "s"), "moments")
        pairs = self.partials.cpu().numpy()[:2 * sum(self.npairs)]
        assert not np.isnan(pairs).any(), "every block writes its pair"
        for which in (0, 1):
            dev_sum = math.fsum(pairs[which::2].tolist())
            bound = ref.nterms * 2.0 ** -53 * ref.abs_sums[which]
            assert abs(dev_sum - fs[which]) <= bound, ("sum", which, dev_sum, fs[which], bound)
        dsum = finish_order_sum(pairs)
        # finish
        self.finish()
        ds = self.read_dstate()
        c32f, _ = self.read_consts()
        fin = ref.finish(carried, sums=dsum)
        assert ds["d_denom"] == dsum[1] and ds["d0"] == sc0["d0"]
        for which in (0, 1):
            assert abs(dsum[which] - fs[which]) <= ref.nterms * 2.0 ** -53 * ref.abs_sums[which]
        for k in ("d", "d_max", "d_numerator", "d_hat"):
            assert abs(ds[k] - ref.sc[k]) <= 1e-12 * abs(ref.sc[k]), (k, ds[k], ref.sc[k])
        assert ds["k"] == ref.sc["k"]
        if fin is None:
            assert c32f["skip"] == 1.0 and ds["k"] == sc0["k"] and ds["d"] == sc0["d"]
        else:
            assert c32f["skip"] == 0.0
            for k in PR.FINISH_F32:
                assert abs(c32f[k] - fin[k]) <= float(np.spacing(np.float32(abs(fin[k])))), ("finish", k, c32f[k], fin[k])
            ref.apply(c32f)
        # apply
        self.apply()
        torch.cuda.synchronize()
        self.same_bits(STATE, "apply")
        for r in range(len(self.sizes)):
            if fin is None:
                assert torch.equal(self.dev[r]["p"], before["p"][r]) and torch.equal(self.dev[r]["w"], before["w"][r])
            else:
                p, w = self.dev[r]["p"].cpu(), self.dev[r]["w"].cpu()
                assert torch.equal(p.view(torch.int16), w.bfloat16().view(torch.int16)), "p == bf16_rne(w)"
                assert torch.equal(p.view(torch.int16), ref.p[r].view(torch.int16))
        return fin is not None


@pytest.fixture(scope="module")
def built():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd._lib import lib
    return lib()


SMALL = [1, 7, 8, 9, 63, 64, 65, 255, 257, 4099]


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32], ids=["g_bf16", "g_fp32"])
@pytest.mark.parametrize("case", range(len(OFFSETS)))
def test_sizes_alignments_gradient_types_and_coefficient(built, case, gdtype):
    for i, n in enumerate(SMALL):
        for coef in (None, 0.37):
            h = Harness([n], OFFSETS[case], gdtype, seed=i, d0=1e-3, weight_decay=0.01 if i % 2 else 0.0)
            assert h.step(coef=coef)


@pytest.mark.parametrize("case", [0, 1, 3])
def test_a_million_elements_and_five(built, case):
    h = Harness([2 ** 20 + 5], OFFSETS[case], torch.bfloat16, seed=40 + case, d0=1e-3)
    assert h.npairs[0] == (2 ** 20 + 5 + 2047) // 2048
    assert h.step(coef=0.37)


def test_every_block_loops_twice_with_a_partial_last_pass(built):
    """Read off the launch geometry: a block covers 256 groups of 8 per pass and the grid is capped (az_prodigy_partials of a huge n);
    two full passes of the capped grid, half a third one, and a tail of 3 elements behind 37 more groups."""
    cap = int(built._fn["az_prodigy_partials"](2 ** 40))
    assert cap >= 8 and cap % 8 == 0
    n = 8 * (2 * cap * 256 + cap * 128 + 37) + 3
    h = Harness([n], ALIGNED, torch.bfloat16, seed=50, d0=1e-3, weight_decay=0.01)
    assert h.npairs[0] == cap
    assert h.step()


def test_three_ranges_with_a_middle_range_of_one_element(built):
    h = Harness([65, 1, 257], ALIGNED, torch.bfloat16, seed=60, d0=1e-3)
    assert sum(h.npairs) == 3
    for _ in range(3):
        assert h.step(coef=0.37)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("safeguard", [False, True])
@pytest.mark.parametrize("bias", [False, True])
def test_ten_consecutive_steps_from_a_fresh_state(built, bias, safeguard, wd):
    h = Harness([4099], ALIGNED, torch.bfloat16, seed=70, fresh=True, pull=True, use_bias_correction=bias, safeguard_warmup=safeguard, weight_decay=wd,
                growth_rate=3.0, d0=1e-5)
    for i in range(10):
        assert h.step(lr=0.5 + 0.05 * i)
    assert h.ref.sc["k"] == 10.0 and h.ref.sc["d"] >= h.ref.sc["d0"]
    # With gradients of a fixed sign the displacement after j steps is about j times the update, lr d bc (1 - b1^j) / sqrt(1 - b2^j) >= lr d
    # (>= 3 lr d without bias correction), and d_hat ~ (dlr / c_s') * update * (k - 1) / 2 with c_s' = dlr or d (safeguard): d must have left
    # d0 within 10 steps unless BOTH options shrink it (bias correction: dlr ~ 0.2 d this early; safeguard: the denominator ignores that).
    if not (bias and safeguard):
        assert h.ref.sc["d"] > h.ref.sc["d0"]


def test_a_step_whose_denominator_is_zero_ends_after_the_moments(built):
    h = Harness([257, 9], ALIGNED, torch.bfloat16, seed=80, d0=1e-3)
    for r in range(2):                               # s = 0 and zero gradients: every |s| term is 0, whatever m and v hold
        h.ref.s[r][:] = 0.0
        h.dev[r]["s"].zero_()
    assert h.step(zero=True) is False
    assert h.read_dstate()["k"] == 0.0
    assert h.step() is True                          # ... and the next step with gradients goes through


def test_n_zero_launches_nothing(built):
    h = Harness([0, 64, 0], ALIGNED, torch.bfloat16, seed=90, d0=1e-3)
    assert h.npairs == [0, 1, 0] and int(built._fn["az_prodigy_partials"](0)) == 0
    assert h.step()
    # all ranges empty: finish over no pairs is a step with d_denom == 0
    e = Harness([0], ALIGNED, torch.bfloat16, seed=91, d0=1e-3)
    assert e.step() is False and e.read_dstate()["k"] == 0.0


def test_argument_errors(built):
    from aozora_sdxl_training_amd._lib import AozoraError
    h = Harness([64], ALIGNED, torch.bfloat16, seed=95)
    d, L, st = h.dev[0], h.L, h.st
    g = torch.zeros(72, dtype=torch.bfloat16, device=DEV)
    P = lambda t, byte=0: vp(t.data_ptr() + byte)
    ok_m = [64, P(d["w"]), P(d["p0"]), P(g), 0, P(d["m"]), P(d["v"]), P(d["s"]), P(h.consts), vp(0), P(h.partials), st]
    ok_a = [64, P(d["p"]), P(d["w"]), P(d["m"]), P(d["v"]), P(h.consts), st]
    L.call("az_prodigy_moments", *ok_m)              # the unmodified calls are fine
    L.call("az_prodigy_apply", *ok_a)

    def bad(name, args, i, value):
        a = list(args)
        a[i] = value
        with pytest.raises(AozoraError, match="argument error"):
            L.call(name, *a)

    bad("az_prodigy_moments", ok_m, 0, -1)
    for i in (1, 2, 3, 5, 6, 7, 8, 10):
        bad("az_prodigy_moments", ok_m, i, vp(0))
    bad("az_prodigy_moments", ok_m, 4, 2)
    bad("az_prodigy_moments", ok_m, 4, -1)
    bad("az_prodigy_moments", ok_m, 1, P(d["w"], 2))         # fp32 not 4-byte aligned
    bad("az_prodigy_moments", ok_m, 3, P(g, 1))              # bf16 not 2-byte aligned
    bad("az_prodigy_moments", ok_m, 10, P(h.partials, 4))    # fp64 not 8-byte aligned
    ok_m32 = list(ok_m); ok_m32[4] = 1
    bad("az_prodigy_moments", ok_m32, 3, P(g, 2))            # an fp32 gradient not 4-byte aligned
    bad("az_prodigy_apply", ok_a, 0, -1)
    for i in (1, 2, 3, 4, 5):
        bad("az_prodigy_apply", ok_a, i, vp(0))
    bad("az_prodigy_apply", ok_a, 1, P(d["p"], 1))
    bad("az_prodigy_apply", ok_a, 2, P(d["w"], 2))
    ok_b = [P(h.dstate), ctypes.cast(h.hyper, ctypes.c_void_p), P(h.consts), st]
    for i in (0, 1, 2):
        bad("az_prodigy_begin", ok_b, i, vp(0))
    bad("az_prodigy_begin", ok_b, 0, P(h.dstate, 4))
    ok_f = [1, P(h.partials), P(h.dstate), P(h.consts), st]
    bad("az_prodigy_finish", ok_f, 0, -1)
    for i in (1, 2, 3):
        bad("az_prodigy_finish", ok_f, i, vp(0))
    assert int(L._fn["az_prodigy_partials"](-1)) < 0
    torch.cuda.synchronize()


def test_two_runs_from_the_same_state_are_identical_bit_for_bit(built):
    outs = []
    for _ in range(2):
        h = Harness([2 ** 18 + 3, 1, 4099], dict(state=1, g=1, p=1), torch.bfloat16, seed=99, d0=1e-3, weight_decay=0.01)
        for i in range(3):
            keep = h.launch(h.grads(), 1.0, 0.37)
        torch.cuda.synchronize()
        del keep
        outs.append(([h.dev[r][k].cpu() for r in range(3) for k in STATE + ("p",)], h.dstate.cpu(), h.consts.cpu(), h.partials.cpu()))
    for a, b in zip(outs[0][0], outs[1][0]):
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16), b.view(torch.int32 if b.dtype == torch.float32 else torch.int16))
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
