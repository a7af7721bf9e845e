"""az_dora_norm_bf16, az_dora_scale_bf16 and az_dora_bwd_bf16 (csrc/az_lora.hip) against tests/dora_ref.py.

Norm: ONE job table of six modules in one launch -- every rank, K below an MFMA step / no multiple of 32 / several chunks, N below a
row tile / no multiple of it / beyond one workgroup, a fresh adapter (B = 0) -- in a flat buffer with 64 sentinel elements around every
slot and around g and inv.  Exactly summable inputs bit for bit (g, inv, and with init the magnitudes); Gaussian inputs within the
derived bound; init = 0 leaves m alone; two launches alike; malformed rows; refusals.  Scale: every element bit for bit, with and
without bias and residual, row strides beyond N with sentinel columns.  Backward: dv bit for bit, dm bit for bit on exactly summable
inputs and within M 2^-24 inv sum |dy v| plus one bf16 rounding on Gaussian ones, accumulation, rows that are no multiple of the split.
One recorded call of each entry point replayed through the native launch tape."""
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
import dora_ref as D                # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GS = 7.5                            # sentinel of the fp32 vectors


def _bits(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


class Packed:
    """The modules of `mods` in one flat device buffer (dora_ref.layout), g and inv with 8 sentinel floats around every module, the table."""

    def __init__(self, mods, m_bits=None):
        from aozora_sdxl_training_amd import dora, lora_norm
        self.mods = mods
        self.offs, total = D.layout(mods)
        host = np.full(total, D.SENTINEL, dtype=np.uint16)
        for i, ((W, A, B, _), (ow, oa, ob, om)) in enumerate(zip(mods, self.offs)):
            host[ow:ow + W.size], host[oa:oa + A.size], host[ob:ob + B.size] = D.to_bits(W).ravel(), D.to_bits(A).ravel(), D.to_bits(B).ravel()
            host[om:om + W.shape[0]] = 0x3FC0 if m_bits is None else m_bits[i]
        self.before = host.copy()
        self.buf = R.bits_to_bf16(host).to(DEV)
        self.goff, off = [], 8
        for W, _, _, _ in mods:
            self.goff.append(off)
            off += W.shape[0] + 8
        self.g = torch.full((off,), GS, dtype=torch.float32, device=DEV)
        self.inv = torch.full((off,), GS, dtype=torch.float32, device=DEV)
        p0, rows, tiles = self.buf.data_ptr(), [], 0
        for (W, A, B, s), (ow, oa, ob, om), go in zip(mods, self.offs, self.goff):
            N, K = W.shape
            rows.append([p0 + 2 * ow, p0 + 2 * oa, p0 + 2 * ob, p0 + 2 * om, self.g.data_ptr() + 4 * go, self.inv.data_ptr() + 4 * go,
                         A.shape[0], K, N, lora_norm.s_bits(s), tiles, 0])
            dora.check_row(rows[-1])
            tiles += (N + dora.TILE_ROWS - 1) // dora.TILE_ROWS
        self.tiles = tiles
        self.table = torch.tensor(rows, dtype=torch.int64, device=DEV)

    def run(self, init):
        from aozora_sdxl_training_amd import ops
        ops.dora_norm(self.table, self.tiles, init)
        torch.cuda.synchronize()
        return _bits(self.buf), self.g.cpu().numpy(), self.inv.cpu().numpy()

    def check_outside(self, got, g, inv, m_written):
        """Everything but the magnitudes of `m_written` is bitwise the input; the sentinels of g and inv stand."""
        mask = np.ones(got.size, dtype=bool)
        for i in m_written:
            mask[self.offs[i][3]:self.offs[i][3] + self.mods[i][0].shape[0]] = False
        assert np.array_equal(got[mask], self.before[mask])
        gm = np.ones(g.size, dtype=bool)
        for (W, _, _, _), go in zip(self.mods, self.goff):
            gm[go:go + W.shape[0]] = False
        assert (g[gm] == GS).all() and (inv[gm] == GS).all()


def test_norm_exactly_summable_inputs_bit_for_bit():
    mods = D.exact_inputs()
    pk = Packed(mods)
    got, g, inv = pk.run(init=True)
    for i, ((W, A, B, s), offs, go) in enumerate(zip(mods, pk.offs, pk.goff)):
        N = W.shape[0]
        inv_w, g_w, m_w = D.gains32(D.n2_64(W, A, B, s))          # n2 is exact in fp32
        assert inv[go:go + N].tobytes() == inv_w.tobytes(), i
        assert g[go:go + N].tobytes() == g_w.tobytes(), i
        assert np.array_equal(got[offs[3]:offs[3] + N], m_w), i
        assert np.abs(g_w - 1.0).max() <= 2.0 ** -8 + 2.0 ** -22, i      # g = bf16(n) / n: within half a bf16 ulp of 1, and not 1 wherever n is no bf16 value
    pk.check_outside(got, g, inv, range(len(mods)))
    # init = 0 on magnitudes of its own: m is read, never written
    rng = np.random.default_rng(5)
    m_bits = [D.to_bits(D.bf_np(rng.uniform(0.5, 3.0, W.shape[0]))) for W, _, _, _ in mods]
    pk = Packed(mods, m_bits)
    got, g, inv = pk.run(init=False)
    for i, ((W, A, B, s), go) in enumerate(zip(mods, pk.goff)):
        inv_w, g_w, _ = D.gains32(D.n2_64(W, A, B, s), m_bits[i])
        assert inv[go:go + W.shape[0]].tobytes() == inv_w.tobytes() and g[go:go + W.shape[0]].tobytes() == g_w.tobytes(), i
    pk.check_outside(got, g, inv, [])


def test_norm_gaussian_inputs_within_the_derived_bound():
    mods = D.gauss_inputs()
    pk = Packed(mods)
    got, g, inv = pk.run(init=True)
    for i, ((W, A, B, s), offs, go) in enumerate(zip(mods, pk.offs, pk.goff)):
        N = W.shape[0]
        n2, nb = D.n2_64(W, A, B, s), D.n2_bound(W, A, B, s)
        inv_g, g_g, m_g = inv[go:go + N].astype(np.float64), g[go:go + N], got[offs[3]:offs[3] + N]
        err = np.abs(inv_g - 1.0 / np.sqrt(n2))
        print(i, W.shape, A.shape[0], "inv error / bound", float((err / D.inv_bound(n2, nb)).max()))
        assert (err <= D.inv_bound(n2, nb)).all(), i
        # m = bf16(root of the kernel's n2): within the bound on the root of one bf16 rounding of the float64 norm, and g = float(m) inv exactly
        root = np.sqrt(n2)
        half = R.half_ulp_bf16(torch.from_numpy(root)).numpy()
        assert (np.abs(D.from_bits(m_g).astype(np.float64) - root) <= half + 0.5 * nb / root + 2.0 * D.U * root).all(), i
        assert g_g.tobytes() == (D.from_bits(m_g) * inv[go:go + N]).astype(np.float32).tobytes(), i
    pk.check_outside(got, g, inv, range(len(mods)))
    pk2 = Packed(mods)
    got2, g2, inv2 = pk2.run(init=True)
    assert np.array_equal(got, got2) and g.tobytes() == g2.tobytes() and inv.tobytes() == inv2.tobytes()


def test_norm_malformed_rows_are_skipped_by_the_kernel():
    """A row the builder would have refused reaches the kernel: nothing of W, A, B, m is touched, g and inv report NaN where their own
    addresses can be trusted; the other rows run."""
    mods = D.gauss_inputs()
    good = Packed(mods)
    _, g_ok, inv_ok = good.run(init=True)
    pk = Packed(mods)
    tab = pk.table.cpu()
    tab[0, 6] = 12                  # a rank outside LORA_RANKS
    tab[1, 7] = 44                  # K % 8 != 0
    tab[2, 2] += 8                  # B not 16-byte aligned
    tab[4, 4] = 0                   # no address for g: nothing at all is written
    pk.table.copy_(tab)
    got, g, inv = pk.run(init=True)
    for i in (0, 1, 2):
        sl = slice(pk.goff[i], pk.goff[i] + mods[i][0].shape[0])
        assert np.isnan(g[sl]).all() and np.isnan(inv[sl]).all(), i
    sl = slice(pk.goff[4], pk.goff[4] + mods[4][0].shape[0])
    assert (g[sl] == GS).all() and (inv[sl] == GS).all()
    for i in (3, 5):
        sl = slice(pk.goff[i], pk.goff[i] + mods[i][0].shape[0])
        assert g[sl].tobytes() == g_ok[sl].tobytes() and inv[sl].tobytes() == inv_ok[sl].tobytes(), i
    pk.check_outside(got, g, inv, [3, 5])


# every other guard of the kernel, one broken row per launch beside five good ones: (column, new value or a function of the old one,
# whether g and inv of the row can still be trusted and report NaN -- else nothing at all is written)
BROKEN = [
    ("W null", 0, 0, True), ("A null", 1, 0, True), ("B null", 2, 0, True), ("m null", 3, 0, True),
    ("W misaligned", 0, lambda v: v + 8, True), ("A misaligned", 1, lambda v: v + 4, True), ("m odd", 3, lambda v: v + 1, True),
    ("g misaligned", 4, lambda v: v + 2, False), ("inv null", 5, 0, False), ("inv misaligned", 5, lambda v: v + 1, False),
    ("K zero", 7, 0, True), ("K negative", 7, -8, True), ("K beyond 2^24", 7, (1 << 24) + 8, True),
    ("N no multiple of 8", 8, lambda v: v - 4, True), ("N zero", 8, 0, False), ("N beyond 2^24", 8, (1 << 24) + 8, False),
    ("rank beyond 32 bits", 6, (1 << 32) + 16, True),
]


@pytest.mark.parametrize("what, col, val, reports", BROKEN, ids=[b[0] for b in BROKEN])
def test_norm_every_guard_of_a_malformed_row(what, col, val, reports):
    mods = D.gauss_inputs()
    good = Packed(mods)
    _, g_ok, inv_ok = good.run(init=True)
    pk = Packed(mods)
    tab = pk.table.cpu()
    i = 2                           # 200 rows: four tiles
    tab[i, col] = val(int(tab[i, col])) if callable(val) else val
    pk.table.copy_(tab)
    got, g, inv = pk.run(init=True)
    N = mods[i][0].shape[0]
    n_rep = int(tab[i, 8]) if col == 8 and reports else N          # a shortened N reports its own rows only
    sl = slice(pk.goff[i], pk.goff[i] + n_rep)
    if reports:
        assert np.isnan(g[sl]).all() and np.isnan(inv[sl]).all(), what
        assert (g[pk.goff[i] + n_rep:pk.goff[i] + N] == GS).all() and (inv[pk.goff[i] + n_rep:pk.goff[i] + N] == GS).all()
    else:
        assert (g[sl] == GS).all() and (inv[sl] == GS).all(), what
    others = [k for k in range(len(mods)) if k != i]
    for k in others:
        s2 = slice(pk.goff[k], pk.goff[k] + mods[k][0].shape[0])
        assert g[s2].tobytes() == g_ok[s2].tobytes() and inv[s2].tobytes() == inv_ok[s2].tobytes(), (what, k)
    pk.check_outside(got, g, inv, others)


def test_norm_refusals_return_their_codes_and_launch_nothing():
    from aozora_sdxl_training_amd import dora, ops
    from aozora_sdxl_training_amd._lib import lib, AozoraError
    fn = lib()._fn["az_dora_norm_bf16"]
    pk = Packed(D.gauss_inputs())
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    T = pk.tiles
    codes = [fn(None, 6, T, 0, st), fn(P(pk.table, 4), 6, T, 0, st), fn(P(pk.table), 0, T, 0, st), fn(P(pk.table), 65536, T, 0, st),
             fn(P(pk.table), 6, 0, 0, st), fn(P(pk.table), 6, -2, 0, st), fn(P(pk.table), 6, 1 << 31, 0, st), fn(P(pk.table), 6, T, 2, st),
             fn(P(pk.table), 6, T, -1, st)]
    assert codes == [-1160, -1160, -1161, -1161, -1162, -1162, -1162, -1163, -1163]
    for bad in (dict(table=pk.table.int()), dict(table=pk.table.cpu()), dict(table=pk.table[:, :11]), dict(table=pk.table.t()), dict(tiles=0),
                dict(tiles=1.5), dict(tiles=True), dict(init=2), dict(init="1")):
        kw = dict(table=pk.table, tiles=T, init=0)
        kw.update(bad)
        with pytest.raises(AozoraError):
            ops.dora_norm(kw["table"], kw["tiles"], kw["init"])
    row = pk.table[2].tolist()
    for col, val in ((6, 12), (7, 44), (8, 0), (0, 0), (2, row[2] + 8), (3, row[3] + 1), (4, row[4] + 2)):
        bad = list(row)
        bad[col] = val
        with pytest.raises(AozoraError):
            dora.check_row(bad)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(pk.buf), pk.before) and bool((pk.g == GS).all()) and bool((pk.inv == GS).all())


# ---------------- scale --------------------------------------------------------------------------------------------------------------
def _padded(bits2d, pad_l=8, pad_r=16):
    """[M][N] bits inside a device buffer [M][pad_l + N + pad_r] of sentinels -> (buffer, the slice view)."""
    M, N = bits2d.shape
    host = np.full((M, pad_l + N + pad_r), D.SENTINEL, dtype=np.uint16)
    host[:, pad_l:pad_l + N] = bits2d
    buf = R.bits_to_bf16(host).to(DEV)
    return buf, buf[:, pad_l:pad_l + N], host


@pytest.mark.parametrize("M", [1, 17, 300])
def test_scale_every_element_bit_for_bit(M):
    from aozora_sdxl_training_amd import ops
    rng = np.random.default_rng(100 + M)
    for N in (8, 72, 320):
        v = D.to_bits(D.bf_np(rng.standard_normal((M, N))))
        res = D.to_bits(D.bf_np(rng.standard_normal((M, N))))
        bias = D.to_bits(D.bf_np(rng.standard_normal(N)))
        g = rng.uniform(0.5, 2.0, N).astype(np.float32)
        g_d = torch.from_numpy(g).to(DEV)
        _, v_d, _ = _padded(v)
        _, r_d, _ = _padded(res, 16, 8)
        b_d = R.bits_to_bf16(bias).to(DEV)
        for use_b in (False, True):
            for use_r in (False, True):
                ybuf, y_d, yhost = _padded(np.zeros((M, N), dtype=np.uint16))
                ops.dora_scale(v_d, g_d, y_d, bias=b_d if use_b else None, residual=r_d if use_r else None)
                torch.cuda.synchronize()
                got = _bits(ybuf).reshape(yhost.shape)
                want = D.scale_bits(v, g, bias if use_b else None, res if use_r else None)
                assert np.array_equal(got[:, 8:8 + N], want), (M, N, use_b, use_r)
                assert (got[:, :8] == D.SENTINEL).all() and (got[:, 8 + N:] == D.SENTINEL).all()


def test_scale_and_bwd_refusals():
    from aozora_sdxl_training_amd import ops
    from aozora_sdxl_training_amd._lib import lib, AozoraError
    M, N = 16, 72
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=DEV)
    v, y, g, b = bf(M, N), bf(M, N), torch.ones(N, device=DEV), bf(N)
    for bad in (dict(v=bf(M, 76)), dict(y=bf(M + 1, N)), dict(g=g.double()), dict(g=g[:64]), dict(g=torch.ones(N + 1, device=DEV)[1:]), dict(bias=bf(N + 8)),
                dict(bias=b.float()), dict(residual=bf(M, N + 8)), dict(y=bf(M, N + 4)[:, :N]), dict(v=bf(M, N + 8)[:, 4:N + 4]), dict(v=v.cpu())):
        kw = dict(v=v, g=g, y=y, bias=None, residual=None)
        kw.update(bad)
        with pytest.raises(AozoraError):
            ops.dora_scale(kw["v"], kw["g"], kw["y"], bias=kw["bias"], residual=kw["residual"])
    dm = bf(N)
    for bad in (dict(dv=bf(M, N + 8)), dict(g=g[:8]), dict(v=None), dict(inv=None), dict(inv=g.double()), dict(dm=bf(N + 8)), dict(dm=dm.float()),
                dict(v=bf(M + 1, N)), dict(dy=bf(M, N + 4)[:, :N])):
        kw = dict(dy=v, g=g, dv=y, v=v, inv=g, dm=dm)
        kw.update(bad)
        with pytest.raises(AozoraError):
            ops.dora_bwd(kw["dy"], kw["g"], kw["dv"], v=kw["v"], inv=kw["inv"], dm=kw["dm"])
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sc, bw = lib()._fn["az_dora_scale_bf16"], lib()._fn["az_dora_bwd_bf16"]
    ws = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    codes = [sc(0, N, P(v), N, P(g), None, None, 0, P(y), N, st), sc(M, 76, P(v), 80, P(g), None, None, 0, P(y), 80, st),
             sc(M, N, None, N, P(g), None, None, 0, P(y), N, st), sc(M, N, P(v, 2), N, P(g), None, None, 0, P(y), N, st),
             sc(M, N, P(v), N, P(g), P(b, 2), None, 0, P(y), N, st), sc(M, N, P(v), 64, P(g), None, None, 0, P(y), N, st),
             sc(M, N, P(v), N, P(g), None, P(v), 76, P(y), N, st),
             bw(M, 0, P(v), N, P(v), N, P(g), P(g), P(y), N, P(dm), P(ws), ws.numel() * 4, st),
             bw(M, N, None, N, P(v), N, P(g), P(g), P(y), N, P(dm), P(ws), ws.numel() * 4, st),
             bw(M, N, P(v), N, None, N, P(g), P(g), P(y), N, P(dm), P(ws), ws.numel() * 4, st),
             bw(M, N, P(v), N, P(v), N, P(g), P(g), P(y), N, P(dm), None, 0, st),
             bw(M, N, P(v), 64, P(v), N, P(g), P(g), P(y), N, P(dm), P(ws), ws.numel() * 4, st),
             bw(M, N, P(v), N, P(v), N, P(g), P(g), P(y), N, P(dm), P(ws), 4 * N - 4, st)]
    torch.cuda.synchronize()
    assert codes == [-1164, -1164, -1165, -1165, -1165, -1166, -1166, -1168, -1169, -1169, -1169, -1170, -1171]
    assert not bool(y.any()) and not bool(dm.any())


# ---------------- backward -------------------------------------------------------------------------------------------------------------
def _bwd(dy, v, g, inv, dm_prev, train=True):
    from aozora_sdxl_training_amd import ops
    M, N = dy.shape
    _, dy_d, _ = _padded(dy)
    _, v_d, _ = _padded(v, 16, 8)
    dvbuf, dv_d, dvhost = _padded(np.zeros((M, N), dtype=np.uint16))
    dmbuf = R.bits_to_bf16(np.concatenate([np.full(64, D.SENTINEL, np.uint16), dm_prev, np.full(64, D.SENTINEL, np.uint16)])).to(DEV)
    g_d, inv_d = torch.from_numpy(g).to(DEV), torch.from_numpy(inv).to(DEV)
    if train:
        ops.dora_bwd(dy_d, g_d, dv_d, v=v_d, inv=inv_d, dm=dmbuf[64:64 + N])
    else:
        ops.dora_bwd(dy_d, g_d, dv_d)
    torch.cuda.synchronize()
    dv = _bits(dvbuf).reshape(dvhost.shape)
    assert (dv[:, :8] == D.SENTINEL).all() and (dv[:, 8 + N:] == D.SENTINEL).all()
    dm = _bits(dmbuf)
    assert (dm[:64] == D.SENTINEL).all() and (dm[-64:] == D.SENTINEL).all()
    return dv[:, 8:8 + N], dm[64:64 + N]


@pytest.mark.parametrize("M, N", [(1, 8), (17, 72), (300, 320), (2500, 72)])
def test_bwd_exactly_summable_inputs_bit_for_bit(M, N):
    """dy, v multiples of 1/4 in [-2, 2], inv a power of two, dm_prev a multiple of 1/8: every sum is exact in fp32, one bf16 rounding.
    300 and 2500 rows are no multiples of the row split (2500 rows of 72 columns: 63 splits of 40 rows, the last one short)."""
    rng = np.random.default_rng(M + N)
    dy, v = (D.to_bits(rng.integers(-8, 9, (M, N)) / 4.0) for _ in range(2))
    g = rng.uniform(0.5, 2.0, N).astype(np.float32)
    inv = np.asarray([0.5, 2.0, 1.0, 0.25], np.float32)[rng.integers(0, 4, N)]
    dm_prev = D.to_bits(rng.integers(-32, 33, N) / 8.0)
    dv, dm = _bwd(dy, v, g, inv, dm_prev)
    assert np.array_equal(dv, D.dv_bits(dy, g))
    want, S = D.dm_64(dy, v, inv, dm_prev)
    assert 64.0 * (S.max() + 4.0) < 2.0 ** 24
    assert np.array_equal(dm, R.bf16_bits_np(want.astype(np.float32)))
    assert np.array_equal(*(_bwd(dy, v, g, inv, dm_prev)[1], dm))                # two launches alike
    dv0, dm0 = _bwd(dy, v, g, inv, dm_prev, train=False)                         # without dm: dv alone, nothing accumulated
    assert np.array_equal(dv0, dv) and np.array_equal(dm0, dm_prev)


@pytest.mark.parametrize("M, N", [(17, 72), (300, 320), (1000, 8)])
def test_bwd_gaussian_inputs_within_the_bound(M, N):
    rng = np.random.default_rng(7 * M + N)
    dy, v = D.to_bits(D.bf_np(rng.standard_normal((M, N)))), D.to_bits(D.bf_np(rng.standard_normal((M, N))))
    g = rng.uniform(0.5, 2.0, N).astype(np.float32)
    inv = rng.uniform(0.2, 3.0, N).astype(np.float32)
    dm_prev = D.to_bits(D.bf_np(rng.standard_normal(N)))
    dv, dm = _bwd(dy, v, g, inv, dm_prev)
    assert np.array_equal(dv, D.dv_bits(dy, g))
    want, S = D.dm_64(dy, v, inv, dm_prev)
    # M 2^-24 inv sum |dy v| plus one bf16 rounding (S already carries inv)
    tol = R.half_ulp_bf16(torch.from_numpy(want)).numpy() + M * D.U * S
    err = np.abs(D.from_bits(dm).astype(np.float64) - want)
    print(M, N, "dm error / bound", float((err / tol).max()))
    assert (err <= tol).all()
    assert np.array_equal(_bwd(dy, v, g, inv, dm_prev)[1], dm)


# ---------------- the native tape ----------------------------------------------------------------------------------------------------
def test_recorded_calls_replay_through_the_native_tape():
    from aozora_sdxl_training_amd import ops
    from aozora_sdxl_training_amd._lib import lib
    from aozora_sdxl_training_amd.tape import NativeTape
    mods = D.gauss_inputs()
    want_bits, want_g, want_inv = Packed(mods).run(init=True)
    pk = Packed(mods)
    rng = np.random.default_rng(3)
    M, N = 40, 72
    bf = lambda a: R.bits_to_bf16(D.to_bits(D.bf_np(a))).to(DEV)
    v, dy, dm0 = bf(rng.standard_normal((M, N))), bf(rng.standard_normal((M, N))), bf(rng.standard_normal(N))
    g = torch.from_numpy(rng.uniform(0.5, 2.0, N).astype(np.float32)).to(DEV)
    y, dv, dm = torch.zeros_like(v), torch.zeros_like(v), dm0.clone()
    L = lib()
    L.recorder = []
    try:
        ops.dora_norm(pk.table, pk.tiles, True)
        ops.dora_scale(v, g, y)
        ops.dora_bwd(dy, g, dv, v=v, inv=g, dm=dm)
        recorded = L.recorder
    finally:
        L.recorder = None
    assert [op.name for op in recorded] == ["az_dora_norm_bf16", "az_dora_scale_bf16", "az_dora_bwd_bf16"]
    torch.cuda.synchronize()
    first = (_bits(pk.buf), pk.g.cpu().numpy(), pk.inv.cpu().numpy(), _bits(y), _bits(dv), _bits(dm))
    assert np.array_equal(first[0], want_bits) and first[1].tobytes() == want_g.tobytes() and first[2].tobytes() == want_inv.tobytes()
    nt = NativeTape(recorded)
    assert nt.n_calls == 3 and not nt.callbacks
    pk.buf.copy_(R.bits_to_bf16(pk.before).to(DEV)); pk.g.fill_(GS); pk.inv.fill_(GS)
    y.zero_(); dv.zero_(); dm.copy_(dm0)
    nt.play()
    torch.cuda.synchronize()
    again = (_bits(pk.buf), pk.g.cpu().numpy(), pk.inv.cpu().numpy(), _bits(y), _bits(dv), _bits(dm))
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
