"""Every kernel and dispatch branch of aozora_sdxl_training_amd/csrc/az_attn.hip bit for bit on closed-form inputs.

tests/attn_ref.py builds selector inputs for which O, delta, dQ, dK and dV are ONE bit pattern per element and lse2 is known to a
few ulp; the comparison (attn_ref.mismatches) is equality of the bf16 outputs and of the fp32 delta, lse2 within 4 fp32 ulp of the
float64 value.  Operands are views inside larger allocations filled with a finite poison (q | k | v column slices of one fused
buffer for self-attention, k | v of one buffer for cross-attention, poisoned rows in front and behind: batch strides differ from
T * ld); outputs, lse and delta are views in sentinel-filled buffers whose sentinels must be bit-identical afterwards.  The output
views hold a stale value before every backward, so no result of an earlier schedule can stand in for a store that did not happen.

A row of a case table is (case, ATTN_PIPE, ATTN_SPLIT_TARGET, parts schedule, workspace, ATTN_XCD).  attn_ref.fwd_kernel /
bwd_kernels mirror the host dispatch; tests/test_attn_ref_cpu.py asserts for every family below that each row reaches the kernels the
family is about and that the family as a whole reaches all of them:

  FWD_DMA      attn_fwd_dma_kernel (bit 0; rotated key order per query block; both group layouts).  Its backward: the merged
               LDS-DMA launch (Tq == Tk), dq_dma<fused> + dkv_dma (128 x 384), the short-key kernel (384 x 128)
  FWD_FULL     attn_fwd_kernel<true>: the same shapes with bit 0 off, and Tk % 128 == 64 by default
  FWD_GENERAL  attn_fwd_kernel<false>: 32 (Tq, Tk) pairs over every boundary value of both axes, bias column.  Backward by default:
               attn_bwd_cross_kernel (Tk <= 128), else attn_bwd_dq_kernel<true, false> + attn_bwd_dkv_kernel (+ reduce)
  MERGED       attn_delta_kernel + attn_bwd_merged_dma_kernel (ATTN_PIPE 15) / attn_bwd_merged_kernel (7), Tq = Tk in 128, 256, 512
  SHORT        attn_bwd_cross_kernel (ATTN_PIPE 13: bit 1 off so that 128 x 128 reaches it): one workgroup per head with a direct
               store (target 1), two splits (target 2 BH), the default and one tile per workgroup (4096), + attn_dkv_reduce_kernel
  DQ_DKV       parts (3, 4) and (1, 2, 4) at ATTN_PIPE 9 / 1: attn_bwd_dq_kernel<fused | plain, full | general>,
               attn_bwd_dq_dma_kernel<fused | plain>, attn_delta_kernel alone, attn_bwd_dkv_kernel without a split, with a split +
               reduce (Tq >= 256; Tk = 154: two key blocks, the second ragged), attn_bwd_dkv_dma_kernel (bit 3, target 1)
  SCHEDULES    parts (7), (3, 4), (1, 6), (1, 2, 4), (5, 2): the same bits
  WORKSPACE    workspace == NULL and a workspace too small for the aimed split, for both query splits: the same bits
  XCD          ATTN_XCD 0 on two rows per family (every other row runs at 15)

then the argument rejections, a uniform layer (Q = 0: the running sum over EVERY key) and a peaked layer (Gaussian inputs with a
largest probability of ~0.5 per row, per-row relative L2 error against float64, bound = 2 x the fp32 emulation's own error with a
floor of 2^-8).  The emulation runs the online softmax of the forward kernel the shape reaches (attn_ref._online_plain /
_online_dma): a probability is rounded to bf16 relative to the RUNNING maximum of its tile (the stale one in the LDS-DMA form), so
two schedules of the same arithmetic draw different rounding errors, and the per-row error of a row whose probability sits on one
key is one scalar (the error of delta) times a vector -- against the emulation of the OTHER schedule 14 dQ rows of (1,2,256,256)
miss the bound on the CPU alone.  Largest kernel / emulation ratio of the per-row error observed on an MI355X, per output, over the
three shapes: O 1.001, dQ 1.506, dK 1.055, dV 1.088 (worst kernel / bound 0.753; the kernels' and the emulation's largest row errors
agree to four digits in every output).

No row of any table needed a kernel change: az_attn.hip passes as it is."""
import contextlib
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import attn_ref as R        # noqa: E402
from attn_ref import Case   # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
F32 = torch.float32
STALE = 7.0

# ---------------- case tables (CPU side) -----------------------------------------------------------------------------------------
# ws: "full" (the library workspace), "null", or a byte count
Row = namedtuple("Row", "case pipe target sched ws xcd", defaults=(15, 384, (7,), "full", 15))


def row_id(r):
    return (f"{R.case_id(r.case)}-pipe{r.pipe}-t{r.target}-p{'.'.join(str(p) for p in r.sched)}"
            f"{'' if r.ws == 'full' else '-ws' + str(r.ws)}{'' if r.xcd == 15 else '-xcd' + str(r.xcd)}")


def _case(B, H, Tq, Tk, i, g=None):
    """Group size, layout, dO / V variant and column rotation go with the row number; the bias column wherever an axis is ragged."""
    c = Case(B, H, Tq, Tk, g if g is not None else (2, 4)[i % 2], ("near", "far")[(i // 2) % 2], False, bool((i // 2 + i) % 2), i)
    return c._replace(bias=R.ragged(c))


DMA_SHAPES = [(2, 3, 256, 256), (1, 2, 512, 512), (1, 2, 128, 384), (1, 1, 384, 128)]
_dma_cases = []
for _i, _s in enumerate(DMA_SHAPES):
    _dma_cases += [_case(*_s, 2 * _i), _case(*_s, 2 * _i + 3)]       # both layouts, both group sizes per shape
_dma_cases.append(Case(1, 2, 512, 512, 1, "near"))                   # g = 1: the forward alone matters (dQ = dK = 0)
FWD_DMA = [Row(c) for c in _dma_cases]
FWD_FULL = ([Row(c, pipe=14) for c in _dma_cases] +
            [Row(_case(1, 2, 128, 192, 0)), Row(_case(1, 2, 128, 192, 3)), Row(_case(1, 2, 256, 64, 1)), Row(_case(1, 2, 256, 64, 2))])

TQ_EDGES = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 257]
TK_EDGES = [1, 2, 31, 32, 33, 63, 64, 65, 77, 96, 97, 127, 128, 129, 154, 191, 193, 257]
GENERAL_PAIRS = [(1, 1), (31, 2), (32, 31), (33, 32), (63, 33), (64, 63), (65, 64), (127, 65), (128, 77), (129, 96), (200, 97), (257, 127),
                 (1, 128), (31, 129), (32, 154), (33, 191), (63, 193), (64, 257), (65, 1), (127, 2), (128, 31), (129, 33), (200, 63),
                 (257, 65), (1, 77), (200, 154), (257, 193), (128, 129), (129, 128), (257, 257), (128, 191), (64, 96)]
FWD_GENERAL = [Row(_case(1, 2, tq, tk, i)) for i, (tq, tk) in enumerate(GENERAL_PAIRS)]

MERGED = [Row(_case(B, H, T, T, i + j), pipe=pipe) for j, pipe in enumerate((15, 7))
          for i, (B, H, T) in enumerate([(1, 2, 128), (2, 3, 256), (1, 2, 256), (1, 2, 512)])]

SHORT_TK = [1, 31, 32, 33, 64, 65, 77, 96, 97, 127, 128]
SHORT_TQ = [1, 35, 128, 200, 257, 640]
SHORT = []
for _i, _tk in enumerate(SHORT_TK):
    for _j in range(2):
        _tq = SHORT_TQ[(_i + 3 * _j) % 6]
        SHORT.append(Row(_case(1, 2, _tq, _tk, _i + _j), pipe=13, target=(1, 384, 4096, 4)[(_i + _j) % 4]))
for _k, _t in enumerate((1, 4, 384, 4096)):          # every split of the two longest query axes: 1, 2, 3 / 5 workgroups per head
    SHORT += [Row(_case(1, 2, 640, 77, _k), pipe=13, target=_t), Row(_case(1, 2, 257, 128, _k + 1), pipe=13, target=_t)]
SHORT.append(Row(_case(2, 3, 640, 97, 1), pipe=13, target=12))      # 2 workgroups of 3 + 2 tiles on six (batch, head)

DQ_SHAPES = [(1, 2, 256, 256), (1, 2, 128, 384), (1, 2, 256, 192), (1, 2, 200, 77), (1, 2, 257, 154), (1, 2, 512, 154), (1, 2, 129, 193),
             (2, 3, 384, 128)]
DQ_DKV = []
for _i, _s in enumerate(DQ_SHAPES):
    for _j, (_pipe, _sched) in enumerate([(9, (3, 4)), (9, (1, 2, 4)), (1, (3, 4)), (1, (1, 2, 4))]):
        DQ_DKV.append(Row(_case(*_s, _i + _j), pipe=_pipe, sched=_sched, target=(384, 1)[(_i + _j // 2) % 2]))
DQ_DKV += [Row(_case(1, 2, 256, 256, 1), pipe=9, sched=(3, 4), target=1), Row(_case(1, 2, 256, 256, 2), pipe=9, sched=(3, 4), target=384),
           Row(_case(1, 2, 512, 154, 3), pipe=1, sched=(3, 4), target=384), Row(_case(1, 2, 512, 154, 0), pipe=1, sched=(1, 2, 4), target=6)]

SCHEDS = [(7,), (3, 4), (1, 6), (1, 2, 4), (5, 2)]
SCHEDULES = [Row(_case(*s, i), sched=sc) for i, s in enumerate([(1, 2, 256, 256), (1, 2, 200, 77), (1, 2, 257, 154)]) for sc in SCHEDS]

# (1, 2, 640, 77): 5 query tiles, the default target aims at 5 splits = 5 * 2 * 64 KiB; (1, 2, 512, 154): 8 tiles of 64 queries, two key
# blocks, 4 splits = 4 * 2 * 2 * 64 KiB
WORKSPACE = [Row(_case(1, 2, 640, 77, 0), ws=ws) for ws in ("full", "null", 3 * 2 * 65536, 65536)] + \
            [Row(_case(1, 2, 512, 154, 1), ws=ws) for ws in ("full", "null", 2 * 2 * 2 * 65536, 65536)]

XCD = [r._replace(xcd=0) for fam in (FWD_DMA, FWD_FULL, FWD_GENERAL, MERGED, SHORT, DQ_DKV) for r in (fam[1], fam[-2])]

UNIFORM_TQ = [128, 200]
PEAKED = [(1, 2, 256, 256), (1, 2, 128, 192), (1, 2, 200, 77)]       # fwd_dma + merged_dma | fwd_full + dq / dkv | fwd_general + short-key

FAMILIES = {"FWD_DMA": FWD_DMA, "FWD_FULL": FWD_FULL, "FWD_GENERAL": FWD_GENERAL, "MERGED": MERGED, "SHORT": SHORT, "DQ_DKV": DQ_DKV,
            "SCHEDULES": SCHEDULES, "WORKSPACE": WORKSPACE, "XCD": XCD}


def ws_bytes_of(r):
    return {"full": R.WS_DEFAULT, "null": 0}.get(r.ws, r.ws)


def kernels_of(r):
    """-> (forward kernel, [kernels of every az_attn_bwd call of the schedule]) by the mirror of the host dispatch."""
    c = r.case
    bwd = []
    for p in r.sched:
        bwd += R.bwd_kernels(c.B, c.H, c.Tq, c.Tk, r.pipe, r.target, p, ws_bytes_of(r))
    return R.fwd_kernel(c.Tq, c.Tk, r.pipe), bwd


# ---------------- GPU side -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def options(**kw):
    from aozora_sdxl_training_amd._lib import get_option, set_option
    old = {k: get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            set_option(k, v)


def btc(x):
    """(B, H, T, 64) numpy -> (B, T, H * 64) bf16 on the device."""
    B, H, T, _ = x.shape
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1, 3), dtype=np.float32)).reshape(B, T, H * 64).to(BF16).to(DEV)


def bhtd(t, H):
    """(B, T, H * 64) device tensor -> (B, H, T, 64) fp32 numpy."""
    B, T, _ = t.shape
    return t.float().cpu().reshape(B, T, H, 64).permute(0, 2, 1, 3).contiguous().numpy()


class Guard:
    """Sentinel-filled buffers and the views the kernels may write: everything else must keep its bits."""
    def __init__(self):
        self.items = []

    def framed(self, shape, index, fill=R.SENTINEL, dtype=BF16):
        buf = torch.full(shape, fill, dtype=dtype, device=DEV)
        keep = torch.ones(shape, dtype=torch.bool, device=DEV)
        keep[index] = False
        self.items.append((buf, buf.clone(), keep))
        return buf[index]

    def check(self):
        for buf, snap, keep in self.items:
            it = torch.int16 if buf.dtype == BF16 else torch.int32
            assert torch.equal(buf.view(it)[keep], snap.view(it)[keep]), f"sentinels of a {tuple(buf.shape)} buffer changed"


class Staged:
    def __init__(self, Q, K, V, dO, lead=2, tail=3):
        B, H, Tq, _ = Q.shape
        Tk = K.shape[2]
        C = H * 64
        self.B, self.H, self.Tq, self.Tk, self.C = B, H, Tq, Tk, C
        rows = lambda T: slice(lead, lead + T)       # noqa: E731
        if Tq == Tk:        # self-attention: q | k | v are column slices of one fused buffer
            fused = torch.full((B, Tq + lead + tail, 3 * C + 8), R.POISON, dtype=BF16, device=DEV)
            self.q, self.k, self.v = (fused[:, rows(Tq), i * C:(i + 1) * C] for i in range(3))
        else:               # cross-attention: q alone, k | v of one buffer
            qb = torch.full((B, Tq + lead + tail, C + 24), R.POISON, dtype=BF16, device=DEV)
            kvb = torch.full((B, Tk + lead + tail, 2 * C + 8), R.POISON, dtype=BF16, device=DEV)
            self.q, self.k, self.v = qb[:, rows(Tq), 8:8 + C], kvb[:, rows(Tk), :C], kvb[:, rows(Tk), C:2 * C]
        dob = torch.full((B, Tq + 1 + 2, C + 8), R.POISON, dtype=BF16, device=DEV)
        self.do = dob[:, 1:1 + Tq, :C]
        for dst, src in ((self.q, Q), (self.k, K), (self.v, V), (self.do, dO)):
            dst.copy_(btc(src))
        g = self.guard = Guard()
        n = B * H * Tq
        self.o = g.framed((B, Tq + lead + tail, C + 16), (slice(None), rows(Tq), slice(8, 8 + C)))
        self.dq = g.framed((B, Tq + lead + tail, C + 8), (slice(None), rows(Tq), slice(0, C)))
        dkv = g.framed((B, Tk + lead + tail, 2 * C + 8), (slice(None), rows(Tk), slice(0, 2 * C)))
        self.dk, self.dv = dkv[..., :C], dkv[..., C:]
        self.lse = g.framed((n + 32,), (slice(0, n),), dtype=F32)
        self.delta = g.framed((n + 32,), (slice(0, n),), dtype=F32)
        self.ws_small = None

    def stale(self):
        for t in (self.dq, self.dk, self.dv, self.delta):
            t.fill_(STALE)

    def workspace(self, ops, ws):
        """-> (tensor or None, bytes): the library's workspace, none, or `ws` bytes in front of sentinels."""
        if ws == "full":
            w = ops.workspace(torch.device(DEV)).attn
            return w, w.numel() * 4
        if ws == "null":
            return None, 0
        if self.ws_small is None:
            self.ws_small = self.guard.framed((ws // 4 + 4096,), (slice(0, ws // 4),), dtype=F32)
        return self.ws_small, ws

    def fwd(self, ops):
        ops.attn_fwd(self.q, self.k, self.v, self.o, self.lse, self.H, R.SCALE)

    def bwd_args(self, ops, parts, ws):
        from aozora_sdxl_training_amd.ops import _ptr, _stream
        w, wb = self.workspace(ops, ws)
        a = [self.B, self.H, self.Tq, self.Tk, float(R.SCALE)]
        for t in (self.q, self.k, self.v, self.o, self.do):
            a += [_ptr(t), t.stride(1), t.stride(0)]
        a += [_ptr(self.lse), _ptr(self.delta)]
        for t in (self.dq, self.dk, self.dv):
            a += [_ptr(t), t.stride(1), t.stride(0)]
        return a + [_ptr(w), wb, int(parts), _stream()]

    def bwd(self, ops, parts=7, ws="full"):
        from aozora_sdxl_training_amd._lib import lib
        lib().call("az_attn_bwd", *self.bwd_args(ops, parts, ws))

    def got(self):
        torch.cuda.synchronize()
        sh = (self.B, self.H, self.Tq)
        return {"O": bhtd(self.o, self.H), "dQ": bhtd(self.dq, self.H), "dK": bhtd(self.dk, self.H), "dV": bhtd(self.dv, self.H),
                "lse": self.lse.cpu().numpy().reshape(sh), "delta": self.delta.cpu().numpy().reshape(sh)}


def run_row(ops, r):
    d = R.build(r.case)
    exp = R.closed_form(d)
    fwdk, bwdk = kernels_of(r)
    with options(ATTN_PIPE=r.pipe, ATTN_XCD=r.xcd, ATTN_SPLIT_TARGET=r.target):
        st = Staged(d.Q, d.K, d.V, d.dO)
        st.fwd(ops)
        st.stale()
        for p in r.sched:
            st.bwd(ops, p, r.ws)
        got = st.got()
    # the one-kernel short-key backward keeps delta to itself; every other schedule leaves it in the buffer
    writes_delta = any(k == "delta" or "fused" in k for k in bwdk)
    names = ["O", "lse", "dQ", "dK", "dV"] + (["delta"] if writes_delta else [])
    bad = R.mismatches(got, exp, names)
    assert not bad, f"{row_id(r)} [{fwdk}; {' '.join(bwdk)}]: " + "; ".join(bad)
    if not writes_delta:
        assert np.all(got["delta"] == STALE), "the short-key backward wrote delta"
    st.guard.check()


def params(rows):
    return pytest.mark.parametrize("row", rows, ids=[row_id(r) for r in rows])


@params(FWD_DMA)
def test_fwd_dma(ops, row):
    run_row(ops, row)


@params(FWD_FULL)
def test_fwd_full(ops, row):
    run_row(ops, row)


@params(FWD_GENERAL)
def test_fwd_general(ops, row):
    run_row(ops, row)


@params(MERGED)
def test_bwd_merged(ops, row):
    run_row(ops, row)


@params(SHORT)
def test_bwd_short_key(ops, row):
    run_row(ops, row)


@params(DQ_DKV)
def test_bwd_dq_dkv(ops, row):
    run_row(ops, row)


@params(SCHEDULES)
def test_parts_schedules(ops, row):
    run_row(ops, row)


@params(WORKSPACE)
def test_workspace_fallbacks(ops, row):
    run_row(ops, row)


@params(XCD)
def test_plain_workgroup_order(ops, row):
    run_row(ops, row)


# ---------------- rejections -------------------------------------------------------------------------------------------------------
def test_rejections(ops):
    """az_attn_fwd / az_attn_bwd return the argument error for a non-positive dimension (51 / 52), a pointer off 16 bytes and an
    ld or batch stride that is no multiple of 8 (50), and launch nothing: the stale outputs and the sentinels keep their bits."""
    from aozora_sdxl_training_amd._lib import lib
    from aozora_sdxl_training_amd.ops import _ptr, _stream
    import ctypes
    d = R.build(Case(1, 2, 128, 77, 2, "near", True))
    st = Staged(d.Q, d.K, d.V, d.dO)
    st.o.fill_(STALE)
    st.lse.fill_(STALE)
    st.stale()
    fwd = lib()._fn["az_attn_fwd"]
    bwd = lib()._fn["az_attn_bwd"]

    def fwd_args():
        a = [st.B, st.H, st.Tq, st.Tk, float(R.SCALE)]
        for t in (st.q, st.k, st.v, st.o):
            a += [_ptr(t), t.stride(1), t.stride(0)]
        return a + [_ptr(st.lse), _stream()]

    def off8(p):
        return ctypes.c_void_p(p.value + 8)

    n_fwd = n_bwd = 0
    for i in range(4):          # non-positive batch, heads, Tq, Tk
        for bad in (0, -1):
            a = fwd_args(); a[i] = bad
            assert fwd(*a) == -1051
            a = st.bwd_args(ops, 7, "full"); a[i] = bad
            assert bwd(*a) == -1052
    for base in (5, 8, 11, 14):            # Q, K, V, O: pointer, ld, batch stride
        a = fwd_args(); a[base] = off8(a[base]); assert fwd(*a) == -1050
        a = fwd_args(); a[base + 1] += 4; assert fwd(*a) == -1050
        a = fwd_args(); a[base + 2] += 4; assert fwd(*a) == -1050
        n_fwd += 3
    for base in (5, 8, 11, 14, 17, 22, 25, 28):      # Q, K, V, O, dO, dQ, dK, dV
        for parts in (7, 3, 4):
            a = st.bwd_args(ops, parts, "full"); a[base] = off8(a[base]); assert bwd(*a) == -1050
            a = st.bwd_args(ops, parts, "full"); a[base + 1] += 4; assert bwd(*a) == -1050
            a = st.bwd_args(ops, parts, "full"); a[base + 2] += 4; assert bwd(*a) == -1050
            n_bwd += 3
    assert n_fwd == 12 and n_bwd == 72
    torch.cuda.synchronize()
    for t in (st.o, st.lse, st.dq, st.dk, st.dv, st.delta):
        assert bool((t == STALE).all()), "a rejected call wrote an output"
    st.guard.check()


# ---------------- uniform layer: the running sum over every key --------------------------------------------------------------------
def bf16_ulp(x):
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.where(x > 0, 2.0 ** (np.floor(np.log2(np.maximum(x, 1e-300))) - 7), 0.0)


def uniform_inputs(Tq, Tk, B=1, H=2):
    rng = np.random.default_rng([Tq, Tk])
    return (np.zeros((B, H, Tq, 64)), rng.integers(-4, 5, size=(B, H, Tk, 64)).astype(np.float64),
            rng.integers(-2, 3, size=(B, H, Tk, 64)).astype(np.float64), rng.integers(-2, 3, size=(B, H, Tq, 64)).astype(np.float64))


def uniform_failures(got, Q, K, V, dO):
    """Q = 0: every key has probability 1 / Tk, the softmax denominator counts EVERY key.  lse2 = log2(Tk) within 4 fp32 ulp (2^-20
    absolute at Tk = 1), O within 1 bf16 ulp of the float64 mean, dK == 0, dV within 2^-7 relative of sum dO / Tk (bf16 P 2^-9, the
    output rounding 2^-9, a factor 2 of slack), dQ at the tolerance of tests/test_kernels_gpu.py (rel. Frobenius 8e-3, max 3e-2).
    (CPU side: tests/test_attn_ref_cpu.py holds attn_ref's emulation to the same.)"""
    Tq, Tk = Q.shape[2], K.shape[2]
    out = []
    lse_ref = np.full(Q.shape[:3], np.log2(float(Tk)))
    tol = 2.0 ** -20 if Tk == 1 else 4.0 * R.ulp32(lse_ref)
    if not np.all(np.abs(got["lse"] - lse_ref) <= tol):
        out.append(f"lse2 off by {np.abs(got['lse'] - lse_ref).max():.3e}")
    o_ref = (V.sum(-2, keepdims=True) / Tk) * np.ones((1, 1, Tq, 1))          # integer sums: exact, zero where the sum is zero
    if not np.all(np.abs(got["O"] - o_ref) <= bf16_ulp(o_ref)):
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(f"O off by {np.nanmax(np.abs(got['O'] - o_ref) / bf16_ulp(o_ref)):.3f} bf16 ulp")
    if not np.all(got["dK"] == 0.0):
        out.append("dK != 0")
    dv_ref = (dO.sum(-2, keepdims=True) / Tk) * np.ones((1, 1, Tk, 1))
    if not np.all(np.abs(got["dV"] - dv_ref) <= 2.0 ** -7 * np.abs(dv_ref)):
        out.append(f"dV off by {np.abs(got['dV'] - dv_ref).max():.3e}")
    dq_ref = R.reference64(Q, K, V, dO)["dQ"]
    err = got["dQ"] - dq_ref
    fro, fro_ref = np.sqrt((err ** 2).sum()), np.sqrt((dq_ref ** 2).sum())
    if not (np.isfinite(got["dQ"]).all() and fro <= 8e-3 * fro_ref and np.abs(err).max() <= 3e-2 * np.abs(dq_ref).max()):
        out.append(f"dQ rel_fro={fro / (fro_ref + 1e-300):.3e} rel_max={np.abs(err).max() / (np.abs(dq_ref).max() + 1e-300):.3e}")
    return out


@pytest.mark.parametrize("Tk", TK_EDGES)
def test_uniform(ops, Tk):
    """The uniform layer (uniform_failures) over the ragged key counts, Tq = 128 and 200."""
    for Tq in UNIFORM_TQ:
        Q, K, V, dO = uniform_inputs(Tq, Tk)
        st = Staged(Q, K, V, dO)
        st.fwd(ops)
        st.stale()
        st.bwd(ops)
        bad = uniform_failures(st.got(), Q, K, V, dO)
        assert not bad, f"uniform {Tq}x{Tk}: " + "; ".join(bad)
        st.guard.check()


# ---------------- peaked layer -----------------------------------------------------------------------------------------------------
PEAKED_FLOOR = 2.0 ** -8


@pytest.mark.parametrize("B,H,Tq,Tk", PEAKED)
def test_peaked(ops, B, H, Tq, Tk):
    """Gaussian q, k with a largest probability of ~0.5 per row.  Per query row (O, dQ) and per key row (dK, dV): the relative L2
    error against float64 is at most 2 x the error of attn_ref's fp32 emulation on the same inputs (summation order and the hardware
    exponential), floor 2^-8 (one bf16 output rounding)."""
    Q, K, V, dO, pmax = R.peaked_inputs(B, H, Tq, Tk, 0)
    ref = R.reference64(Q, K, V, dO)
    emu = R.emulate_arrays(Q, K, V, dO, fwd="dma" if R.fwd_kernel(Tq, Tk) == "fwd_dma" else "plain")
    st = Staged(Q, K, V, dO)
    st.fwd(ops)
    st.stale()
    st.bwd(ops)
    got = st.got()
    st.guard.check()
    fails = []
    for n in ("O", "dQ", "dK", "dV"):
        ek, ee = R.row_rel_l2(got[n], ref[n]), R.row_rel_l2(emu[n], ref[n])
        bound = np.maximum(2.0 * ee, PEAKED_FLOOR)
        print(f"peaked {B}x{H}x{Tq}x{Tk} pmax={pmax:.3f} {n}: kernel max {ek.max():.3e} emulation max {ee.max():.3e} "
              f"largest ratio {float((ek / ee).max()):.3f} worst kernel/bound {float((ek / bound).max()):.3f}")
        if not np.all(ek <= bound):
            fails.append(f"{n}: {int((ek > bound).sum())} rows above the bound, worst kernel/bound {float((ek / bound).max()):.3f}")
    assert not fails, "; ".join(fails)
