"""Every entry point of aozora_sdxl_training_amd/csrc/az_gemm.hip (and az_gemm8.inc) bit for bit on exactly summable inputs.

tests/gemm_ref.py builds operands whose products and sums are exact in fp32 in any order, so the expected output is ONE bit pattern
per element (float64 result, rounded once to bf16, nearest even) and the comparison is torch.equal on bf16 bits: of the outputs and
of the sentinels around them.  A wrong rounding, a lost k-chunk at a ragged edge, a term mis-added in one epilogue piece or a slab
left out of a reduce changes a bit.  Operands sit inside larger allocations whose every other element is the finite poison
3 * 2^40 wherever include/aozora_hip.h lets the kernels ignore memory.  The exceptions to bit equality: the fused GEGLU `out`
(elem_ref's "geglu_out" bound) and the Gaussian layer at the end (gemm_ref.gauss_bound, derived, for cancellation and exponent
spread).  The case tables and the CPU-side builders live here; tests/test_gemm_ref_cpu.py imports them and checks `exact_ok` and the
share of non-representable results for every row without a GPU.

Two cases of the contract the tables keep as rejections: a k-contiguous A (forms nt and nn) needs K % 8 == 0 (aozora_hip.h, "K,
lda, ldb multiples of 8").  The odd k-depths run for tn and are asserted to be refused for nn: az_gemm_bf16 itself returns argument
error 2 (gemm_impl, `(K & 7) && !transA && !transB`).  For nt the library does not check the rule; K = 300 is refused by the
operand check of ops.gemm ("K must be a multiple of 8"), which is what the test asserts, and K = 304 runs in its place."""
import contextlib
import functools
import json
import os
import sys
from collections import namedtuple

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gemm_ref as R        # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16

# the ten variants of tests/test_kernels_gpu.py's fixture and (128, 160, 72): 4 stages of 64-deep k-tiles
TILES = [(0, 0, 0), (256, 256, 0), (128, 160, 8), (128, 160, 24), (128, 128, 8), (128, 160, 40), (128, 160, 56), (256, 256, 32),
         (256, 256, 8), (256, 320, 8), (128, 160, 72)]
TILES_SPLIT = [(0, 0, 0), (256, 256, 0), (128, 160, 72)]
TILES_GEGLU = [(0, 0, 0), (256, 256, 0), (256, 256, 8)]
TILES_GAUSS = [(0, 0, 0), (128, 160, 40), (128, 160, 56), (128, 160, 72), (256, 256, 32)]      # the heuristic and the deepest rings (4 / 5 / 4 / 4 stages)


def tile_id(t):
    return f"tile{t[0]}x{t[1]}w{t[2]}"


# ---------------- case tables (CPU side) -----------------------------------------------------------------------------------------
# form M N K | bias, rps (rows per row-bias segment, 0 = none), rb_pad (row-bias stride - N), res, acc | split | n_real (fused bias
# gradient, tn) | pa, pb: leading-dimension padding of A / B beyond their width rounded up to 8 | pc: ldc - N - c_off | c_off: column
# offset of the output view | pr: ldr - N - r_off (None: residual laid out like C) | r_off | lead, tail: poisoned rows around A, B,
# residual and C
G = namedtuple("G", "form M N K bias rps rb_pad res acc split n_real pa pb pc c_off pr r_off lead tail",
               defaults=(False, 0, 0, False, False, 1, None, 0, 0, 0, 0, None, 0, 0, 0))

K_NT = [8, 24, 32, 40, 64, 72, 128, 136, 192, 200, 256, 264, 320, 328, 384, 392]      # 1..7 k-tiles of 64, 1..13 of 32, with and without a tail
K_ODD = [1, 7, 9, 63, 65, 100]                                                          # tn only: nn is refused (K % 8)
SWEEP_M, SWEEP_N = 130, 168          # one row past a 128-row tile, one 8-chunk past a 160-wide tile


def ksweep_cases(form):
    if form == "nt":
        return [G("nt", SWEEP_M, SWEEP_N, K, bias=True, res=True) for K in K_NT]
    if form == "nn":
        return [G("nn", SWEEP_M, SWEEP_N, K, acc=True) for K in K_NT]
    out = []
    for K in K_NT + K_ODD:
        out += [G("tn", SWEEP_M, SWEEP_N, K, acc=True), G("tn", SWEEP_M, SWEEP_N, K, acc=True, n_real=SWEEP_M),
                G("tn", SWEEP_M, SWEEP_N, K, acc=True, n_real=SWEEP_M - 3)]
    return out


EDGE_MN = [(1, 8), (127, 160), (129, 168), (256, 256), (257, 264), (257, 328), (255, 320)]
EDGE_K = [64, 192, 448]            # K % 64 == 0: the 8-wave tile takes them when forced; 1, 3 and 7 k-tiles
EDGE_CASES = [G("nt", M, N, K, bias=True, res=True) for M, N in EDGE_MN for K in EDGE_K]

SCALAR_CASES = ([G("nt", 130, N, 72, bias=True, res=True, pc=pc) for N in (4, 77, 100) for pc in (0, 3)] +
                [G("nt", 130, 168, 72, bias=True, res=True, c_off=4, pc=4, pr=0),      # vector-shaped output at an 8-byte offset: the scalar path
                 G("nt", 130, 168, 72, bias=True, res=True, r_off=4, pr=4),            # residual at an 8-byte offset while C is aligned
                 G("nt", 130, 168, 72, bias=True, res=True, pc=8, pr=24),              # ldr != ldc on the vector path
                 G("nt", 130, 168, 72, bias=True, res=True, pc=0, pr=3),               # an odd ldr alone
                 G("nn", 130, 77, 72, acc=True, pc=3), G("tn", 130, 100, 100, acc=True, pc=0),
                 G("tn", 130, 77, 65, acc=True, pc=3, n_real=127)])

ROWBIAS_CASES = ([G("nt", 130, 168, 72, rps=rps) for rps in (1, 50, 64, 130, 1000)] +
                 [G("nt", 130, 168, 72, rps=50, rb_pad=8), G("nt", 130, 168, 72, rps=64, rb_pad=8, bias=True, acc=True),
                  G("nt", 130, 100, 72, rps=50, bias=True, acc=True, pc=3), G("nn", 130, 168, 72, rps=64, acc=True)])

STRIDE_CASES = {
    "nt": [G("nt", 130, 168, 72, bias=True, res=True, pa=24, pb=8, pc=8, lead=3, tail=2),
           G("nt", 130, 168, 200, bias=True, res=True, acc=True, pa=24, pb=8, pc=8, pr=16, lead=1, tail=1)],
    "nn": [G("nn", 130, 168, 72, acc=True, res=True, pa=24, pb=8, pc=8, lead=3, tail=2),
           G("nn", 130, 163, 200, acc=True, pa=24, pb=8, pc=8, lead=1, tail=1)],
    "tn": [G("tn", 130, 168, 100, acc=True, pa=24, pb=8, pc=8, lead=3, tail=2),
           G("tn", 130, 163, 72, acc=True, n_real=127, pa=24, pb=8, pc=8, lead=1, tail=1)],
}

SPLIT_MN = [(72, 320), (200, 136), (130, 168), (200, 100)]      # N = 136: vector reduce, N = 100: scalar reduce
SPLIT_K = {"tn": [64, 300, 520, 1000], "nt": [64, 304, 520, 1000]}      # nt: K = 300 is refused (K % 8), 304 stands in
SPLITS = [0, 1, 2, 3, 4, 7, 64]     # split > k-tiles; counts that ceil(ktiles / s) shrinks (5 k-tiles asked in 4 -> 3 slabs)


def split_cases(form, M, N):
    out = []
    for K in SPLIT_K[form]:
        for s in SPLITS:
            if form == "tn":
                out += [G("tn", M, N, K, acc=True, split=s), G("tn", M, N, K, acc=True, split=s, n_real=M - 3)]
            else:       # the scalar reduce adds no residual (argument error 6): bias + accumulate there
                out.append(G("nt", M, N, K, bias=True, res=(N % 8 == 0), acc=True, split=s))
    return out


BIG_SPLIT_CASES = [G("nt", 1024, 1280, 2048, bias=True, res=True, acc=True),
                   # 20 tiles of 256x256 in at most 4 slabs score 0.25 < 0.7 in gemm_impl: the product above stays unsplit.  10 x 5 tiles in 4
                   # slabs (200 of 256 CUs, score 0.72) is the smallest grid the big_split path takes at NT_SPLIT_BIG = 4
                   G("nt", 2305, 1280, 2048, bias=True, res=True, acc=True)]
BIG_FILL_CASE = G("nt", 257, 328, 192, bias=True, res=True)


def big_split_score(c, max_split, gemm8):
    """gemm_impl's choice for a k-heavy nt product: the best score tiles * splits / 256 - 0.02 (splits - 1) over widths 256 and (N % 320
    == 0, GEMM8 on) 320 and 2 .. max_split splits with >= 8 k-tiles each on at most 256 workgroups, grids of > 128 tiles excluded; the
    path is taken at >= 0.7.  -> (score, splits, width)"""
    best = (0.0, 0, 256)
    for bn in (256, 320):
        if bn == 320 and (c.N % 320 or not gemm8):
            continue
        tl = -(-c.M // 256) * -(-c.N // bn)
        if tl > 128:
            continue
        for sp in range(2, max_split + 1):
            if (c.K // 64) // sp < 8 or tl * sp > 256:
                break
            score = tl * sp / 256.0 - 0.02 * (sp - 1)
            if score > best[0] + 1e-9:
                best = (score, sp, bn)
    return best

NTG_M, NTG_K, NTG_WIDTHS = [4, 130], [8, 72, 192], [168, 8, 320, 160, 328]
TNG_PRODUCTS = [(130, 8, 64), (72, 328, 520), (200, 136, 300), (8, 168, 1)]
GEGLU_M, GEGLU_H, GEGLU_K = [1, 130, 257], [8, 64, 72, 200], [8, 72, 192]

CONV_GRIDS = [(1, 1, 5), (2, 5, 1), (2, 3, 3), (3, 5, 7), (2, 8, 8), (3, 16, 12), (3, 24, 24), (2, 28, 20)]
# per grid: (Cin, Cout, ks, stride).  Every grid has at least two channel pairs, every channel pair both strides; 1-high / 1-wide grids
# take the general gather, the others the multiply-high fast path across sample boundaries; (8, 4) / (72, 40): cout_real < cpad
CONV_TABLE = {
    (1, 1, 5): [(8, 4, 3, 1), (72, 40, 3, 2), (64, 64, 1, 1)],
    (2, 5, 1): [(8, 168, 3, 1), (64, 8, 3, 2)],
    (2, 3, 3): [(64, 64, 3, 2), (128, 136, 1, 1), (8, 4, 3, 1)],
    (3, 5, 7): [(72, 40, 3, 1), (8, 4, 3, 2), (64, 64, 1, 2)],
    (2, 8, 8): [(64, 64, 3, 1), (64, 8, 3, 1), (8, 168, 3, 2), (128, 136, 3, 1)],
    (3, 16, 12): [(128, 136, 3, 1), (64, 64, 3, 1), (72, 40, 1, 1)],
    (3, 24, 24): [(128, 136, 3, 2), (64, 8, 1, 1), (64, 64, 3, 1)],
    (2, 28, 20): [(64, 64, 3, 1), (8, 4, 3, 1), (8, 168, 1, 2)],
}
CONV_SPLITS = [0, 1, 2, 4]
UPS_SOURCES = [(2, 4, 4), (1, 3, 5), (2, 5, 7)]
UPS_CHANNELS = [(64, 64), (72, 40)]


def seed_of(*v):
    s = 12345
    for x in v:
        s = (s * 1000003 + int(x) + 17) % 2147483647
    return s


@functools.lru_cache(maxsize=None)
def make_gemm(c, gaussian=False):
    """Inputs (CPU bf16), float64 reference, S and expected bits of one plain-product case; computed once, shared by every tile."""
    form, M, N, K = c.form, c.M, c.N, c.K
    s = seed_of(M, N, K, {"nt": 0, "nn": 1, "tn": 2}[form], c.rps, c.split)
    mk = (lambda shape, i, lim=4, scale=1.0: R.gauss(shape, s + i, scale)) if gaussian else (lambda shape, i, lim=4, scale=1.0: R.quarters(shape, s + i, lim))
    d = {}
    d["a"] = mk((K, M) if form == "tn" else (M, K), 1)
    d["b"] = mk((N, K) if form == "nt" else (K, N), 2, scale=(K ** -0.5 if form != "tn" else 1.0))
    d["bias"] = mk(N, 3) if c.bias else None
    d["rowbias"] = mk(((M + c.rps - 1) // c.rps, N), 4) if c.rps else None
    d["res"] = mk((M, N), 5) if c.res else None
    d["prev"] = mk((M, N), 6, lim=8) if c.acc else None
    d["ref"], d["S"] = R.gemm(form, d["a"], d["b"], bias=d["bias"], rowbias=d["rowbias"], rows_per_seg=c.rps, residual=d["res"],
                              prev=d["prev"], exact=not gaussian)
    d["want"] = R.expected_bits(d["ref"])
    if c.n_real is not None:
        d["bold"] = mk(c.n_real, 7, lim=8)
        d["bref"], d["bS"] = R.bias_grad(d["a"], c.n_real, d["bold"], exact=not gaussian)
        d["bwant"] = R.expected_bits(d["bref"])
    return d


ConvCase = namedtuple("ConvCase", "B H W Cin Cout ks stride up_h up_w", defaults=(0, 0))      # up_h / up_w: upsample target extents (0: no upsample)


@functools.lru_cache(maxsize=None)
def make_conv(c, gaussian=False):
    """One convolution case: x, w, bias, rowbias, residual, dy, previous dW / dx and the references of forward, dgrad (overwrite,
    accumulate, residual form), wgrad (+ accumulate) and the channel sums."""
    B, H, W, Cin, Cout, ks, st = c.B, c.H, c.W, c.Cin, c.Cout, c.ks, c.stride
    s = seed_of(B, H, W, Cin, Cout, ks, st, c.up_h, c.up_w)
    mk = (lambda shape, i, lim=4, scale=1.0: R.gauss(shape, s + i, scale)) if gaussian else (lambda shape, i, lim=4, scale=1.0: R.quarters(shape, s + i, lim))
    ups = (c.up_h, c.up_w) if c.up_h else None
    Hc, Wc = ups if ups else (H, W)                     # extents the conv sees
    Ho, Wo = R.conv_out(Hc, ks, st), R.conv_out(Wc, ks, st)
    ex = not gaussian
    d = dict(Ho=Ho, Wo=Wo, ups=ups)
    d["x"], d["w"] = mk((B, H, W, Cin), 1), mk((Cout, ks, ks, Cin), 2, scale=(ks * ks * Cin) ** -0.5)
    d["bias"], d["rowbias"], d["res"] = mk(Cout, 3), mk((B, Cout), 4), mk((B, Ho, Wo, Cout), 5)
    d["y"], d["yS"] = R.conv_fwd(d["x"], d["w"], st, bias=d["bias"], rowbias=d["rowbias"], residual=d["res"], out_hw=ups, exact=ex)
    d["dy"] = mk((B, Ho, Wo, Cout), 6)
    d["dwprev"] = mk((Cout, ks, ks, Cin), 7, lim=8)
    d["dw"], d["dwS"] = R.conv_wgrad(d["dy"], d["x"], ks, st, Cout, prev=d["dwprev"], out_hw=ups, exact=ex)
    d["bold"] = mk(Cout, 8, lim=8)
    d["seg"], d["segS"], d["bg"], d["bgS"] = R.conv_sums(d["dy"], Cout, d["bold"], exact=ex)
    if ks == 3 and not ups:
        d["dxprev"], d["dxres"] = mk((B, H, W, Cin), 9, lim=8), mk((B, H, W, Cin), 10)
        d["dx"], d["dxS"] = R.conv_dgrad(d["dy"], d["w"], st, (H, W), exact=ex)
        d["dx_acc"], d["dx_accS"] = R.conv_dgrad(d["dy"], d["w"], st, (H, W), prev=d["dxprev"], exact=ex)
        d["dx_res"], d["dx_resS"] = R.conv_dgrad(d["dy"], d["w"], st, (H, W), residual=d["dxres"], exact=ex)
    return d


def conv_cases():
    return [ConvCase(*g, *ch) for g in CONV_GRIDS for ch in CONV_TABLE[g]]


def ups_cases(src):
    B, H, W = src
    return [ConvCase(B, H, W, ci, co, 3, 1, th, tw) for ci, co in UPS_CHANNELS for th in (2 * H, 2 * H - 1) for tw in (2 * W, 2 * W - 1)]


@functools.lru_cache(maxsize=None)
def make_geglu(M, H, K, with_bias):
    s = seed_of(M, H, K, 77)
    x, w = R.quarters((M, K), s + 1), R.quarters((2 * H, K), s + 2)
    b = R.quarters(2 * H, s + 3) if with_bias else None
    proj, S, out, bound = R.geglu_fwd(x, w, b)
    return dict(x=x, w=w, bias=b, proj=proj, S=S, out=out, bound=bound, want=R.expected_bits(proj))


@functools.lru_cache(maxsize=None)
def make_nt_grouped(M, K):
    s = seed_of(M, K, 88)
    a = R.quarters((M, K), s)
    ws = [R.quarters((N, K), s + 10 + i) for i, N in enumerate(NTG_WIDTHS)]
    bs = [R.quarters(N, s + 30 + i) if i % 2 == 0 else None for i, N in enumerate(NTG_WIDTHS)]
    return dict(a=a, ws=ws, bs=bs, refs=R.nt_grouped(a, ws, bs))


@functools.lru_cache(maxsize=None)
def make_tn_grouped(with_bias):
    jobs = []
    for i, (M, N, K) in enumerate(TNG_PRODUCTS):
        s = seed_of(M, N, K, 99)
        jobs.append((R.quarters((K, M), s + 1), R.quarters((K, N), s + 2), R.quarters((M, N), s + 3, lim=8),
                     R.quarters(M - 3 if M % 8 else M, s + 4, lim=8) if with_bias else None))
    return dict(jobs=jobs, refs=R.tn_grouped(jobs))


def all_plain_cases():
    """Every row of every plain-product table (for the CPU checks of exact_ok and the inexact share)."""
    out = []
    for f in ("nt", "nn", "tn"):
        out += ksweep_cases(f) + STRIDE_CASES[f]
    out += EDGE_CASES + SCALAR_CASES + ROWBIAS_CASES + BIG_SPLIT_CASES + [BIG_FILL_CASE]
    for f in ("tn", "nt"):
        for M, N in SPLIT_MN:
            out += split_cases(f, M, N)
    return out


# ---------------- GPU side -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def forced_tile(t):
    from aozora_sdxl_training_amd._lib import lib
    lib().call("az_gemm_set_tile_ex", *t)
    try:
        yield
    finally:
        lib().call("az_gemm_set_tile", 0, 0)


@pytest.fixture(params=TILES, ids=tile_id)
def tile(request, ops):
    with forced_tile(request.param):
        yield request.param


@pytest.fixture(params=TILES_SPLIT, ids=tile_id)
def tile_split(request, ops):
    with forced_tile(request.param):
        yield request.param


@pytest.fixture(params=TILES_GEGLU, ids=tile_id)
def tile_geglu(request, ops):
    with forced_tile(request.param):
        yield request.param


@pytest.fixture(params=TILES_GAUSS, ids=tile_id)
def tile_gauss(request, ops):
    with forced_tile(request.param):
        yield request.param


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


def nhwc(v, B, H, W):
    """[B*H*W][C] view at row stride ld -> (B, H, W, C) with the uniform pixel stride spelled out (unflatten leaves extent-1 axes any stride)."""
    ld = v.stride(0)
    return v.as_strided((B, H, W, v.shape[1]), (H * W * ld, W * ld, ld, 1))


def ibits(t):
    return t.view(torch.int16)


class Out:
    """An output inside a poisoned allocation on the device: `want` is the whole allocation as it must look after the call (the
    expected bits inside, every sentinel untouched), so one torch.equal checks both."""

    def __init__(self, want, ld=None, lead=0, tail=0, col_offset=0, prev=None, shape=None):
        want2 = want.reshape(-1, want.shape[-1]) if want.dim() != 2 else want
        rows, cols = want2.shape
        ld = cols if ld is None else ld
        init = prev.reshape(rows, cols) if prev is not None else torch.full((rows, cols), R.POISON, dtype=BF16)
        self.emb = R.embed(init, ld, lead, tail, col_offset)
        self.pristine = self.emb.buf.to(DEV)
        self.want = self.pristine.clone()
        self.emb.view(self.want).copy_(want2.to(DEV))
        self.buf = self.pristine.clone()
        self.shape, self.flat = shape, False

    def reset(self):
        self.buf.copy_(self.pristine)
        return self

    def view(self):
        v = self.emb.view(self.buf)
        if self.shape is None:
            return v
        return v.view(self.shape) if self.flat else nhwc(v, *self.shape[:-1])

    def check(self, name):
        if torch.equal(ibits(self.buf), ibits(self.want)):
            return
        msg = R.first_mismatch(self.emb.view(self.buf), self.emb.view(self.want))
        if msg is None:
            ne = (ibits(self.buf) != ibits(self.want)).nonzero()[0]
            msg = f"sentinel overwritten at allocation row {int(ne[0])} column {int(ne[1])} (view starts at row {self.emb.lead}, column {self.emb.off})"
        raise AssertionError(f"{name}: {msg}")


def flat_out(want, prev=None):
    """A contiguous output of any shape with 64 sentinels in front and behind (weights, bias and per-sample gradients)."""
    n = want.numel()
    o = Out(want.reshape(1, n), ld=n + 128, col_offset=64, prev=prev.reshape(1, n) if prev is not None else None)
    o.shape, o.flat = tuple(want.shape), True
    return o


def dev_in(t, ld=None, lead=0, tail=0, col_offset=0):
    """An input [rows][cols] inside a poisoned allocation on the device -> the logical view."""
    e = R.embed(t, t.shape[1] if ld is None else ld, lead, tail, col_offset)
    return e.view(e.buf.to(DEV))


def dev_nhwc(t, pad=8):
    """(B, H, W, C) input at pixel stride C + pad, the pad poisoned."""
    B, H, W, C = t.shape
    return nhwc(dev_in(t.reshape(-1, C), ld=C + pad), B, H, W)


_DEV = {}        # device operands per case, uploaded once for all tile variants (inputs are never written, outputs are reset per run)


def _gemm_inputs(c, d, gaussian=False):
    """Device operands of a plain-product case."""
    key = ("gemm", c, gaussian)
    if key not in _DEV:
        a, b = d["a"], d["b"]
        g = {"a": dev_in(a, R.up8(a.shape[1]) + c.pa, c.lead, c.tail), "b": dev_in(b, R.up8(b.shape[1]) + c.pb, c.lead, c.tail)}
        g["bias"] = d["bias"].to(DEV) if d["bias"] is not None else None
        g["rowbias"] = dev_in(d["rowbias"], c.N + c.rb_pad) if d["rowbias"] is not None else None
        if d["res"] is not None:
            pr = c.pc + c.c_off if c.pr is None else c.pr
            g["res"] = dev_in(d["res"], c.r_off + c.N + pr, c.lead, c.tail, c.r_off)
        else:
            g["res"] = None
        g["out"] = Out(d["want"], c.c_off + c.N + c.pc, c.lead, c.tail, c.c_off, prev=d["prev"])
        if c.n_real is not None:
            g["bg"] = flat_out(d["bwant"], prev=d["bold"])
        _DEV[key] = g
    return _DEV[key]


def run_gemm(ops, c, what, gaussian=False):
    d = make_gemm(c, gaussian)
    g = _gemm_inputs(c, d, gaussian)
    out = g["out"].reset()
    kw = dict(trans_a=c.form == "tn", trans_b=c.form == "nt", bias=g["bias"], rowbias=g["rowbias"], rows_per_seg=c.rps,
              residual=g["res"], accumulate=c.acc, split_k=c.split)
    if c.n_real is not None:
        bg = g["bg"].reset()
        ops.gemm(g["a"], g["b"], out.view(), trans_a=True, trans_b=False, accumulate=c.acc, split_k=c.split, bias_grad=bg.view().view(-1))
    else:
        ops.gemm(g["a"], g["b"], out.view(), **kw)
    name = f"{what} {c.form} {c.M}x{c.N}x{c.K} {c._asdict()}"
    if gaussian:
        return d, g
    out.check(name)
    if c.n_real is not None:
        g["bg"].check(name + " fused bias gradient")
    return d, g


def rejected(ops, c):
    """A case outside the contract must be refused, not computed."""
    from aozora_sdxl_training_amd._lib import AozoraError
    a = torch.zeros((c.M, c.K + 8 - c.K % 8), dtype=BF16, device=DEV)[:, :c.K]
    b = torch.zeros((c.N, c.K + 8 - c.K % 8) if c.form == "nt" else (c.K, c.N), dtype=BF16, device=DEV)
    b = b[:, :c.K] if c.form == "nt" else b
    out = torch.zeros((c.M, c.N), dtype=BF16, device=DEV)
    with pytest.raises(AozoraError):
        ops.gemm(a, b, out, trans_a=False, trans_b=c.form == "nt")


# ---------------- plain products under every tile variant --------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["nt", "nn", "tn"])
def test_k_sweep(ops, tile, form):
    """130 x 168 over every k-depth from fewer k-tiles than ring stages to 7 (13) of them, with and without a k-tail."""
    for c in ksweep_cases(form):
        run_gemm(ops, c, f"k-sweep {tile_id(tile)}")
    if form == "nn":       # a k-contiguous A needs K % 8 == 0 (aozora_hip.h: "K, lda, ldb multiples of 8")
        for K in K_ODD:
            rejected(ops, G("nn", SWEEP_M, SWEEP_N, K))


def test_tile_edges(ops, tile):
    for c in EDGE_CASES:
        run_gemm(ops, c, f"tile edges {tile_id(tile)}")


def test_scalar_epilogue(ops, tile):
    for c in SCALAR_CASES:
        run_gemm(ops, c, f"scalar epilogue {tile_id(tile)}")


def test_rowbias(ops, tile):
    for c in ROWBIAS_CASES:
        run_gemm(ops, c, f"rowbias {tile_id(tile)}")


@pytest.mark.parametrize("form", ["nt", "nn", "tn"])
def test_strided_poisoned_operands(ops, tile, form):
    for c in STRIDE_CASES[form]:
        run_gemm(ops, c, f"strides {tile_id(tile)}")


# ---------------- split-K ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", SPLIT_MN)
@pytest.mark.parametrize("form", ["tn", "nt"])
def test_split_k(ops, tile_split, form, M, N):
    """Every split count under INKERNEL_FINISH x XCD_SPLIT (x GEMM8 for nt): exact inputs, so every setting must give the same bits."""
    cases = split_cases(form, M, N)
    for fin in (0, 1):
        for xs in (1, 0):
            for g8 in ((1, 0) if form == "nt" else (1,)):
                with options(INKERNEL_FINISH=fin, XCD_SPLIT=xs, GEMM8=g8):
                    for c in cases:
                        run_gemm(ops, c, f"split-K {tile_id(tile_split)} INKERNEL_FINISH={fin} XCD_SPLIT={xs} GEMM8={g8}")
    if form == "nt":
        rejected(ops, G("nt", M, N, 300))


@pytest.mark.parametrize("gemm8", [0, 1])
def test_nt_big_split(ops, gemm8):
    """The k-split 256-row product of gemm_impl (`big_split`).  Both paths give the same bits, so the preconditions of the path are
    made to hold here rather than observed: no forced tile, no row bias, split_k = 1, LDS_EXCLUSIVE = 0 (so NT_SPLIT_BIG is the knob
    read), K % 64 == 0 and K >= NT_SPLIT_MINK, a vector-shaped output and residual, a workspace that holds the slabs, and a grid
    whose best (width, splits) pair scores >= 0.7 -- big_split_score restates that arithmetic."""
    assert big_split_score(BIG_SPLIT_CASES[0], 4, gemm8)[0] < 0.7 <= big_split_score(BIG_SPLIT_CASES[1], 4, gemm8)[0]
    assert big_split_score(BIG_SPLIT_CASES[1], 4, gemm8)[1:] == (4, 256)
    ws = ops.workspace(torch.device(DEV)).splitk
    assert ws.data_ptr() % 16 == 0 and all(4 * c.M * c.N * 4 <= ws.numel() * 4 - 16384 for c in BIG_SPLIT_CASES)
    with options(NT_SPLIT_BIG=4, NT_SPLIT_MINK=2048, GEMM8=gemm8, LDS_EXCLUSIVE=0, INKERNEL_FINISH=0):
        for c in BIG_SPLIT_CASES:
            assert c.form == "nt" and c.split == 1 and not c.rps and c.K % 64 == 0 and c.K >= 2048 and c.N % 8 == 0 and not (c.pc or c.c_off or c.r_off or c.pr)
            run_gemm(ops, c, f"NT_SPLIT_BIG=4 NT_SPLIT_MINK=2048 GEMM8={gemm8}")


@pytest.mark.parametrize("gemm8", [0, 1])
def test_big_fill_heuristic_tiles(ops, gemm8):
    """BIG_FILL = 0: the heuristic itself picks the 256-row tile (16 waves, or the 8-wave ping-pong kernel) without a force."""
    with options(BIG_FILL=0, GEMM8=gemm8):
        run_gemm(ops, BIG_FILL_CASE, f"BIG_FILL=0 GEMM8={gemm8}")


# ---------------- grouped launches -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exclusive", [0, 1])
@pytest.mark.parametrize("M", NTG_M)
def test_nt_grouped(ops, M, exclusive):
    for K in NTG_K:
        d = make_nt_grouped(M, K)
        a = dev_in(d["a"], K + 8)
        Wd = [dev_in(w, K + 8 * (i % 2)) for i, w in enumerate(d["ws"])]
        bd = [b.to(DEV) if b is not None else None for b in d["bs"]]
        outs = [Out(R.expected_bits(ref), N + 8 + 8 * (i % 2), lead=1, tail=1) for i, (N, (ref, _)) in enumerate(zip(NTG_WIDTHS, d["refs"]))]
        recs, tiles = [], 0
        for w, b, o in zip(Wd, bd, outs):
            recs.append([w.data_ptr(), o.view().data_ptr(), b.data_ptr() if b is not None else 0, w.shape[0], w.stride(0), o.view().stride(0), tiles])
            tiles += (w.shape[0] + 159) // 160
        table = torch.tensor(recs, dtype=torch.int64, device=DEV)
        with options(LDS_EXCLUSIVE=exclusive):
            ops.gemm_nt_grouped(a, table, len(recs), tiles)
        for N, o in zip(NTG_WIDTHS, outs):
            o.check(f"nt grouped M={M} K={K} LDS_EXCLUSIVE={exclusive} group N={N}")


@pytest.mark.parametrize("with_bias", [False, True])
def test_tn_grouped(ops, with_bias):
    d = make_tn_grouped(with_bias)
    jobs, outs, bouts = [], [], []
    for i, ((dy, x, prev, bold), (ref, _, bref, _)) in enumerate(zip(d["jobs"], d["refs"])):
        M, N = prev.shape
        off = 4 if i == 2 else 0           # (200, 136, 300): dW at an 8-byte offset -> vec = 0, the scalar epilogue
        o = Out(R.expected_bits(ref), off + N + 8 - off, lead=1, tail=1, col_offset=off, prev=prev)
        bo = flat_out(R.expected_bits(bref), prev=bold) if bold is not None else None
        jobs.append((dev_in(dy, R.up8(M) + 8, 0, 1), dev_in(x, R.up8(N) + 16, 0, 1), o.view(), bo.view().view(-1) if bo is not None else None))
        outs.append(o); bouts.append(bo)
    tab = ops.tn_group_table(jobs, torch.device(DEV))
    vecs = sorted(int(v) for v in tab[0][:, 14].tolist())
    assert vecs.count(0) >= 1 and vecs.count(1) >= 1, f"both epilogues must run: vec flags {vecs}"
    ops.gemm_tn_grouped(*tab)
    for (M, N, K), o, bo in zip(TNG_PRODUCTS, outs, bouts):
        o.check(f"tn grouped {M}x{N}x{K} bias={with_bias}")
        if bo is not None:
            bo.check(f"tn grouped {M}x{N}x{K} bias gradient")


# ---------------- fused GEGLU forward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", GEGLU_M)
def test_geglu_fwd(ops, tile_geglu, M):
    for H in GEGLU_H:
        for K in GEGLU_K:
            for with_bias in (True, False):
                d = make_geglu(M, H, K, with_bias)
                name = f"fused GEGLU {tile_id(tile_geglu)} M={M} H={H} K={K} bias={with_bias}"
                proj = Out(d["want"], 2 * H + 8, lead=1, tail=1)
                oemb = R.embed(torch.full((M, H), R.POISON, dtype=BF16), H + 16, 1, 1)
                obuf = oemb.buf.to(DEV)
                ops.gemm_geglu_fwd(dev_in(d["x"], K + 8), dev_in(d["w"], K + 8), d["bias"].to(DEV) if with_bias else None, proj.view(), oemb.view(obuf))
                proj.check(name + " proj")
                got = oemb.view(obuf).cpu().double()
                err = (got - d["out"]).abs()
                bad = ~(err <= d["bound"])
                if bool(bad.any()):
                    m, n = (int(v) for v in bad.nonzero()[0])
                    raise AssertionError(f"{name} out: {int(bad.sum())} outside the bound, first at ({m}, {n}): got {float(got[m, n])!r} "
                                         f"expected {float(d['out'][m, n])!r} bound {float(d['bound'][m, n]):.3g}")
                assert oemb.guards_intact(obuf), name + ": a sentinel around `out` was overwritten"


# ---------------- convolutions ---------------------------------------------------------------------------------------------------------
def _conv_dev(c, d):
    if ("conv", c) in _DEV:
        return _DEV[("conv", c)]
    B, H, W, Cin, Cout, ks = c.B, c.H, c.W, c.Cin, c.Cout, c.ks
    Ho, Wo = d["Ho"], d["Wo"]
    cpad = R.up8(Cout)
    g = dict(cpad=cpad)
    g["x"] = dev_nhwc(d["x"])                           # pixel stride Cin + 8, poisoned
    g["w"] = d["w"].to(DEV)
    g["wt"] = d["w"].permute(3, 1, 2, 0).contiguous().to(DEV)
    g["bias"], g["rowbias"] = d["bias"].to(DEV), dev_in(d["rowbias"], Cout + 8)
    g["res"] = d["res"].to(DEV)
    # dY [B][Ho][Wo][cpad]: the channels from cout_real to cpad are poisoned (dgrad: their weights do not exist and count as zero;
    # wgrad: they are the elements m >= M of the last 8-chunk of a transposed-A row)
    dy = dev_in(d["dy"].reshape(-1, Cout), cpad)
    g["dy_pad"] = dy.as_strided((B, Ho, Wo, cpad), (Ho * Wo * cpad, Wo * cpad, cpad, 1))
    g["y"] = Out(R.expected_bits(d["y"]), Cout + 8, lead=1, tail=1, shape=(B, Ho, Wo, Cout))
    g["dw"] = flat_out(R.expected_bits(d["dw"]), prev=d["dwprev"])
    g["bg"] = flat_out(R.expected_bits(d["bg"]), prev=d["bold"])
    g["seg"] = flat_out(R.expected_bits(d["seg"]))
    if "dx" in d:
        g["dxres"] = dev_nhwc(d["dxres"])
        for k, prev in (("dx", None), ("dx_acc", d["dxprev"]), ("dx_res", None)):
            g[k] = Out(R.expected_bits(d[k]), Cin + 8, lead=1, tail=1, prev=prev, shape=(B, H, W, Cin))
    _DEV[("conv", c)] = g
    return g


def run_conv(ops, c, what):
    d = make_conv(c)
    g = _conv_dev(c, d)
    name = f"{what} {c._asdict()}"
    ups = d["ups"] is not None
    y = g["y"].reset()
    ops.conv_fwd(g["x"], g["w"], y.view(), stride=c.stride, bias=g["bias"], rowbias=g["rowbias"], residual=g["res"], upsample=ups)
    y.check(name + " forward")
    if "dx" in d:
        for wt in ((False, True) if c.Cout % 8 == 0 else (False,)):
            for k, kw in (("dx", {}), ("dx_acc", dict(accumulate=True)), ("dx_res", dict(residual=g["dxres"]))):
                o = g[k].reset()
                if wt:
                    ops.conv_dgrad_wt(g["dy_pad"], g["wt"], o.view(), stride=c.stride, **kw)
                else:
                    ops.conv_dgrad(g["dy_pad"], g["w"], o.view(), stride=c.stride, cout_real=c.Cout, **kw)
                o.check(name + f" dgrad{'_wt' if wt else ''} {k}")
    with_seg = (d["Ho"] * d["Wo"]) % 64 == 0
    for fin in (0, 1):
        with options(INKERNEL_FINISH=fin):
            for split in CONV_SPLITS:
                dw = g["dw"].reset()
                ops.conv_wgrad(g["dy_pad"], g["x"], dw.view(), stride=c.stride, cout_real=c.Cout, accumulate=True, split_k=split, upsample=ups)
                dw.check(name + f" wgrad split={split} INKERNEL_FINISH={fin}")
                dw.reset(); bg = g["bg"].reset(); seg = g["seg"].reset() if with_seg else None
                ops.conv_wgrad(g["dy_pad"], g["x"], dw.view(), stride=c.stride, cout_real=c.Cout, accumulate=True, split_k=split,
                               bias_grad=bg.view().view(-1), seg_grad=seg.view().view(-1) if seg is not None else None, upsample=ups)
                dw.check(name + f" wgrad + sums split={split} INKERNEL_FINISH={fin}")
                bg.check(name + f" bias gradient split={split} INKERNEL_FINISH={fin}")
                if seg is not None:
                    seg.check(name + f" per-sample sums split={split} INKERNEL_FINISH={fin}")


@pytest.mark.parametrize("grid", CONV_GRIDS, ids=lambda g: "grid%dx%dx%d" % g)
def test_conv(ops, tile, grid):
    for ch in CONV_TABLE[grid]:
        run_conv(ops, ConvCase(*grid, *ch), f"conv {tile_id(tile)}")


@pytest.mark.parametrize("src", UPS_SOURCES, ids=lambda g: "src%dx%dx%d" % g)
def test_conv_upsample_gather(ops, tile, src):
    """Forward and weight gradient through the nearest-2x gather, even and cropped (2n - 1) targets on each axis independently."""
    for c in ups_cases(src):
        run_conv(ops, c, f"upsample conv {tile_id(tile)}")


# ---------------- Gaussian layer: cancellation and exponent spread under the derived bound -------------------------------------------------
OBSERVED = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    """AZ_GEMM_EXCESS_REPORT=path: the largest excess per family, in units of n 2^-24 S (profiles/gemm_exact_excess.json)."""
    yield
    path = os.environ.get("AZ_GEMM_EXCESS_REPORT")
    if path and OBSERVED:
        with open(path, "w") as f:
            json.dump(OBSERVED, f, indent=1, sort_keys=True)


def within(got, ref, S, n, family, name):
    got, ref, S = got.detach().cpu().double().reshape(-1), ref.reshape(-1), S.reshape(-1)
    assert torch.isfinite(got).all(), name + ": non-finite output"
    x = R.excess(got, ref, S, n)
    OBSERVED[family] = max(OBSERVED.get(family, 0.0), x)
    print(f"{name}: excess {x:.4f} x n 2^-24 S (n = {n})")
    bad = (got - ref).abs() > R.gauss_bound(ref, S, n)
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} outside 2^-8 |ref| + 2 n 2^-24 S; first at flat {i}: got "
                             f"{float(got[i])!r} expected {float(ref[i])!r}; needed {x:.2f} n 2^-24 S (allowed 2)")


GAUSS_GEMM = [G("nt", 130, 168, 392, bias=True, res=True), G("nn", 130, 168, 104, acc=True),      # nn: K = 100 is refused (K % 8), 104 stands in
              G("tn", 200, 136, 1000, acc=True, split=3)]
GAUSS_CONV = ConvCase(3, 5, 7, 72, 40, 3, 1)


@pytest.mark.parametrize("c", GAUSS_GEMM, ids=lambda c: c.form)
def test_gaussian_gemm(ops, tile_gauss, c):
    d, g = run_gemm(ops, c, "gaussian", gaussian=True)
    n = c.K + int(c.bias) + int(c.res) + int(c.acc) + (3 if c.split > 1 else 1)
    within(g["out"].view(), d["ref"], d["S"], n, "gemm_" + c.form, f"gaussian {c.form} {c.M}x{c.N}x{c.K} {tile_id(tile_gauss)}")
    guard = g["out"].buf.clone()
    g["out"].emb.view(guard).copy_(g["out"].emb.view(g["out"].pristine))
    assert torch.equal(ibits(guard), ibits(g["out"].pristine)), "sentinel overwritten"


def test_gaussian_conv(ops, tile_gauss):
    c = GAUSS_CONV
    d = make_conv(c, gaussian=True)
    B, H, W, Cin, Cout = c.B, c.H, c.W, c.Cin, c.Cout
    x, w, dy = d["x"].to(DEV), d["w"].to(DEV), d["dy"].to(DEV)
    t = tile_id(tile_gauss)
    y = torch.empty(B, H, W, Cout, dtype=BF16, device=DEV)
    ops.conv_fwd(x, w, y, stride=1, bias=d["bias"].to(DEV), rowbias=d["rowbias"].to(DEV), residual=d["res"].to(DEV))
    within(y, d["y"], d["yS"], 9 * Cin + 3 + 1, "conv_fwd", f"gaussian conv forward {t}")
    dx = d["dxprev"].to(DEV).clone()
    ops.conv_dgrad(dy, w, dx, stride=1, cout_real=Cout, accumulate=True)
    within(dx, d["dx_acc"], d["dx_accS"], 9 * Cout + 1 + 1, "conv_dgrad", f"gaussian conv dgrad {t}")
    for split in (1, 2):
        dw = d["dwprev"].to(DEV).clone()
        ops.conv_wgrad(dy, x, dw, stride=1, cout_real=Cout, accumulate=True, split_k=split)
        within(dw, d["dw"], d["dwS"], B * H * W + 1 + split, "conv_wgrad", f"gaussian conv wgrad split={split} {t}")
