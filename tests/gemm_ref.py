"""Float64 restatements of every entry point of aozora_sdxl_training_amd/csrc/az_gemm.hip (plain, split-K, grouped and GEGLU-fused products, the implicit-GEMM
convolutions with their gathers) on inputs whose result is EXACT in fp32 whatever the summation order.  The product never imports
this file; tests/test_gemm_exact_gpu.py compares the HIP kernels against it bit for bit and tests/test_gemm_ref_cpu.py checks it
without a GPU.  Plain torch on the CPU.

Exactly summable inputs.  Every operand element (A, B, bias, rowbias, residual, dY) is a multiple of 2^-2 in [-4, 4]: 33 values of at
most 5 significant bits, all bf16-exact.  The previous contents of an accumulated output use [-8, 8].  Every product is then a
multiple of 2^-4, and so is every partial sum of products and epilogue terms, in any order and any grouping (tiles, k-splits, slabs,
MFMA-internal adders).  With S = sum |a||b| + |bias| + |rowbias| + |residual| + |prev| of an output element every such partial sum
is at most S in magnitude, i.e. an integer multiple of 2^-4 below 2^24 * 2^-4 when 16 S < 2^24: representable in fp32.  Nothing
rounds before the one store, so the expected output is a single bit pattern: ref.float().bfloat16(), round to nearest even, which
is what f2bf in az_common.h does.  `exact_ok(S)` asserts the condition; every reference function calls it and returns S.

Gaussian inputs (a second, smaller layer for cancellation and exponent spread) come with the derived bound
    |out - ref| <= 2^-8 |ref| + 2 n 2^-24 S,     n = K + (number of epilogue terms) + ksplit:
n 2^-24 S is the worst case of n round-to-nearest fp32 additions in any order, the factor 2 is margin for the MFMA's internal
adder (its rounding is not documented), 2^-8 |ref| is the one bf16 rounding.  `excess` reports what an output needed in units of
n 2^-24 S: above 1.0 is more than the round-to-nearest worst case (a finding), above 2.0 fails."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import elem_ref        # noqa: E402

U_F32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
POISON = 3.0 * 2.0 ** 40          # finite and bf16-exact: times a masked (zero-filled) partner it is 0, where NaN would stay NaN


# ---------------- inputs -------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def quarters(shape, seed, lim=4):
    """bf16 multiples of 2^-2 in [-lim, lim]."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return (torch.randint(-4 * lim, 4 * lim + 1, shape, generator=gen(seed)).double() * 0.25).bfloat16()


def gauss(shape, seed, scale=1.0):
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return (scale * torch.randn(*shape, generator=gen(seed))).bfloat16()


def exact_ok(S):
    """Every partial sum of the terms behind S is fp32-exact: 16 S < 2^24."""
    m = float(S.max()) if S.numel() else 0.0
    assert 16.0 * m < 2.0 ** 24, f"inputs are not exactly summable in fp32: max S = {m}"
    return True


def expected_bits(ref):
    """The one bf16 bit pattern of an exact result: round to nearest even (f2bf)."""
    return ref.float().bfloat16()


def inexact_share(ref):
    """Share of the outputs that are not bf16-representable (so that the store's rounding is exercised)."""
    return float((ref.float().bfloat16().double() != ref).double().mean())


def bits(t):
    return t.contiguous().view(torch.int16)


def first_mismatch(got, want):
    """None when two bf16 tensors agree bit for bit, else 'index got expected' of the first differing element."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    ne = bits(got) != bits(want)
    if not bool(ne.any()):
        return None
    idx = tuple(int(v) for v in ne.nonzero()[0])
    return f"{int(ne.sum())} of {ne.numel()} wrong, first at {idx}: got {float(got[idx])!r} expected {float(want[idx])!r}"


# ---------------- plain products -----------------------------------------------------------------------------------------------
def _finish(P, S, exact):
    if exact:
        exact_ok(S)
    return P, S


def gemm(form, a, b, bias=None, rowbias=None, rows_per_seg=0, residual=None, prev=None, exact=True):
    """C[M][N] = op(a) op(b) (+ bias[n]) (+ rowbias[m // rows_per_seg][n]) (+ residual) (+ prev).
    nt: a [M][K], b [N][K];  nn: a [M][K], b [K][N];  tn: a [K][M], b [K][N].  -> (ref float64, S)."""
    A, B = a.double(), b.double()
    if form == "nt":
        P, S = A @ B.t(), A.abs() @ B.abs().t()
    elif form == "nn":
        P, S = A @ B, A.abs() @ B.abs()
    else:
        assert form == "tn", form
        P, S = A.t() @ B, A.abs().t() @ B.abs()
    if bias is not None:
        P, S = P + bias.double(), S + bias.double().abs()
    if rowbias is not None:
        seg = torch.arange(P.shape[0]) // rows_per_seg
        rb = rowbias.double()[seg]
        P, S = P + rb, S + rb.abs()
    if residual is not None:
        P, S = P + residual.double(), S + residual.double().abs()
    if prev is not None:
        P, S = P + prev.double(), S + prev.double().abs()
    return _finish(P, S, exact)


def bias_grad(dy, n_real, bias_old, exact=True):
    """bias_old[n_real] + dY[K][M].sum(0)[:n_real] -> (ref, S)."""
    d = dy.double()
    return _finish(bias_old.double() + d.sum(0)[:n_real], bias_old.double().abs() + d.abs().sum(0)[:n_real], exact)


def nt_grouped(a, ws, biases):
    """C_g = a . W_g^T (+ bias_g) for every group -> list of (ref, S)."""
    return [gemm("nt", a, w, bias=b) for w, b in zip(ws, biases)]


def tn_grouped(jobs):
    """jobs: (dy [K][M], x [K][N], prev [M][N], bias_old [n_real] or None) -> list of (ref, S, bias ref or None, bias S or None)."""
    out = []
    for dy, x, prev, bold in jobs:
        r, s = gemm("tn", dy, x, prev=prev)
        br, bs = bias_grad(dy, bold.numel(), bold) if bold is not None else (None, None)
        out.append((r, s, br, bs))
    return out


def geglu_fwd(x, w, bias):
    """proj[M][2H] = x . w^T + bias (exact) and out[M][H] = value * gelu(gate) of the bf16-ROUNDED projection (az_gemm.hip computes
    out from the rounded projection: bit for bit az_gemm_bf16 followed by az_geglu_fwd).  -> (proj ref, S, out ref, out bound)."""
    proj, S = gemm("nt", x, w, bias=bias)
    out, So = elem_ref.geglu_fwd_ref(expected_bits(proj))
    return proj, S, out, elem_ref.bound(out, So, "geglu_out")


# ---------------- convolutions -------------------------------------------------------------------------------------------------
def conv_out(n, ks, stride):
    pad = 1 if ks == 3 else 0
    return (n + 2 * pad - ks) // stride + 1


def conv_index(B, H, W, ks, stride, ups=False, fault=None):
    """Gather table of the implicit GEMM: idx[B*Ho*Wo][ks*ks] = flat source pixel ((b * Hs + y) * Ws + x) of tap (ky, kx) of an
    output pixel, -1 where the tap falls on the zero padding.  H, W: extents of the conv's input; ups: that input is the nearest
    upsample (pixel (y >> 1, x >> 1)) of a stored [ceil(H/2)][ceil(W/2)] grid, H / W odd = the 2x image cropped by one.
    fault: 'neighbour' -- a tap past the bottom edge is not padding but continues into the flat pixel sequence (the next sample's
    first row); 'crop_row' -- row H - 2 of a cropped upsample is read at (y >> 1) + 1."""
    pad = 1 if ks == 3 else 0
    Ho, Wo = conv_out(H, ks, stride), conv_out(W, ks, stride)
    Hs, Ws = ((H + 1) >> 1, (W + 1) >> 1) if ups else (H, W)
    b = torch.arange(B).view(B, 1, 1, 1, 1)
    oy = torch.arange(Ho).view(1, Ho, 1, 1, 1)
    ox = torch.arange(Wo).view(1, 1, Wo, 1, 1)
    ky = torch.arange(ks).view(1, 1, 1, ks, 1)
    kx = torch.arange(ks).view(1, 1, 1, 1, ks)
    iy, ix = oy * stride + ky - pad, ox * stride + kx - pad
    ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    sy, sx = (iy >> 1, ix >> 1) if ups else (iy, ix)
    if fault == "crop_row":
        assert ups and H % 2 == 1 and H >= 3
        sy = torch.where(iy == H - 2, sy + 1, sy)          # the last row whose neighbour (y >> 1) + 1 still exists in the source
    src = (b * Hs + sy) * Ws + sx
    if fault == "neighbour":
        ok = ok | ((iy == H) & (ix >= 0) & (ix < W) & (b < B - 1))
    idx = torch.where(ok, src, torch.full_like(src, -1))
    return idx.expand(B, Ho, Wo, ks, ks).reshape(B * Ho * Wo, ks * ks)


def _im2col(x2, idx):
    """x2 [pixels][Cin] float64, idx [P][taps] -> [P][taps * Cin] with zeros where idx < 0."""
    z = torch.cat([x2, torch.zeros(1, x2.shape[1], dtype=x2.dtype)], 0)
    return z[idx].reshape(idx.shape[0], -1)


def conv_fwd(x, w, stride, bias=None, rowbias=None, residual=None, out_hw=None, fault=None, exact=True):
    """x [B][Hs][Ws][Cin], w [Cout][ks][ks][Cin] -> y [B][Ho][Wo][Cout] (+ bias[co]) (+ rowbias[b][co]) (+ residual).
    out_hw: (H, W) = the extents x is nearest-upsampled to in front of the conv (2Hs or 2Hs - 1, 2Ws or 2Ws - 1); None: no upsample."""
    B, Hs, Ws, Cin = x.shape
    Cout, ks = w.shape[0], w.shape[1]
    H, W = out_hw if out_hw is not None else (Hs, Ws)
    idx = conv_index(B, H, W, ks, stride, ups=out_hw is not None, fault=fault)
    Ho, Wo = conv_out(H, ks, stride), conv_out(W, ks, stride)
    cols = _im2col(x.double().reshape(-1, Cin), idx)
    rb = rowbias.double().reshape(B, -1)[:, :Cout] if rowbias is not None else None
    res = residual.double().reshape(B * Ho * Wo, Cout) if residual is not None else None
    P, S = gemm("nt", cols, w.double().reshape(Cout, -1), bias=bias, rowbias=rb, rows_per_seg=Ho * Wo, residual=res, exact=exact)
    return P.reshape(B, Ho, Wo, Cout), S.reshape(B, Ho, Wo, Cout)


def conv_dgrad(dy, w, stride, in_hw, prev=None, residual=None, exact=True):
    """dy [B][Ho][Wo][>= Cout] (channels from Cout on are ignored), w [Cout][3][3][Cin] -> dx [B][H][W][Cin] (+ prev) (+ residual)."""
    B, Ho, Wo, _ = dy.shape
    Cout, ks, Cin = w.shape[0], w.shape[1], w.shape[3]
    H, W = in_hw
    idx = conv_index(B, H, W, ks, stride)
    d, wf = dy.double()[..., :Cout].reshape(-1, Cout), w.double().reshape(Cout, -1)
    out = []
    for dd, ww in ((d, wf), (d.abs(), wf.abs())):
        G = (dd @ ww).reshape(-1, Cin)                                        # [P * taps][Cin]: what each tap sends back to its source pixel
        acc = torch.zeros(B * H * W + 1, Cin, dtype=torch.float64)
        acc.index_add_(0, torch.where(idx < 0, torch.full_like(idx, B * H * W), idx).reshape(-1), G)
        out.append(acc[:-1].reshape(B, H, W, Cin))
    P, S = out
    for t in (prev, residual):
        if t is not None:
            P, S = P + t.double(), S + t.double().abs()
    return _finish(P, S, exact)


def conv_wgrad(dy, x, ks, stride, cout, prev=None, out_hw=None, fault=None, exact=True):
    """dw [Cout][ks][ks][Cin] = dy[..., :Cout]^T . im2col(x) (+ prev)."""
    B, Hs, Ws, Cin = x.shape
    H, W = out_hw if out_hw is not None else (Hs, Ws)
    idx = conv_index(B, H, W, ks, stride, ups=out_hw is not None, fault=fault)
    cols = _im2col(x.double().reshape(-1, Cin), idx)
    d = dy.double()[..., :cout].reshape(-1, cout)
    P, S = gemm("tn", d, cols, prev=prev.reshape(cout, -1) if prev is not None else None, exact=exact)
    return P.reshape(cout, ks, ks, Cin), S.reshape(cout, ks, ks, Cin)


def conv_sums(dy, cout, bias_old=None, exact=True, fault=None):
    """Per-sample channel sums seg[b][co] of dy[..., :Cout] and bias_old + their total -> (seg ref, seg S, bias ref, bias S).
    fault 'segment': the first 64-pixel k-tile of sample 1 is counted in sample 0."""
    d = dy.double()[..., :cout].reshape(dy.shape[0], -1, cout)
    seg, Sseg = d.sum(1), d.abs().sum(1)
    if fault == "segment":
        assert d.shape[0] > 1 and d.shape[1] >= 64
        t = d[1, :64].sum(0)
        seg = seg.clone(); seg[0] += t; seg[1] -= t
    tot, Stot = seg.sum(0), Sseg.sum(0)
    if bias_old is not None:
        tot, Stot = tot + bias_old.double(), Stot + bias_old.double().abs()
    if exact:
        exact_ok(Stot)
    return seg, Sseg, tot, Stot


# ---------------- poisoned embedding --------------------------------------------------------------------------------------------
class Embedded:
    """A 2-D operand [rows][cols] inside a larger allocation [lead + rows + tail][ld] whose every other element is `poison`."""

    def __init__(self, t, ld, lead_rows=0, tail_rows=0, col_offset=0, poison=POISON):
        rows, cols = t.shape
        assert col_offset + cols <= ld, (col_offset, cols, ld)
        self.rows, self.cols, self.ld, self.lead, self.off, self.poison = rows, cols, ld, lead_rows, col_offset, poison
        self.buf = torch.full((lead_rows + rows + tail_rows, ld), poison, dtype=t.dtype)
        self.view(self.buf).copy_(t)

    def view(self, buf=None):
        buf = self.buf if buf is None else buf
        return buf[self.lead:self.lead + self.rows, self.off:self.off + self.cols]

    def byte_offset(self):
        return (self.lead * self.ld + self.off) * self.buf.element_size()

    def guards_intact(self, buf=None):
        """Every element outside the logical extent still holds the poison, bit for bit."""
        buf = (self.buf if buf is None else buf).detach().cpu()
        mask = torch.ones(buf.shape, dtype=torch.bool)
        self.view(mask).fill_(False)
        want = torch.full((1,), self.poison, dtype=buf.dtype)
        return bool((bits(buf)[mask] == bits(want)[0]).all())


def embed(t, ld, lead_rows=0, tail_rows=0, col_offset=0, poison=POISON):
    """Place t [rows][cols] at row lead_rows, column col_offset of a [lead + rows + tail][ld] allocation filled with `poison`.
    Poison is put only where include/aozora_hip.h lets a kernel ignore memory: the columns between the logical width and the
    leading dimension, the rows before and after the operand (and with them the elements m >= M of the last 8-chunk of a transposed
    A row, and dY's channels from cout_real to cpad).  Where the header asks for zeros (the activation pad channels that Cin counts,
    the W operand's own extent) the caller keeps zeros."""
    return Embedded(t, ld, lead_rows, tail_rows, col_offset, poison)


def up8(v):
    return (v + 7) // 8 * 8


# ---------------- Gaussian layer: derived bound ------------------------------------------------------------------------------------
def gauss_bound(ref, S, n):
    return U_BF16 * ref.abs() + 2.0 * n * U_F32 * S


def excess(out, ref, S, n):
    """What an output needed beyond its bf16 rounding, in units of n 2^-24 S (the worst case of n round-to-nearest fp32 additions):
    max over elements of (|out - ref| - 2^-8 |ref|) / (n 2^-24 S), >= 0.  The bound allows 2.0."""
    d = (out.double() - ref).abs() - U_BF16 * ref.abs()
    r = d / (n * U_F32 * S).clamp_min(1e-300)
    return max(float(r.max()), 0.0) if r.numel() else 0.0


# ---------------- seeded faults: a kernel's output with one defect ---------------------------------------------------------------
def store_truncating(ref):
    """bf16 store that truncates instead of rounding to nearest even."""
    return (ref.float().view(torch.int32) & -65536).view(torch.float32).bfloat16()


def fault_truncating_store(a, b, bias, residual):
    return store_truncating(gemm("nt", a, b, bias=bias, residual=residual, exact=False)[0])


def fault_product_rounded_first(a, b, bias, residual):
    """The product rounded to bf16 before bias and residual are added."""
    P = gemm("nt", a, b, exact=False)[0].float().bfloat16().double()
    return expected_bits(P + bias.double() + residual.double())


def fault_k_chunk_dropped(a, b, bias, residual, row=-1):
    """The last 8-deep k-chunk dropped in one row (the last by default)."""
    ref = gemm("nt", a, b, bias=bias, residual=residual, exact=False)[0].clone()
    ref[row] -= a[row, -8:].double() @ b[:, -8:].double().t()
    return expected_bits(ref)


def fault_term_scaled(a, b, bias, residual):
    """residual x 0.98 in the last 8-column piece of the last row."""
    r2 = residual.double().clone()
    r2[-1, -8:] *= 0.98
    return expected_bits(gemm("nt", a, b, bias=bias, exact=False)[0] + r2)


def _slabs(a, b, nslab):
    K = a.shape[1]
    per = -(-(-(-K // 64)) // nslab) * 64
    return [gemm("nt", a[:, k:k + per], b[:, k:k + per], exact=False)[0] for k in range(0, K, per)]


def fault_bf16_slabs(a, b, bias, residual, nslab=4):
    """Split-K slabs kept in bf16 instead of fp32."""
    P = sum(s.float().bfloat16().double() for s in _slabs(a, b, nslab))
    return expected_bits(P + bias.double() + residual.double())


def fault_slab_skipped(a, b, bias, residual, nslab=3):
    """The last split-K slab left out of the reduce."""
    P = sum(_slabs(a, b, nslab)[:-1])
    return expected_bits(P + bias.double() + residual.double())


FIRST_FIVE_FAULTS = [fault_truncating_store, fault_product_rounded_first, fault_k_chunk_dropped, fault_term_scaled, fault_bf16_slabs]
