"""Tensor-level wrappers over the C ABI (include/aozora_hip.h).

PyTorch is used only for device memory and streams: every function checks operand shapes,
strides, dtypes and alignment on the host (a faulting kernel can take the whole node down), then
passes raw pointers and the current HIP stream to libaozora_hip.so.  No function here has a CPU
or eager-PyTorch fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from ._lib import lib, AozoraError

BF16 = torch.bfloat16
F32 = torch.float32


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(cond, msg):
    if not cond:
        raise AozoraError("operand check failed: " + msg)


def _rows(t: torch.Tensor, dtype=BF16):
    """2-D row-major view check -> (rows, cols, ld)."""
    _req(t.is_cuda and t.dtype == dtype, f"need cuda {dtype} tensor, got {t.device} {t.dtype}")
    _req(t.dim() == 2 and t.stride(1) == 1, f"need 2-D tensor with unit inner stride, got {tuple(t.shape)} {t.stride()}")
    return t.shape[0], t.shape[1], t.stride(0)


def as3(t: torch.Tensor, B, HW):
    """[B*HW][C] row view (any row stride) -> (B,HW,C) view."""
    ld = t.stride(0)
    return t.as_strided((B, HW, t.shape[1]), (HW * ld, ld, 1))


def as4(t: torch.Tensor, B, H, W_):
    """[B*H*W][C] row view (any row stride) -> (B,H,W,C) view."""
    ld = t.stride(0)
    return t.as_strided((B, H, W_, t.shape[1]), (H * W_ * ld, W_ * ld, ld, 1))


class Profiler:
    """Brackets every ABI launch with HIP events on the stream it runs on and aggregates by op class
    (bench.py uses it for the per-kernel roofline; tests never enable it)."""

    def __init__(self):
        self.rec = []

    def add(self, key, flops, nbytes, e0, e1):
        self.rec.append((key, flops, nbytes, e0, e1))

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        ms = ctypes.c_float()
        for key, flops, nbytes, e0, e1 in self.rec:
            lib().call("az_event_elapsed_ms", e0, e1, ctypes.byref(ms))
            d = out.setdefault(key, dict(calls=0, ms=0.0, flops=0.0, bytes=0.0))
            d["calls"] += 1; d["ms"] += ms.value; d["flops"] += flops; d["bytes"] += nbytes
            lib().call("az_event_destroy", e0); lib().call("az_event_destroy", e1)
        self.rec = []
        return out


PROFILER: Optional[Profiler] = None
PROFILE_SHAPES = False


class _prof:
    def __init__(self, key, flops=0.0, nbytes=0.0):
        self.key, self.flops, self.nbytes = key, flops, nbytes

    def __enter__(self):
        if PROFILER is not None:
            self.e0, self.e1 = ctypes.c_void_p(), ctypes.c_void_p()
            lib().call("az_event_create", ctypes.byref(self.e0)); lib().call("az_event_create", ctypes.byref(self.e1))
            lib().call("az_event_record", self.e0, _stream())
        return self

    def __exit__(self, *a):
        if PROFILER is not None:
            lib().call("az_event_record", self.e1, _stream())
            PROFILER.add(self.key, self.flops, self.nbytes, self.e0, self.e1)
        return False


class Workspace:
    """Per-device scratch owned by the caller side of the ABI (allocated once; graph-capture safe)."""

    def __init__(self, device, splitk_bytes: int = 192 << 20, scratch_floats: int = 64 << 20, attn_bytes: int = 96 << 20):
        self.device = device
        # GEMM / conv workspace: split-K slabs, column-sum slots and -- in its last 16 KiB -- the arrival counters of the
        # in-kernel finish, which must be ZERO when first handed over and are written by the library only (include/aozora_hip.h);
        # hence zeros, and a separate buffer for the attention partials
        self.splitk = torch.zeros(splitk_bytes // 4, dtype=F32, device=device)
        self.attn = torch.empty(attn_bytes // 4, dtype=F32, device=device)
        self.scratch = torch.empty(scratch_floats, dtype=F32, device=device)
        self.small = torch.zeros(4096 + 64, dtype=F32, device=device)   # [4096:] = reserved scalars


_ws = {}


_ws_slot = [0]     # 0 = main stream, 1 = the executor's forked wgrad stream (own scratch: no sharing hazards)


def set_workspace_slot(slot: int):
    _ws_slot[0] = slot


def workspace(device=None) -> Workspace:
    device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (device, _ws_slot[0])
    if key not in _ws:
        _ws[key] = Workspace(device)
    return _ws[key]


# ---------------------------------------------------------------------------------------------
# GEMM / conv
# ---------------------------------------------------------------------------------------------

def gemm(a, b, out, *, trans_a=False, trans_b=True, bias=None, rowbias=None, rows_per_seg=0, residual=None,
         accumulate=False, split_k=1, bias_grad=None):
    """out[M,N] (+)= op(a) @ op(b) (+bias) (+rowbias[m // rows_per_seg]) (+residual). See az_gemm_bf16.
    bias_grad (weight-gradient form trans_a=True, trans_b=False only): bf16 [M], += column sums of `a` in the same pass."""
    ar, ac, lda = _rows(a)
    br, bc, ldb = _rows(b)
    M, K = (ac, ar) if trans_a else (ar, ac)
    N, Kb = (br, bc) if trans_b else (bc, br)
    _req(K == Kb, f"K mismatch {K} vs {Kb}")
    _req(not (trans_a and trans_b), "transA & transB unsupported")
    om, on, ldc = _rows(out)
    _req((om, on) == (M, N), f"out shape {(om, on)} != {(M, N)}")
    _req(lda % 8 == 0 and ldb % 8 == 0, "lda/ldb must be multiples of 8")
    _req(a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0, "A/B must be 16-byte aligned")
    if not trans_a and trans_b:
        _req(K % 8 == 0, "K must be a multiple of 8")
    if trans_a:
        _req(a.shape[1] % 8 == 0 or lda >= ((M + 7) // 8) * 8, "transposed A rows must be readable in 8-element chunks")
    if not trans_b:
        _req(ldb >= ((N + 7) // 8) * 8, "B rows must be readable in 8-element chunks")
    if bias is not None:
        _req(bias.dtype == BF16 and bias.numel() == N and bias.is_contiguous(), "bias must be contiguous bf16 [N]")
    ld_rb = 0
    if rowbias is not None:
        rr, rc, ld_rb = _rows(rowbias)
        _req(rc == N and rows_per_seg > 0 and rr * rows_per_seg >= M, "rowbias shape")
    ldr = 0
    if residual is not None:
        rm, rn, ldr = _rows(residual)
        _req((rm, rn) == (M, N), "residual shape")
    ws = workspace(out.device)
    if bias_grad is not None:
        _req(trans_a and not trans_b and bias is None and rowbias is None and residual is None, "bias_grad needs the wgrad form")
        _req(bias_grad.dtype == BF16 and bias_grad.is_contiguous() and bias_grad.numel() <= M, "bias_grad must be contiguous bf16 [<=M]")
        with _prof("gemm_tn" + (f" {M}x{N}x{K}+b" if PROFILE_SHAPES else ""), 2.0 * M * N * K, 2.0 * (M * K + N * K + M * N)):
            lib().call("az_gemm_wgrad_bias_bf16", M, N, K, _ptr(a), lda, _ptr(b), ldb, _ptr(out), ldc, int(accumulate), int(split_k),
                       _ptr(ws.splitk), ws.splitk.numel() * 4, _ptr(bias_grad), bias_grad.numel(), _stream())
        return out
    with _prof("gemm_" + ("tn" if trans_a else ("nt" if trans_b else "nn")) + (f" {M}x{N}x{K}" if PROFILE_SHAPES else ""), 2.0 * M * N * K, 2.0 * (M * K + N * K + M * N)):
      lib().call("az_gemm_bf16", int(trans_a), int(trans_b), M, N, K, _ptr(a), lda, _ptr(b), ldb, _ptr(out), ldc,
               _ptr(bias), _ptr(rowbias), int(rows_per_seg), ld_rb, _ptr(residual), ldr, int(accumulate), int(split_k),
               _ptr(ws.splitk), ws.splitk.numel() * 4, _stream())
    return out


def gemm_nt_grouped(a, table, ngroups: int, total_tiles_n: int, sum_n: int = 0):
    """Many products sharing the A operand in one launch (az_gemm_nt_grouped_bf16): table = device int64 [ngroups][7]
    (W, C, bias or 0, N, ldb, ldc, first 160-wide tile column); the caller built it from tensors it checked.
    sum_n: total output columns (profiling only: algorithmic FLOPs / bytes of the launch)."""
    M, K, lda = _rows(a)
    _req(K % 8 == 0 and lda % 8 == 0 and a.data_ptr() % 16 == 0, "grouped gemm: A layout")
    with _prof("gemm_nt" + (f" grouped {M}x{sum_n}x{K} ({ngroups})" if PROFILE_SHAPES else ""), 2.0 * M * sum_n * K,
               2.0 * (M * K + sum_n * K + M * sum_n)):
        lib().call("az_gemm_nt_grouped_bf16", M, K, _ptr(a), lda, _ptr(table), int(ngroups), int(total_tiles_n), _stream())


def tn_group_table(jobs, device):
    """Record table of a grouped weight-gradient launch (az_gemm_tn_grouped_bf16).  jobs: list of (dy [K, M], x [K, N], dw [M, N],
    bias_grad bf16 [n_real <= M] or None); every operand is checked here (the records live in device memory, the library cannot).
    Products with the deepest k-range come first (their tiles start first: shorter tail).  -> (table, ngroups, total_tiles, flops, bytes)"""
    recs, tiles, flops, nbytes = [], 0, 0.0, 0.0
    for dy, x, dw, bg in sorted(jobs, key=lambda j: -j[0].shape[0]):
        K, M, lda = _rows(dy)
        Kx, N, ldb = _rows(x)
        Mw, Nw, ldc = _rows(dw)
        _req(Kx == K and (Mw, Nw) == (M, N), f"grouped wgrad shapes {tuple(dy.shape)} {tuple(x.shape)} {tuple(dw.shape)}")
        _req(lda % 8 == 0 and ldb % 8 == 0 and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0, "grouped wgrad: operand alignment")
        _req((M % 8 == 0 or lda >= ((M + 7) // 8) * 8) and ldb >= ((N + 7) // 8) * 8, "grouped wgrad: rows must be readable in 8-element chunks")
        _req((K * lda + M + 8) * 2 < 0x7FFFFFF0 and (K * ldb + N + 8) * 2 < 0x7FFFFFF0, "grouped wgrad: operand extent >= 2 GiB")
        n_real = 0
        if bg is not None:
            _req(bg.dtype == BF16 and bg.is_contiguous() and bg.numel() <= M, "grouped wgrad: bias_grad must be contiguous bf16 [<= M]")
            n_real = bg.numel()
        vec = int(N % 8 == 0 and ldc % 8 == 0 and dw.data_ptr() % 16 == 0)
        tm, tn = (M + 127) // 128, (N + 127) // 128
        recs.append([dy.data_ptr(), x.data_ptr(), dw.data_ptr(), bg.data_ptr() if bg is not None else 0, M, N, K, lda, ldb, ldc, tiles, tm, tn, n_real, vec, 0])
        tiles += tm * tn
        flops += 2.0 * M * N * K
        nbytes += 2.0 * (M * K + N * K + M * N)
    return torch.tensor(recs, dtype=torch.int64, device=device), len(recs), tiles, flops, nbytes


def gemm_tn_grouped(table, ngroups: int, total_tiles: int, flops: float = 0.0, nbytes: float = 0.0):
    """dW_g += dY_g^T X_g (+ bias gradients) for every record of `table` (tn_group_table) in ONE launch, no split-K."""
    with _prof("gemm_tn" + (f" grouped ({ngroups}) {total_tiles} tiles" if PROFILE_SHAPES else ""), flops, nbytes):
        lib().call("az_gemm_tn_grouped_bf16", _ptr(table), int(ngroups), int(total_tiles), _stream())


def gemm_geglu_fwd(x, w, bias, proj, out):
    """proj[M, 2H] = x @ w^T + bias and out[M, H] = proj[:, :H] * gelu(proj[:, H:]) in one launch (az_gemm_geglu_fwd_bf16)."""
    M, K, lda = _rows(x)
    H2, Kw, ldb = _rows(w)
    Mp, H2p, ldp = _rows(proj)
    Mo, H, ldo = _rows(out)
    _req(Kw == K and H2 == 2 * H and (Mp, Mo, H2p) == (M, M, H2) and (bias is None or bias.numel() == H2), "fused GEGLU forward shapes")
    with _prof("gemm_nt" + (f" {M}x{H2}x{K}+geglu" if PROFILE_SHAPES else ""), 2.0 * M * H2 * K, 2.0 * (M * K + H2 * K + M * H2 + M * H)):
        lib().call("az_gemm_geglu_fwd_bf16", M, H, K, _ptr(x), lda, _ptr(w), ldb, _ptr(bias), _ptr(proj), ldp, _ptr(out), ldo, _stream())
    return out


def _nhwc(t: torch.Tensor):
    """(B,H,W,C) tensor whose last dim is contiguous and whose pixel stride is uniform -> ld."""
    _req(t.is_cuda and t.dtype == BF16 and t.dim() == 4, "need cuda bf16 (B,H,W,C)")
    B, H, W, C = t.shape
    ld = t.stride(2)
    _req(t.stride(3) == 1 and t.stride(1) == W * ld and t.stride(0) == H * W * ld, f"non-uniform NHWC strides {t.stride()}")
    _req(ld % 8 == 0 and t.data_ptr() % 16 == 0, "pixel stride must be a multiple of 8 and base 16-byte aligned")
    return B, H, W, C, ld


def _upsampled_extents(H, W, t):
    """Target extents of a nearest upsample of an H x W grid, taken from the (B,Ho,Wo,C) tensor at that resolution."""
    _req(t.dim() == 4 and t.shape[1] in (2 * H - 1, 2 * H) and t.shape[2] in (2 * W - 1, 2 * W),
         f"upsample target {tuple(t.shape[1:3])} must be (2H or 2H-1, 2W or 2W-1) of the source {(H, W)}")
    return t.shape[1], t.shape[2]


def conv_fwd(x, w, out, *, stride=1, bias=None, rowbias=None, residual=None, upsample=False):
    """x (B,H,W,Cin) ; w [Cout][k][k][Cin] contiguous ; out (B,Ho,Wo,Cout).
    upsample: x is the HALF-resolution input of a nearest upsample (Upsample2D) to out's extents, each 2H or 2H - 1 / 2W or 2W - 1
    (F.interpolate(scale_factor=2) / (size=): the 2x image with its last row / column cropped); the conv reads it through the gather."""
    B, H, W, Cin, ldx = _nhwc(x)
    if upsample:
        _req(stride == 1 and w.shape[1] == 3, "the upsample gather exists for 3x3 stride-1 convolutions")
        H, W = _upsampled_extents(H, W, out)
    _req(w.dtype == BF16 and w.is_contiguous() and w.dim() == 4 and w.shape[3] == Cin and w.shape[1] == w.shape[2], "weight layout")
    Cout, ks = w.shape[0], w.shape[1]
    pad = 1 if ks == 3 else 0
    Ho = (H + 2 * pad - ks) // stride + 1
    Wo = (W + 2 * pad - ks) // stride + 1
    _req(out.is_cuda and out.dtype == BF16 and tuple(out.shape) == (B, Ho, Wo, Cout) and out.stride(3) == 1, "out shape")
    ldo = out.stride(2)
    _req(out.stride(1) == Wo * ldo and out.stride(0) == Ho * Wo * ldo, "out strides")
    ld_rb = 0
    if rowbias is not None:
        _req(rowbias.dtype == BF16 and tuple(rowbias.shape) == (B, Cout) and rowbias.stride(1) == 1, "rowbias [B][Cout]")
        ld_rb = rowbias.stride(0)
    ldr = 0
    if residual is not None:
        _req(tuple(residual.shape) == tuple(out.shape) and residual.stride(3) == 1, "residual shape")
        ldr = residual.stride(2)
    if bias is not None:
        _req(bias.dtype == BF16 and bias.numel() == Cout and bias.is_contiguous(), "bias")
    with _prof('conv_fwd' + (f' {B}x{H}x{W} {Cin}->{Cout} k{ks}s{stride}' if PROFILE_SHAPES else ''), 2.0 * B * Ho * Wo * Cout * ks * ks * Cin, 0.0):
        lib().call("az_conv2d_bf16", 16 if upsample else 0, B, H, W, Cin, Ho, Wo, Cout, ks, stride, pad, 0, _ptr(x), ldx, _ptr(w), _ptr(None), 0,
               _ptr(out), ldo, _ptr(bias), _ptr(rowbias), ld_rb, _ptr(residual), ldr, 0, 1, _ptr(None), 0, _stream())
    return out


def conv_dgrad(dy, w, dx, *, stride=1, cout_real=None, accumulate=False, residual=None):
    """dy (B,Ho,Wo,Cpad) ; w [Cout][3][3][Cin] ; dx (B,H,W,Cin) (overwritten, accumulated in place, or = residual + gradient)."""
    B, Ho, Wo, Cpad, lddy = _nhwc(dy)
    Bx, H, W, Cin, lddx = _nhwc(dx)
    Cout = w.shape[0] if cout_real is None else cout_real
    _req(w.dtype == BF16 and w.is_contiguous() and tuple(w.shape) == (Cout, 3, 3, Cin), "weight layout")
    _req(Bx == B and Cpad >= Cout and Cpad % 8 == 0, "dy/dx batch or channel padding")
    _req(Ho == (H + 2 - 3) // stride + 1 and Wo == (W + 2 - 3) // stride + 1, "geometry")
    with _prof('conv_dgrad' + (f' {B}x{H}x{W} {Cin}<-{Cout} s{stride}' if PROFILE_SHAPES else ''), 2.0 * B * Ho * Wo * Cin * 9 * Cout, 0.0):
        ldr = _nhwc(residual)[4] if residual is not None else 0
        lib().call("az_conv2d_bf16", 1, B, H, W, Cin, Ho, Wo, Cout, 3, stride, 1, Cpad, _ptr(None), 0, _ptr(w), _ptr(dy), lddy,
               _ptr(dx), lddx, _ptr(None), _ptr(None), 0, _ptr(residual), ldr, int(accumulate), 1, _ptr(None), 0, _stream())
    return dx


def conv_dgrad_wt(dy, wt, dx, *, stride=1, accumulate=False, residual=None):
    """dgrad with the pre-transposed weight copy wt [Cin][3][3][Cout]; residual (B,H,W,Cin): dx = residual + gradient."""
    B, Ho, Wo, Cout, lddy = _nhwc(dy)
    Bx, H, W, Cin, lddx = _nhwc(dx)
    _req(wt.dtype == BF16 and wt.is_contiguous() and tuple(wt.shape) == (Cin, 3, 3, Cout) and Cout % 8 == 0, "transposed weight layout")
    _req(Bx == B and Ho == (H + 2 - 3) // stride + 1 and Wo == (W + 2 - 3) // stride + 1, "geometry")
    with _prof('conv_dgrad' + (f' {B}x{H}x{W} {Cin}<-{Cout} s{stride}' if PROFILE_SHAPES else ''), 2.0 * B * Ho * Wo * Cin * 9 * Cout, 0.0):
        ldr = _nhwc(residual)[4] if residual is not None else 0
        lib().call("az_conv2d_bf16", 3, B, H, W, Cin, Ho, Wo, Cout, 3, stride, 1, Cout, _ptr(None), 0, _ptr(wt), _ptr(dy), lddy,
                   _ptr(dx), lddx, _ptr(None), _ptr(None), 0, _ptr(residual), ldr, int(accumulate), 1, _ptr(None), 0, _stream())
    return dx


def conv_wgrad(dy, x, dw, *, stride=1, cout_real=None, accumulate=True, split_k=0, bias_grad=None, seg_grad=None, upsample=False):
    """dw [Cout][k][k][Cin] (+)= dy^T . im2col(x).  bias_grad (bf16 [Cout], +=) and seg_grad (bf16 [B][Cout], overwritten:
    per-sample channel sums of dy) are produced in the same pass when given.  upsample: x is the half-resolution input of a
    nearest upsample to dy's extents (see conv_fwd) in front of the conv."""
    B, Ho, Wo, Cdy, lddy = _nhwc(dy)
    Bx, H, W, Cin, ldx = _nhwc(x)
    if upsample:
        _req(stride == 1 and dw.shape[1] == 3, "the upsample gather exists for 3x3 stride-1 convolutions")
        H, W = _upsampled_extents(H, W, dy)
    Cout = Cdy if cout_real is None else cout_real
    _req(dw.dtype == BF16 and dw.is_contiguous() and dw.dim() == 4 and dw.shape[0] == Cout and dw.shape[3] == Cin, "dw layout")
    ks = dw.shape[1]
    pad = 1 if ks == 3 else 0
    _req(Bx == B and Ho == (H + 2 * pad - ks) // stride + 1 and Wo == (W + 2 * pad - ks) // stride + 1, "geometry")
    _req(lddy >= ((Cout + 7) // 8) * 8, "dy rows must be readable in 8-element chunks")
    ws = workspace(dw.device)
    if bias_grad is not None or seg_grad is not None:
        if bias_grad is not None:
            _req(bias_grad.dtype == BF16 and bias_grad.is_contiguous() and bias_grad.numel() == Cout, "bias_grad must be contiguous bf16 [Cout]")
        if seg_grad is not None:
            _req(seg_grad.dtype == BF16 and seg_grad.is_contiguous() and seg_grad.numel() == B * Cout, "seg_grad must be contiguous bf16 [B][Cout]")
            _req((Ho * Wo) % 64 == 0, "per-sample sums need Hout*Wout to be a multiple of 64")
        with _prof('conv_wgrad' + (f' {B}x{H}x{W} {Cin}x{Cout} k{ks}s{stride}+b' if PROFILE_SHAPES else ''), 2.0 * B * Ho * Wo * Cout * ks * ks * Cin, 0.0):
            lib().call("az_conv2d_wgrad_bias_bf16", B, H, W, Cin, Ho, Wo, Cout, ks | (16 if upsample else 0), stride, pad, _ptr(x), ldx, _ptr(dy), lddy, _ptr(dw),
                       int(accumulate), int(split_k), _ptr(ws.splitk), ws.splitk.numel() * 4, _ptr(bias_grad), _ptr(seg_grad), _stream())
        return dw
    with _prof('conv_wgrad' + (f' {B}x{H}x{W} {Cin}x{Cout} k{ks}s{stride}' if PROFILE_SHAPES else ''), 2.0 * B * Ho * Wo * Cout * ks * ks * Cin, 0.0):
        lib().call("az_conv2d_bf16", 18 if upsample else 2, B, H, W, Cin, Ho, Wo, Cout, ks, stride, pad, 0, _ptr(x), ldx, _ptr(None), _ptr(dy), lddy,
               _ptr(dw), ks * ks * Cin, _ptr(None), _ptr(None), 0, _ptr(None), 0, int(accumulate), int(split_k),
               _ptr(ws.splitk), ws.splitk.numel() * 4, _stream())
    return dw


# ---------------------------------------------------------------------------------------------
# LoRA adapter products (az_lora_*)
# ---------------------------------------------------------------------------------------------

def _lora_parts(total, parts, what):
    _req(1 <= parts <= 3 and total % parts == 0, f"{what}: {total} rows / columns do not split into {parts} parts")
    return total // parts


def lora_down(x, w, out, *, parts=1, scale=1.0):
    """out[:, p r:(p+1) r] = scale * x_p @ w_p^T (az_lora_down_bf16).  w [parts * r][K] (the parts stacked by rows), out [M][parts * r].
    x [M][K] is shared by the parts (parts must then be 1: a stacked w is one product of rank parts * r), or x [M][parts * K] holds one
    column slice per part (du = s dy B: x = dy of a fused projection, w = the stacked B^T copies)."""
    M, xc, ldx = _rows(x)
    wr, K, ldw = _rows(w)
    om, oc, ldo = _rows(out)
    r = _lora_parts(wr, parts, "lora_down w")
    _req(xc == parts * K and (om, oc) == (M, parts * r), f"lora_down shapes x {tuple(x.shape)} w {tuple(w.shape)} out {tuple(out.shape)}")
    _req(K % 8 == 0 and r % 4 == 0 and 4 <= r and parts * r <= 192, f"lora_down: K {K} % 8, rank {r} % 4, parts * rank <= 192")
    _req(ldx % 8 == 0 and ldw % 8 == 0 and ldo % 4 == 0 and x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0 and out.data_ptr() % 8 == 0,
         "lora_down: operand alignment")
    with _prof("lora_down" + (f" {M}x{parts}x{r}x{K}" if PROFILE_SHAPES else ""), 2.0 * M * parts * r * K, 2.0 * (M * parts * K + parts * r * K + M * parts * r)):
        lib().call("az_lora_down_bf16", M, K, r, parts, float(scale), _ptr(x), ldx, K, _ptr(w), ldw, r * ldw, _ptr(out), ldo, _stream())
    return out


def lora_up(u, w, y, *, parts=1, scale=1.0):
    """y[:, p N:(p+1) N] += scale * u[:, p r:(p+1) r] @ w_p^T in place (az_lora_up_bf16).  u [M][parts * r], w [parts * N][r] (the
    parts stacked by rows), y [M][parts * N] -- the column slices of a fused output."""
    M, uc, ldu = _rows(u)
    wr, r, ldw = _rows(w)
    ym, yc, ldy = _rows(y)
    N = _lora_parts(wr, parts, "lora_up w")
    _req(uc == parts * r and (ym, yc) == (M, parts * N), f"lora_up shapes u {tuple(u.shape)} w {tuple(w.shape)} y {tuple(y.shape)}")
    _req(N % 4 == 0 and r % 4 == 0 and 4 <= r <= 192, f"lora_up: N {N} % 4, rank {r} % 4 and <= 192")
    _req(ldu % 4 == 0 and ldw % 4 == 0 and ldy % 4 == 0 and u.data_ptr() % 8 == 0 and w.data_ptr() % 8 == 0 and y.data_ptr() % 8 == 0,
         "lora_up: operand alignment")
    with _prof("lora_up" + (f" {M}x{parts}x{N}x{r}" if PROFILE_SHAPES else ""), 2.0 * M * parts * N * r, 2.0 * (2 * M * parts * N + parts * N * r + M * parts * r)):
        lib().call("az_lora_up_bf16", M, N, r, parts, float(scale), _ptr(u), ldu, r, _ptr(w), ldw, N * ldw, _ptr(y), ldy, N, _stream())
    return y


def lora_up_geglu(u, w, proj, out, *, scale=1.0):
    """proj += scale * u @ w^T in place and out = proj[:, :H] * gelu(proj[:, H:]) on the rounded proj (az_lora_up_geglu_bf16): the up
    product of ff.net.0.proj with az_geglu_fwd in its epilogue.  u [M][r], w [2 H][r] (value rows, then gate rows), proj [M][2 H], out [M][H]."""
    M, r, ldu = _rows(u)
    H2, wr, ldw = _rows(w)
    Mp, H2p, ldp = _rows(proj)
    Mo, H, ldo = _rows(out)
    _req(wr == r and H2 == 2 * H and (Mp, Mo, H2p) == (M, M, H2),
         f"lora_up_geglu shapes u {tuple(u.shape)} w {tuple(w.shape)} proj {tuple(proj.shape)} out {tuple(out.shape)}")
    _req(H % 8 == 0 and r % 4 == 0 and 4 <= r <= 64, f"lora_up_geglu: H {H} % 8, rank {r} % 4 and <= 64")
    _req(ldu % 4 == 0 and ldw % 4 == 0 and ldp % 4 == 0 and ldo % 4 == 0 and u.data_ptr() % 8 == 0 and w.data_ptr() % 8 == 0
         and proj.data_ptr() % 8 == 0 and out.data_ptr() % 8 == 0, "lora_up_geglu: operand alignment")
    with _prof("lora_up" + (f" {M}x{H2}x{r}+geglu" if PROFILE_SHAPES else ""), 2.0 * M * H2 * r, 2.0 * (2 * M * H2 + M * H + H2 * r + M * r)):
        lib().call("az_lora_up_geglu_bf16", M, H, r, float(scale), _ptr(u), ldu, _ptr(w), ldw, _ptr(proj), ldp, _ptr(out), ldo, _stream())
    return out


def lora_dropout(u, r, parts, rows_per_sample, mids, thresholds, inv, seed, step_word):
    """In place on u [rows][parts * r] (the down product, or du): network / rank / module dropout of az_lora_dropout_bf16.  mids: the
    module id of each part; thresholds (t_net, t_rank, t_mod), 0 = that kind off, at least one on; inv: the rescale of the kept
    elements; step_word: a one-element int32 / uint32 DEVICE tensor that holds the micro-step when the launch runs."""
    rows, uc, ldu = _rows(u)
    _req(1 <= parts <= 3 and uc == parts * r and len(mids) == parts, f"lora_dropout: u {tuple(u.shape)} is not {parts} parts of rank {r} with ids {list(mids)}")
    _req(rows_per_sample > 0 and rows % rows_per_sample == 0, f"lora_dropout: {rows} rows are no whole samples of {rows_per_sample}")
    _req(len(thresholds) == 3 and all(int(t) == t and 0 <= t <= 65535 for t in thresholds) and any(thresholds),
         f"lora_dropout: thresholds {tuple(thresholds)} (three in [0, 65535], at least one on)")
    _req(isinstance(step_word, torch.Tensor) and step_word.is_cuda and step_word.device == u.device and step_word.numel() == 1
         and step_word.dtype in (torch.int32, torch.uint32), "lora_dropout: step_word must be one int32 / uint32 on u's device")
    m = [int(x) for x in mids] + [0] * (3 - parts)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    with _prof("lora_dropout" + (f" {rows}x{parts}x{r}" if PROFILE_SHAPES else ""), 0.0, 4.0 * rows * parts * r):
        lib().call("az_lora_dropout_bf16", rows, r, parts, int(rows_per_sample), _ptr(u), ldu, m[0], m[1], m[2], int(thresholds[0]),
                   int(thresholds[1]), int(thresholds[2]), float(inv), seed - (1 << 64) if seed >= (1 << 63) else seed, _ptr(step_word), _stream())
    return u


def lora_max_norm(table, max_norm, stats, stream=None):
    """Max-norm regularisation of every adapted module in ONE launch (az_lora_max_norm_bf16): table is the int64 DEVICE job table
    [n][8] (lora_norm.job_rows: address of A, of B, r, K, out, fp32 bits of s, address of the fp32 master of A or 0, of B or 0), stats
    the fp32 device array [n][2] that receives (norm before scaling, q) per module, on `stream` (default: the current one)."""
    import math
    _req(isinstance(table, torch.Tensor) and table.is_cuda and table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == 8
         and table.is_contiguous() and 1 <= table.shape[0] <= 65535, "lora_max_norm: table must be a contiguous cuda int64 [n][8], 1 <= n <= 65535")
    _req(isinstance(stats, torch.Tensor) and stats.is_cuda and stats.device == table.device and stats.dtype == F32 and stats.is_contiguous()
         and tuple(stats.shape) == (table.shape[0], 2), "lora_max_norm: stats must be a contiguous fp32 [n][2] on the table's device")
    _req(not isinstance(max_norm, bool) and isinstance(max_norm, (int, float)) and math.isfinite(max_norm) and max_norm > 0
         and float(max_norm) <= 3.4028234663852886e38, f"lora_max_norm: max_norm must be a positive finite number, got {max_norm!r}")
    st = ctypes.c_void_p(stream.cuda_stream) if stream is not None else _stream()
    lib().call("az_lora_max_norm_bf16", _ptr(table), int(table.shape[0]), float(max_norm), _ptr(stats), st)
    return stats


# ---------------------------------------------------------------------------------------------
# DoRA (az_dora_*)
# ---------------------------------------------------------------------------------------------

def dora_norm(table, tiles, init=False, stream=None):
    """The row norms of W + s B A of every adapted module and their gains in ONE launch (az_dora_norm_bf16): table is the int64 DEVICE
    job table [n][12] (dora.job_rows: addresses of W, A, B, m, g, inv; r, K, N; fp32 bits of s; first tile; 0), tiles the 64-row tiles
    of all its rows together.  init: also write m = bf16(norm).  On `stream` (default: the current one)."""
    _req(isinstance(table, torch.Tensor) and table.is_cuda and table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == 12
         and table.is_contiguous() and 1 <= table.shape[0] <= 65535, "dora_norm: table must be a contiguous cuda int64 [n][12], 1 <= n <= 65535")
    _req(not isinstance(tiles, bool) and isinstance(tiles, int) and 1 <= tiles <= 0x7FFFFFF0, f"dora_norm: tiles must be a positive int, got {tiles!r}")
    _req(isinstance(init, (bool, int)) and int(init) in (0, 1), f"dora_norm: init must be 0 or 1, got {init!r}")
    st = ctypes.c_void_p(stream.cuda_stream) if stream is not None else _stream()
    lib().call("az_dora_norm_bf16", _ptr(table), int(table.shape[0]), int(tiles), int(init), st)
    return table


def _dora_gain(g, N, dev, what):
    _req(isinstance(g, torch.Tensor) and g.is_cuda and g.device == dev and g.dtype == F32 and g.dim() == 1 and g.numel() == N and g.stride(0) == 1
         and g.data_ptr() % 16 == 0, f"{what} must be a dense fp32 [{N}] on the activation's device, 16-byte aligned")


def _dora_rows(t, M, N, what):
    m, n, ld = _rows(t)
    _req((m, n) == (M, N) and ld % 8 == 0 and t.data_ptr() % 16 == 0, f"{what} must be [{M}][{N}] with a row stride % 8 and 16-byte aligned, got {tuple(t.shape)} ld {ld}")
    return ld


def dora_scale(v, g, y, *, bias=None, residual=None):
    """y = bf16(fmaf(g[o], v, bias[o] or 0) + (residual or 0)) (az_dora_scale_bf16).  v, y, residual [M][N] with their own row strides
    (column slices of fused outputs; columns outside are untouched), g fp32 [N], bias bf16 [N]."""
    M, N, ldv = _rows(v)
    _req(N % 8 == 0, f"dora_scale: N {N} % 8")
    _dora_rows(v, M, N, "dora_scale: v")
    ldy = _dora_rows(y, M, N, "dora_scale: y")
    _dora_gain(g, N, v.device, "dora_scale: g")
    if bias is not None:
        _req(bias.is_cuda and bias.dtype == BF16 and bias.dim() == 1 and bias.numel() == N and bias.stride(0) == 1 and bias.data_ptr() % 16 == 0,
             f"dora_scale: bias must be a dense bf16 [{N}], 16-byte aligned")
    ldr = _dora_rows(residual, M, N, "dora_scale: residual") if residual is not None else 0
    with _prof("dora_scale" + (f" {M}x{N}" if PROFILE_SHAPES else ""), 2.0 * M * N, 2.0 * M * N * (2 + (residual is not None))):
        lib().call("az_dora_scale_bf16", M, N, _ptr(v), ldv, _ptr(g), _ptr(bias), _ptr(residual), ldr, _ptr(y), ldy, _stream())
    return y


def dora_bwd(dy, g, dv, *, v=None, inv=None, dm=None):
    """dv = bf16(g[o] dy) and, with dm, dm[o] += inv[o] sum_rows dy v in fixed order (az_dora_bwd_bf16: the partial sums go through the
    library workspace and are finished by the same call).  dm None: dv alone (a part of a fused group that carries no adapter: g = 1)."""
    M, N, lddy = _rows(dy)
    _req(N % 8 == 0, f"dora_bwd: N {N} % 8")
    _dora_rows(dy, M, N, "dora_bwd: dy")
    lddv = _dora_rows(dv, M, N, "dora_bwd: dv")
    _dora_gain(g, N, dy.device, "dora_bwd: g")
    ldv, ws_ptr, ws_bytes = 0, _ptr(None), 0
    if dm is not None:
        _req(v is not None and inv is not None, "dora_bwd: dm needs v and inv")
        ldv = _dora_rows(v, M, N, "dora_bwd: v")
        _dora_gain(inv, N, dy.device, "dora_bwd: inv")
        _req(dm.is_cuda and dm.device == dy.device and dm.dtype == BF16 and dm.dim() == 1 and dm.numel() == N and dm.stride(0) == 1,
             f"dora_bwd: dm must be a dense bf16 [{N}]")
        ws = workspace(dy.device)
        ws_ptr, ws_bytes = _ptr(ws.splitk), ws.splitk.numel() * 4 - (16 << 10)        # the last 16 KiB are the GEMM core's arrival counters
    else:
        v = inv = None
    with _prof("dora_bwd" + (f" {M}x{N}" if PROFILE_SHAPES else ""), 3.0 * M * N, 2.0 * M * N * (2 + (dm is not None))):
        lib().call("az_dora_bwd_bf16", M, N, _ptr(dy), lddy, _ptr(v), ldv, _ptr(g), _ptr(inv), _ptr(dv), lddv, _ptr(dm), ws_ptr, ws_bytes, _stream())
    return dv


def lora_wgrad(small, big, out, *, parts=1, scale=1.0, accumulate=True, small_major=True):
    """out (+)= scale * small_p^T @ big_p, summed over the rows (az_lora_wgrad_bf16).  small [M][parts * ns] (du or u), big [M][parts * nb]
    (x or dy).  small_major: out [parts * ns][nb] (dA_cat = du^T x); else out [parts * nb][ns] (the stacked dB_p = s dy_p^T u_p)."""
    M, sc, ld_s = _rows(small)
    Mb, bc, ld_g = _rows(big)
    orows, ocols, ldo = _rows(out)
    ns, nb = _lora_parts(sc, parts, "lora_wgrad small"), _lora_parts(bc, parts, "lora_wgrad big")
    _req(Mb == M and (orows, ocols) == ((parts * ns, nb) if small_major else (parts * nb, ns)),
         f"lora_wgrad shapes small {tuple(small.shape)} big {tuple(big.shape)} out {tuple(out.shape)}")
    _req(ns % 4 == 0 and 4 <= ns <= 192 and nb % 8 == 0, f"lora_wgrad: small width {ns} % 4 and <= 192, big width {nb} % 8")
    _req(ld_s % 4 == 0 and ld_g % 8 == 0 and small.data_ptr() % 8 == 0 and big.data_ptr() % 16 == 0, "lora_wgrad: operand alignment")
    ws = workspace(out.device)
    ws_bytes = ws.splitk.numel() * 4 - (16 << 10)            # the last 16 KiB are the GEMM core's arrival counters
    os_s, os_b, ops_ = (ldo, 1, ns * ldo) if small_major else (1, ldo, nb * ldo)
    with _prof("lora_wgrad" + (f" {parts}x{ns}x{nb}x{M}" if PROFILE_SHAPES else ""), 2.0 * M * parts * ns * nb, 2.0 * (M * parts * (ns + nb) + 2 * parts * ns * nb)):
        lib().call("az_lora_wgrad_bf16", M, ns, nb, parts, float(scale), _ptr(small), ld_s, ns, _ptr(big), ld_g, nb, _ptr(out), os_s, os_b, ops_,
                   int(accumulate), _ptr(ws.splitk), ws_bytes, _stream())
    return out


def _lora_conv_geom(geom, x, what):
    """(B, H, W) and an activation [B H W][C] (2-D rows, any row stride) -> (B, H, W, C, ld)."""
    _req(len(geom) == 3 and all(int(v) > 0 for v in geom), f"{what}: geometry (B, H, W) {geom}")
    B, H, W = (int(v) for v in geom)
    M, C, ld = _rows(x)
    _req(M == B * H * W, f"{what}: {M} rows are not the {B} x {H} x {W} pixels")
    return B, H, W, C, ld


def _lora_conv_rank(Cin, r, what):
    _req(Cin % 8 == 0 and r % 4 == 0 and 4 <= r <= 64, f"{what}: Cin {Cin} % 8, rank {r} % 4 and 4 <= rank <= 64")


def lora_conv_down(x, geom, a, out, *, scale=1.0):
    """out[m] = scale * sum over the nine taps of x[nbr(m, tap)] @ a[:, tap]^T (az_lora_conv_down_bf16): the down product of an adapter
    on a 3x3 / stride 1 / pad 1 convolution.  x [B H W][Cin] rows (any row stride), geom (B, H, W), a [r][3][3][Cin] contiguous (the
    base conv weight's layout), out [B H W][r]."""
    B, H, W, Cin, ldx = _lora_conv_geom(geom, x, "lora_conv_down x")
    om, r, ldo = _rows(out)
    _req(a.is_cuda and a.dtype == BF16 and a.is_contiguous() and tuple(a.shape) == (r, 3, 3, Cin) and om == B * H * W,
         f"lora_conv_down shapes x {tuple(x.shape)} a {tuple(a.shape)} out {tuple(out.shape)}")
    _lora_conv_rank(Cin, r, "lora_conv_down")
    _req(ldx % 8 == 0 and ldo % 4 == 0 and x.data_ptr() % 16 == 0 and a.data_ptr() % 16 == 0 and out.data_ptr() % 8 == 0,
         "lora_conv_down: operand alignment")
    with _prof("lora_conv_down" + (f" {B}x{H}x{W} {Cin}->{r}" if PROFILE_SHAPES else ""), 18.0 * B * H * W * r * Cin, 2.0 * B * H * W * (Cin + r)):
        lib().call("az_lora_conv_down_bf16", B, H, W, Cin, r, float(scale), _ptr(x), ldx, _ptr(a), _ptr(out), ldo, _stream())
    return out


def lora_conv_dgrad(du, geom, at, dx, *, scale=1.0):
    """dx[m] += scale * sum over the mirrored taps of du[nbr'(m, tap)] @ at[:, tap]^T in place (az_lora_conv_dgrad_bf16).  du [B H W][r],
    at [Cin][3][3][r] contiguous (the transposed copy of the down matrix), dx [B H W][Cin] rows (any row stride), disjoint from du."""
    B, H, W, r, ldu = _lora_conv_geom(geom, du, "lora_conv_dgrad du")
    xm, Cin, ldx = _rows(dx)
    _req(at.is_cuda and at.dtype == BF16 and at.is_contiguous() and tuple(at.shape) == (Cin, 3, 3, r) and xm == B * H * W,
         f"lora_conv_dgrad shapes du {tuple(du.shape)} at {tuple(at.shape)} dx {tuple(dx.shape)}")
    _lora_conv_rank(Cin, r, "lora_conv_dgrad")
    _req(ldu % 4 == 0 and ldx % 4 == 0 and du.data_ptr() % 8 == 0 and at.data_ptr() % 8 == 0 and dx.data_ptr() % 8 == 0,
         "lora_conv_dgrad: operand alignment")
    u0, x0 = du.data_ptr(), dx.data_ptr()
    _req(u0 + 2 * ((xm - 1) * ldu + r) <= x0 or x0 + 2 * ((xm - 1) * ldx + Cin) <= u0, "lora_conv_dgrad: du and dx overlap")
    with _prof("lora_conv_dgrad" + (f" {B}x{H}x{W} {Cin}<-{r}" if PROFILE_SHAPES else ""), 18.0 * B * H * W * r * Cin, 2.0 * B * H * W * (2 * Cin + r)):
        lib().call("az_lora_conv_dgrad_bf16", B, H, W, Cin, r, float(scale), _ptr(du), ldu, _ptr(at), _ptr(dx), ldx, _stream())
    return dx


def lora_conv_wgrad(du, x, geom, da, *, scale=1.0, accumulate=True):
    """da[j][tap] (+)= scale * sum over the pixels of du[m][j] * x[nbr(m, tap)] (az_lora_conv_wgrad_bf16).  du [B H W][r], x [B H W][Cin]
    rows (any row stride), da [r][3][3][Cin] contiguous."""
    B, H, W, Cin, ldx = _lora_conv_geom(geom, x, "lora_conv_wgrad x")
    um, r, ldu = _rows(du)
    _req(da.is_cuda and da.dtype == BF16 and da.is_contiguous() and tuple(da.shape) == (r, 3, 3, Cin) and um == B * H * W,
         f"lora_conv_wgrad shapes du {tuple(du.shape)} x {tuple(x.shape)} da {tuple(da.shape)}")
    _lora_conv_rank(Cin, r, "lora_conv_wgrad")
    _req(ldu % 4 == 0 and ldx % 8 == 0 and du.data_ptr() % 8 == 0 and x.data_ptr() % 16 == 0, "lora_conv_wgrad: operand alignment")
    ws = workspace(da.device)
    ws_bytes = ws.splitk.numel() * 4 - (16 << 10)            # the last 16 KiB are the GEMM core's arrival counters
    with _prof("lora_conv_wgrad" + (f" {B}x{H}x{W} {r}x{Cin}" if PROFILE_SHAPES else ""), 18.0 * B * H * W * r * Cin, 2.0 * B * H * W * (9 * Cin + r)):
        lib().call("az_lora_conv_wgrad_bf16", B, H, W, Cin, r, float(scale), _ptr(du), ldu, _ptr(x), ldx, _ptr(da), int(accumulate),
                   _ptr(ws.splitk), ws_bytes, _stream())
    return da


# ---------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------

def _attn_view(t, heads):
    """(B,T,>=heads*64) view with unit inner stride -> (B, T, ld, sb)."""
    _req(t.is_cuda and t.dtype == BF16 and t.dim() == 3 and t.stride(2) == 1, "attention operand must be (B,T,C) bf16")
    _req(t.shape[2] == heads * 64, "last dim must be heads*64")
    _req(t.stride(1) % 8 == 0 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0, "attention operand alignment")
    return t.shape[0], t.shape[1], t.stride(1), t.stride(0)


def attn_fwd(q, k, v, o, lse, heads, scale):
    B, Tq, ldq, sq = _attn_view(q, heads)
    Bk, Tk, ldk, sk = _attn_view(k, heads)
    Bv, Tv, ldv, sv = _attn_view(v, heads)
    Bo, To, ldo, so = _attn_view(o, heads)
    _req(B == Bk == Bv == Bo and Tk == Tv and To == Tq, "attention shapes")
    _req(lse.dtype == F32 and lse.is_contiguous() and lse.numel() == B * heads * Tq, "lse buffer")
    with _prof('attn_fwd' + (f' {B}x{heads} {Tq}x{Tk}' if PROFILE_SHAPES else ''), 4.0 * B * heads * Tq * Tk * 64, 0.0):
        lib().call("az_attn_fwd", B, heads, Tq, Tk, float(scale), _ptr(q), ldq, sq, _ptr(k), ldk, sk, _ptr(v), ldv, sv,
               _ptr(o), ldo, so, _ptr(lse), _stream())
    return o


def attn_bwd(q, k, v, o, do, lse, delta, dq, dk, dv, heads, scale, parts=7):
    B, Tq, ldq, sq = _attn_view(q, heads)
    _, Tk, ldk, sk = _attn_view(k, heads)
    _, _, ldv, sv = _attn_view(v, heads)
    _, _, ldo, so = _attn_view(o, heads)
    _, _, lddo, sdo = _attn_view(do, heads)
    Bq, Tq2, lddq, sdq = _attn_view(dq, heads)
    Bk, Tk2, lddk, sdk = _attn_view(dk, heads)
    Bv, Tk3, lddv, sdv = _attn_view(dv, heads)
    _req(Tq2 == Tq and Tk2 == Tk and Tk3 == Tk and Bq == B and Bk == B and Bv == B, "attention bwd shapes")
    _req(lse.dtype == F32 and lse.numel() == B * heads * Tq and delta.dtype == F32 and delta.numel() >= B * heads * Tq, "lse/delta")
    with _prof('attn_bwd' + (f' {B}x{heads} {Tq}x{Tk}' if PROFILE_SHAPES else ''), 10.0 * B * heads * Tq * Tk * 64 * (((parts >> 1) & 1) * 3 + ((parts >> 2) & 1) * 4) / 7.0, 0.0):
        lib().call("az_attn_bwd", B, heads, Tq, Tk, float(scale), _ptr(q), ldq, sq, _ptr(k), ldk, sk, _ptr(v), ldv, sv,
               _ptr(o), ldo, so, _ptr(do), lddo, sdo, _ptr(lse), _ptr(delta), _ptr(dq), lddq, sdq, _ptr(dk), lddk, sdk,
               _ptr(dv), lddv, sdv, _ptr(workspace(q.device).attn), workspace(q.device).attn.numel() * 4, int(parts), _stream())


# ---------------------------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------------------------

def gn_scratch_floats(B, HW, C, G):
    return int(lib().raw("az_gn_scratch_floats")(B, HW, C, G))


def groupnorm_fwd(x, gamma, beta, y, stats, G, eps, silu):
    """x,y (B,HW,C) bf16 with unit channel stride; stats (B,G,2) fp32."""
    _req(x.dim() == 3 and y.shape == x.shape and x.stride(2) == 1 and y.stride(2) == 1, "groupnorm operands")
    B, HW, C = x.shape
    _req(x.stride(0) == HW * x.stride(1) and y.stride(0) == HW * y.stride(1), "batch stride")
    _req(stats.dtype == F32 and stats.numel() == B * G * 2 and stats.is_contiguous(), "stats")
    ws = workspace(x.device)
    _req(gn_scratch_floats(B, HW, C, G) <= ws.scratch.numel(), "scratch too small")
    with _prof('gn_fwd', 0.0, 4.0 * B * HW * C):
        lib().call("az_groupnorm_fwd", B, HW, C, G, float(eps), int(silu), _ptr(x), x.stride(1), _ptr(gamma), _ptr(beta),
               _ptr(y), y.stride(1), _ptr(stats), _ptr(ws.scratch), _stream())
    return y


def groupnorm_bwd(x, gamma, beta, stats, dy, dx, dgamma, dbeta, G, silu, accumulate_dx=False, dx_add=None):
    """dx_add: dx = dx_add + gradient (dx_add may be dx itself = accumulate_dx=True)."""
    B, HW, C = x.shape
    if accumulate_dx and dx_add is None:
        dx_add = dx
    _req(dx_add is None or (dx is not None and dx_add.shape == x.shape and dx_add.stride(2) == 1 and dx_add.stride(0) == HW * dx_add.stride(1)), "dx_add layout")
    _req(dy.shape == x.shape and (dx is None or dx.shape == x.shape), "groupnorm bwd shapes")
    _req(x.stride(2) == 1 and dy.stride(2) == 1 and x.stride(0) == HW * x.stride(1) and dy.stride(0) == HW * dy.stride(1), "strides")
    ws = workspace(x.device)
    _req(gn_scratch_floats(B, HW, C, G) <= ws.scratch.numel(), "scratch too small")
    with _prof('gn_bwd', 0.0, 10.0 * B * HW * C):
        lib().call("az_groupnorm_bwd_ex", B, HW, C, G, int(silu), _ptr(x), x.stride(1), _ptr(gamma), _ptr(beta), _ptr(stats),
               _ptr(dy), dy.stride(1), _ptr(dx), dx.stride(1) if dx is not None else 0, _ptr(dx_add), dx_add.stride(1) if dx_add is not None else 0,
               _ptr(dgamma), _ptr(dbeta), _ptr(ws.scratch), _stream())


def layernorm_fwd(x, gamma, beta, y, stats, eps=1e-5):
    M, C, ldx = _rows(x)
    My, Cy, ldy = _rows(y)
    _req((M, C) == (My, Cy) and stats.dtype == F32 and stats.numel() == 2 * M, "layernorm operands")
    with _prof('ln_fwd', 0.0, 4.0 * M * C):
        lib().call("az_layernorm_fwd", M, C, float(eps), _ptr(x), ldx, _ptr(gamma), _ptr(beta), _ptr(y), ldy, _ptr(stats), _stream())
    return y


def layernorm_bwd(x, gamma, stats, dy, dx, dgamma, dbeta, accumulate_dx=False, dx_add=None):
    """dx may be None (parameter gradients only) and dgamma/dbeta may be None (data gradient only).
    dx_add: dx = dx_add + gradient (dx_add may be dx itself = accumulate_dx=True)."""
    M, C, ldx = _rows(x)
    if accumulate_dx and dx_add is None:
        dx_add = dx
    ld_add = 0
    if dx_add is not None:
        Ma, Ca, ld_add = _rows(dx_add)
        _req(dx is not None and (Ma, Ca) == (M, C), "dx_add shape")
    _, _, lddy = _rows(dy)
    lddx = _rows(dx)[2] if dx is not None else 0
    ws = workspace(x.device)
    _req(int(lib().raw("az_ln_scratch_floats")(M, C)) <= ws.scratch.numel(), "scratch too small")
    with _prof('ln_bwd' if dx is not None else 'ln_bwd_param', 0.0, (8.0 if dx is not None else 4.0) * M * C):
        lib().call("az_layernorm_bwd_ex", M, C, _ptr(x), ldx, _ptr(gamma), _ptr(stats), _ptr(dy), lddy, _ptr(dx), lddx,
               _ptr(dx_add), ld_add, _ptr(dgamma), _ptr(dbeta), _ptr(ws.scratch), _stream())


def ln_partial_blocks(M: int) -> int:
    return int(lib().raw("az_ln_partial_blocks")(int(M)))


def layernorm_bwd_partial(x, gamma, stats, dy, dx, partial, dx_add=None, nblk=None):
    """One-pass LayerNorm backward: dx final (= dx_add + gradient), gamma / beta gradients left as partial[nblk][C][2] fp32
    (finished later, many LayerNorms at a time, by ln_param_finish_multi)."""
    M, C, ldx = _rows(x)
    _, _, lddy = _rows(dy)
    _, _, lddx = _rows(dx)
    ld_add = 0
    if dx_add is not None:
        Ma, Ca, ld_add = _rows(dx_add)
        _req((Ma, Ca) == (M, C), "dx_add shape")
    if nblk is None:
        nblk = ln_partial_blocks(M)
    _req(partial.dtype == F32 and partial.is_contiguous() and partial.numel() >= nblk * C * 2, "partial buffer")
    with _prof('ln_bwd', 0.0, 8.0 * M * C):
        lib().call("az_layernorm_bwd_partial", M, C, _ptr(x), ldx, _ptr(gamma), _ptr(stats), _ptr(dy), lddy, _ptr(dx), lddx,
                   _ptr(dx_add), ld_add, _ptr(partial), int(nblk), _stream())


def ln_param_finish_multi(table, njobs: int, nblocks: int):
    """table: device int64 [njobs][6] (partial, dgamma, dbeta, nparts, C, first block), see az_ln_param_finish_multi."""
    with _prof('ln_bwd_param', 0.0, 0.0):
        lib().call("az_ln_param_finish_multi", _ptr(table), int(njobs), int(nblocks), _stream())


# ---------------------------------------------------------------------------------------------
# elementwise
# ---------------------------------------------------------------------------------------------

def geglu_fwd(proj, out):
    M, H2, ldp = _rows(proj)
    Mo, H, ldo = _rows(out)
    _req(Mo == M and H2 == 2 * H, "geglu shapes")
    with _prof('geglu_fwd', 0.0, 6.0 * M * H):
        lib().call("az_geglu_fwd", M, H, _ptr(proj), ldp, _ptr(out), ldo, _stream())
    return out


def geglu_bwd(proj, dout, dproj):
    M, H2, ldp = _rows(proj)
    _, H, lddo = _rows(dout)
    Md, Hd, lddp = _rows(dproj)
    _req(H2 == 2 * H and (Md, Hd) == (M, H2), "geglu bwd shapes")
    with _prof('geglu_bwd', 0.0, 10.0 * M * H):
        lib().call("az_geglu_bwd", M, H, _ptr(proj), ldp, _ptr(dout), lddo, _ptr(dproj), lddp, _stream())
    return dproj


def silu_fwd(x, y):
    _req(x.is_contiguous() and y.is_contiguous() and x.numel() == y.numel() and x.dtype == BF16, "silu operands")
    lib().call("az_silu_fwd", x.numel(), _ptr(x), _ptr(y), _stream())
    return y


def silu_bwd(x, dy, dx, accumulate=False):
    _req(x.is_contiguous() and dy.is_contiguous() and dx.is_contiguous() and x.numel() == dy.numel() == dx.numel(), "silu bwd")
    lib().call("az_silu_bwd", x.numel(), _ptr(x), _ptr(dy), _ptr(dx), int(accumulate), _stream())
    return dx


def add_rows(a, b, y):
    """y = a + b (row-strided 2-D views) ; b None -> strided copy."""
    R, C, lda = _rows(a)
    Ry, Cy, ldy = _rows(y)
    _req((R, C) == (Ry, Cy), "add_rows shapes")
    ldb = 0
    if b is not None:
        Rb, Cb, ldb = _rows(b)
        _req((Rb, Cb) == (R, C), "add_rows b shape")
    with _prof('add_rows', 0.0, 6.0 * R * C):
        lib().call("az_add_rows", R, C, _ptr(a), lda, _ptr(b), ldb, _ptr(y), ldy, _stream())
    return y


def upsample2x_fwd(x, y):
    B, H, W, C = x.shape
    _req(x.is_contiguous() and y.is_contiguous() and tuple(y.shape) == (B, 2 * H, 2 * W, C) and x.dtype == BF16, "upsample")
    with _prof('upsample', 0.0, 10.0 * B * H * W * C):
        lib().call("az_upsample2x_fwd", B, H, W, C, _ptr(x), _ptr(y), _stream())
    return y


def upsample2x_bwd(dy, dx):
    B, H, W, C = dx.shape
    _req(dx.is_contiguous() and dy.is_contiguous() and tuple(dy.shape) == (B, 2 * H, 2 * W, C), "upsample bwd")
    with _prof('upsample', 0.0, 10.0 * B * H * W * C):
        lib().call("az_upsample2x_bwd", B, H, W, C, _ptr(dy), _ptr(dx), _stream())
    return dx


def upsample_nearest_fwd(x, y):
    """x (B,H,W,C) -> y (B,Ho,Wo,C) with Ho in {2H-1, 2H}, Wo in {2W-1, 2W}: F.interpolate(size=(Ho, Wo), mode="nearest")."""
    B, H, W, C = x.shape
    _req(x.is_contiguous() and y.is_contiguous() and y.dim() == 4 and (y.shape[0], y.shape[3]) == (B, C) and x.dtype == BF16 and y.dtype == BF16,
         "sized upsample")
    Ho, Wo = _upsampled_extents(H, W, y)
    with _prof('upsample', 0.0, 2.5 * B * Ho * Wo * C):
        lib().call("az_upsample_nearest_fwd", B, H, W, Ho, Wo, C, _ptr(x), _ptr(y), _stream())
    return y


def upsample_nearest_bwd(dy, dx):
    """The adjoint of upsample_nearest_fwd: dx (B,H,W,C) = the 2x2 fold of dy (B,Ho,Wo,C), cropped edges receiving fewer terms."""
    B, H, W, C = dx.shape
    _req(dx.is_contiguous() and dy.is_contiguous() and dy.dim() == 4 and (dy.shape[0], dy.shape[3]) == (B, C) and dx.dtype == BF16 and dy.dtype == BF16,
         "sized upsample bwd")
    Ho, Wo = _upsampled_extents(H, W, dy)
    with _prof('upsample', 0.0, 2.5 * B * Ho * Wo * C):
        lib().call("az_upsample_nearest_bwd", B, H, W, Ho, Wo, C, _ptr(dy), _ptr(dx), _stream())
    return dx


def colsum(x, rows_per_seg, out_f32):
    R, C, ldx = _rows(x)
    _req(R % rows_per_seg == 0 and out_f32.dtype == F32 and out_f32.numel() >= (R // rows_per_seg) * C, "colsum")
    ws = workspace(x.device)
    need = int(lib().raw("az_colsum_scratch_floats")(R, C, int(rows_per_seg)))
    half = ws.scratch.numel() // 2
    _req(need <= half, "colsum scratch too small")
    # partials live in the upper half of the shared scratch (out_f32 may be its lower half)
    with _prof('colsum', 0.0, 2.0 * R * C):
        lib().call("az_colsum", R, C, int(rows_per_seg), _ptr(x), ldx, _ptr(out_f32), _ptr(ws.scratch[half:]), _stream())
    return out_f32


def colsum_grad(x, rows_per_seg, seg_out, bias_grad, n_real):
    """Fused bias-gradient form of colsum: seg_out [nseg][C] bf16 (optional) and bias_grad[:n_real] += column sums."""
    R, C, ldx = _rows(x)
    _req(R % rows_per_seg == 0 and n_real <= C, "colsum_grad shapes")
    nseg = R // rows_per_seg
    if seg_out is not None:
        _req(seg_out.dtype == BF16 and seg_out.is_contiguous() and seg_out.numel() == nseg * C, "seg_out")
    if bias_grad is not None:
        _req(bias_grad.dtype == BF16 and bias_grad.is_contiguous() and bias_grad.numel() >= n_real, "bias_grad")
    ws = workspace(x.device)
    need = int(lib().raw("az_colsum_scratch_floats")(R, C, int(rows_per_seg)))
    _req(need <= ws.scratch.numel(), "colsum scratch too small")
    with _prof('colsum', 0.0, 2.0 * R * C):
        lib().call("az_colsum_grad", R, C, int(rows_per_seg), _ptr(x), ldx, _ptr(seg_out), _ptr(bias_grad), int(n_real),
                   _ptr(ws.scratch), _stream())


def reduce_segs_to_bf16(src_f32, nseg, n, dst, accumulate):
    _req(src_f32.dtype == F32 and src_f32.numel() >= nseg * n and dst.dtype == BF16 and dst.numel() == n and dst.is_contiguous(), "reduce_segs")
    lib().call("az_reduce_segs_to_bf16", nseg, n, _ptr(src_f32), _ptr(dst), int(accumulate), _stream())


def transpose(src, dst):
    """dst[c][r] = src[r][c] (2-D bf16, unit inner strides)."""
    R, C, lds = _rows(src)
    Rd, Cd, ldd = _rows(dst)
    _req((Rd, Cd) == (C, R), "transpose shapes")
    lib().call("az_transpose_bf16", R, C, _ptr(src), lds, _ptr(dst), ldd, _stream())
    return dst


def transpose_batched(src, dst):
    """dst[b][c][r] = src[b][r][c] for 3-D bf16 views (unit inner strides, arbitrary batch / row strides)."""
    _req(src.dim() == 3 and dst.dim() == 3 and src.dtype == BF16 and dst.dtype == BF16, "transpose_batched rank/dtype")
    nb, R, C = src.shape
    _req(tuple(dst.shape) == (nb, C, R) and src.stride(2) == 1 and dst.stride(2) == 1, "transpose_batched shapes")
    lib().call("az_transpose_bf16_batched", nb, R, C, _ptr(src), src.stride(1), src.stride(0), _ptr(dst), dst.stride(1),
               dst.stride(0), _stream())
    return dst


def f32_to_bf16(src, dst):
    _req(src.dtype == F32 and dst.dtype == BF16 and src.numel() == dst.numel() and src.is_contiguous() and dst.is_contiguous(), "cast")
    lib().call("az_f32_to_bf16", src.numel(), _ptr(src), _ptr(dst), _stream())


def timestep_embed(t_f32, dim, out):
    n = t_f32.numel()
    _req(t_f32.dtype == F32 and t_f32.is_contiguous() and out.dtype == BF16 and out.dim() == 2 and out.shape[0] == n
         and out.shape[1] == dim and out.stride(1) == 1, "timestep_embed")
    lib().call("az_timestep_embed", n, dim, _ptr(t_f32), _ptr(out), out.stride(0), _stream())
    return out


def nchw_to_nhwc_pad(src, dst, C):
    """src (B,C,H,W) fp32|bf16 contiguous -> dst (B,H,W,Cpad) bf16 contiguous (zero padded channels)."""
    B, Cs, H, W = src.shape
    _req(Cs == C and src.is_contiguous() and dst.is_contiguous() and tuple(dst.shape[:3]) == (B, H, W) and dst.dtype == BF16, "nchw->nhwc")
    lib().call("az_nchw_to_nhwc_pad", B, C, H * W, dst.shape[3], _ptr(src), int(src.dtype == F32), _ptr(dst), _stream())
    return dst


def nhwc_to_nchw(src, dst, C):
    B, H, W, ld = src.shape
    _req(src.is_contiguous() and dst.is_contiguous() and tuple(dst.shape) == (B, C, H, W), "nhwc->nchw")
    lib().call("az_nhwc_to_nchw", B, C, H * W, ld, _ptr(src), _ptr(dst), int(dst.dtype == F32), _stream())
    return dst


def noise_target(mode, latents, noise, coef_a, coef_b, noisy_nhwc, target):
    B, C, H, W = latents.shape
    _req(latents.dtype == BF16 and noise.dtype == F32 and latents.is_contiguous() and noise.is_contiguous() and
         noise.shape == latents.shape and coef_a.dtype == F32 and coef_b.dtype == F32 and coef_a.numel() == B and coef_b.numel() == B and
         noisy_nhwc.is_contiguous() and tuple(noisy_nhwc.shape[:3]) == (B, H, W) and noisy_nhwc.dtype == BF16 and
         target.dtype == F32 and target.shape == latents.shape and target.is_contiguous(), "noise_target operands")
    lib().call("az_noise_target", int(mode), B, C, H * W, noisy_nhwc.shape[3], _ptr(latents), _ptr(noise), _ptr(coef_a), _ptr(coef_b),
               _ptr(noisy_nhwc), _ptr(target), _stream())


def noise_partial_blocks(HW):
    """Pairs (sum u, sum u^2) per sample that az_noise_shape writes and az_noise_target_ex reads."""
    return min((int(HW) + 255) // 256, 64)


def noise_shape(noise, o, offset, fields, table, levels, partials):
    """az_noise_shape, in place over noise (B,C,H,W) fp32: + offset * o (o (B,C) fp32 or None) + the weighted bilinear resamplings of
    the packed level fields.  levels: the host rows (offset, h, w, weight) that `table` (device int32 [n][4], noise.table_tensor) holds
    -- checked against `fields` here, since the table itself is out of the host's sight; [] / None with fields and table None for no
    levels.  partials: (B, noise_partial_blocks(H * W), 2) fp32 or None."""
    _req(noise.dim() == 4 and noise.dtype == F32 and noise.is_contiguous() and noise.is_cuda, "noise_shape noise")
    B, C, H, W = noise.shape
    _req(B > 0 and C * H * W < (1 << 24) and float(offset) >= 0.0, "noise_shape sizes")
    if o is not None:
        _req(o.dtype == F32 and tuple(o.shape) == (B, C) and o.is_contiguous() and o.device == noise.device, "noise_shape offset draw")
    levels = list(levels or [])
    _req(len(levels) <= 8, "noise_shape levels")
    nfields = 0
    if levels:
        _req(fields is not None and table is not None and fields.dtype == F32 and fields.is_contiguous() and fields.device == noise.device and
             table.dtype == torch.int32 and table.is_contiguous() and table.device == noise.device and table.numel() == 4 * len(levels),
             "noise_shape level fields / table")
        nfields = fields.numel()
        for off, h, w, _ in levels:
            _req(h >= 1 and w >= 1 and off >= 0 and off + B * C * h * w <= nfields, "noise_shape level geometry")
    else:
        _req(fields is None and table is None, "noise_shape: level fields without levels")
    if partials is not None:
        _req(partials.dtype == F32 and partials.is_contiguous() and partials.device == noise.device and
             tuple(partials.shape) == (B, noise_partial_blocks(H * W), 2), "noise_shape partials")
    lib().call("az_noise_shape", B, C, H, W, _ptr(noise), _ptr(o), float(offset), _ptr(fields), nfields, _ptr(table), len(levels),
               _ptr(partials), _stream())


def noise_target_ex(mode, latents, noise, coef_a, coef_b, partials, xi, perturb, noisy_nhwc, target):
    """az_noise_target_ex: noise_target with the per-sample normalisation from az_noise_shape's partials (or None) and the input
    perturbation xi (B,C,H,W) fp32 weighed by perturb (or None)."""
    B, C, H, W = latents.shape
    _req(latents.dtype == BF16 and noise.dtype == F32 and latents.is_contiguous() and noise.is_contiguous() and
         noise.shape == latents.shape and coef_a.dtype == F32 and coef_b.dtype == F32 and coef_a.numel() == B and coef_b.numel() == B and
         noisy_nhwc.is_contiguous() and tuple(noisy_nhwc.shape[:3]) == (B, H, W) and noisy_nhwc.dtype == BF16 and noisy_nhwc.shape[3] >= C and
         target.dtype == F32 and target.shape == latents.shape and target.is_contiguous(), "noise_target_ex operands")
    nblk = 0
    if partials is not None:
        nblk = noise_partial_blocks(H * W)
        _req(partials.dtype == F32 and partials.is_contiguous() and tuple(partials.shape) == (B, nblk, 2) and 2 <= C * H * W < (1 << 24),
             "noise_target_ex partials")
    if xi is not None:
        _req(xi.dtype == F32 and xi.is_contiguous() and xi.shape == latents.shape and float(perturb) >= 0.0, "noise_target_ex perturbation")
    lib().call("az_noise_target_ex", int(mode), B, C, H * W, noisy_nhwc.shape[3], _ptr(latents), _ptr(noise), _ptr(coef_a), _ptr(coef_b),
               _ptr(partials), nblk, _ptr(xi), float(perturb) if xi is not None else 0.0, _ptr(noisy_nhwc), _ptr(target), _stream())


def mse_loss_fwd_bwd(pred_nhwc, target, w, grad_scale, loss_out, per_sample, dpred):
    B, H, W, ldp = pred_nhwc.shape
    C = target.shape[1]
    _req(pred_nhwc.dtype == BF16 and pred_nhwc.is_contiguous() and target.dtype == F32 and target.is_contiguous() and
         tuple(target.shape) == (B, C, H, W) and w.dtype == F32 and w.numel() == B and loss_out.dtype == F32 and
         per_sample.dtype == F32 and per_sample.numel() == B, "mse operands")
    cpad = 0
    if dpred is not None:
        _req(dpred.dtype == BF16 and dpred.is_contiguous() and tuple(dpred.shape[:3]) == (B, H, W), "dpred")
        cpad = dpred.shape[3]
    lib().call("az_mse_loss_fwd_bwd", B, C, H * W, _ptr(pred_nhwc), ldp, _ptr(target), _ptr(w), float(grad_scale), _ptr(loss_out),
               _ptr(per_sample), _ptr(dpred), cpad if dpred is not None else C, _ptr(workspace(pred_nhwc.device).scratch), _stream())


ROBUST_KINDS = {"l1": 1, "huber": 2, "smooth_l1": 3}


def robust_loss_fwd_bwd(kind, pred_nhwc, target, w, c, grad_scale, loss_out, per_sample, dpred):
    """az_robust_loss_fwd_bwd: kind "l1" | "huber" | "smooth_l1" (or 1..3), operands as mse_loss_fwd_bwd plus c, the per-sample width
    (fp32 [B]; None for l1 only).  The squared error is mse_loss_fwd_bwd's: it is not a kind here."""
    B, H, W, ldp = pred_nhwc.shape
    C = target.shape[1]
    _req(pred_nhwc.dtype == BF16 and pred_nhwc.is_contiguous() and target.dtype == F32 and target.is_contiguous() and
         tuple(target.shape) == (B, C, H, W) and w.dtype == F32 and w.numel() == B and loss_out.dtype == F32 and
         per_sample.dtype == F32 and per_sample.numel() == B, "robust loss operands")
    if c is not None:
        _req(c.dtype == F32 and c.numel() == B and c.is_contiguous(), "robust loss widths")
    cpad = C
    if dpred is not None:
        _req(dpred.dtype == BF16 and dpred.is_contiguous() and tuple(dpred.shape[:3]) == (B, H, W), "dpred")
        cpad = dpred.shape[3]
    lib().call("az_robust_loss_fwd_bwd", int(ROBUST_KINDS.get(kind, kind)), B, C, H * W, _ptr(pred_nhwc), ldp, _ptr(target), _ptr(w), _ptr(c),
               float(grad_scale), _ptr(loss_out), _ptr(per_sample), _ptr(dpred), cpad, _ptr(workspace(pred_nhwc.device).scratch), _stream())


# ---------------------------------------------------------------------------------------------
# optimizer
# ---------------------------------------------------------------------------------------------

def sumsq(g, out_f32, accumulate):
    _req(g.is_contiguous() and g.dtype in (BF16, F32), "sumsq operand")
    ws = workspace(out_f32.device)
    lib().call("az_sumsq", g.numel(), _ptr(g), int(g.dtype == F32), _ptr(out_f32), int(accumulate), _ptr(ws.scratch), _stream())


def clip_coef(sumsq_f32, max_norm, coef, norm, unscale=1.0):
    lib().call("az_clip_coef", _ptr(sumsq_f32), float(max_norm), float(unscale), _ptr(coef), _ptr(norm), _stream())


def ema_flat(p, ema, one_minus_decay, stream=None):
    """ema <- ema - omd * (ema - float(p)) in place: p bf16 (read only), ema fp32, both 1-D and contiguous, on `stream` (default: the
    current one).  An empty range launches nothing."""
    _req(p.is_cuda and ema.is_cuda and p.device == ema.device and p.dtype == BF16 and ema.dtype == F32, "ema_flat needs cuda bf16 p and fp32 ema")
    _req(p.dim() == 1 and ema.dim() == 1 and p.numel() == ema.numel() and p.is_contiguous() and ema.is_contiguous(), "ema_flat shapes")
    if p.numel() == 0:             # (an empty tensor has no address to hand over)
        return
    st = ctypes.c_void_p(stream.cuda_stream) if stream is not None else _stream()
    lib().call("az_ema_flat", p.numel(), _ptr(p), _ptr(ema), float(one_minus_decay), st)


MOMENT_CODE = {BF16: 0, F32: 1, torch.float16: 2}      # mdtype of the C ABI


def adamw_range(n, p, g, gdtype, m, v, mdtype, hyper, coef, stream, *, master=None, sr=None, host_pipeline=None, groups=None):
    """The Raven / Titan AdamW update of ONE flat range of n elements -- the one place that names the az_adamw_flat* / az_raven_step*
    entry points.  Everything is a raw address or handle (optimizers.RavenAdamW works on storage spans, not tensors), checked by the
    caller: p bf16 parameters, g gradients (gdtype 0 bf16, 1 fp32), m / v moments of torch dtype `mdtype`, hyper the fp32 vector of
    az_adamw_flat, coef the fp32 clip coefficient (None / 0: none), stream the compute stream.
      master=address           fp32 master copy, read and written; p receives bf16(master) (az_adamw_flat_master)
      sr=(seed, step, domain, elem0)                                   stochastic rounding of the bf16 write (az_adamw_flat_sr)
      host_pipeline=(staging address, chunk_elems, h2d stream, d2h stream)    m / v are PINNED HOST memory, streamed in chunks through
                               the device staging buffer on the two copy streams (az_raven_step_ex / az_raven_step_sr)
      groups=(seg_end address, seg_gid address, nseg, ghyper address, ngroups, elem0)      parameter groups: wd_factor and step_size
                               per element from the segment tables (GroupTables.args), everything in ONE launch (az_adamw_flat_seg);
                               with master or sr too, elem0 the global index of the range's first element (sr names the same one)
    master combines with neither of sr / host_pipeline, groups not with host_pipeline: no entry point."""
    if master is not None and (sr is not None or host_pipeline is not None):
        raise AozoraError("adamw_range: master weights combine with neither stochastic rounding nor the pinned-host pipeline")
    if groups is not None and host_pipeline is not None:
        raise AozoraError("adamw_range: parameter groups do not combine with the pinned-host pipeline (no segmented form of the chunk pipeline)")
    vp = ctypes.c_void_p
    rest = (vp(g), int(gdtype), vp(m), vp(v), MOMENT_CODE[mdtype], vp(hyper), vp(coef or 0))
    if groups is not None:
        seg_end, seg_gid, nseg, ghyper, ngroups, elem0 = groups
        if sr is not None and int(sr[3]) != int(elem0):
            raise AozoraError("adamw_range: stochastic rounding and the segment lookup must name the same global element index")
        seed, step, domain = (int(x) for x in sr[:3]) if sr is not None else (0, 0, 0)
        lib().call("az_adamw_flat_seg", int(n), vp(p), vp(master or 0), *rest, vp(seg_end), vp(seg_gid), int(nseg), vp(ghyper), int(ngroups),
                   int(elem0), int(sr is not None), seed, step, domain, vp(stream))
        return
    sr = tuple(int(x) for x in sr) if sr is not None else ()
    if master is not None:
        lib().call("az_adamw_flat_master", int(n), vp(p), vp(master), *rest, vp(stream))
    elif host_pipeline is None:
        lib().call("az_adamw_flat_sr" if sr else "az_adamw_flat_ex", int(n), vp(p), *rest, *sr, vp(stream))
    else:
        staging, chunk_elems, h2d, d2h = host_pipeline
        lib().call("az_raven_step_sr" if sr else "az_raven_step_ex", int(n), vp(p), *rest, vp(staging), int(chunk_elems), vp(stream), vp(h2d),
                   vp(d2h), *sr)


def check_group_tables(seg_end, seg_gid, ngroups, ranges=()):
    """The host copy of a segment table (adamw_range's groups=) before it is uploaded: as many ids as ends, ends ascending, ids in
    [0, ngroups), 1 <= ngroups <= 255, and every updated range [a, b) of `ranges` inside [0, last end)."""
    seg_end, seg_gid = [int(x) for x in seg_end], [int(x) for x in seg_gid]
    _req(len(seg_end) > 0 and len(seg_end) == len(seg_gid), "segment table: seg_end and seg_gid need one entry per segment, at least one")
    _req(1 <= int(ngroups) <= 255, "segment table: 1 to 255 groups")
    _req(seg_end[0] > 0 and all(a < b for a, b in zip(seg_end, seg_end[1:])), "segment table: ends must be positive and strictly ascending")
    _req(all(0 <= g < int(ngroups) for g in seg_gid), "segment table: a group id outside [0, number of groups)")
    _req(all(0 <= a <= b <= seg_end[-1] for a, b in ranges), "segment table: an updated range is not covered by the segments")
    return seg_end, seg_gid


def upload_group_tables(seg_end, seg_gid, ngroups, ranges, device):
    """check_group_tables, then the two tables on `device` once (they never change during a run) -> (int64 ends, int32 ids)."""
    seg_end, seg_gid = check_group_tables(seg_end, seg_gid, ngroups, ranges)
    return torch.tensor(seg_end, dtype=torch.int64).to(device), torch.tensor(seg_gid, dtype=torch.int32).to(device)


def adamw_flat_master(p, w, g, m, v, hyper, coef=None, stream=None):
    """The Raven / Titan AdamW update with an fp32 master copy: w (fp32, read and written) is the parameter operand, p (bf16) receives
    bf16(w) and is never read; g bf16 or fp32, m / v bf16, fp32 or fp16, hyper the fp32 vector of az_adamw_flat, coef None or a device
    fp32 scalar.  All 1-D, contiguous, of one length, on `stream` (default: the current one).  An empty range launches nothing."""
    ts = (p, w, g, m, v)
    _req(all(t.is_cuda and t.device == p.device for t in ts + (hyper,)) and (coef is None or (coef.is_cuda and coef.device == p.device)),
         "adamw_flat_master needs cuda tensors on one device")
    _req(p.dtype == BF16 and w.dtype == F32 and g.dtype in (BF16, F32) and m.dtype in MOMENT_CODE and v.dtype == m.dtype,
         "adamw_flat_master needs bf16 p, fp32 w, bf16 / fp32 g and bf16 / fp32 / fp16 moments of one type")
    _req(all(t.dim() == 1 and t.is_contiguous() and t.numel() == p.numel() for t in ts), "adamw_flat_master shapes")
    _req(hyper.dtype == F32 and hyper.is_contiguous() and hyper.numel() >= 7, "adamw_flat_master needs the fp32 hyper vector of 7+ entries")
    _req(coef is None or (coef.dtype == F32 and coef.numel() >= 1), "adamw_flat_master needs an fp32 clip coefficient")
    if p.numel() == 0:             # (an empty tensor has no address to hand over)
        return
    adamw_range(p.numel(), p.data_ptr(), g.data_ptr(), int(g.dtype == F32), m.data_ptr(), v.data_ptr(), m.dtype, hyper.data_ptr(),
                coef.data_ptr() if coef is not None else None, (stream if stream is not None else torch.cuda.current_stream()).cuda_stream,
                master=w.data_ptr())
