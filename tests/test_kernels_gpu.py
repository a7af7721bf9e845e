"""Per-kernel parity: every HIP entry point (through the C ABI) vs the same op in fp32 PyTorch on
the CPU, on identical bf16-rounded inputs.  Tolerance (stated per north_star: floating point):
bf16 outputs carry 2^-9 relative rounding, so we require relative Frobenius error <= 4e-3 and
max abs error <= 2e-2 * max|ref| unless a test says otherwise."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd import ops as _ops
    return _ops


def bf(t):
    return t.to(torch.bfloat16)


def check(out, ref, name, fro=4e-3, mx=2e-2):
    out = out.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    assert torch.isfinite(out).all(), name + ": non-finite output"
    denom = ref.norm().item() + 1e-12
    e_fro = (out - ref).norm().item() / denom
    e_max = (out - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)
    assert e_fro <= fro and e_max <= mx, f"{name}: rel_fro={e_fro:.3e} (<= {fro}) rel_max={e_max:.3e} (<= {mx})"


_ctr = [0]


def rnd(*shape, scale=1.0, seed=None):
    _ctr[0] += 1
    g = torch.Generator().manual_seed(seed if seed is not None else (1000 + _ctr[0]))
    return bf(torch.randn(*shape, generator=g) * scale)


@pytest.fixture(params=[(0, 0, 0), (256, 256, 0), (128, 160, 8), (128, 160, 24), (128, 128, 8),
                        (128, 160, 40), (128, 160, 56), (256, 256, 32),      # 40 / 56 / 32: rings of 4 / 5 / 4 stages of 32-deep k-tiles
                        (256, 256, 8), (256, 320, 8), (128, 160, 72)],        # the 8-wave ping-pong tile (az_gemm8.inc), 256 / 320 wide; 72: 4 stages of 64-deep k-tiles
                ids=lambda t: f"tile{t[0]}x{t[1]}w{t[2]}")
def tile(request, ops):
    """GEMM / conv tests run under the heuristic and under every forced cooperative tile (the 128x160 tile exists for
    k-contiguous B only; the other products ignore that force and use 128x128)."""
    from aozora_sdxl_training_amd._lib import lib
    lib().call("az_gemm_set_tile_ex", *request.param)
    yield request.param
    lib().call("az_gemm_set_tile", 0, 0)


# ------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(128, 128, 64), (300, 200, 136), (4, 1280, 320), (308, 1280, 2048), (1000, 640, 1280), (513, 72, 64), (64, 8, 2048), (700, 520, 264),
               (600, 960, 192), (257, 328, 64), (1100, 648, 448)]      # K % 64 == 0: the shapes the 8-wave tile takes when forced (ragged rows / columns, 1 and 3 and 7 k-tiles)


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_nt_bias_residual(ops, tile, M, N, K):
    a, w, bias, res = rnd(M, K), rnd(N, K, scale=K ** -0.5), rnd(N), rnd(M, N)
    ref = a.float() @ w.float().t() + bias.float() + res.float()
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    ops.gemm(a.to(DEV), w.to(DEV), out, trans_b=True, bias=bias.to(DEV), residual=res.to(DEV))
    check(out, ref, f"gemm_nt {M}x{N}x{K}")


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_nn_dgrad_accumulate(ops, tile, M, N, K):
    # dX[M,N] += dY[M,K] @ W[K,N]
    dy, w, prev = rnd(M, K), rnd(K, N, scale=K ** -0.5), rnd(M, N)
    ref = prev.float() + dy.float() @ w.float()
    out = prev.to(DEV).clone()
    ops.gemm(dy.to(DEV), w.to(DEV), out, trans_b=False, accumulate=True)
    check(out, ref, f"gemm_nn {M}x{N}x{K}")


@pytest.mark.parametrize("M,N,K,split", [(128, 128, 64, 1), (640, 640, 4096, 0), (1280, 320, 308, 0), (72, 320, 1000, 4), (8, 2880, 520, 0), (200, 136, 304, 3)])
def test_gemm_tn_wgrad_splitk(ops, tile, M, N, K, split):
    # dW[M,N] (+)= dY[K,M]^T @ X[K,N]
    dy, x, prev = rnd(K, M), rnd(K, N), rnd(M, N, scale=0.1)
    ref = prev.float() + dy.float().t() @ x.float()
    out = prev.to(DEV).clone()
    ops.gemm(dy.to(DEV), x.to(DEV), out, trans_a=True, trans_b=False, accumulate=True, split_k=split)
    check(out, ref, f"gemm_tn {M}x{N}x{K} split={split}")
    # the same product with the bias gradient (column sums of dY) fused in: identical dW, bias += dY.sum(0)
    n_real = M if M % 8 else M - 3            # also a bias shorter than the padded output-channel count
    bprev = rnd(n_real, scale=0.1)
    out2, bg = prev.to(DEV).clone(), bprev.to(DEV).clone()
    ops.gemm(dy.to(DEV), x.to(DEV), out2, trans_a=True, trans_b=False, accumulate=True, split_k=split, bias_grad=bg)
    assert torch.equal(out2, out), "fused bias gradient must not change dW"
    check(bg, bprev.float() + dy.float().sum(0)[:n_real], f"fused bias grad {M}x{N}x{K} split={split}", fro=4e-3, mx=3e-2)


def test_gemm_tn_grouped_many_weight_gradients_in_one_launch(ops):
    """az_gemm_tn_grouped_bf16: independent products dW_g += dY_g^T X_g (+ fused bias gradients) of different shapes and k-depths in
    ONE launch, every product over its whole k-range (no split-K): each equals the fp32 reference, strided operands and padding are
    respected, a repeated launch is bitwise reproducible, and untouched memory stays untouched."""
    shapes = [(640, 640, 1000, True), (1280, 320, 308, True), (72, 328, 520, False), (200, 136, 304, True), (130, 8, 64, True), (384, 1288, 2048, False)]
    jobs, refs, brefs, keep = [], [], [], []
    for g, (M, N, K, with_b) in enumerate(shapes):
        up8 = lambda v: ((v + 7) // 8) * 8
        dy_w = torch.zeros(K, up8(M) + 8, dtype=torch.bfloat16, device=DEV); x_w = torch.zeros(K, up8(N) + 16, dtype=torch.bfloat16, device=DEV)
        dy, x, prev = rnd(K, M), rnd(K, N), rnd(M, N, scale=0.1)
        dy_w[:, :M] = dy.to(DEV); x_w[:, :N] = x.to(DEV)
        dw_w = torch.full((M, up8(N) + 8), 3.0, dtype=torch.bfloat16, device=DEV); dw_w[:, :N] = prev.to(DEV)
        n_real = M if M % 8 else M - 3
        bprev = rnd(n_real, scale=0.1)
        bg = bprev.to(DEV).clone() if with_b else None
        jobs.append((dy_w[:, :M], x_w[:, :N], dw_w[:, :N], bg))
        refs.append(prev.float() + dy.float().t() @ x.float())
        brefs.append(bprev.float() + dy.float().sum(0)[:n_real] if with_b else None)
        keep.append((dw_w, prev, bprev))
    tab = ops.tn_group_table(jobs, torch.device(DEV))
    assert tab[1] == len(shapes) and tab[2] == sum(((M + 127) // 128) * ((N + 127) // 128) for M, N, _, _ in shapes)
    ops.gemm_tn_grouped(*tab)
    outs = [(j[2].clone(), j[3].clone() if j[3] is not None else None) for j in jobs]
    order = sorted(range(len(shapes)), key=lambda g: -shapes[g][2])          # the table is sorted by k-depth; jobs keep their own tensors
    for g in range(len(shapes)):
        M, N, K, with_b = shapes[g]
        check(jobs[g][2], refs[g], f"grouped wgrad product {g} {M}x{N}x{K}")
        assert float((keep[g][0][:, N:] - 3.0).abs().max()) == 0.0, "padding columns of dW were written"
        if with_b:
            check(jobs[g][3], brefs[g], f"grouped wgrad bias gradient {g}", fro=4e-3, mx=3e-2)
    # reproducible: reset the targets and launch again
    for g, (dw_w, prev, bprev) in enumerate(keep):
        dw_w[:, :shapes[g][1]] = prev.to(DEV)
        if jobs[g][3] is not None:
            jobs[g][3].copy_(bprev.to(DEV))
    ops.gemm_tn_grouped(*tab)
    for g in range(len(shapes)):
        assert torch.equal(jobs[g][2], outs[g][0]) and (outs[g][1] is None or torch.equal(jobs[g][3], outs[g][1])), "grouped wgrad not reproducible"
    assert order[0] == 5


@pytest.mark.parametrize("M,K", [(308, 2048), (4, 1280), (200, 136)])
def test_gemm_nt_grouped_matches_separate_products(ops, M, K):
    """az_gemm_nt_grouped_bf16: products that share A in one launch (K/V of the text context for every cross-attention layer,
    time_emb_proj of every resnet) == each product on its own, bit for bit where the same tile is used, and vs fp32."""
    a = rnd(M, K, seed=5)
    Ns = [2560, 1280, 320, 168, 640]
    Ws = [rnd(N, K, scale=K ** -0.5, seed=10 + i) for i, N in enumerate(Ns)]
    bs = [rnd(N, seed=30 + i) if i % 2 == 0 else None for i, N in enumerate(Ns)]
    ad = a.to(DEV)
    Wd = [w.to(DEV) for w in Ws]
    bd = [b.to(DEV) if b is not None else None for b in bs]
    outs = [torch.full((M, N + 8), 3.0, dtype=torch.bfloat16, device=DEV)[:, :N] for N in Ns]       # strided outputs
    recs, tiles = [], 0
    for w, b, o in zip(Wd, bd, outs):
        recs.append([w.data_ptr(), o.data_ptr(), b.data_ptr() if b is not None else 0, w.shape[0], w.stride(0), o.stride(0), tiles])
        tiles += (w.shape[0] + 159) // 160
    table = torch.tensor(recs, dtype=torch.int64, device=DEV)
    for exclusive in (0, 1):           # 2-stage and 3-stage (forward pass) variants
        from aozora_sdxl_training_amd._lib import set_option
        set_option("LDS_EXCLUSIVE", exclusive)
        try:
            for o in outs:
                o.fill_(3.0)
            ops.gemm_nt_grouped(ad, table, len(recs), tiles)
        finally:
            set_option("LDS_EXCLUSIVE", 0)
        for w, b, o in zip(Ws, bs, outs):
            ref = a.float() @ w.float().t() + (b.float() if b is not None else 0.0)
            check(o, ref, f"grouped nt {M}x{w.shape[0]}x{K}")
            assert bool((o.as_strided((M, 8), (o.stride(0), 1), o.shape[1]) == 3.0).all())       # padding columns untouched


def test_gemm_rowbias_strided_views(ops, tile):
    # strided operands (lda > K, ldc > N) and a per-segment row bias (time-embedding add)
    M, N, K = 256, 192, 128
    abuf, cbuf = rnd(M, K + 64), torch.zeros(M, N + 64, dtype=torch.bfloat16)
    w, rb = rnd(N, K, scale=K ** -0.5), rnd(4, N)
    ref = abuf[:, :K].float() @ w.float().t() + rb.float().repeat_interleave(64, dim=0)
    ad, cd = abuf.to(DEV), cbuf.to(DEV)
    ops.gemm(ad[:, :K], w.to(DEV), cd[:, 32:32 + N], trans_b=True, rowbias=rb.to(DEV), rows_per_seg=64)
    check(cd[:, 32:32 + N], ref, "gemm rowbias strided")
    assert cd[:, :32].abs().max().item() == 0 and cd[:, 32 + N:].abs().max().item() == 0


# ------------------------------------------------------------------------------------------------
CONV_CASES = [  # B, H, W, Cin, Cout, ks, stride
    (2, 16, 16, 64, 64, 3, 1), (1, 12, 20, 320, 128, 3, 1), (2, 16, 16, 64, 128, 3, 2), (2, 9, 7, 72, 40, 3, 1),
    (2, 8, 8, 128, 64, 1, 1), (2, 16, 16, 8, 320, 3, 1), (2, 16, 16, 320, 4, 3, 1), (1, 14, 14, 64, 64, 3, 2),
    # fast gathers (tap as a scalar, validity masks, multiply-high pixel decode) on grids that are no powers of two and span
    # several samples: the 768 px bucket's 24 x 24 level, a ragged 28 x 20 one
    (3, 24, 24, 128, 64, 3, 1), (2, 28, 20, 64, 192, 3, 1),
]


def _conv_ref(x, w, b, stride, ks):
    xn = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    wn = w.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.conv2d(xn, wn, b.float() if b is not None else None, stride=stride, padding=1 if ks == 3 else 0)
    return xn, wn, y


@pytest.mark.parametrize("B,H,W,Cin,Cout,ks,stride", CONV_CASES)
def test_conv_fwd_dgrad_wgrad(ops, tile, B, H, W, Cin, Cout, ks, stride):
    x, w, b = rnd(B, H, W, Cin), rnd(Cout, ks, ks, Cin, scale=(ks * ks * Cin) ** -0.5), rnd(Cout)
    xn, wn, y = _conv_ref(x, w, b, stride, ks)
    Ho, Wo = y.shape[2], y.shape[3]
    rb, res = rnd(B, Cout), rnd(B, Ho, Wo, Cout)
    yref = y + rb.float()[:, :, None, None] + res.float().permute(0, 3, 1, 2)
    out = torch.empty(B, Ho, Wo, Cout, dtype=torch.bfloat16, device=DEV)
    ops.conv_fwd(x.to(DEV), w.to(DEV), out, stride=stride, bias=b.to(DEV), rowbias=rb.to(DEV), residual=res.to(DEV))
    check(out, yref.permute(0, 2, 3, 1), f"conv_fwd {B,H,W,Cin,Cout,ks,stride}")

    cpad = ((Cout + 7) // 8) * 8
    dy = torch.zeros(B, Ho, Wo, cpad, dtype=torch.bfloat16)
    dy[..., :Cout] = rnd(B, Ho, Wo, Cout)
    y.backward(dy[..., :Cout].float().permute(0, 3, 1, 2))
    dyd = dy.to(DEV)
    if ks == 3:
        dx = torch.empty(B, H, W, Cin, dtype=torch.bfloat16, device=DEV)
        ops.conv_dgrad(dyd, w.to(DEV), dx, stride=stride, cout_real=Cout)
        check(dx, xn.grad.permute(0, 2, 3, 1), f"conv_dgrad {B,H,W,Cin,Cout,ks,stride}")
        if Cout % 8 == 0:      # NT-form dgrad on the pre-transposed weight copy W'[Cin][3][3][Cout]
            wt = w.permute(3, 1, 2, 0).contiguous().to(DEV)
            dx2 = torch.empty_like(dx)
            ops.conv_dgrad_wt(dyd, wt, dx2, stride=stride)
            check(dx2, xn.grad.permute(0, 2, 3, 1), f"conv_dgrad_wt {B,H,W,Cin,Cout,ks,stride}")
    prev = rnd(Cout, ks, ks, Cin, scale=0.05)
    dw = prev.to(DEV).clone()
    ops.conv_wgrad(dyd, x.to(DEV), dw, stride=stride, cout_real=Cout, accumulate=True, split_k=0)
    check(dw, prev.float() + wn.grad.permute(0, 2, 3, 1), f"conv_wgrad {B,H,W,Cin,Cout,ks,stride}")
    # fused bias gradient and per-sample channel sums (time-embedding gradient) in the same pass
    bprev = rnd(Cout, scale=0.1)
    dw2, bg = prev.to(DEV).clone(), bprev.to(DEV).clone()
    seg = torch.full((B, Cout), 9.0, dtype=torch.bfloat16, device=DEV) if (Ho * Wo) % 64 == 0 else None
    ops.conv_wgrad(dyd, x.to(DEV), dw2, stride=stride, cout_real=Cout, accumulate=True, split_k=0, bias_grad=bg, seg_grad=seg)
    assert torch.equal(dw2, dw), "fused channel sums must not change dW"
    sums = dy[..., :Cout].float().sum((1, 2))
    check(bg, bprev.float() + sums.sum(0), f"conv fused bias grad {B,H,W,Cin,Cout,ks,stride}", fro=4e-3, mx=3e-2)
    if seg is not None:
        check(seg, sums, f"conv fused per-sample sums {B,H,W,Cin,Cout,ks,stride}", fro=4e-3, mx=3e-2)


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,heads,Tq,Tk", [(2, 3, 128, 128), (1, 5, 200, 77), (2, 2, 1024, 1024), (1, 2, 333, 154), (1, 1, 64, 64),
                                           (1, 2, 784, 784), (1, 1, 576, 576), (2, 1, 35, 35), (1, 1, 3136, 3136),   # ragged self-attention: 896 / 768 px buckets
                                           (16, 8, 1024, 1024), (16, 8, 1000, 154),    # grids of >= 1024 workgroups
                                           (2, 3, 1024, 256), (1, 2, 256, 1024)])      # Tq != Tk on whole 128-row blocks: the LDS-DMA backward bodies outside self-attention
def test_attention_fwd_bwd(ops, B, heads, Tq, Tk):
    C = heads * 64
    # q,k,v as column slices of one fused projection buffer (the layout the UNet uses)
    qkv = rnd(B, Tq, 3 * C, scale=1.0) if Tq == Tk else None
    if qkv is not None:
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        qkvd = qkv.to(DEV)
        qd, kd, vd = qkvd[..., :C], qkvd[..., C:2 * C], qkvd[..., 2 * C:]
    else:
        q = rnd(B, Tq, C)
        kv = rnd(B, Tk, 2 * C)
        k, v = kv[..., :C], kv[..., C:]
        qd = q.to(DEV); kvd = kv.to(DEV); kd, vd = kvd[..., :C], kvd[..., C:]
    do = rnd(B, Tq, C)
    qf = q.float().reshape(B, Tq, heads, 64).transpose(1, 2).requires_grad_(True)
    kf = k.float().reshape(B, Tk, heads, 64).transpose(1, 2).requires_grad_(True)
    vf = v.float().reshape(B, Tk, heads, 64).transpose(1, 2).requires_grad_(True)
    s = (qf @ kf.transpose(-1, -2)) * 0.125
    o_ref = (torch.softmax(s, dim=-1) @ vf)
    lse_ref = torch.logsumexp(s, dim=-1) * math.log2(math.e)
    o_ref.backward(do.float().reshape(B, Tq, heads, 64).transpose(1, 2))
    o = torch.empty(B, Tq, C, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B * heads * Tq, dtype=torch.float32, device=DEV)
    ops.attn_fwd(qd, kd, vd, o, lse, heads, 0.125)
    check(o, o_ref.transpose(1, 2).reshape(B, Tq, C), f"attn_fwd {B,heads,Tq,Tk}")
    check(lse.view(B, heads, Tq), lse_ref, "attn lse", fro=1e-4, mx=1e-3)
    dq = torch.empty(B, Tq, C, dtype=torch.bfloat16, device=DEV)
    dkv = torch.empty(B, Tk, 2 * C, dtype=torch.bfloat16, device=DEV)
    delta = torch.empty(B * heads * Tq, dtype=torch.float32, device=DEV)
    ops.attn_bwd(qd, kd, vd, o, do.to(DEV), lse, delta, dq, dkv[..., :C], dkv[..., C:], heads, 0.125)
    check(dq, qf.grad.transpose(1, 2).reshape(B, Tq, C), "attn dq", fro=8e-3, mx=3e-2)
    check(dkv[..., :C], kf.grad.transpose(1, 2).reshape(B, Tk, C), "attn dk", fro=8e-3, mx=3e-2)
    check(dkv[..., C:], vf.grad.transpose(1, 2).reshape(B, Tk, C), "attn dv", fro=8e-3, mx=3e-2)


@pytest.mark.parametrize("spike_row,spike", [(700, 6.0), (70, 3.0), (1023, 8.0)])
def test_attention_forward_deferred_maximum_rescale(ops, spike_row, spike):
    """The pipelined forward raises its running maximum only when a tile's scores exceed it by more than 2^4 (az_attn.hip, guide
    T13): random data never takes that branch after the first tile, so one key row is made large at a chosen tile (guide 5.4
    rule 26: an input that FORCES the branch, checked against a full fp32 reference).  Backward on the same inputs."""
    B, heads, T = 2, 3, 1024
    C = heads * 64
    qkv = rnd(B, T, 3 * C, scale=1.0, seed=5)
    k = qkv[..., C:2 * C]
    k[:, spike_row, :] = bf(torch.where(torch.arange(C) % 2 == 0, -spike, spike).float()).expand(B, C)
    q, v = qkv[..., :C], qkv[..., 2 * C:]
    qkvd = qkv.to(DEV)
    qd, kd, vd = qkvd[..., :C], qkvd[..., C:2 * C], qkvd[..., 2 * C:]
    do = rnd(B, T, C, seed=6)
    qf = q.float().reshape(B, T, heads, 64).transpose(1, 2).requires_grad_(True)
    kf = k.float().reshape(B, T, heads, 64).transpose(1, 2).requires_grad_(True)
    vf = v.float().reshape(B, T, heads, 64).transpose(1, 2).requires_grad_(True)
    s = (qf @ kf.transpose(-1, -2)) * 0.125
    before = s.detach()[..., :max(64, spike_row - spike_row % 64)].amax(-1)
    assert ((s.detach()[..., spike_row] - before) * math.log2(math.e)).max() > 4.0, "spike too small to force a rescale"
    o_ref = torch.softmax(s, dim=-1) @ vf
    lse_ref = torch.logsumexp(s, dim=-1) * math.log2(math.e)
    o_ref.backward(do.float().reshape(B, T, heads, 64).transpose(1, 2))
    o = torch.empty(B, T, C, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B * heads * T, dtype=torch.float32, device=DEV)
    ops.attn_fwd(qd, kd, vd, o, lse, heads, 0.125)
    check(o, o_ref.transpose(1, 2).reshape(B, T, C), f"attn_fwd with a spiked key row {spike_row}")
    check(lse.view(B, heads, T), lse_ref, "attn lse", fro=1e-4, mx=2e-3)
    dqkv = torch.empty(B, T, 3 * C, dtype=torch.bfloat16, device=DEV)
    delta = torch.empty(B * heads * T, dtype=torch.float32, device=DEV)
    ops.attn_bwd(qd, kd, vd, o, do.to(DEV), lse, delta, dqkv[..., :C], dqkv[..., C:2 * C], dqkv[..., 2 * C:], heads, 0.125)
    check(dqkv[..., :C], qf.grad.transpose(1, 2).reshape(B, T, C), "attn dq", fro=8e-3, mx=6e-2)
    check(dqkv[..., C:2 * C], kf.grad.transpose(1, 2).reshape(B, T, C), "attn dk", fro=8e-3, mx=6e-2)
    check(dqkv[..., 2 * C:], vf.grad.transpose(1, 2).reshape(B, T, C), "attn dv", fro=8e-3, mx=6e-2)


@pytest.mark.parametrize("B,heads,Tq,Tk", [(2, 3, 1024, 77), (1, 5, 200, 77), (2, 2, 1000, 128), (4, 20, 1024, 77)])
def test_attention_backward_forms_agree(ops, B, heads, Tq, Tk):
    """Short key axis: the one-kernel backward (parts = 7, option ATTN_PIPE bit 2) against the three-launch form the executor uses
    when it puts dK / dV on the parameter-gradient stream (parts 3 + 4): dQ bit for bit, dK / dV to fp32 summation order."""
    C = heads * 64
    q, kv, do = rnd(B, Tq, C, seed=31).to(DEV), rnd(B, Tk, 2 * C, seed=32).to(DEV), rnd(B, Tq, C, seed=33).to(DEV)
    k, v = kv[..., :C], kv[..., C:]
    o = torch.empty(B, Tq, C, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B * heads * Tq, dtype=torch.float32, device=DEV)
    ops.attn_fwd(q, k, v, o, lse, heads, 0.125)
    outs = []
    for parts in ((7,), (3, 4)):
        dq = torch.full((B, Tq, C), 7.0, dtype=torch.bfloat16, device=DEV)
        dkv = torch.full((B, Tk, 2 * C), 7.0, dtype=torch.bfloat16, device=DEV)
        delta = torch.empty(B * heads * Tq, dtype=torch.float32, device=DEV)
        for p in parts:
            ops.attn_bwd(q, k, v, o, do, lse, delta, dq, dkv[..., :C], dkv[..., C:], heads, 0.125, parts=p)
        outs.append((dq, dkv))
    assert torch.equal(outs[0][0], outs[1][0]), "dQ of the fused and the three-launch backward differ"
    check(outs[0][1], outs[1][1].float().cpu(), "fused dK | dV vs three-launch form", fro=2e-3, mx=2e-2)


def _attn_run(ops, qkvd, do, heads, C, B, T):
    qd, kd, vd = qkvd[..., :C], qkvd[..., C:2 * C], qkvd[..., 2 * C:]
    o = torch.full((B, T, C), 3.0, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B * heads * T, dtype=torch.float32, device=DEV)
    ops.attn_fwd(qd, kd, vd, o, lse, heads, 0.125)
    dqkv = torch.full((B, T, 3 * C), 5.0, dtype=torch.bfloat16, device=DEV)
    delta = torch.empty(B * heads * T, dtype=torch.float32, device=DEV)
    ops.attn_bwd(qd, kd, vd, o, do, lse, delta, dqkv[..., :C], dqkv[..., C:2 * C], dqkv[..., 2 * C:], heads, 0.125)
    torch.cuda.synchronize()
    return o, lse, dqkv


@pytest.mark.parametrize("B,heads,T", [(2, 3, 1024), (1, 2, 4096), (3, 5, 256), (16, 8, 1024)])
def test_attention_option_toggles_keep_the_fallback_kernels_honest(ops, B, heads, T):
    """The default attention paths are option-selected (ATTN_PIPE bit 0: pipelined LDS-DMA forward, bit 1: dQ and dK/dV roles in one
    launch, bit 3: LDS-DMA backward bodies; ATTN_XCD: workgroup order), so the plain kernels only run for odd shapes unless a test
    turns the options off.  Workgroup
    placement (ATTN_XCD 0 vs 15) must not change a single bit of O, lse, dQ, dK, dV; the merged backward must match the two-launch
    form given the same O / lse (same bodies, other grid, delta summed in another order); the pipelined forward (other summation order, deferred
    maximum, rotated key order) agrees with the plain one to bf16 rounding.  The last shape has grids of 1024 / 2048 workgroups
    (the remap's n % 8 == 0 case); (3, 5, 256) has 30 of them (n % 8 != 0: the bijective form)."""
    from aozora_sdxl_training_amd._lib import set_option, get_option
    C = heads * 64
    qkvd, do = rnd(B, T, 3 * C, seed=41).to(DEV), rnd(B, T, C, seed=42).to(DEV)
    pipe0 = get_option("ATTN_PIPE")
    try:
        res = {}
        for pipe in (15, 14, 13, 12, 7, 6, 5, 4):        # bit 0: forward form, bit 1: merged backward, bit 3: LDS-DMA backward bodies
            for xcd in (15, 0):
                set_option("ATTN_PIPE", pipe); set_option("ATTN_XCD", xcd)
                res[(pipe, xcd)] = _attn_run(ops, qkvd, do, heads, C, B, T)
            for a, b in zip(res[(pipe, 15)], res[(pipe, 0)]):
                assert torch.equal(a, b), f"ATTN_XCD changed a result under ATTN_PIPE={pipe}"
        # same forward (bit 0 equal) -> merged and two-launch backward agree to the summation order of delta = rowsum(dO o O)
        # (its own kernel in front of the merged launch, the dQ kernel's resident fragments in the two-launch form)
        for dma in (8, 0):
            for fw in (1, 0):
                a, b = res[(dma | 6 | fw, 15)], res[(dma | 4 | fw, 15)]
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
                check(a[2], b[2].float().cpu(), "merged backward vs the dQ + dK/dV launches", fro=1e-3, mx=2e-2)
        # the LDS-DMA backward bodies run the same MFMAs in the same order on the same values as the register-staged ones: bit for bit
        for low in (7, 6, 5, 4):
            for a, b in zip(res[(8 | low, 15)], res[(low, 15)]):
                assert torch.equal(a, b), f"LDS-DMA backward bodies differ from the register-staged ones under ATTN_PIPE={low}"
        # pipelined vs plain forward: to rounding; the backward sees O / lse of its own forward
        pl, pi = res[(14, 15)], res[(15, 15)]
        check(pi[0], pl[0].float().cpu(), "pipelined vs plain forward O", fro=4e-3, mx=2e-2)
        check(pi[1], pl[1].cpu(), "pipelined vs plain forward lse", fro=1e-4, mx=2e-3)
        check(pi[2], pl[2].float().cpu(), "backward behind either forward", fro=4e-3, mx=3e-2)
    finally:
        set_option("ATTN_PIPE", pipe0); set_option("ATTN_XCD", 15)


@pytest.mark.parametrize("B,heads,Tq,Tk", [(2, 3, 1024, 77), (4, 20, 1024, 77), (1, 5, 200, 154)])
def test_attention_workgroup_order_is_bitwise_neutral_for_short_keys(ops, B, heads, Tq, Tk):
    """ATTN_XCD 0 vs 15 for the cross-attention kernels (plain forward, one-kernel backward and the query-split dK/dV kernel with its
    ordered reduce, whose (x, z, y) decode differs from the plain (x, y, z) one): bit for bit."""
    from aozora_sdxl_training_amd._lib import set_option
    C = heads * 64
    q, kv, do = rnd(B, Tq, C, seed=51).to(DEV), rnd(B, Tk, 2 * C, seed=52).to(DEV), rnd(B, Tq, C, seed=53).to(DEV)
    k, v = kv[..., :C], kv[..., C:]
    outs = []
    try:
        for xcd in (15, 0):
            set_option("ATTN_XCD", xcd)
            o = torch.empty(B, Tq, C, dtype=torch.bfloat16, device=DEV)
            lse = torch.empty(B * heads * Tq, dtype=torch.float32, device=DEV)
            ops.attn_fwd(q, k, v, o, lse, heads, 0.125)
            got = [o, lse]
            for parts in ((7,), (3, 4)):
                dq = torch.full((B, Tq, C), 7.0, dtype=torch.bfloat16, device=DEV)
                dkv = torch.full((B, Tk, 2 * C), 7.0, dtype=torch.bfloat16, device=DEV)
                delta = torch.empty(B * heads * Tq, dtype=torch.float32, device=DEV)
                for p in parts:
                    ops.attn_bwd(q, k, v, o, do, lse, delta, dq, dkv[..., :C], dkv[..., C:], heads, 0.125, parts=p)
                got += [dq, dkv]
            torch.cuda.synchronize()
            outs.append(got)
        for a, b in zip(*outs):
            assert torch.equal(a, b), "ATTN_XCD changed a cross-attention result"
    finally:
        set_option("ATTN_XCD", 15)


def test_xcd_split_option_is_bitwise_neutral(ops):
    """Option XCD_SPLIT deals the k-SPLITS of a split-K weight gradient to the XCDs (1-D split-major grid) instead of the tiles of
    every split: 'speed only, any placement computes the same slabs' -- asserted bit for bit on a linear weight gradient with a fused
    bias gradient (5 and automatic splits) and on a convolution weight gradient with per-sample sums."""
    from aozora_sdxl_training_amd._lib import set_option
    res = []
    try:
        for xs in (1, 0):
            set_option("XCD_SPLIT", xs)
            got = []
            for M, N, K, split in ((1280, 1280, 4096, 5), (640, 640, 16384, 0), (1280, 320, 4096, 3)):
                dy, x, prev, bprev = rnd(K, M, seed=61), rnd(K, N, seed=62), rnd(M, N, scale=0.1, seed=63), rnd(M, scale=0.1, seed=64)
                out, bg = prev.to(DEV).clone(), bprev.to(DEV).clone()
                ops.gemm(dy.to(DEV), x.to(DEV), out, trans_a=True, trans_b=False, accumulate=True, split_k=split, bias_grad=bg)
                got += [out, bg]
            B, H, W, Ci, Co = 2, 32, 32, 320, 320
            xc, dyc = rnd(B, H, W, Ci, seed=65), rnd(B, H, W, Co, seed=66)
            dw = torch.zeros(Co, 3, 3, Ci, dtype=torch.bfloat16, device=DEV)
            bgc = torch.zeros(Co, dtype=torch.bfloat16, device=DEV)
            seg = torch.zeros(B, Co, dtype=torch.bfloat16, device=DEV)
            ops.conv_wgrad(dyc.to(DEV), xc.to(DEV), dw, accumulate=True, split_k=0, bias_grad=bgc, seg_grad=seg)
            torch.cuda.synchronize()
            res.append(got + [dw, bgc, seg])
        for a, b in zip(*res):
            assert torch.equal(a, b), "XCD_SPLIT changed a weight gradient"
    finally:
        set_option("XCD_SPLIT", 1)


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW,C,G,silu,eps", [(2, 256, 320, 32, True, 1e-5), (2, 100, 640, 32, False, 1e-6), (1, 64, 2560, 32, True, 1e-5),
                                               (3, 49, 32, 8, True, 1e-5), (2, 1024, 960, 32, True, 1e-5)])
def test_groupnorm_fwd_bwd(ops, B, HW, C, G, silu, eps):
    x = bf(rnd(B, HW, C).float() * 1.5 + 0.3)
    gamma, beta, dy = bf(1 + 0.2 * rnd(C).float()), rnd(C, scale=0.2), rnd(B, HW, C)
    xf = x.float().permute(0, 2, 1).requires_grad_(True)   # (B,C,HW)
    gf, bfl = gamma.float().requires_grad_(True), beta.float().requires_grad_(True)
    y = F.group_norm(xf, G, gf, bfl, eps)
    if silu:
        y = F.silu(y)
    y.backward(dy.float().permute(0, 2, 1))
    xd, yd = x.to(DEV), torch.empty(B, HW, C, dtype=torch.bfloat16, device=DEV)
    stats = torch.empty(B * G * 2, dtype=torch.float32, device=DEV)
    ops.groupnorm_fwd(xd, gamma.to(DEV), beta.to(DEV), yd, stats, G, eps, silu)
    check(yd, y.permute(0, 2, 1), f"gn_fwd {B,HW,C,G,silu}")
    prev_dx = rnd(B, HW, C, scale=0.1)
    dx = prev_dx.to(DEV).clone()
    dg = torch.zeros(C, dtype=torch.bfloat16, device=DEV)
    db = torch.zeros(C, dtype=torch.bfloat16, device=DEV)
    ops.groupnorm_bwd(xd, gamma.to(DEV), beta.to(DEV), stats, dy.to(DEV), dx, dg, db, G, silu, accumulate_dx=True)
    check(dx, prev_dx.float() + xf.grad.permute(0, 2, 1), "gn_bwd dx", fro=6e-3, mx=3e-2)
    check(dg, gf.grad, "gn_bwd dgamma", fro=6e-3, mx=3e-2)
    check(db, bfl.grad, "gn_bwd dbeta", fro=6e-3, mx=3e-2)
    # out-of-place accumulation (az_groupnorm_bwd_ex: dx = dx_add + gradient, dx_add untouched) == the in-place form, bit for bit
    src = prev_dx.to(DEV).clone()
    dx2 = torch.full_like(src, 3.0)
    ops.groupnorm_bwd(xd, gamma.to(DEV), beta.to(DEV), stats, dy.to(DEV), dx2, None, None, G, silu, dx_add=src)
    assert torch.equal(dx2, dx) and torch.equal(src, prev_dx.to(DEV))


def test_norm_backward_reads_bf16_rounded_statistics_like_the_reference(ops):
    """Option NORM_STAT_BF16 (default 1).  Under the reference's dataflow (train.py:273: bf16 autocast, bf16 parameters) torch saves
    GroupNorm's / LayerNorm's mean and rstd for the backward in bf16, so every (sample, group) / row of the data gradient carries the
    rounding of its rstd as a coherent scale.  Checked here where it is sharpest -- the per-group / per-row SCALE of dx against an
    fp32 backward: with the option on it must equal rstd_bf16 / rstd_fp32 of that group (from the kernel's own fp32 statistics)
    to 3e-4, with the option off it must be 1 to 3e-4 -- and, for the whole tensor, against torch's own bf16 CPU autograd."""
    from aozora_sdxl_training_amd._lib import set_option
    B, HW, C, G, eps = 2, 1024, 320, 32, 1e-5
    x = bf(rnd(B, HW, C, seed=71).float() * 1.7 + 0.4)
    gamma, beta, dy = bf(1 + 0.2 * rnd(C, seed=72).float()), rnd(C, scale=0.2, seed=73), rnd(B, HW, C, seed=74)
    xf = x.float().permute(0, 2, 1).requires_grad_(True)
    F.group_norm(xf, G, gamma.float(), beta.float(), eps).backward(dy.float().permute(0, 2, 1))
    dx32 = xf.grad.permute(0, 2, 1)                                              # fp32 statistics
    xb = x.permute(0, 2, 1).clone().requires_grad_(True)                          # torch's bf16 path: statistics saved in bf16
    F.group_norm(xb, G, gamma, beta, eps).backward(dy.permute(0, 2, 1))
    dx16 = xb.grad.float().permute(0, 2, 1)
    xd, yd = x.to(DEV), torch.empty(B, HW, C, dtype=torch.bfloat16, device=DEV)
    stats = torch.empty(B * G * 2, dtype=torch.float32, device=DEV)
    ops.groupnorm_fwd(xd, gamma.to(DEV), beta.to(DEV), yd, stats, G, eps, False)
    rstd = stats.view(B, G, 2)[..., 1].cpu()
    want = rstd.bfloat16().float() / rstd                                        # the scale a rounded rstd puts on the group's dx (to first order)
    try:
        got = {}
        for on in (1, 0):
            set_option("NORM_STAT_BF16", on)
            dx = torch.empty(B, HW, C, dtype=torch.bfloat16, device=DEV)
            ops.groupnorm_bwd(xd, gamma.to(DEV), beta.to(DEV), stats, dy.to(DEV), dx, None, None, G, False)
            d = dx.float().cpu().view(B, HW, G, C // G); r = dx32.reshape(B, HW, G, C // G)
            got[on] = (d * r).sum((1, 3)) / (r * r).sum((1, 3))                  # per (sample, group) slope against the fp32 backward
            got[(on, "dx")] = dx.float().cpu()
        assert (want - 1).abs().max() > 5e-4, "no group whose rstd rounds noticeably: the case proves nothing"
        assert (got[1] - want).abs().max() < 3e-4, (got[1] - want).abs().max()
        assert (got[0] - 1).abs().max() < 3e-4, (got[0] - 1).abs().max()
        # whole tensor against torch's bf16 autograd: closer with the option on than off
        e_on = (got[(1, "dx")] - dx16).norm() / dx16.norm(); e_off = (got[(0, "dx")] - dx16).norm() / dx16.norm()
        assert e_on < 3.5e-3 and e_on < e_off, (float(e_on), float(e_off))
        # LayerNorm: the forward kernel saves what the backward reads
        M, Cl = 512, 1280
        xl = bf(rnd(M, Cl, seed=75).float() * 2 - 0.5)
        gl, bl, dyl = bf(1 + 0.2 * rnd(Cl, seed=76).float()), rnd(Cl, scale=0.2, seed=77), rnd(M, Cl, seed=78)
        xlf = xl.float().requires_grad_(True)
        F.layer_norm(xlf, (Cl,), gl.float(), bl.float(), 1e-5).backward(dyl.float())
        for on in (1, 0):
            set_option("NORM_STAT_BF16", on)
            yl = torch.empty(M, Cl, dtype=torch.bfloat16, device=DEV)
            st = torch.empty(2 * M, dtype=torch.float32, device=DEV)
            ops.layernorm_fwd(xl.to(DEV), gl.to(DEV), bl.to(DEV), yl, st)
            rs = st.view(M, 2)[:, 1].cpu()
            if on:
                assert torch.equal(rs, rs.bfloat16().float()), "saved rstd is not a bf16 value"
                saved = rs
            else:
                wantl = saved / rs                                               # rounded / exact rstd per row
            dxl = torch.empty(M, Cl, dtype=torch.bfloat16, device=DEV)
            ops.layernorm_bwd(xl.to(DEV), gl.to(DEV), st, dyl.to(DEV), dxl, None, None)
            slope = (dxl.float().cpu() * xlf.grad).sum(1) / (xlf.grad * xlf.grad).sum(1)
            got[("ln", on)] = slope
        assert (got[("ln", 1)] - wantl).abs().max() < 6e-4 and (got[("ln", 0)] - 1).abs().max() < 6e-4
    finally:
        set_option("NORM_STAT_BF16", 1)


@pytest.mark.parametrize("M,C", [(512, 640), (300, 1280), (77, 64), (4096, 1280)])
def test_layernorm_fwd_bwd(ops, M, C):
    x = bf(rnd(M, C).float() * 2 - 0.5)
    gamma, beta, dy = bf(1 + 0.2 * rnd(C).float()), rnd(C, scale=0.2), rnd(M, C)
    xf, gf, bfl = x.float().requires_grad_(True), gamma.float().requires_grad_(True), beta.float().requires_grad_(True)
    y = F.layer_norm(xf, (C,), gf, bfl, 1e-5)
    y.backward(dy.float())
    xd, yd = x.to(DEV), torch.empty(M, C, dtype=torch.bfloat16, device=DEV)
    stats = torch.empty(2 * M, dtype=torch.float32, device=DEV)
    ops.layernorm_fwd(xd, gamma.to(DEV), beta.to(DEV), yd, stats)
    check(yd, y, f"ln_fwd {M,C}")
    dx = torch.empty(M, C, dtype=torch.bfloat16, device=DEV)
    dg = torch.zeros(C, dtype=torch.bfloat16, device=DEV)
    db = torch.zeros(C, dtype=torch.bfloat16, device=DEV)
    ops.layernorm_bwd(xd, gamma.to(DEV), stats, dy.to(DEV), dx, dg, db)
    check(dx, xf.grad, "ln_bwd dx", fro=6e-3, mx=3e-2)
    check(dg, gf.grad, "ln_bwd dgamma", fro=6e-3, mx=3e-2)
    check(db, bfl.grad, "ln_bwd dbeta", fro=6e-3, mx=3e-2)
    # the split form (data gradient alone, parameter gradients alone) agrees with the one-pass form; dx bit for bit
    dx2 = torch.empty_like(dx)
    dg2, db2 = torch.zeros_like(dg), torch.zeros_like(db)
    ops.layernorm_bwd(xd, gamma.to(DEV), stats, dy.to(DEV), dx2, None, None)
    ops.layernorm_bwd(xd, gamma.to(DEV), stats, dy.to(DEV), None, dg2, db2)
    assert torch.equal(dx, dx2)
    check(dg2, gf.grad, "ln_bwd dgamma (split)", fro=6e-3, mx=3e-2)
    check(db2, bfl.grad, "ln_bwd dbeta (split)", fro=6e-3, mx=3e-2)
    # accumulate into dx / into existing parameter gradients
    prev = rnd(M, C)
    dx3 = prev.to(DEV).clone()
    ops.layernorm_bwd(xd, gamma.to(DEV), stats, dy.to(DEV), dx3, dg, db, accumulate_dx=True)
    check(dx3, prev.float() + xf.grad, "ln_bwd dx accumulate", fro=6e-3, mx=3e-2)
    check(dg, 2 * gf.grad, "ln_bwd dgamma accumulate", fro=8e-3, mx=4e-2)
    check(db, 2 * bfl.grad, "ln_bwd dbeta accumulate", fro=8e-3, mx=4e-2)
    # partial sums parked and finished later, two LayerNorms in ONE launch (az_layernorm_bwd_partial + az_ln_param_finish_multi):
    # dx and both parameter gradients equal the immediate form bit for bit
    nblk = ops.ln_partial_blocks(M)
    parts = [torch.empty(nblk * C * 2, dtype=torch.float32, device=DEV) for _ in range(2)]
    dxs = [torch.empty(M, C, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    dgs = [torch.zeros(C, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    dbs = [torch.zeros(C, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    for k in range(2):
        ops.layernorm_bwd_partial(xd, gamma.to(DEV), stats, dy.to(DEV), dxs[k], parts[k])
    nb = (C + 31) // 32
    table = torch.tensor([[parts[0].data_ptr(), dgs[0].data_ptr(), dbs[0].data_ptr(), nblk, C, 0],
                          [parts[1].data_ptr(), dgs[1].data_ptr(), 0, nblk, C, nb]], dtype=torch.int64, device=DEV)
    ops.ln_param_finish_multi(table, 2, 2 * nb)
    dg1, db1 = torch.zeros_like(dg), torch.zeros_like(db)
    dx1 = torch.empty_like(dx)
    ops.layernorm_bwd(xd, gamma.to(DEV), stats, dy.to(DEV), dx1, dg1, db1)
    assert torch.equal(dxs[0], dx1) and torch.equal(dxs[1], dx1)
    assert torch.equal(dgs[0], dg1) and torch.equal(dbs[0], db1) and torch.equal(dgs[1], dg1) and float(dbs[1].abs().max()) == 0.0
    # the block count is the caller's (what it sized `partial` and the finish job for), not the LN_RPB option's value at launch
    # time: with the option changed behind a recorded launch, the same call still runs with ITS block count and the same bits,
    # and a count the buffer was not sized by (a fresh query under the new option) is refused when the buffer is too small
    from aozora_sdxl_training_amd._lib import set_option, get_option, AozoraError
    rpb0 = get_option("LN_RPB")
    try:
        set_option("LN_RPB", 4 if rpb0 != 4 else 16)
        guard = torch.full((nblk * C * 2 + 64,), 7.0, dtype=torch.float32, device=DEV)
        dx5 = torch.empty_like(dx1)
        ops.layernorm_bwd_partial(xd, gamma.to(DEV), stats, dy.to(DEV), dx5, guard[:nblk * C * 2], nblk=nblk)
        assert torch.equal(dx5, dx1) and torch.equal(guard[:nblk * C * 2], parts[0]) and float((guard[nblk * C * 2:] - 7.0).abs().max()) == 0.0
        nblk2 = ops.ln_partial_blocks(M)
        if nblk2 > nblk:
            with pytest.raises(AozoraError):
                ops.layernorm_bwd_partial(xd, gamma.to(DEV), stats, dy.to(DEV), dx5, guard[:nblk * C * 2], nblk=nblk2)
        with pytest.raises(AozoraError):
            ops.layernorm_bwd_partial(xd, gamma.to(DEV), stats, dy.to(DEV), dx5, guard[:nblk * C * 2], nblk=0)
    finally:
        set_option("LN_RPB", rpb0)
    # out-of-place accumulation (az_layernorm_bwd_ex) == in place, bit for bit, in the one-pass and in the data-gradient-only form;
    # the source (a strided view here) is left untouched
    wide = torch.zeros(M, C + 16, dtype=torch.bfloat16, device=DEV)
    wide[:, :C] = prev.to(DEV)
    for with_params in (True, False):
        dx4 = torch.full((M, C), 5.0, dtype=torch.bfloat16, device=DEV)
        dg4, db4 = (torch.zeros_like(dg), torch.zeros_like(db)) if with_params else (None, None)
        ops.layernorm_bwd(xd, gamma.to(DEV), stats, dy.to(DEV), dx4, dg4, db4, dx_add=wide[:, :C])
        assert torch.equal(dx4, dx3) and torch.equal(wide[:, :C], prev.to(DEV))


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,H,K", [(300, 640, 320),        # 128x128 tile, ragged rows
                                   (1700, 5120, 1280),    # 256x256 tile (the grid fills whole waves of CUs), ragged rows
                                   (200, 200, 64),        # H not a multiple of the tile's 64 value columns
                                   (4096, 5120, 1280)])   # the benchmark's own product
def test_gemm_with_fused_geglu_forward(ops, M, H, K):
    """az_gemm_geglu_fwd_bf16 == az_gemm_bf16 followed by az_geglu_fwd, bit for bit (projection AND output), into strided
    destinations whose padding stays untouched; and both agree with fp32 torch."""
    x, w, b = rnd(M, K), rnd(2 * H, K, scale=0.05), rnd(2 * H, scale=0.3)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    proj = torch.empty(M, 2 * H, dtype=torch.bfloat16, device=DEV)
    ops.gemm(xd, wd, proj, trans_b=True, bias=bd)
    out = torch.empty(M, H, dtype=torch.bfloat16, device=DEV)
    ops.geglu_fwd(proj, out)
    wide_p = torch.full((M, 2 * H + 8), 7.0, dtype=torch.bfloat16, device=DEV)
    wide_o = torch.full((M, H + 16), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.gemm_geglu_fwd(xd, wd, bd, wide_p[:, :2 * H], wide_o[:, :H])
    assert torch.equal(wide_p[:, :2 * H], proj) and torch.equal(wide_o[:, :H], out)
    assert float((wide_p[:, 2 * H:] - 7.0).abs().max()) == 0.0 and float((wide_o[:, H:] - 7.0).abs().max()) == 0.0
    pf = x.float() @ w.float().t() + b.float()
    check(proj, pf, "fused geglu fwd: projection")
    check(out, pf[:, :H] * F.gelu(pf[:, H:]), "fused geglu fwd: output", fro=6e-3, mx=3e-2)
    nobias = torch.empty_like(proj); out2 = torch.empty_like(out)
    ops.gemm_geglu_fwd(xd, wd, None, nobias, out2)
    check(nobias, x.float() @ w.float().t(), "fused geglu fwd: no bias")


def test_geglu_silu_add_upsample_colsum(ops):
    M, H = 300, 640
    proj, dout = rnd(M, 2 * H), rnd(M, H)
    pf = proj.float().requires_grad_(True)
    a, g = pf.chunk(2, dim=-1)
    y = a * F.gelu(g)
    y.backward(dout.float())
    pd = proj.to(DEV)
    out = torch.empty(M, H, dtype=torch.bfloat16, device=DEV)
    ops.geglu_fwd(pd, out)
    check(out, y, "geglu_fwd")
    dproj = torch.empty(M, 2 * H, dtype=torch.bfloat16, device=DEV)
    ops.geglu_bwd(pd, dout.to(DEV), dproj)
    check(dproj, pf.grad, "geglu_bwd")

    x, dy = rnd(4, 1280), rnd(4, 1280)
    xf = x.float().requires_grad_(True)
    F.silu(xf).backward(dy.float())
    yd = torch.empty_like(x, device=DEV)
    ops.silu_fwd(x.to(DEV), yd)
    check(yd, F.silu(x.float()), "silu_fwd")
    dxd = torch.empty_like(x, device=DEV)
    ops.silu_bwd(x.to(DEV), dy.to(DEV), dxd)
    check(dxd, xf.grad, "silu_bwd")

    a2, b2 = rnd(100, 64), rnd(100, 64)
    cat = torch.zeros(100, 192, dtype=torch.bfloat16, device=DEV)
    ops.add_rows(a2.to(DEV), b2.to(DEV), cat[:, 64:128])
    check(cat[:, 64:128], a2.float() + b2.float(), "add_rows")
    ops.add_rows(a2.to(DEV), None, cat[:, 128:])
    assert torch.equal(cat[:, 128:].cpu(), a2)

    xu = rnd(2, 5, 7, 64)
    yu = torch.empty(2, 10, 14, 64, dtype=torch.bfloat16, device=DEV)
    ops.upsample2x_fwd(xu.to(DEV), yu)
    ref = F.interpolate(xu.float().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(yu.float().cpu(), ref)
    dyu = rnd(2, 10, 14, 64)
    dxu = torch.empty(2, 5, 7, 64, dtype=torch.bfloat16, device=DEV)
    ops.upsample2x_bwd(dyu.to(DEV), dxu)
    refb = dyu.float().reshape(2, 5, 2, 7, 2, 64).sum(dim=(2, 4))
    check(dxu, refb, "upsample_bwd")

    xs = rnd(4 * 96, 320)
    cs = torch.empty(4 * 320, dtype=torch.float32, device=DEV)
    ops.colsum(xs.to(DEV), 96, cs)
    check(cs.view(4, 320), xs.float().view(4, 96, 320).sum(1), "colsum", fro=1e-5, mx=1e-4)
    dst = rnd(320, scale=0.1)
    dd = dst.to(DEV).clone()
    ops.reduce_segs_to_bf16(cs, 4, 320, dd, True)
    check(dd, dst.float() + xs.float().sum(0), "reduce_segs")


@pytest.mark.parametrize("R,C", [(64, 64), (640, 1920), (1280, 320), (200, 136), (4, 320), (77, 65), (8, 8)])
def test_transpose_exact(ops, R, C):
    """W^T copies (refreshed per optimizer step): pure data movement, bit-exact; vector and 2-byte paths, strided views."""
    g = torch.Generator().manual_seed(R * 1000 + C)
    src = torch.randn(R, C + 8, generator=g).bfloat16().to(DEV)[:, :C]           # strided rows
    dst = torch.full((C, R + 16), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.transpose(src, dst[:, :R])
    assert torch.equal(dst[:, :R], src.t()) and bool((dst[:, R:] == 7.0).all())
    # conv weight [Co][9][Ci] -> [Ci][9][Co], all taps in one launch
    w = torch.randn(R, 9, C, generator=g).bfloat16().to(DEV)
    wt = torch.empty(C, 9, R, dtype=torch.bfloat16, device=DEV)
    ops.transpose_batched(w.permute(1, 0, 2), wt.permute(1, 0, 2))
    assert torch.equal(wt, w.permute(2, 1, 0).contiguous())


def test_transpose_multi_one_launch_for_many_matrices(ops):
    """az_transpose_multi_bf16 (the W^T refresh of a parameter region): a job table of plain [N][K] weights and of the nine
    strided taps of a conv weight [Co][9][Ci] -> [Ci][9][Co], one launch, bit-exact; bytes outside the jobs untouched."""
    import ctypes
    from aozora_sdxl_training_amd._lib import lib
    g = torch.Generator().manual_seed(99)
    shapes = [(1280, 320), (640, 640), (200, 136), (8, 2816), (3840, 64)]
    flat_src = torch.randn(4_000_000, generator=g).bfloat16().to(DEV)
    flat_dst = torch.full((4_000_000,), 9.0, dtype=torch.bfloat16, device=DEV)
    jobs, off, tiles, expect = [], 0, 0, []

    def add(so, do, R, C, lds, ldd):
        nonlocal tiles
        tc = (C + 63) // 64
        jobs.append([flat_src.data_ptr() + 2 * so, flat_dst.data_ptr() + 2 * do, R, C, lds, ldd, tiles, tc])
        tiles += tc * ((R + 63) // 64)
    for R, C in shapes:
        add(off, off, R, C, C, R)
        expect.append((off, R, C, None))
        off += (R * C + 63) // 64 * 64
    co, ci = 320, 64
    for tap in range(9):
        add(off + tap * ci, off + tap * co, co, ci, 9 * ci, 9 * co)
    expect.append((off, co, ci, 9))
    end = off + co * 9 * ci
    tab = torch.tensor(jobs, dtype=torch.int64, device=DEV)
    lib().call("az_transpose_multi_bf16", ctypes.c_void_p(tab.data_ptr()), len(jobs), tiles,
               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    for o, R, C, taps in expect:
        if taps is None:
            assert torch.equal(flat_dst[o:o + R * C].view(C, R), flat_src[o:o + R * C].view(R, C).t())
        else:
            assert torch.equal(flat_dst[o:o + R * taps * C].view(C, taps, R), flat_src[o:o + R * taps * C].view(R, taps, C).permute(2, 1, 0))
    assert bool((flat_dst[end:] == 9.0).all())


def test_timestep_embed_and_layout(ops):
    from oracle.unet_ref import timestep_embedding
    t = torch.tensor([0.0, 1.0, 10.0, 500.0, 999.0, 1024.0, 804.0])
    for dim in (320, 256, 32):
        out = torch.empty(t.numel(), dim, dtype=torch.bfloat16, device=DEV)
        ops.timestep_embed(t.to(DEV), dim, out)
        ref = timestep_embedding(t, dim)
        assert (out.float().cpu() - ref).abs().max().item() <= 8e-3, dim  # bf16 resolution of values in [-1,1]
    x = torch.randn(2, 4, 6, 5)
    d = torch.empty(2, 6, 5, 8, dtype=torch.bfloat16, device=DEV)
    ops.nchw_to_nhwc_pad(x.to(DEV), d, 4)
    assert torch.equal(d[..., :4].cpu(), bf(x).permute(0, 2, 3, 1)) and d[..., 4:].abs().max().item() == 0
    back = torch.empty(2, 4, 6, 5, dtype=torch.float32, device=DEV)
    ops.nhwc_to_nchw(d, back, 4)
    assert torch.equal(back.cpu(), bf(x).float())


@pytest.mark.parametrize("mode", ["epsilon", "v_prediction", "rectified_flow"])
def test_noise_target_and_loss_vs_oracle(ops, mode, golden_tensors):
    from oracle import step_ref as R
    from aozora_sdxl_training_amd import schedule as S
    B, C, H, W = 3, 4, 8, 6
    g = torch.Generator().manual_seed(5)
    lat = bf(torch.randn(B, C, H, W, generator=g))
    noise = torch.randn(B, C, H, W, generator=g)
    ts = torch.tensor([10, 500, 999])
    jit = torch.rand(B, generator=g)
    noisy_ref, tgt_ref, _ = R.make_noisy_and_target(mode, lat, noise, ts, R.ddpm_alphas_cumprod(), jit)
    if mode == "rectified_flow":
        tc = ((ts.float() + jit) / 1000.0).clamp(0, 1)
        ca, cb = 1 - tc, tc
    else:
        ta, tb = S.ddpm_coef_tables(torch.bfloat16)
        ca, cb = ta[ts], tb[ts]
    noisy = torch.empty(B, H, W, 8, dtype=torch.bfloat16, device=DEV)
    tgt = torch.empty(B, C, H, W, dtype=torch.float32, device=DEV)
    ops.noise_target({"epsilon": 0, "v_prediction": 1, "rectified_flow": 2}[mode], lat.to(DEV), noise.to(DEV),
                     ca.float().contiguous().to(DEV), cb.float().contiguous().to(DEV), noisy, tgt)
    assert torch.equal(noisy[..., :4].cpu(), bf(noisy_ref).permute(0, 2, 3, 1)), "noisy latents must be bit-exact"
    assert torch.allclose(tgt.cpu(), tgt_ref.float(), rtol=1e-6, atol=1e-6)
    # loss + dpred vs the oracle loss (itself pinned to the reference by tests/test_oracle_golden.py)
    curve = golden_tensors["curve_bell"]
    pred = bf(torch.randn(B, C, H, W, generator=g))
    pr = pred.float().requires_grad_(True)
    l = R.weighted_mse_loss(pr, tgt_ref, ts, curve)
    (l / 2).backward()
    pn = torch.empty(B, H, W, 4, dtype=torch.bfloat16, device=DEV)
    pn.copy_(pred.permute(0, 2, 3, 1))
    loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    per = torch.zeros(B, dtype=torch.float32, device=DEV)
    dpred = torch.empty(B, H, W, 8, dtype=torch.bfloat16, device=DEV)
    ops.mse_loss_fwd_bwd(pn, tgt, curve[ts].to(DEV), 0.5, loss, per, dpred)
    assert abs(loss.item() - l.item()) <= 2e-6 * abs(l.item()) + 1e-7
    check(dpred[..., :4], pr.grad.permute(0, 2, 3, 1), "dpred")
    assert dpred[..., 4:].abs().max().item() == 0


def test_sumsq_and_clip(ops):
    g = rnd(1_000_003, scale=0.01)
    out = torch.zeros(1, dtype=torch.float32, device=DEV)
    ops.sumsq(g.to(DEV), out, False)
    ref = (g.double() ** 2).sum().item()
    assert abs(out.item() - ref) <= 1e-5 * ref
    ops.sumsq(g.to(DEV)[:4096].float().contiguous(), out, True)
    ref2 = ref + (g[:4096].double() ** 2).sum().item()
    assert abs(out.item() - ref2) <= 1e-5 * ref2
    coef = torch.zeros(1, dtype=torch.float32, device=DEV)
    norm = torch.zeros(1, dtype=torch.float32, device=DEV)
    ops.clip_coef(out, 0.5, coef, norm)
    n = math.sqrt(ref2)
    assert abs(norm.item() - n) <= 1e-5 * n and abs(coef.item() - min(1.0, 0.5 / (n + 1e-6))) <= 1e-6


# ------------------------------------------------------------------------------------------------
def test_stream_picker_returns_streams_that_work_side_by_side(ops):
    """streams.pick(): the returned stream passes the ping-pong probe against the ones it was asked to run beside, a stream
    is never its own partner, independent kernels on the three streams run concurrently, and az_spin rejects absurd
    durations."""
    import ctypes
    import time
    from aozora_sdxl_training_amd import streams
    from aozora_sdxl_training_amd._lib import lib, AozoraError
    side = streams.pick(DEV, 0, what="test side")
    main = streams.pick(DEV, -1, beside=[side], what="test main")
    comm = streams.pick(DEV, 0, beside=[main, side], what="test comm")
    assert streams.overlaps(main, side) and streams.overlaps(comm, main) and streams.overlaps(comm, side)
    assert not streams.overlaps(main, main)
    # three probes side by side take the time of one
    for s in (main, side, comm):
        s.synchronize()
    t0 = time.perf_counter()
    for s in (main, side, comm):
        lib().call("az_spin", 2000, ctypes.c_void_p(s.cuda_stream))
    for s in (main, side, comm):
        s.synchronize()
    assert time.perf_counter() - t0 < 2 * 2000e-6
    with pytest.raises(AozoraError):
        lib().call("az_spin", 10 ** 7, ctypes.c_void_p(main.cuda_stream))


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 8, 8, 64, 64), (1, 6, 10, 128, 72), (2, 16, 16, 320, 320)])
def test_conv_with_nearest2x_upsample_gather(ops, tile, B, H, W, Cin, Cout):
    """Upsample2D (diffusers: F.interpolate(scale_factor=2, mode="nearest") -> 3x3 conv) with the upsample folded into the
    conv's operand gather: forward and weight gradient read the HALF-resolution tensor, the upsampled one never exists."""
    x, w, b = rnd(B, H, W, Cin), rnd(Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5), rnd(Cout)
    xn = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    wn = w.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    up = F.interpolate(xn, scale_factor=2.0, mode="nearest")
    y = F.conv2d(up, wn, b.float(), padding=1)
    out = torch.empty(B, 2 * H, 2 * W, Cout, dtype=torch.bfloat16, device=DEV)
    ops.conv_fwd(x.to(DEV), w.to(DEV), out, bias=b.to(DEV), upsample=True)
    check(out, y.permute(0, 2, 3, 1), f"conv_fwd upsample {B,H,W,Cin,Cout}")
    # the same through the explicit upsample kernel: bit-identical (same products, same order)
    xu = torch.empty(B, 2 * H, 2 * W, Cin, dtype=torch.bfloat16, device=DEV)
    ops.upsample2x_fwd(x.to(DEV), xu)
    out2 = torch.empty_like(out)
    ops.conv_fwd(xu, w.to(DEV), out2, bias=b.to(DEV))
    assert torch.equal(out, out2)
    dy = rnd(B, 2 * H, 2 * W, Cout)
    y.backward(dy.float().permute(0, 3, 1, 2))
    prev = rnd(Cout, 3, 3, Cin, scale=0.05)
    dw, bg = prev.to(DEV).clone(), torch.zeros(Cout, dtype=torch.bfloat16, device=DEV)
    ops.conv_wgrad(dy.to(DEV), x.to(DEV), dw, accumulate=True, split_k=0, bias_grad=bg, upsample=True)
    check(dw, prev.float() + wn.grad.permute(0, 2, 3, 1), f"conv_wgrad upsample {B,H,W,Cin,Cout}")
    dw2 = prev.to(DEV).clone()
    ops.conv_wgrad(dy.to(DEV), xu, dw2, accumulate=True, split_k=0)
    assert torch.equal(dw, dw2)
    check(bg, dy.float().sum((0, 1, 2)), "bias grad", fro=4e-3, mx=3e-2)


@pytest.mark.parametrize("M,N,K,split", [(640, 640, 4096, 0), (1280, 320, 308, 0), (72, 320, 1000, 4), (200, 136, 304, 3), (1280, 1280, 4096, 5)])
def test_inkernel_finish_option_equals_separate_reduce(ops, M, N, K, split):
    """Option INKERNEL_FINISH (the tile's last-arriving workgroup sums the split-K slabs and finishes the fused column sums,
    write-through slab stores + agent-scope acquire): bitwise the same dW and bias gradient as the separate reduce launch --
    the summation order is the split index in both -- and reproducible run to run; conv weight gradients with per-sample sums too."""
    from aozora_sdxl_training_amd._lib import set_option
    dy, x, prev = rnd(K, M), rnd(K, N), rnd(M, N, scale=0.1)
    n_real = M if M % 8 else M - 3
    bprev = rnd(n_real, scale=0.1)
    res = {}
    try:
        for mode in (0, 1, 1):
            set_option("INKERNEL_FINISH", mode)
            out, bg = prev.to(DEV).clone(), bprev.to(DEV).clone()
            ops.gemm(dy.to(DEV), x.to(DEV), out, trans_a=True, trans_b=False, accumulate=True, split_k=split, bias_grad=bg)
            out2 = prev.to(DEV).clone()
            ops.gemm(dy.to(DEV), x.to(DEV), out2, trans_a=True, trans_b=False, accumulate=True, split_k=split)
            torch.cuda.synchronize()
            assert torch.equal(out, out2)
            if mode in res:
                assert torch.equal(res[mode][0], out) and torch.equal(res[mode][1], bg)
            res[mode] = (out, bg)
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        check(res[1][0], prev.float() + dy.float().t() @ x.float(), f"in-kernel finish {M}x{N}x{K}")
        # conv weight gradient with bias gradient and per-sample sums
        B, H, W, Ci, Co = 2, 16, 16, 64, 128
        xc, dyc = rnd(B, H, W, Ci), rnd(B, H, W, Co)
        outs = []
        for mode in (0, 1):
            set_option("INKERNEL_FINISH", mode)
            dw = torch.zeros(Co, 3, 3, Ci, dtype=torch.bfloat16, device=DEV)
            bgc = torch.zeros(Co, dtype=torch.bfloat16, device=DEV)
            seg = torch.zeros(B, Co, dtype=torch.bfloat16, device=DEV)
            ops.conv_wgrad(dyc.to(DEV), xc.to(DEV), dw, accumulate=True, split_k=0, bias_grad=bgc, seg_grad=seg)
            torch.cuda.synchronize()
            outs.append((dw, bgc, seg))
        assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    finally:
        set_option("INKERNEL_FINISH", 0)


def test_split_product_with_residual_keeps_it_under_every_finish_option(ops):
    """A split-K product with an out-of-place residual (the ff.net.0 data gradient: K = 10240, g_new = g + dY W) must add the residual
    whether the slabs are summed by the reduce launch or -- option INKERNEL_FINISH with the 16-wave tile (GEMM8 = 0) or a caller's
    split_k > 1 -- the in-kernel finish is asked for: that path adds no residual, so the launcher falls back to the reduce launch."""
    from aozora_sdxl_training_amd._lib import set_option
    M, N, K = 512, 1280, 10240
    a, w, r = rnd(M, K, scale=0.3), rnd(N, K, scale=0.3), rnd(M, N)
    ref = r.float() + a.float() @ w.float().t()
    outs = []
    try:
        for fin, g8, big, split in ((0, 1, 3, 0), (1, 1, 3, 0), (1, 0, 3, 0), (1, 0, 0, 3), (0, 0, 0, 3)):
            set_option("INKERNEL_FINISH", fin); set_option("GEMM8", g8); set_option("NT_SPLIT_BIG", big)
            out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
            ops.gemm(a.to(DEV), w.to(DEV), out, residual=r.to(DEV), split_k=split)
            torch.cuda.synchronize()
            check(out, ref, f"split product + residual (INKERNEL_FINISH={fin}, GEMM8={g8}, NT_SPLIT_BIG={big}, split_k={split})")
            outs.append(out)
        assert torch.equal(outs[3], outs[4]), "the same split must sum in the same order under both finish options"
    finally:
        set_option("INKERNEL_FINISH", 0); set_option("GEMM8", 1); set_option("NT_SPLIT_BIG", 3)


def test_stage_inputs_segments_and_host_floats_in_one_launch(ops):
    """az_stage_inputs (the micro-step's input placements, train.py:2731-2760): segments of ragged word counts, 16-byte-aligned and
    only 4-byte-aligned pointers, an empty coefficient table, 256 host floats that the caller overwrites right after the call;
    bit-exact, bytes outside the destinations untouched; argument errors for > 8 segments, > 256 floats, a byte count % 4 != 0."""
    import ctypes
    from aozora_sdxl_training_amd._lib import lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(5)
    words = [4 * 4 * 128 * 128 // 2, 4 * 4 * 128 * 128, 4 * 77 * 2048 // 2, 4 * 1280 // 2, 24, 4096 * 3 + 5, 1, 4095]
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (sum(words) + 64,), generator=g, dtype=torch.int64).to(torch.int32).to(DEV)
    dst = torch.full((sum(words) + 64 + 8 * 3,), 7, dtype=torch.int32, device=DEV)
    so, do, segs = 0, 0, []
    for i, w in enumerate(words):
        do += (i % 3)                        # destinations off the 16-byte grid for some segments
        segs.append((so, do, w)); so += w; do += w
    coef_dev = torch.zeros(300, dtype=torch.float32, device=DEV)

    def call(segs, coef):
        n = len(segs)
        s = (ctypes.c_void_p * max(1, n))(*[src.data_ptr() + 4 * a for a, _, _ in segs])
        d = (ctypes.c_void_p * max(1, n))(*[dst.data_ptr() + 4 * b for _, b, _ in segs])
        nb = (ctypes.c_long * max(1, n))(*[4 * w for _, _, w in segs])
        return lib()._fn["az_stage_inputs"](n, ctypes.cast(s, ctypes.c_void_p), ctypes.cast(d, ctypes.c_void_p), ctypes.cast(nb, ctypes.c_void_p),
                                            0 if coef is None else coef.numel(), None if coef is None else ctypes.c_void_p(coef.data_ptr()),
                                            ctypes.c_void_p(coef_dev.data_ptr()), st)
    coef = torch.randn(256, generator=g)
    keep = coef.clone()
    assert call(segs, coef) == 0
    coef.zero_()                              # the floats were read during the call
    torch.cuda.synchronize()
    covered = torch.zeros_like(dst, dtype=torch.bool)
    for a, b, w in segs:
        assert torch.equal(dst[b:b + w], src[a:a + w])
        covered[b:b + w] = True
    assert bool((dst[~covered] == 7).all())
    assert torch.equal(coef_dev[:256].cpu(), keep) and bool((coef_dev[256:] == 0).all())
    dst.fill_(7)
    assert call(segs[:2], None) == 0 and call([], keep[:3]) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst[segs[1][1]:segs[1][1] + segs[1][2]], src[segs[1][0]:segs[1][0] + segs[1][2]])
    assert bool((dst[segs[2][1]:] == 7).all())
    assert call(segs + [segs[0]], None) != 0 and call([], torch.zeros(257)) != 0
    bad = (ctypes.c_long * 1)(6); one = (ctypes.c_void_p * 1)(src.data_ptr()); two = (ctypes.c_void_p * 1)(dst.data_ptr())
    assert lib()._fn["az_stage_inputs"](1, ctypes.cast(one, ctypes.c_void_p), ctypes.cast(two, ctypes.c_void_p), ctypes.cast(bad, ctypes.c_void_p), 0, None, None, st) != 0
