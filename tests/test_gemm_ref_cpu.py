"""tests/gemm_ref.py checked without a GPU: every reference against an independently written restatement (einsum, float64
F.conv2d / F.conv_transpose2d, explicit loops over taps and pixels), `exact_ok` and the share of non-representable results for every
row of the case tables tests/test_gemm_exact_gpu.py runs (imported, so they cannot drift), the seeded faults, the poison helper, and
the record of the gap: five faults the suite's old tolerance check passes and the new comparisons reject."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gemm_ref as R        # noqa: E402
import test_gemm_exact_gpu as T        # noqa: E402


# ---------------- restatements ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,M,N,K", [("nt", 5, 12, 16), ("nn", 7, 9, 24), ("tn", 6, 11, 13), ("nt", 130, 168, 72)])
def test_products_match_einsum(form, M, N, K):
    a = R.quarters((K, M) if form == "tn" else (M, K), 1)
    b = R.quarters((N, K) if form == "nt" else (K, N), 2)
    bias, rb, res, prev = R.quarters(N, 3), R.quarters(((M + 3) // 4, N), 4), R.quarters((M, N), 5), R.quarters((M, N), 6, lim=8)
    ref, S = R.gemm(form, a, b, bias=bias, rowbias=rb, rows_per_seg=4, residual=res, prev=prev)
    eq = {"nt": "mk,nk->mn", "nn": "mk,kn->mn", "tn": "km,kn->mn"}[form]
    want = torch.einsum(eq, a.double(), b.double())
    Sw = torch.einsum(eq, a.double().abs(), b.double().abs())
    for m in range(M):
        for n in range(N):
            e = float(bias[n]) + float(rb[m // 4, n]) + float(res[m, n]) + float(prev[m, n])
            ea = abs(float(bias[n])) + abs(float(rb[m // 4, n])) + abs(float(res[m, n])) + abs(float(prev[m, n]))
            assert float(ref[m, n]) == float(want[m, n]) + e and float(S[m, n]) == float(Sw[m, n]) + ea
    bold = R.quarters(M - 3, 7, lim=8) if form == "tn" else None
    if bold is not None:
        br, bS = R.bias_grad(a, M - 3, bold)
        assert torch.equal(br, torch.stack([bold[m].double() + sum(a[k, m].double() for k in range(K)) for m in range(M - 3)]))
        assert torch.equal(bS, bold.double().abs() + a.double().abs().sum(0)[:M - 3])


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


CONV_SMALL = [(2, 5, 7, 8, 4, 3, 1), (2, 5, 7, 8, 12, 3, 2), (1, 1, 5, 8, 4, 3, 1), (2, 5, 1, 16, 8, 3, 2), (2, 4, 4, 8, 8, 1, 1), (3, 6, 5, 8, 8, 1, 2),
              (2, 8, 8, 16, 8, 3, 2)]


@pytest.mark.parametrize("B,H,W,Cin,Cout,ks,st", CONV_SMALL)
def test_convs_match_torch_convolutions(B, H, W, Cin, Cout, ks, st):
    x, w = R.quarters((B, H, W, Cin), 1), R.quarters((Cout, ks, ks, Cin), 2)
    pad = 1 if ks == 3 else 0
    y = F.conv2d(_nchw(x), _nchw(w), stride=st, padding=pad)
    Ho, Wo = y.shape[2], y.shape[3]
    bias, rb, res = R.quarters(Cout, 3), R.quarters((B, Cout), 4), R.quarters((B, Ho, Wo, Cout), 5)
    ref, S = R.conv_fwd(x, w, st, bias=bias, rowbias=rb, residual=res)
    assert torch.equal(ref, (y + bias.double()[None, :, None, None] + rb.double()[:, :, None, None] + _nchw(res)).permute(0, 2, 3, 1))
    Sw = F.conv2d(_nchw(x).abs(), _nchw(w).abs(), stride=st, padding=pad) + bias.double().abs()[None, :, None, None] + rb.double().abs()[:, :, None, None] + _nchw(res).abs()
    assert torch.equal(S, Sw.permute(0, 2, 3, 1))
    cpad = R.up8(Cout) + 8
    dy = torch.full((B, Ho, Wo, cpad), R.POISON, dtype=torch.bfloat16)            # channels from Cout on must be ignored
    dy[..., :Cout] = R.quarters((B, Ho, Wo, Cout), 6)
    prev, dres = R.quarters((B, H, W, Cin), 7, lim=8), R.quarters((B, H, W, Cin), 8)
    op = (H - ((Ho - 1) * st - 2 * pad + ks), W - ((Wo - 1) * st - 2 * pad + ks))
    dx = F.conv_transpose2d(_nchw(dy[..., :Cout]), _nchw(w), stride=st, padding=pad, output_padding=op).permute(0, 2, 3, 1)
    got, _ = R.conv_dgrad(dy, w, st, (H, W), prev=prev, residual=dres)
    assert torch.equal(got, dx + prev.double() + dres.double())
    # weight gradient: explicit loops over taps and pixels
    dwp = R.quarters((Cout, ks, ks, Cin), 9, lim=8)
    want = dwp.double().clone()
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                for ky in range(ks):
                    for kx in range(ks):
                        iy, ix = oy * st + ky - pad, ox * st + kx - pad
                        if 0 <= iy < H and 0 <= ix < W:
                            want[:, ky, kx, :] += torch.outer(dy[b, oy, ox, :Cout].double(), x[b, iy, ix].double())
    got, _ = R.conv_wgrad(dy, x, ks, st, Cout, prev=dwp)
    assert torch.equal(got, want)
    seg, Sseg, tot, Stot = R.conv_sums(dy, Cout, R.quarters(Cout, 10, lim=8))
    assert torch.equal(seg, dy[..., :Cout].double().sum((1, 2))) and torch.equal(tot, seg.sum(0) + R.quarters(Cout, 10, lim=8).double())


@pytest.mark.parametrize("B,Hs,Ws", [(2, 4, 4), (1, 3, 5), (2, 1, 3)])
@pytest.mark.parametrize("crop_h,crop_w", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_upsample_convs_match_interpolate(B, Hs, Ws, crop_h, crop_w):
    Cin, Cout = 8, 8
    H, W = 2 * Hs - crop_h, 2 * Ws - crop_w
    x, w = R.quarters((B, Hs, Ws, Cin), 1), R.quarters((Cout, 3, 3, Cin), 2)
    up = F.interpolate(_nchw(x), size=(H, W), mode="nearest")
    assert torch.equal(up, _nchw(x)[:, :, torch.arange(H) >> 1][:, :, :, torch.arange(W) >> 1])        # the header's (y >> 1, x >> 1)
    ref, _ = R.conv_fwd(x, w, 1, out_hw=(H, W))
    assert torch.equal(ref, F.conv2d(up, _nchw(w), padding=1).permute(0, 2, 3, 1))
    dy = R.quarters((B, H, W, Cout), 3)
    got, _ = R.conv_wgrad(dy, x, 3, 1, Cout, out_hw=(H, W))
    want, _ = R.conv_wgrad(dy, up.permute(0, 2, 3, 1), 3, 1, Cout)
    assert torch.equal(got, want)


def test_geglu_reference_uses_the_rounded_projection():
    x, w, b = R.quarters((9, 72), 1), R.quarters((16, 72), 2), R.quarters(16, 3)
    proj, S, out, bound = R.geglu_fwd(x, w, b)
    assert torch.equal(proj, x.double() @ w.double().t() + b.double())
    pb = proj.float().bfloat16().double()
    gate = pb[:, 8:]
    want = pb[:, :8] * gate * 0.5 * torch.special.erfc(-gate * 0.5 ** 0.5)
    assert float((out - want).abs().max()) <= 1e-9 * float(want.abs().max()) and bool((bound > 0).all())


def test_grouped_references_are_the_single_products():
    d = T.make_nt_grouped(4, 72)
    for w, b, (ref, _) in zip(d["ws"], d["bs"], d["refs"]):
        assert torch.equal(ref, R.gemm("nt", d["a"], w, bias=b)[0])
    d = T.make_tn_grouped(True)
    for (dy, x, prev, bold), (ref, _, bref, _) in zip(d["jobs"], d["refs"]):
        assert torch.equal(ref, torch.einsum("km,kn->mn", dy.double(), x.double()) + prev.double())
        assert torch.equal(bref, bold.double() + dy.double().sum(0)[:bold.numel()])


# ---------------- conditions on the inputs, for every row the GPU file runs ----------------------------------------------------------
def _on_grid(t, lim):
    v = t.double() * 4.0
    return bool((v == v.round()).all()) and float(t.double().abs().max()) <= lim


def test_every_plain_case_is_exactly_summable_and_exercises_the_rounding():
    cases = list(dict.fromkeys(T.all_plain_cases()))
    assert len(cases) > 300
    n_deep = 0
    for c in cases:
        d = T.make_gemm(c)                     # the reference asserts exact_ok itself
        assert R.exact_ok(d["S"]) and ("bS" not in d or R.exact_ok(d["bS"]))
        assert all(_on_grid(d[k], 4) for k in ("a", "b", "bias", "rowbias", "res") if d[k] is not None) and (d["prev"] is None or _on_grid(d["prev"], 8))
        if c.K >= 128:
            n_deep += 1
            share = R.inexact_share(d["ref"])
            assert share >= 0.25, (c, share)
    assert n_deep > 100


def test_every_conv_geglu_and_grouped_case_is_exactly_summable():
    deep = []
    for c in T.conv_cases() + [u for s in T.UPS_SOURCES for u in T.ups_cases(s)]:
        d = T.make_conv(c)
        for k in ("yS", "dwS", "segS", "bgS", "dxS", "dx_accS", "dx_resS"):
            assert k not in d or R.exact_ok(d[k])
        if 9 * c.Cin >= 128 and c.ks == 3:
            deep.append(R.inexact_share(d["y"]))
            assert deep[-1] >= 0.25, (c, deep[-1])
    assert len(deep) >= 10
    for M in T.GEGLU_M:
        for H in T.GEGLU_H:
            for K in T.GEGLU_K:
                for wb in (True, False):
                    d = T.make_geglu(M, H, K, wb)
                    assert R.exact_ok(d["S"]) and (K < 128 or R.inexact_share(d["proj"]) >= 0.25)
    for M in T.NTG_M:
        for K in T.NTG_K:
            for ref, S in T.make_nt_grouped(M, K)["refs"]:
                assert R.exact_ok(S) and (K < 128 or R.inexact_share(ref) >= 0.25)
    for wb in (True, False):
        for (M, N, K), (ref, S, bref, bS) in zip(T.TNG_PRODUCTS, T.make_tn_grouped(wb)["refs"]):
            assert R.exact_ok(S) and (bS is None or R.exact_ok(bS)) and (K < 128 or R.inexact_share(ref) >= 0.25)


def test_case_tables_cover_what_the_issue_asks():
    assert len(T.TILES) == 11 and (128, 160, 72) in T.TILES
    grids = {c[:3] for c in T.conv_cases()}
    assert grids == set(T.CONV_GRIDS)
    pairs = {}
    for c in T.conv_cases():
        pairs.setdefault((c.Cin, c.Cout), set()).add(c.stride)
    assert set(pairs) == {(8, 4), (8, 168), (64, 64), (72, 40), (128, 136), (64, 8)} and all(s == {1, 2} for s in pairs.values())
    assert all(len(v) >= 2 for v in T.CONV_TABLE.values())
    assert any(c.ks == 1 for c in T.conv_cases()) and any(c.Cout % 8 for c in T.conv_cases())
    assert any((T.make_conv(c)["Ho"] * T.make_conv(c)["Wo"]) % 64 == 0 for c in T.conv_cases())


def test_exact_ok_refuses_sums_that_could_round():
    with pytest.raises(AssertionError):
        R.exact_ok(torch.tensor([2.0 ** 20]))
    assert R.exact_ok(torch.tensor([2.0 ** 20 - 1.0]))


# ---------------- the seeded faults -----------------------------------------------------------------------------------------------
def _nt_inputs(M, N, K, gaussian):
    if gaussian:
        return R.gauss((M, K), 11), R.gauss((N, K), 12, K ** -0.5), R.gauss(N, 13), R.gauss((M, N), 14)
    return R.quarters((M, K), 11), R.quarters((N, K), 12), R.quarters(N, 13), R.quarters((M, N), 14)


def test_every_seeded_fault_changes_an_expected_bit_on_exact_inputs():
    a, b, bias, res = _nt_inputs(130, 168, 392, False)
    ref, S = R.gemm("nt", a, b, bias=bias, residual=res)
    want = R.expected_bits(ref)
    for f in R.FIRST_FIVE_FAULTS + [R.fault_slab_skipped]:
        assert R.first_mismatch(f(a, b, bias, res), want) is not None, f.__name__
    # a k-tile counted in the wrong column-sum segment
    dy = R.quarters((3, 16, 12, 8), 21)
    seg = R.conv_sums(dy, 8)[0]
    assert R.first_mismatch(R.expected_bits(R.conv_sums(dy, 8, fault="segment")[0]), R.expected_bits(seg)) is not None
    assert torch.equal(R.conv_sums(dy, 8, fault="segment")[2], R.conv_sums(dy, 8)[2])            # ... which the total alone does not see
    # a source pixel taken from the neighbouring sample at a grid edge
    x, w = R.quarters((2, 3, 3, 8), 22), R.quarters((8, 3, 3, 8), 23)
    good = R.expected_bits(R.conv_fwd(x, w, 1)[0])
    bad = R.expected_bits(R.conv_fwd(x, w, 1, fault="neighbour")[0])
    assert R.first_mismatch(bad, good) is not None and torch.equal(bad[1], good[1]) and torch.equal(bad[0, :2], good[0, :2])
    # a cropped upsample row read at (dst >> 1) + 1
    x = R.quarters((2, 4, 4, 8), 24)
    good = R.expected_bits(R.conv_fwd(x, w, 1, out_hw=(7, 8))[0])
    bad = R.expected_bits(R.conv_fwd(x, w, 1, out_hw=(7, 8), fault="crop_row")[0])
    assert R.first_mismatch(bad, good) is not None and torch.equal(bad[:, :4], good[:, :4])


def old_check(out, ref, fro=4e-3, mx=2e-2):
    """check() of tests/test_kernels_gpu.py, copied: relative Frobenius error <= 4e-3 and max error <= 2e-2 max|ref| against fp32."""
    out, ref = out.float(), ref.float()
    e_fro = (out - ref).norm().item() / (ref.norm().item() + 1e-12)
    e_max = (out - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)
    return (e_fro <= fro and e_max <= mx), e_fro, e_max


def test_the_old_check_passes_five_faults_that_the_new_comparisons_reject(capsys):
    """The gap this file closes, at the suite's own shape 308 x 1280 x 2048 (NT + bias + residual), Gaussian inputs: the tolerance
    check passes the first five faults; the float64 bound 2^-8 |ref| + 2 n 2^-24 S rejects each, and so does the bit comparison on
    exact inputs of the same shape.
    The dropped k-chunk is the exception to 'passes': what it costs depends on the row's eight values.  In the LAST row, with these
    seeds, the old check's Frobenius criterion passes (2.7e-3 <= 4e-3) and its max criterion does not (2.5e-2 > 2e-2; 2.0e-2 .. 3.5e-2
    over eight seeds tried, against the 1.6e-2 of one earlier measurement).  Asserted for that fault instead: the new comparisons
    reject the last row, and rows exist (counted over all 308, printed) in which the old check passes the same fault."""
    M, N, K = 308, 1280, 2048
    a, b, bias, res = _nt_inputs(M, N, K, True)
    ref, S = R.gemm("nt", a, b, bias=bias, residual=res, exact=False)
    ref32 = a.float() @ b.float().t() + bias.float() + res.float()
    n = K + 2 + 1
    clean = R.expected_bits(ref)
    assert old_check(clean, ref32)[0] and bool(((clean.double() - ref).abs() <= R.gauss_bound(ref, S, n)).all())
    assert R.excess(clean, ref, S, n) == 0.0
    ea, eb, ebias, eres = _nt_inputs(M, N, K, False)
    eref, eS = R.gemm("nt", ea, eb, bias=ebias, residual=eres)
    assert float(eS.max()) * 16 < 2 ** 24 and R.inexact_share(eref) >= 0.25
    ewant = R.expected_bits(eref)
    for f in R.FIRST_FIVE_FAULTS:
        out = f(a, b, bias, res)
        ok, e_fro, e_max = old_check(out, ref32)
        if f is R.fault_k_chunk_dropped:
            # the same fault in every row at once: row r of `every` is row r of the output whose row r lost its last chunk
            every = R.expected_bits(ref - a[:, -8:].double() @ b[:, -8:].double().t()).float()
            assert torch.equal(every[-1], out.float()[-1])
            e0, e1 = (clean.float() - ref32) ** 2, (every - ref32) ** 2
            fro = ((e0.sum() - e0.sum(1) + e1.sum(1)).sqrt() / ref32.norm())
            mx = torch.maximum(e1.sqrt().amax(1), e0.sqrt().max()) / ref32.abs().max()
            passing = int(((fro <= 4e-3) & (mx <= 2e-2)).sum())
            with capsys.disabled():
                print(f"\n(dropped chunk: the old check passes it in {passing} of {M} rows; last row rel_fro={e_fro:.2e} rel_max={e_max:.2e})", end="")
            assert e_fro <= 4e-3 and passing > 0
        outside = int(((out.double() - ref).abs() > R.gauss_bound(ref, S, n)).sum())
        wrong_bits = int((R.bits(f(ea, eb, ebias, eres)) != R.bits(ewant)).sum())
        with capsys.disabled():
            print(f"\n{f.__name__}: old check rel_fro={e_fro:.2e} rel_max={e_max:.2e} pass={ok}; outside the float64 bound: {outside}; "
                  f"excess {R.excess(out, ref, S, n):.2f}; wrong bits on exact inputs: {wrong_bits} of {ewant.numel()}")
        assert ok or f is R.fault_k_chunk_dropped, f"{f.__name__}: the old check was expected to pass this fault"      # (the last row of the dropped chunk: see the docstring)
        assert outside > 0, f"{f.__name__}: the float64 bound does not reject this fault"
        assert wrong_bits > 0, f"{f.__name__}: the bit comparison does not reject this fault"


# ---------------- the poison helper ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld,lead,tail,off,align", [(176, 3, 2, 0, 16), (176, 1, 0, 4, 8), (168, 0, 0, 0, 16), (171, 0, 1, 0, 16), (176, 2, 2, 8, 16)])
def test_embed_round_trips_guards_and_aligns(ld, lead, tail, off, align):
    t = R.quarters((130, 168), 5)
    e = R.embed(t, ld, lead, tail, off)
    assert torch.equal(e.view(), t) and e.buf.shape == (lead + 130 + tail, ld) and e.guards_intact()
    assert float(torch.tensor(R.POISON).bfloat16()) == R.POISON                       # bf16-exact, finite
    assert e.byte_offset() == e.view().data_ptr() - e.buf.data_ptr()
    assert e.byte_offset() % align == 0 and (align == 16 or e.byte_offset() % 16 != 0)
    if ld > 168 + off:
        e.buf[lead, off + 168] = 1.0
        assert not e.guards_intact()
        e.buf[lead, off + 168] = R.POISON
    if lead:
        e.buf[lead - 1, ld - 1] = -R.POISON
        assert not e.guards_intact()
        e.buf[lead - 1, ld - 1] = R.POISON
    e.view().fill_(0.0)
    assert e.guards_intact()
