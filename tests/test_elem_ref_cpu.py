"""tests/elem_ref.py without a GPU: its table K is derived here (each kernel's own formula in float32 torch against the float64
restatement over the test inputs; an entry below 4 x measured fails), the erfc polynomial meets the claim of az_common.h, the
bit-level restatements agree with torch's own CPU operations and with the Raven golden vectors, and the Python port of colsum_geom
shows every colsum case of tests/test_elem_gpu.py reaching the branch it is listed for."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import elem_ref as R        # noqa: E402

ZERO = torch.zeros((), dtype=torch.float64)
MEASURED = set()          # the quantities measure() has derived


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def measure(quantity, out32, ref, S, rounding=None, flush=None):
    """The K the float32 value itself needs (no storage rounding), checked against the table with the 4x margin; then the value
    rounded as the kernel stores it stays inside the bound."""
    k = R.excess(out32, ref, S, ZERO, flush)
    MEASURED.add(quantity)
    print(f"K[{quantity}] measured {k:.3f} table {R.K[quantity]}")
    assert R.K[quantity] >= 4.0 * k, f"K[{quantity}] = {R.K[quantity]} is below 4 x the measured {k:.3f}"
    stored = out32.bfloat16() if rounding is None else out32
    assert bool(((stored.double() - ref).abs() <= R.bound(ref, S, quantity, rounding, flush)).all()), quantity
    return k


# ---------------- K -------------------------------------------------------------------------------------------------------------
def test_k_geglu():
    proj, dout = R.geglu_inputs(300, 1000, seed=1)
    ref, S = R.geglu_fwd_ref(proj)
    measure("geglu_out", R.geglu_fwd_f32(proj), ref, S)
    ref, S = R.geglu_bwd_ref(proj, dout)
    o = R.geglu_bwd_f32(proj, dout)
    measure("geglu_da", o[:, :1000], ref[:, :1000], S[:, :1000])
    measure("geglu_dg", o[:, 1000:], ref[:, 1000:], S[:, 1000:])


def test_k_silu():
    x, dy, dx = R.silu_inputs(300000, seed=2)
    ref, S, fl = R.silu_fwd_ref(x)
    measure("silu_y", R.silu_fwd_f32(x), ref, S, flush=fl)
    for old in (None, dx):
        ref, S, fl = R.silu_bwd_ref(x, dy, old)
        measure("silu_dx", R.silu_bwd_f32(x, dy, old), ref, S, flush=fl)


def test_k_upsample_and_sums():
    dy = R.gauss_bf16((2, 6, 10, 64), seed=3)
    ref, S = R.upsample_bwd_ref(dy)
    measure("upsample_dx", R.upsample_bwd_f32(dy), ref, S)
    for (rows, C, rps), _ in R.COLSUM_CASES:
        x = R.gauss_bf16((rows, C), seed=rows + C)
        bias = R.gauss_bf16((C,), seed=C, scale=3.0)
        ref, S = R.colsum_ref(x, rps)
        measure("colsum", R.colsum_f32(x, rps), ref, S, rounding=R.f32_rounding(ref))
        seg, S_seg, b, S_b = R.colsum_grad_ref(x, rps, bias, C - 3)
        seg32, b32 = R.colsum_grad_f32(x, rps, bias, C - 3)
        measure("colsum", seg32, seg, S_seg)
        measure("colsum", b32, b, S_b)
    src = torch.randn(5, 1000, generator=R.gen(4))
    old = R.gauss_bf16((1000,), seed=5)
    for nseg in (1, 5):
        for o in (None, old):
            ref, S = R.reduce_segs_ref(src[:nseg], nseg, 1000, o)
            measure("reduce_segs", R.reduce_segs_f32(src[:nseg], nseg, 1000, o), ref, S)


def test_k_mse_temb_sumsq_clip():
    for B, C, HW, ldp in ((3, 4, 255, 8), (2, 4, 16384 + 300, 8)):
        pred = R.gauss_bf16((B, HW, ldp), seed=HW)
        target = torch.randn(B, C, HW, generator=R.gen(HW + 1))
        w = torch.tensor([1.3, 0.0, 0.7][:B])
        r = R.mse_ref(pred, target, w, 0.5)
        dp, mean, loss = R.mse_f32(pred, target, w, 0.5)
        measure("mse_dpred", dp, r["dpred"], r["S_dpred"])
        measure("mse_mean", mean, r["mean"], r["S_mean"], rounding=R.f32_rounding(r["mean"]))
        measure("mse_loss", loss, r["loss"], r["S_loss"], rounding=R.f32_rounding(r["loss"]))
    t = torch.tensor([0.0, 1.0, 37.0, 500.5, 999.0])
    ref, S = R.temb_ref(t, 320)
    measure("temb", R.temb_f32(t, 320), ref, S)
    for n, f32 in ((R.SUMSQ_SWEEP + 8 * 300 + 5, False), (9, False), (262144 + 3, True)):
        g = torch.randn(n, generator=R.gen(n))
        g = g if f32 else g.bfloat16()
        for prev in (0.0, 123.5):
            ref, S = R.sumsq_ref(g, prev)
            measure("sumsq", R.sumsq_f32(g, prev), ref, S, rounding=R.f32_rounding(ref))
    for unscale in (1.0, 1.0 / 128):
        for ss in (1e-3, 7.5, 3.0e6):
            for mx in (0.5, 1e9):
                ref = torch.tensor(R.clip_coef_ref(ss, mx, unscale), dtype=torch.float64)
                out = torch.tensor(R.clip_coef_f32(ss, mx, unscale), dtype=torch.float64)
                measure("clip_coef", out, ref, ref.abs(), rounding=R.f32_rounding(ref))


def test_every_quantity_of_the_table_was_derived_here():
    MEASURED.clear()
    for t in (test_k_geglu, test_k_silu, test_k_upsample_and_sums, test_k_mse_temb_sumsq_clip):
        t()
    assert MEASURED == set(R.K), (sorted(MEASURED - set(R.K)), sorted(set(R.K) - MEASURED))
    assert all(v >= 1.0 and float(np.log2(v)).is_integer() for v in R.K.values())


# ---------------- the bound's rounding term ------------------------------------------------------------------------------------
def test_half_ulp_is_what_a_correct_rounding_needs_and_no_more():
    """half_ulp_bf16 admits torch's own round-to-nearest cast of any float64 and is attained; 2^-9 |ref| is not attainable (the cast
    itself exceeds it), 2^-8 |ref| is up to twice as wide."""
    x = torch.cat([torch.randn(200000, dtype=torch.float64, generator=R.gen(7)) * 3.0,
                   torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -30, 1.0, 2.0 - 2.0 ** -20, 0.0, 3e-40, -1.5e-39], dtype=torch.float64)])
    err = (x.float().bfloat16().double() - x).abs()          # float64 -> fp32 -> bf16: the kernel's own store of an fp32 value
    h = R.half_ulp_bf16(x)
    assert bool((err <= h + R.U_F32 * x.abs()).all())
    assert float((err / h).max()) > 0.999
    assert bool((err > 2.0 ** -9 * x.abs()).any())
    assert bool((h >= 2.0 ** -9 * x.abs()).all()) and bool((h[x.abs() > 1e-30] <= 2.0 ** -8 * x.abs()[x.abs() > 1e-30]).all())


# ---------------- the erfc polynomial ------------------------------------------------------------------------------------------
def test_erfc_polynomial_meets_the_claim_of_az_common():
    """gelu and gelu' from the Abramowitz & Stegun 7.1.26 form with the constants of az_common.h: at most 4.3e-7 absolute against
    float64, on a dense grid over [-40, 40] plus +-0."""
    g = torch.cat([torch.linspace(-40.0, 40.0, 2000001, dtype=torch.float64), torch.linspace(-6.0, 6.0, 1200001, dtype=torch.float64),
                   torch.tensor([0.0, -0.0], dtype=torch.float64)])
    ge, dge = R.gelu64(g)
    pe, pde = R.gelu_pair_formula(g)
    e1, e2 = float((pe - ge).abs().max()), float((pde - dge).abs().max())
    print(f"erfc polynomial: max |gelu error| {e1:.3e}, max |gelu' error| {e2:.3e}")
    assert e1 <= 4.3e-7 and e2 <= 4.3e-7
    z = R.gelu_pair_formula(torch.tensor([0.0, -0.0]))
    assert bool((z[0] == 0).all()) and bool(((z[1] - 0.5).abs() < 1e-6).all())


# ---------------- bit-level restatements against torch ---------------------------------------------------------------------------
def same_or_both_nan(a, b):
    return bool(((bits(a) == bits(b)) | (a.isnan() & b.isnan())).all())


def test_cast_and_scale_restatements_equal_torch():
    x = torch.cat([R.cast_edges(), torch.randn(100000, generator=R.gen(8)) * 1e3, torch.randn(1000, generator=R.gen(9)) * 1e-39])
    got, want = R.f32_to_bf16_bits(x), x.bfloat16()
    assert same_or_both_nan(got, want)
    assert bool((got.isnan() == x.isnan()).all()) and bool((bits(got)[~x.isnan()] == bits(want)[~x.isnan()]).all())
    assert bits(got)[0] == 0x3F80 and bits(got)[1] == 0x3F82 and got[8] == float("inf") and got[9] == torch.finfo(torch.bfloat16).max
    g = torch.cat([R.cast_edges().bfloat16(), R.gauss_bf16((100000,), seed=10, scale=50.0)])
    for c in (0.37, -3.0, 1e-30):
        assert same_or_both_nan(R.scale_bf16_bits(g, c), (g.float() * c).bfloat16()), c
    assert torch.equal(bits(R.scale_bf16_bits(g, 1.0)), bits(g))            # untouched: NaN payloads included
    xf = torch.randn(1000, generator=R.gen(11))
    assert torch.equal(R.scale_f32_bits(xf, 0.37), xf * torch.tensor(0.37))
    gh = torch.randn(1000, generator=R.gen(12))
    gb = R.gauss_bf16((1000,), seed=13)
    assert torch.equal(R.titan_offload_bits(gb, gh, 1), gh + gb.float()) and torch.equal(R.titan_offload_bits(gb, gh, 0), gb.float())
    a, b = R.gauss_bf16((1000,), seed=14), R.gauss_bf16((1000,), seed=15)
    assert torch.equal(R.add_rows_bits(a, b), (a.float() + b.float()).bfloat16())


def test_noise_target_restatement_equals_torch_tensor_ops():
    """The reference dataflow: separate fp32 tensor operations; bf16 coefficient x bf16 latent products in the DDPM modes."""
    B, C, HW = 2, 4, 333
    lat = R.gauss_bf16((B, C, HW), seed=16)
    noise = torch.randn(B, C, HW, generator=R.gen(17))
    ca, cb = torch.tensor([0.83, 0.21]).bfloat16().float(), torch.tensor([0.55, 0.97]).bfloat16().float()
    a, s = ca[:, None, None], cb[:, None, None]
    for mode in (0, 1, 2):
        noisy, tg = R.noise_target_bits(mode, lat, noise, ca, cb, 8)
        if mode == 2:
            xt, want = a * lat.float() + s * noise, noise - lat.float()
        else:
            xt = (a.bfloat16() * lat).float() + s * noise
            want = a * noise - (s.bfloat16() * lat).float() if mode == 1 else noise
        assert torch.equal(bits(noisy[..., :C]), bits(xt.bfloat16().permute(0, 2, 1))) and bool((noisy[..., C:] == 0).all()), mode
        assert torch.equal(tg, want), mode


def test_fma32_is_correctly_rounded():
    """Against exact rational arithmetic, on products that cancel against the addend (where a double rounding would show)."""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(3000).astype(np.float32), rng.standard_normal(3000).astype(np.float32)
    c = (-(a.astype(np.float64) * b)).astype(np.float32) * rng.choice([1.0, -1.0, 0.5, 3.0], 3000).astype(np.float32)
    r = R.fma32(a, b, c)
    for i in range(3000):
        ex = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        d = abs(Fraction(float(r[i])) - ex)
        for nb in (np.nextafter(r[i], np.float32(-np.inf)), np.nextafter(r[i], np.float32(np.inf))):
            assert d <= abs(Fraction(float(nb)) - ex), (i, a[i], b[i], c[i], r[i])


def test_adamw_restatement_follows_the_raven_goldens(golden_host, golden_tensors):
    """adamw_bits from zero moments over the recorded gradients, under the per-element allowance of
    test_raven_titan_against_reference_goldens (tests/test_model_gpu.py) and no looser one."""
    DT = {"torch.bfloat16": torch.bfloat16, "torch.float32": torch.float32}
    off = total = 0
    for c in golden_host["raven"]:
        if c["pdt"] != "torch.bfloat16":
            continue
        k = c["key"]
        p = golden_tensors[k + "_init"].clone().reshape(-1)
        m = torch.zeros(p.numel(), dtype=DT[c["mdt"]])
        v = torch.zeros_like(m)
        for s in range(c["steps"]):
            hy = R.adamw_hyper(c["lr"], c["betas"], c["wd"], c["eps"], c["debias"], s + 1)
            p, m, v = R.adamw_bits(p, golden_tensors[f"{k}_g{s}"].reshape(-1).bfloat16(), m, v, hy)
            want = golden_tensors[f"{k}_p{s}"].reshape(-1).float()
            err = (p.float() - want).abs()
            assert bool(((err <= want.abs() * 2.0 ** -7 + 1e-30) | (err <= 0.02 * 4e-3)).all()), (k, s, float(err.max()))
            assert float((err > 0).float().mean()) <= 0.005 or err.numel() < 64, (k, s)
            assert torch.allclose(m.float(), golden_tensors[f"{k}_m{s}"].reshape(-1).float(), rtol=1e-2, atol=2e-5), (k, s)
            off += int((err > 0).sum()); total += err.numel()
    print(f"adamw restatement vs goldens: {off} of {total} parameter values differ")
    assert total > 0


# ---------------- colsum geometry ----------------------------------------------------------------------------------------------
def test_every_colsum_case_reaches_the_branch_it_is_listed_for():
    seen = set()
    for (rows, C, rps), want in R.COLSUM_CASES:
        g, br = R.colsum_geom(rows, C, rps)
        print(f"colsum ({rows}, {C}, {rps}): {g} -> {sorted(br)}")
        assert br == set(want), ((rows, C, rps), sorted(br), sorted(want))
        assert g["nseg"] * rps == rows and g["nchunk"] * g["rpc"] >= rps and g["rpc"] % g["by"] == 0 and g["bx"] * g["zb"] * 8 >= C
        seen |= br
    assert seen == {"bx1", "by_clamped", "rpc_floor", "chunks_1", "chunks_256", "zb2", "zb3", "ragged", "small_block", "rpc_above_floor"}
    g, _ = R.colsum_geom(2 * 100, 1032, 100)
    assert g["bx"] == 128 and 1032 // 8 - 128 == 1                       # zb = 2 with one live lane in the second column block
    g, _ = R.colsum_geom(77 * 7, 40, 7)
    assert g["bx"] * g["by"] == 160
