"""NOISE_MODE without a GPU: tests/noise_ref.py's float64 reference against F.interpolate and torch's own std, its fp32 restatement of
the kernels within elem_ref.bound of that reference (K as derived there), the grammar of noise.parse_noise_mode, the draws of
noise.draw_aux and the NOISE_MODE of config.TrainingConfig."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import elem_ref as R        # noqa: E402
import noise_ref as N       # noqa: E402
from aozora_sdxl_training_amd import noise as nz      # noqa: E402

U = 2.0 ** -24


# ---------------- the float64 reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(4, 4), (5, 7), (9, 6), (16, 12)])
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_float64_reference_equals_interpolate_and_torch_ops(H, W, levels):
    B, C = 2, 4
    eps, o, zs, xi, _ = N.draws((B, C, H, W), levels, seed=H * 100 + W + levels)
    for z in zs:
        want = TF.interpolate(z.double(), size=(H, W), mode="bilinear", align_corners=False)
        assert float((torch.from_numpy(N.upsample64(z.numpy(), H, W)) - want).abs().max()) <= 1e-12
    assert [tuple(z.shape[2:]) for z in zs] == nz.level_shapes(H, W, levels) == N.level_shapes(H, W, levels)
    spec = nz.parse_noise_mode(f"pyramid:levels={levels},discount=0.4,offset=0.07,perturb=0.2")
    u = eps.double() + 0.07 * o.double()[:, :, None, None]
    for l, z in enumerate(zs, start=1):
        u = u + 0.4 ** l * TF.interpolate(z.double(), size=(H, W), mode="bilinear", align_corners=False)
    e1 = u / u.reshape(B, -1).std(dim=1, unbiased=True)[:, None, None, None]
    got, mix = N.shaped64(spec, eps, nz.NoiseAux(o, zs, xi))
    assert float((torch.from_numpy(got) - e1).abs().max()) <= 1e-12
    assert float((torch.from_numpy(mix) - (e1 + 0.2 * xi.double())).abs().max()) <= 1e-12
    # offset alone: no normalisation
    got, mix = N.shaped64(nz.parse_noise_mode("offset:offset=0.07"), eps, nz.NoiseAux(o, None, None))
    assert float((torch.from_numpy(got) - (eps.double() + 0.07 * o.double()[:, :, None, None])).abs().max()) <= 1e-12 and mix is got


# ---------------- the fp32 restatement ----------------------------------------------------------------------------------------------
def _within(out, ref, S, k, rounding=None):
    ref, S = torch.as_tensor(ref), torch.as_tensor(S)
    out = torch.as_tensor(out).double()
    assert bool(torch.isfinite(out).all())
    b = R.bound(ref, S, k, R.f32_rounding(ref) if rounding is None else rounding)
    assert bool(((out - ref).abs() <= b).all()), (k, R.excess(out, ref, S, R.f32_rounding(ref) if rounding is None else rounding), R.K[k])


@pytest.mark.parametrize("shape,levels", N.CASES)
def test_fp32_restatement_lies_within_the_bound_of_the_float64_reference(shape, levels):
    B, C, H, W = shape
    HW = H * W
    eps, o, zs, xi, lat = N.draws(shape, levels, seed=7 * HW + levels)
    disc, off, pert = 0.6, 0.05, 0.1
    assert 8 + levels <= 4 + 12 * levels and R.K.get(N.k_shape(0), 3.0) <= 4
    for with_o, with_l in ((True, False), (False, True), (True, True)):
        zz = [z.numpy() for z in zs] if with_l else []
        u32 = N.shape_bits(eps.numpy(), o.numpy() if with_o else None, off, zz, N.weights_of(disc, levels))
        u64, S = N.shape64(eps.numpy(), o.numpy() if with_o else None, off, zz, disc)
        _within(u32, u64, S, N.k_shape(levels if with_l else 0))
    # partial sums and r_b against float64 OF THE fp32 u (each kernel against its own input)
    part = N.partials_bits(u32)
    assert part.shape == (B, N.nblk_of(HW), 2) and part.dtype == np.float32
    p64, S64 = N.partials64(u32)
    _within(part, p64, S64, N.k_partial(C, HW))
    r = N.rb_bits(part, C, HW).astype(np.float64)
    r64 = 1.0 / N.std64(u32)
    assert np.all(np.abs(r - r64) <= (N.rb_chain(C, HW) + 4) * U * r64), (np.abs(r / r64 - 1).max() / U, N.rb_chain(C, HW) + 4)
    ut = torch.from_numpy(u32).view(B, C, HW)
    for mode in (0, 1, 2):
        ca, cb = N.coefs(B, mode, HW)
        for normalise, perturb in ((True, False), (False, True), (True, True)):
            noisy, tg = N.target_ex_bits(mode, lat.view(B, C, HW), ut, ca, cb, 8, part if normalise else None,
                                         xi.view(B, C, HW) if perturb else None, pert)
            ref = N.target_ex64(mode, lat.view(B, C, HW), ut, ca, cb, normalise, xi.view(B, C, HW) if perturb else None, pert)
            k = N.k_target(C, HW, normalise)
            _within(noisy[..., :C].float(), ref["noisy"], ref["S_noisy"], k, rounding=R.half_ulp_bf16(ref["noisy"]))
            assert bool((noisy[..., C:].view(torch.int16) == 0).all())
            _within(tg, ref["target"], ref["S_target"], k)


def test_restatement_with_null_extras_is_the_noise_target_restatement():
    B, C, H, W = 2, 4, 5, 7
    eps, _, _, _, lat = N.draws((B, C, H, W), 1, seed=3)
    for mode in (0, 1, 2):
        ca, cb = N.coefs(B, mode, 5)
        a = N.target_ex_bits(mode, lat.view(B, C, -1), eps.view(B, C, -1), ca, cb, 8)
        b = R.noise_target_bits(mode, lat.view(B, C, -1), eps.view(B, C, -1), ca, cb, 8)
        assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_partial_geometry_and_sums_do_not_depend_on_the_batch():
    eps, o, zs, _, _ = N.draws((3, 4, 9, 6), 2, seed=11)
    w = N.weights_of(0.3, 2)
    u = N.shape_bits(eps.numpy(), o.numpy(), 0.05, [z.numpy() for z in zs], w)
    part = N.partials_bits(u)
    for b in range(3):
        ub = N.shape_bits(eps.numpy()[b:b + 1], o.numpy()[b:b + 1], 0.05, [z.numpy()[b:b + 1] for z in zs], w)
        assert np.array_equal(ub.view(np.int32), u[b:b + 1].view(np.int32))
        assert np.array_equal(N.partials_bits(ub).view(np.int32), part[b:b + 1].view(np.int32))


# ---------------- grammar -------------------------------------------------------------------------------------------------------------
def test_grammar_accepts():
    S = nz.NoiseSpec
    for s in (None, "", "  ", "normal", "NORMAL", " Normal "):
        assert nz.parse_noise_mode(s) == S("normal", 0.0, 0, 0.3, 0.0)
        assert not nz.parse_noise_mode(s).needs_aux and nz.parse_noise_mode(s).describe() == "normal"
    assert nz.parse_noise_mode("offset") == S("offset", 0.05, 0, 0.3, 0.0)
    assert nz.parse_noise_mode("Offset:OFFSET=0.1, perturb=0.2") == S("offset", 0.1, 0, 0.3, 0.2)
    assert nz.parse_noise_mode("pyramid") == S("pyramid", 0.0, 6, 0.3, 0.0)
    assert nz.parse_noise_mode("PYRAMID:Levels=8,discount=1,offset=0,perturb=0") == S("pyramid", 0.0, 8, 1.0, 0.0)
    assert nz.parse_noise_mode("pyramid:levels=2,offset=0.05,perturb=0.1") == S("pyramid", 0.05, 2, 0.3, 0.1)
    assert nz.parse_noise_mode("normal:perturb=0.1") == S("normal", 0.0, 0, 0.3, 0.1)
    spec = nz.parse_noise_mode("pyramid:levels=2,offset=0.05,perturb=0.1")
    assert nz.parse_noise_mode(spec) is spec and spec.normalises and spec.needs_shape and spec.needs_aux
    assert "pyramid" in spec.describe() and "2 levels" in spec.describe() and "0.1" in spec.describe()
    p = nz.parse_noise_mode("normal:perturb=0.1")
    assert p.needs_aux and not p.needs_shape and not p.normalises
    assert not nz.parse_noise_mode("offset:offset=0").needs_aux and nz.parse_noise_mode("offset").needs_shape


@pytest.mark.parametrize("text", [
    "pyramyd", "gaussian:offset=1", ":offset=1",                                 # unknown kind
    "offset:scale=1", "pyramid:level=3", "offset:offset", "offset:=1",            # unknown key / not key=value
    "offset:offset=0.1,offset=0.2", "pyramid:levels=2,LEVELS=3",                  # repeated key
    "normal:offset=0.1", "offset:levels=2", "offset:discount=0.5", "normal:levels=1", "normal:discount=0.3",     # key on the wrong kind
    "offset:offset=abc", "pyramid:levels=2.5", "pyramid:levels=x", "normal:perturb=", "pyramid:discount=nan",
    "offset:offset=inf", "normal:perturb=nan", "pyramid:offset=-inf",             # not a number / not finite
    "offset:offset=-0.1", "pyramid:levels=0", "pyramid:levels=9", "pyramid:discount=0", "pyramid:discount=1.01",
    "pyramid:discount=-0.3", "normal:perturb=-1",                                 # out of range
])
def test_grammar_refuses(text):
    with pytest.raises(ValueError, match="NOISE_MODE"):
        nz.parse_noise_mode(text)


# ---------------- draws ---------------------------------------------------------------------------------------------------------------
def test_draw_aux_is_deterministic_and_draws_nothing_for_normal(monkeypatch):
    shape = (3, 4, 9, 6)
    spec = nz.parse_noise_mode("pyramid:levels=3,offset=0.05,perturb=0.1")
    a, b = nz.draw_aux(spec, shape, 1234, 17), nz.draw_aux(spec, shape, 1234, 17)
    assert tuple(a.o.shape) == (3, 4) and [tuple(z.shape) for z in a.z] == [(3, 4, 5, 3), (3, 4, 3, 2), (3, 4, 2, 1)] and tuple(a.xi.shape) == shape
    for x, y in zip([a.o, a.xi] + a.z, [b.o, b.xi] + b.z):
        assert x.dtype == torch.float32 and x.device.type == "cpu" and torch.equal(x, y)
    c = nz.draw_aux(spec, shape, 1234, 18)
    d = nz.draw_aux(spec, shape, 1235, 17)
    assert not torch.equal(a.o, c.o) and not torch.equal(a.xi, c.xi) and not torch.equal(a.z[0], c.z[0]) and not torch.equal(a.o, d.o)
    # every draw has its own domain, none of them the rectified-flow jitter's
    doms = [nz.DOMAIN_OFFSET, nz.DOMAIN_PERTURB] + [nz.DOMAIN_LEVEL + l for l in range(1, nz.MAX_LEVELS + 1)]
    assert len(set(doms)) == len(doms) and 0x5D1 not in doms
    assert not torch.equal(a.xi.reshape(-1)[:12], a.o.reshape(-1)) and not torch.equal(a.z[0].reshape(-1)[:12], a.o.reshape(-1))
    # members the spec does not use are None
    off = nz.draw_aux(nz.parse_noise_mode("offset"), shape, 1234, 17)
    assert off.z is None and off.xi is None and torch.equal(off.o, a.o)
    per = nz.draw_aux(nz.parse_noise_mode("normal:perturb=0.5"), shape, 1234, 17)
    assert per.o is None and per.z is None and torch.equal(per.xi, a.xi)
    pyr = nz.draw_aux(nz.parse_noise_mode("pyramid:levels=1"), shape, 1234, 17)
    assert pyr.o is None and pyr.xi is None and len(pyr.z) == 1 and torch.equal(pyr.z[0], a.z[0])
    # "normal": None, and no generator is even made
    def boom(*a, **k):
        raise AssertionError("normal noise must not draw")
    monkeypatch.setattr(nz, "seeded_torch_generator", boom)
    assert nz.draw_aux(nz.parse_noise_mode("normal"), shape, 1234, 17) is None
    assert nz.draw_aux(nz.parse_noise_mode(None), shape, 1234, 17) is None


def test_rows_of_a_global_draw_are_the_rows_themselves():
    spec = nz.parse_noise_mode("pyramid:levels=2,offset=0.05,perturb=0.1")
    g = nz.draw_aux(spec, (5, 4, 8, 8), 99, 3)
    for sl in (slice(0, 3), slice(3, 5), slice(2, 2)):
        r = g.rows(sl)
        assert torch.equal(r.o, g.o[sl]) and torch.equal(r.xi, g.xi[sl]) and all(torch.equal(a, b[sl]) for a, b in zip(r.z, g.z))
        rows, total = nz.level_table(sl.stop - sl.start, 4, 8, 8, spec)
        if sl.stop > sl.start:
            assert r.packed().numel() == total and torch.equal(r.packed()[rows[1].offset:], g.z[1][sl].reshape(-1))
    assert nz.draw_aux(nz.parse_noise_mode("offset"), (5, 4, 8, 8), 99, 3).rows(slice(1, 2)).z is None
    # the shaped noise of a sample does not depend on the rows it travels with (float64 reference, per-sample std)
    eps = torch.randn(5, 4, 8, 8, generator=torch.Generator().manual_seed(1))
    whole, _ = N.shaped64(spec, eps, g)
    part, _ = N.shaped64(spec, eps[3:5], g.rows(slice(3, 5)))
    assert np.array_equal(whole[3:5], part)


def test_level_table_and_device_table_layout():
    spec = nz.parse_noise_mode("pyramid:levels=3,discount=0.5")
    rows, total = nz.level_table(2, 4, 5, 7, spec)
    assert [(r.h, r.w) for r in rows] == [(3, 4), (2, 2), (1, 1)] and [r.offset for r in rows] == [0, 96, 128] and total == 136
    assert [r.weight for r in rows] == [0.5, 0.25, 0.125]
    t = nz.table_tensor(rows)
    assert t.dtype == torch.int32 and tuple(t.shape) == (3, 4) and t[:, :3].tolist() == [[0, 3, 4], [96, 2, 2], [128, 1, 1]]
    assert t[:, 3].contiguous().view(torch.float32).tolist() == [0.5, 0.25, 0.125]
    assert nz.partial_blocks(16) == 1 and nz.partial_blocks(257) == 2 and nz.partial_blocks(90 * 180) == 64 == N.nblk_of(90 * 180)


# ---------------- config ----------------------------------------------------------------------------------------------------------------
def test_training_config_reads_the_active_blocks_noise_mode(tmp_path):
    from aozora_sdxl_training_amd.config import TrainingConfig, flatten_preset
    assert TrainingConfig(argv=[]).NOISE_MODE == "normal"
    p = tmp_path / "preset.json"
    p.write_text(json.dumps({"active_mode": "sdxl", "sdxl": {"sdxl_batch_size": 3, "sdxl_noise_mode": "pyramid:levels=4"},
                             "anima": {"anima_noise_mode": "offset"}}))
    cfg = TrainingConfig(config_path=str(p))
    assert cfg.NOISE_MODE == "pyramid:levels=4" and cfg.BATCH_SIZE == 3
    assert "NOISE_MODE" not in flatten_preset(json.loads(p.read_text()))          # no row in the table: the flat preset is the reference's
    p.write_text(json.dumps({"active_mode": "sdxl", "sdxl": {"sdxl_batch_size": 3}}))
    assert TrainingConfig(config_path=str(p)).NOISE_MODE == "normal"
    p.write_text(json.dumps({"active_mode": "anima", "sdxl": {"sdxl_noise_mode": "pyramid"}, "anima": {"anima_noise_mode": "offset"}}))
    assert TrainingConfig(config_path=str(p)).NOISE_MODE == "offset"


def test_step_refuses_draws_it_cannot_use_before_anything_is_launched():
    """TrainStep._check_noise_aux is host logic: exercised here on a bare object, without a device."""
    from aozora_sdxl_training_amd._lib import AozoraError
    from aozora_sdxl_training_amd.train_step import TrainStep
    step = object.__new__(TrainStep)
    spec = nz.parse_noise_mode("pyramid:levels=2,offset=0.05,perturb=0.1")
    aux = nz.draw_aux(spec, (2, 4, 8, 8), 1, 1)
    step.noise_spec = spec
    step._check_noise_aux(aux, 2, 4, 8, 8)
    with pytest.raises(AozoraError, match="noise_aux"):
        step._check_noise_aux(None, 2, 4, 8, 8)
    for bad in (aux._replace(o=None), aux._replace(z=aux.z[:1]), aux._replace(xi=aux.xi[:1]), aux._replace(o=aux.o.double()),
                aux.rows(slice(0, 1)), aux._replace(z=[aux.z[1], aux.z[0]])):
        with pytest.raises(AozoraError, match="noise_aux"):
            step._check_noise_aux(bad, 2, 4, 8, 8)
    step.noise_spec = nz.parse_noise_mode("normal")
    step._check_noise_aux(None, 2, 4, 8, 8)
    with pytest.raises(AozoraError, match="noise_aux"):
        step._check_noise_aux(aux, 2, 4, 8, 8)
