"""LoRA max-norm (LORA_PARAMS "scale_weight_norms") without a GPU: the reference's two forms of the norm agree on the inputs the GPU
test uses, no Gaussian case sits where the decision could go either way, the exactly summable inputs are what they claim to be, and
the option travels from LORA_PARAMS through LoraSpec into the adapter file's metadata -- refused where it cannot be read, and absent =
today's spec."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import lora_maxnorm_ref as N        # noqa: E402


def test_gram_identity_equals_the_materialised_norm():
    for mods in (N.exact_inputs(), N.gauss_inputs()):
        for A, B, s in mods:
            g, p = N.n2_gram(A, B, s), N.n2_product(A, B, s)
            assert abs(g - p) <= 1e-12 * max(p, 1e-300), (A.shape, B.shape, g, p)


def test_no_gaussian_case_sits_on_the_decision():
    """A condition on the INPUTS: |norm / max_norm - 1| is at least 10 times the relative bound on the kernel's norm (half of n2's)."""
    over = []
    for i, (A, B, s) in enumerate(N.gauss_inputs()):
        n2 = N.n2_gram(A, B, s)
        norm, _, o = N.rule64(n2, N.MAX_NORM)
        over.append(o)
        if i == N.B_ZERO:
            assert n2 == 0.0 and not o
            continue
        rel = N.n2_bound(A, B, s) / n2 / 2.0 + N.U
        assert abs(norm / N.MAX_NORM - 1.0) >= 10.0 * rel, (i, norm, rel)
        assert abs(norm / N.MAX_NORM - N.GAUSS_RATIO[i]) < 1e-3 * N.GAUSS_RATIO[i]
        assert N.q_bound(A, B, s) < 1e-2          # the bound says something (rank 64: r^2 u on sums of absolute values)
    assert sum(over) == 3 and len(over) == 6      # half of the modules are above the limit


def test_exact_inputs_are_exactly_summable():
    """Integers (quarter-integers in B) small enough that every partial sum is exact in fp32 in ANY order, n2 a perfect square,
    max_norm / norm a power of 4 for the modules above the limit, and one module exactly ON the limit."""
    over = []
    for i, ((A, B, s), (_, norm_want)) in enumerate(zip(N.exact_inputs(), N.EXACT)):
        assert np.array_equal(A, np.round(A)) and np.array_equal(4 * B, np.round(4 * B))
        ga, gb = np.abs(A) @ np.abs(A).T, np.abs(B).T @ np.abs(B)
        assert (ga * gb).sum() < 2 ** 22          # the sums of absolute values: every partial sum is a multiple of 1/4 below 2^24 / 4
        assert math.log2(s) == int(math.log2(s))
        n2 = N.n2_gram(A, B, s)
        norm, q, o = N.rule64(n2, N.MAX_NORM)
        assert norm == norm_want and n2 == norm_want ** 2
        n32, q32, o32 = N.rule32(n2, N.MAX_NORM)
        assert (float(n32), float(q32), o32) == (norm, q, o)          # nothing is rounded on the way
        if o:
            assert math.log(N.MAX_NORM / norm, 4) == int(math.log(N.MAX_NORM / norm, 4))
        over.append(o)
    assert over == [True, False, True, False, True, False] and N.EXACT[1][1] == N.MAX_NORM


def test_element_update_rounds_to_nearest_even():
    bits = np.array([0x3F80, 0x3F81, 0x3F82, 0xBF81, 0x0000, 0x7F80, 0x7FC0], dtype=np.uint16)
    q = np.float32(0.5) + np.float32(2.0 ** -9)          # 1.0078125 * q = 0.50784..: a tie of the product is broken to even
    got = N.scale_bits(bits, q)
    x = (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        want64 = x * float(q)
    back = (got.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    ok = np.isfinite(want64)
    assert np.all(np.abs(back[ok] - want64[ok]) <= 2.0 ** -8 * np.abs(want64[ok]))          # within half a bf16 ulp
    assert got[4] == 0 and got[5] == 0x7F80 and (got[6] & 0x7FFF) > 0x7F80
    w, b = N.scale_master(np.array([1.00390625, -3.0], dtype=np.float32), 0.5)
    assert w.tolist() == [0.501953125, -1.5] and b.tolist() == [0x3F00, 0xBFC0]           # the tie 0.501953125 goes to even


# ---------------- the option --------------------------------------------------------------------------------------------------------------
def _options(**hp):
    from aozora_sdxl_training_amd import lora
    from aozora_sdxl_training_amd.unet_spec import mini_config
    return lora.options(SimpleNamespace(LORA_PARAMS=hp), cfg=mini_config())[0]


@pytest.mark.parametrize("value, want", [(1.0, 1.0), (2, 2.0), ("0.75", 0.75), (1e-3, 1e-3), (None, None)])
def test_options_accept_scale_weight_norms(value, want):
    spec = _options(rank=8, scale_weight_norms=value)
    assert spec.max_norm == want and (want is None or isinstance(spec.max_norm, float))


@pytest.mark.parametrize("value", [0, 0.0, -1.0, float("inf"), float("-inf"), float("nan"), True, False, [1.0], (1.0,), {"a": 1}, "one", "", "nan", "inf"])
def test_options_refuse_what_is_no_positive_finite_number(value):
    with pytest.raises(ValueError, match="scale_weight_norms"):
        _options(rank=8, scale_weight_norms=value)


def test_spec_without_the_key_equals_todays():
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    assert _options(rank=8, alpha=4.0) == LoraSpec(8, 4.0)
    assert _options(rank=8, alpha=4.0, scale_weight_norms=None) == LoraSpec(8, 4.0)
    assert LoraSpec(8, 4.0).max_norm is None
    assert _options(rank=8, alpha=4.0, scale_weight_norms=1.5) == LoraSpec(8, 4.0, max_norm=1.5) != LoraSpec(8, 4.0)
    # the field is the LAST one: every positional construction of today means what it meant
    assert LoraSpec(8, 4.0, "", "unet", 4, 2.0, 0.1, 0.2, 0.3) == LoraSpec(8, 4.0, "", "unet", 4, 2.0, 0.1, 0.2, 0.3, None)
    for bad in (0, -1.0, float("inf"), float("nan"), True, "1.0", [1.0]):
        with pytest.raises(ValueError, match="max_norm"):
            LoraSpec(8, 4.0, max_norm=bad)


def test_file_metadata_carries_the_key_only_when_set():
    from aozora_sdxl_training_amd import lora
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    assert "ss_scale_weight_norms" not in lora.file_metadata(LoraSpec(8, 4.0))
    meta = lora.file_metadata(LoraSpec(8, 4.0, max_norm=0.75))
    assert float(meta["ss_scale_weight_norms"]) == 0.75
    rest = {k: v for k, v in meta.items() if k != "ss_scale_weight_norms"}
    assert rest == lora.file_metadata(LoraSpec(8, 4.0))


def test_job_row_checks():
    """The table builder's refusals (the kernel skips such a row; the builder never writes one)."""
    from aozora_sdxl_training_amd import lora_norm
    from aozora_sdxl_training_amd._lib import AozoraError
    good = [4096, 8192, 16, 64, 16, lora_norm.s_bits(0.5), 0, 0]
    lora_norm.check_row(good)
    assert lora_norm.s_bits(0.5) == 0x3F000000
    for k, v in ((2, 12), (2, 128), (3, 0), (3, 12), (4, 20), (4, -8), (0, 0), (1, 0), (0, 4104), (6, 8), (7, 4)):
        bad = list(good)
        bad[k] = v
        with pytest.raises(AozoraError):
            lora_norm.check_row(bad)
    for bad in (0, -1.0, float("inf"), float("nan"), True, "1", None):
        with pytest.raises(ValueError):
            lora_norm.check_max_norm(bad)
