"""lora_exec.LoraRoutes and lora_exec.wt_jobs without a device: the shipped thresholds, every routing predicate on both sides of its
edges (the table is read off the rules as they stood inside AozoraUNet), the independence of per-instance overrides, and the
transposed-copy jobs of small adapter tables laid out by params.ParamStore."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from aozora_sdxl_training_amd._lib import AozoraError                      # noqa: E402
from aozora_sdxl_training_amd.lora_exec import LoraRoutes, wt_jobs        # noqa: E402
from aozora_sdxl_training_amd.params import ParamStore                    # noqa: E402

T, F = True, False
DEFAULTS = dict(DOWN_GEMM_ROWS=8192, DOWN_GEMM_RANK=64, UP_FEW_ROWS=512, UP_FEW_RANK=32, UP_FUSED_ROWS=4096, UP_FUSED_RANK=16,
                UP_GEGLU_ROWS=8192, UP_GEGLU_RANK=64, CONV_DOWN_GEMM=((65536, 16), (16384, 64)), CONV_DGRAD_GEMM=((4096, 16),),
                CONV_WGRAD_GEMM=((4096, 16),))


def test_shipped_thresholds():
    assert len(DEFAULTS) == 11
    for name, value in DEFAULTS.items():
        assert getattr(LoraRoutes, name) == value and getattr(LoraRoutes(), name) == value, name


@pytest.mark.parametrize("args, want", [((8192, 64), T), ((8191, 64), F), ((8192, 56), F), ((8192, 68), F), ((16384, 192), T)])
def test_down_general(args, want):
    assert LoraRoutes().down_general(*args) is want


@pytest.mark.parametrize("args, want", [((4096, 16, 0.5, 1), T), ((4096, 4, 1.0, 1), T), ((4096, 12, 1.0, 1), T), ((512, 32, 1.0, 1), T),
                                        ((513, 32, 1.0, 1), F), ((512, 40, 1.0, 1), F), ((4096, 16, 1.0, 3), T), ((4097, 16, 1.0, 3), F),
                                        ((4096, 24, 1.0, 3), F), ((4096, 16, 1.0, 2), F)])
def test_up_own(args, want):
    assert LoraRoutes().up_own(*args) is want
    if args[3] == 1:
        assert LoraRoutes().up_own(*args[:3]) is want          # parts defaults to 1


@pytest.mark.parametrize("args, want", [((4096, 16, 0.5), T), ((8192, 64, 0.5), F), ((8192, 32, 0.5), T), ((8191, 64, 0.5), T),
                                        ((4096, 16, 1.0), F), ((512, 16, 1.0), T)])
def test_up_geglu_fused(args, want):
    assert LoraRoutes().up_geglu_fused(*args) is want


@pytest.mark.parametrize("args, want", [((1.0, 16), T), ((1.0, 4), F), ((2.0, 16), F)])
def test_tall_general(args, want):
    assert LoraRoutes().tall_general(*args) is want


@pytest.mark.parametrize("args, want", [((65536, 16), T), ((65535, 16), F), ((16384, 64), T), ((16384, 32), F), ((65536, 8), F), ((65536, 20), F)])
def test_conv_general_down(args, want):
    R = LoraRoutes()
    assert R.conv_general(R.CONV_DOWN_GEMM, *args) is want


@pytest.mark.parametrize("rule", ["CONV_DGRAD_GEMM", "CONV_WGRAD_GEMM"])
@pytest.mark.parametrize("args, want", [((4096, 16), T), ((4095, 16), F), ((4096, 8), F), ((1 << 20, 4), F)])
def test_conv_general_dgrad_wgrad(rule, args, want):
    R = LoraRoutes()
    assert R.conv_general(getattr(R, rule), *args) is want


def test_instances_are_independent():
    a, b = LoraRoutes(), LoraRoutes()
    a.DOWN_GEMM_ROWS, a.UP_FEW_ROWS, a.CONV_DGRAD_GEMM = 1000, 0, ((0, 0),)
    assert a.down_general(1000, 64) and not a.up_own(512, 32, 1.0) and a.conv_general(a.CONV_DGRAD_GEMM, 8, 8)
    assert not b.down_general(1000, 64) and b.up_own(512, 32, 1.0) and not b.conv_general(b.CONV_DGRAD_GEMM, 8, 8)
    for name, value in DEFAULTS.items():
        assert getattr(b, name) == value and getattr(LoraRoutes, name) == value, name


# ---------------- the transposed-copy jobs: slots as ParamStore._layout makes them, name -> (offset, storage shape, logical shape) -------------
A_, B_ = ".lora_A.weight", ".lora_B.weight"


def _slots(entries):
    """(name, logical shape) in table order -> (table, slots) of the real layout: a store of adapter entries only, on the CPU.  The store's
    constructor makes the same wt_jobs call over them: a table that wt_jobs refuses is refused in here already, with the same error."""
    return entries, ParamStore(None, entries, 0, "cpu")._slots


def test_three_adjacent_down_matrices_are_one_job():
    r, K, N = 4, 128, 128
    table, slots = _slots([(p + A_, (r, K)) for p in ("q", "k", "v")] + [(p + B_, (N, r)) for p in ("q", "k", "v")] + [("o" + A_, (r, K)), ("o" + B_, (N, r))])
    lin, conv = wt_jobs(table, slots)
    assert conv == []
    assert lin == [(0, 3 * r, K)] + [(slots[p + B_][0], N, r) for p in ("q", "k", "v")] + [(slots["o" + A_][0], r, K), (slots["o" + B_][0], N, r)]
    assert slots["k" + A_][0] == r * K and slots["v" + A_][0] == 2 * r * K          # the stack is adjacent: one [3r][K] matrix


def test_a_fourth_adjacent_down_matrix_is_refused():
    with pytest.raises(AozoraError, match="at most 3 parts"):
        wt_jobs(*_slots([(p + A_, (4, 128)) for p in ("q", "k", "v", "w")]))


def test_a_4d_down_matrix_is_a_conv_job():
    r, Cin, N = 8, 64, 128
    table, slots = _slots([("c1" + A_, (r, Cin, 3, 3)), ("c1" + B_, (N, r)), ("sc" + A_, (4, 64)), ("sc" + B_, (N, 4))])
    lin, conv = wt_jobs(table, slots)
    assert conv == [(0, r, Cin)]
    assert lin == [(slots["c1" + B_][0], N, r), (slots["sc" + A_][0], 4, 64), (slots["sc" + B_][0], N, 4)]


def test_a_slot_that_is_no_multiple_of_64_elements_is_refused():
    with pytest.raises(AozoraError, match="64-element slots"):
        wt_jobs(*_slots([("q" + A_, (4, 24)), ("q" + B_, (128, 4))]))
