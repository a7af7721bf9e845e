"""tests/attn_ref.py and the case tables of tests/test_attn_exact_gpu.py, without a GPU: every case is exact (`exact_ok`) and the fp32
emulation with the kernels' rounding points gives the closed form bit for bit; every family reaches the kernels it is about (by the
mirror of the host dispatch); the cases of a kernel path cover every head-dim column, every row position and every key position of
a 128-row block; and the comparison the GPU test uses rejects each planted defect."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import attn_ref as R                  # noqa: E402
import test_attn_exact_gpu as T       # noqa: E402

ALL_CASES = sorted({r.case for rows in T.FAMILIES.values() for r in rows})


@pytest.mark.parametrize("case", ALL_CASES, ids=R.case_id)
def test_case_is_exact_and_emulation_matches(case):
    assert R.exact_ok(case)
    assert case.bias or not R.ragged(case), "a ragged case without the bias column"
    d = R.build(case)
    assert R.mismatches(R.emulate(d), R.closed_form(d)) == []
    if case.Tq % 128 == 0 and case.Tk % 128 == 0:
        assert R.mismatches(R.emulate(d, fwd="dma"), R.closed_form(d)) == []


def test_lse_comparison():
    """4 fp32 ulp pass, 5 do not; a key counted twice or not at all moves lse2 by >= log2(3/2) = 0.58."""
    e = {"lse": np.array([-1915.7, 1038.4, 2.0])}
    u = R.ulp32(e["lse"])
    assert R.mismatches({"lse": e["lse"] + 4 * u}, e, ("lse",)) == []
    assert R.mismatches({"lse": e["lse"] - 5 * u}, e, ("lse",))
    assert R.mismatches({"lse": e["lse"] + np.log2(1.5)}, e, ("lse",))
    assert R.mismatches({"lse": np.array([np.nan, 1038.4, 2.0])}, e, ("lse",))
    assert R.mismatches({"O": np.array([np.nan])}, {"O": np.array([0.0])}, ("O",))


# ---------------- every listed path is taken -------------------------------------------------------------------------------------
def _union(rows):
    return {k for r in rows for k in T.kernels_of(r)[1]}


def test_paths_forward():
    assert all(T.kernels_of(r)[0] == "fwd_dma" for r in T.FWD_DMA)
    assert {(r.case.B, r.case.H, r.case.Tq, r.case.Tk) for r in T.FWD_DMA} == set(T.DMA_SHAPES)
    for s in T.DMA_SHAPES:
        assert {r.case.layout for r in T.FWD_DMA if (r.case.B, r.case.H, r.case.Tq, r.case.Tk) == s} == {"near", "far"}
    assert _union(T.FWD_DMA) >= {"merged_dma", "dq_dma_fused", "dkv_dma", "cross[3]", "reduce"}
    assert all(T.kernels_of(r)[0] == "fwd_full" for r in T.FWD_FULL)
    assert {(r.case.Tq, r.case.Tk) for r in T.FWD_FULL if r.pipe == 15} == {(128, 192), (256, 64)}
    assert all(T.kernels_of(r)[0] == "fwd_general" and r.case.bias for r in T.FWD_GENERAL)
    assert {r.case.Tq for r in T.FWD_GENERAL} == set(T.TQ_EDGES) and {r.case.Tk for r in T.FWD_GENERAL} == set(T.TK_EDGES)
    assert 28 <= len(T.FWD_GENERAL) <= 34


def test_paths_backward():
    for r in T.MERGED:
        assert T.kernels_of(r)[1] == ["delta", "merged_dma" if r.pipe & 8 else "merged"]
    assert {(r.case.Tq, r.pipe) for r in T.MERGED} == {(t, p) for t in (128, 256, 512) for p in (15, 7)}
    assert all(T.kernels_of(r)[1][0].startswith("cross[") for r in T.SHORT)
    assert {r.case.Tk for r in T.SHORT} == set(T.SHORT_TK) and {r.case.Tq for r in T.SHORT} == set(T.SHORT_TQ)
    assert _union(T.SHORT) >= {"cross[1]", "cross[2]", "cross[3]", "cross[5]", "reduce"}
    assert any(T.kernels_of(r)[1] == ["cross[1]"] and r.case.Tq == 640 for r in T.SHORT), "direct store after five tiles"
    u = _union(T.DQ_DKV)
    assert u >= {"delta", "dq_fused_full", "dq_fused_general", "dq_plain_full", "dq_plain_general", "dq_dma_fused", "dq_dma_plain",
                 "dkv[1]", "dkv[2]", "dkv[4]", "dkv_dma", "reduce"}
    assert not any(k.startswith(("merged", "cross")) for k in u)
    assert any("dkv[4]" in T.kernels_of(r)[1] and r.case.Tk == 154 for r in T.DQ_DKV)
    for s in {r.case for r in T.SCHEDULES}:
        assert [r.sched for r in T.SCHEDULES if r.case == s] == [(7,), (3, 4), (1, 6), (1, 2, 4), (5, 2)]
    want = ["cross[5]", "cross[1]", "cross[3]", "cross[1]", "dkv[4]", "dkv[1]", "dkv[2]", "dkv[1]"]
    assert [next(k for k in T.kernels_of(r)[1] if k.startswith(("cross", "dkv"))) for r in T.WORKSPACE] == want
    assert all(r.xcd == 0 for r in T.XCD) and len(T.XCD) == 12
    assert all(r.xcd == 15 for n, rows in T.FAMILIES.items() if n != "XCD" for r in rows)


# ---------------- coverage -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["FWD_DMA", "FWD_FULL", "FWD_GENERAL", "MERGED", "SHORT", "DQ_DKV"])
def test_coverage(family):
    """Over the cases of a kernel path: O, dQ, dK, dV are non-zero in every head-dim column and at every row position mod 128
    (as far as the path's rows reach), and every key position mod 128 is selected by some query."""
    cols = {n: np.zeros(64, bool) for n in ("O", "dQ", "dK", "dV")}
    rows = {n: np.zeros(128, bool) for n in cols}
    keys = np.zeros(128, bool)
    tq = max(r.case.Tq for r in T.FAMILIES[family])
    tk = max(r.case.Tk for r in T.FAMILIES[family])
    for c in sorted({r.case for r in T.FAMILIES[family]}):
        e = R.closed_form(R.build(c))
        for n in cols:
            nz = e[n] != 0
            cols[n] |= nz.any(axis=(0, 1, 2))
            r = nz.any(axis=(0, 1, 3))
            np.logical_or.at(rows[n], np.arange(len(r)) % 128, r)
        sel = (e["P"] > 0).any(axis=(0, 1, 2))
        np.logical_or.at(keys, np.arange(len(sel)) % 128, sel)
    for n in cols:
        assert cols[n].all(), f"{family}: {n} is zero in columns {np.flatnonzero(~cols[n])}"
        lim = min(128, tq if n in ("O", "dQ") else tk)
        assert rows[n][:lim].all(), f"{family}: {n} is zero at row positions {np.flatnonzero(~rows[n][:lim])}"
    assert keys[:min(128, tk)].all(), f"{family}: key positions {np.flatnonzero(~keys[:min(128, tk)])} are never selected"


# ---------------- sensitivity ------------------------------------------------------------------------------------------------------
def _sensitive(c):
    """Cases in which every defect of attn_ref.DEFECTS has something to break: a ragged last key tile, every group selected, a
    second 64-query slab, two heads."""
    return c.Tk % 64 != 0 and c.Tk >= 2 and c.Tq >= 128 and c.H >= 2 and c.g >= 2 and R.key_groups(c.Tk, c.g, c.layout)[1] <= c.Tq


SENSITIVE = [c for c in ALL_CASES if _sensitive(c)]


def test_sensitive_cases_exist():
    assert len(SENSITIVE) >= 8 and {c.layout for c in SENSITIVE} == {"near", "far"} and {c.g for c in SENSITIVE} == {2, 4}


@pytest.mark.parametrize("defect", R.DEFECTS)
@pytest.mark.parametrize("case", SENSITIVE, ids=R.case_id)
def test_defect_is_rejected(case, defect):
    """The emulation with one planted defect -- a key dropped, the last-tile mask off by one either way, padded keys unmasked, lse
    of the neighbouring query, two rows of a 32-row block swapped, a query slab left out of the dK / dV sum, delta of the wrong
    head -- does not pass the comparison of the GPU test."""
    d = R.build(case)
    bad = R.mismatches(R.emulate(d, defect), R.closed_form(d))
    assert bad, f"{defect} passes on {R.case_id(case)}"
    hit = {b.split(":")[0] for b in bad}
    want = {"drop_key": {"O", "lse", "dK", "dV"}, "mask_short": {"O", "lse", "dV"}, "mask_long": {"O", "lse", "dQ"},
            "unmasked": {"O", "lse", "dQ"}, "lse_neighbour": {"dQ", "dK", "dV"}, "swap_rows": {"O", "dQ"}, "drop_slab": {"dK", "dV"},
            "delta_wrong_head": {"dQ", "dK"}}[defect]
    assert want <= hit, f"{defect} on {R.case_id(case)} is seen by {sorted(hit)} only"


# ---------------- peaked inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,Tq,Tk", T.PEAKED)
def test_peaked_inputs(B, H, Tq, Tk):
    Q, K, V, dO, pmax = R.peaked_inputs(B, H, Tq, Tk, 0)
    assert all(R.is_bf16(x) for x in (Q, K, V, dO))
    P = R.reference64(Q, K, V, dO)["P"]
    assert abs(float(np.median(P.max(-1))) - 0.5) <= 0.05 and abs(pmax - 0.5) <= 0.05
    ref, emu = R.reference64(Q, K, V, dO), R.emulate_arrays(Q, K, V, dO)
    # the emulation is a sane yardstick: a few bf16 roundings for the typical row (a row whose probability sits on ONE key has
    # dS = P (dP - delta) ~ 0 by cancellation and a large relative error in dQ, in the emulation as in the kernels)
    for n in ("O", "dQ", "dK", "dV"):
        assert float(np.median(R.row_rel_l2(emu[n], ref[n]))) < 2.0 ** -7, n


@pytest.mark.parametrize("Tk", T.TK_EDGES)
def test_uniform_layer_on_the_emulation(Tk):
    """The assertions of the uniform layer hold for the emulation: they ask nothing a correct kernel cannot give."""
    for Tq in T.UNIFORM_TQ:
        Q, K, V, dO = T.uniform_inputs(Tq, Tk)
        assert T.uniform_failures(R.emulate_arrays(Q, K, V, dO), Q, K, V, dO) == []
