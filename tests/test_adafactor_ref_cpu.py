"""The Adafactor contract without a GPU: tests/adafactor_ref.py (float64) against the pinned fixture tests/golden/adafactor_golden.pt
(transformers 5.15.0) always, and against the live package where it imports; the state schema; the constructor refusals that need no
device.

Bounds (U = 2^-24, an independent float64 state carried over the steps):
  state       |s_pkg - s| <= (N + 8) U step |s|, N the number of terms of the mean (C for row, R for col, 1 for v): sums of N positive
              fp32 terms in any order, plus the roundings of the square, the division and the moving average;
  parameters  |p_pkg - x| <= half the bf16 spacing at max(|x|, |p_pkg|) + 2 (R + C + 32) U step |u| + 4 U |p_before|, x the unrounded
              float64 result and u the float64 update;
  exp_avg     |m_pkg - m| <= 2 (R + C + 32) U step avg|u|, the slack the parameter bound grants the update, averaged as exp_avg
              averages it.
Every element is checked, none is exempt."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adafactor_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "adafactor_golden.pt")
ISSUE_SHAPES = [(1,), (7,), (320,), (16, 1), (1, 16), (3, 5), (64, 64), (130, 257), (4, 1280), (1280, 4), (520, 72), (4, 5, 3, 3), (8, 4, 1, 1),
                (16, 24, 3, 3)]


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)


def test_fixture_is_the_pin(golden):
    assert golden["transformers"] == "5.15.0"
    assert [tuple(s) for s in golden["shapes"]] == R.FIXTURE_SHAPES and tuple(golden["grad_scales"]) == R.GRAD_SCALES
    assert os.path.getsize(GOLDEN) < 200 * 1000
    for rec, opt in zip(golden["sets"], R.OPTION_SETS):
        assert rec["options"] == {k: (list(v) if isinstance(v, tuple) else v) for k, v in opt.items()}


@pytest.mark.parametrize("si", range(len(R.OPTION_SETS)))
def test_restatement_agrees_with_the_fixture(golden, si):
    shapes, opt, rec = R.FIXTURE_SHAPES, R.OPTION_SETS[si], golden["sets"][si]
    un = lambda t: R.unpack(t.view(torch.bfloat16), shapes)
    st_shapes = [R.state_shape(k, s) for s in shapes for k in R.state_names(s, opt)]
    states = []
    for flat in rec["state"]:
        it = iter(R.unpack(flat, st_shapes))
        states.append([{k: next(it) for k in R.state_names(s, opt)} for s in shapes])
    worst = R.check_run(shapes, opt, un(golden["p0"]), [un(g) for g in golden["grads"]], [un(p) for p in rec["p"]], states)
    print("excess over the bounds (<= 1 passes):", worst)
    assert worst["state"] <= 1.0 and worst["param"] <= 1.0 and worst["exp_avg"] <= 1.0, worst


@pytest.mark.parametrize("si", range(len(R.OPTION_SETS)))
def test_restatement_agrees_with_the_live_package(si):
    """The shapes of the GPU tests at full size, where transformers is installed."""
    opt_mod = pytest.importorskip("transformers.optimization")
    opt = R.OPTION_SETS[si]
    gen = torch.Generator().manual_seed(77 + si)
    p0 = [(torch.randn(s, generator=gen) * 0.05).bfloat16() for s in ISSUE_SHAPES]
    grads = [[(torch.randn(s, generator=gen) * sc).bfloat16() for s in ISSUE_SHAPES] for sc in R.GRAD_SCALES]
    params = [torch.nn.Parameter(p.clone()) for p in p0]
    o = opt_mod.Adafactor(params, **opt)
    p_after, states = [], []
    for g in grads:
        for p, gi in zip(params, g):
            p.grad = gi.clone()
        o.step()
        p_after.append([p.detach().clone() for p in params])
        states.append([{k: o.state[p][k].clone() for k in R.state_names(s, opt)} for p, s in zip(params, ISSUE_SHAPES)])
    worst = R.check_run(ISSUE_SHAPES, opt, p0, grads, p_after, states)
    print("excess over the bounds (<= 1 passes):", worst)
    assert worst["state"] <= 1.0 and worst["param"] <= 1.0 and worst["exp_avg"] <= 1.0, worst


def test_lr_zero_leaves_parameters_and_moves_state():
    opt = R.options(lr=0.0)
    p = (torch.randn(5, 7) * 0.05).bfloat16()
    st = R.new_state((5, 7), opt)
    x, u = R.step(p.double(), torch.randn(5, 7).bfloat16().double(), st, 1, opt)
    assert torch.equal(x, p.double()) and float(u.abs().max()) == 0.0 and float(st["exp_avg_sq_row"].min()) > 0.0


def test_one_by_one_kernels_have_a_unit_row_factor():
    """(O, I, 1, 1): row = col = upd per element, so u = g / sqrt(upd) before the clip."""
    opt = R.options(lr=1.0, clip_threshold=1e9)
    g = torch.randn(8, 4, 1, 1).bfloat16().double()
    st = R.new_state((8, 4, 1, 1), opt)
    x, u = R.step(torch.zeros(8, 4, 1, 1).double(), g, st, 1, opt)
    assert torch.allclose(u, g / torch.sqrt(g * g + 1e-30), rtol=1e-12, atol=0)
    assert st["exp_avg_sq_row"].shape == (8, 4, 1) and st["exp_avg_sq_col"].shape == (8, 4, 1)


# ---- the state schema and the refusals that need no device ---------------------------------------------------------------------------
def _saved(named_shapes, beta1):
    from aozora_sdxl_training_amd.optimizers.adafactor import STATE_VERSION, state_shapes
    return {"version": STATE_VERSION, "options": {"beta1": beta1}, "step": 2,
            "state": {n: {k: torch.zeros(s) for k, s in state_shapes(shape, beta1).items()} for n, shape in named_shapes}}


def test_state_schema_round_trip(tmp_path):
    from aozora_sdxl_training_amd.optimizers.adafactor import check_state, state_shapes
    named = [("a.weight", (6, 5)), ("a.bias", (6,)), ("c.weight", (4, 3, 3, 3)), ("d.weight", (4, 2, 1, 1))]
    for beta1 in (None, 0.9):
        assert state_shapes((4, 3, 3, 3), beta1)["exp_avg_sq_row"] == (4, 3, 3) and state_shapes((4, 3, 3, 3), beta1)["exp_avg_sq_col"] == (4, 3, 3)
        assert {k: tuple(v) for k, v in state_shapes((6,), beta1).items()} == ({"exp_avg_sq": (6,)} if beta1 is None else {"exp_avg_sq": (6,), "exp_avg": (6,)})
        st = _saved(named, beta1)
        torch.save(st, tmp_path / "s.pt")
        back = torch.load(tmp_path / "s.pt")
        check_state(back, named, beta1)
        assert sorted(back["state"]["a.weight"]) == sorted(["exp_avg_sq_row", "exp_avg_sq_col"] + (["exp_avg"] if beta1 else []))
    st = _saved(named, None)
    with pytest.raises(ValueError, match="freeze mask"):
        check_state(st, named[:-1], None)                                     # another freeze mask: other names
    with pytest.raises(ValueError, match="shape"):
        check_state(st, [("a.weight", (6, 4))] + named[1:], None)             # another shape
    with pytest.raises(ValueError, match="beta1"):
        check_state(st, named, 0.9)                                           # exp_avg missing


def test_constructor_refusals_without_a_device():
    from aozora_sdxl_training_amd.optimizers import Adafactor
    from aozora_sdxl_training_amd._lib import AozoraError
    p = torch.nn.Parameter(torch.zeros(4, 4, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="warmup_init"):
        Adafactor([p], lr=1e-3, warmup_init=True)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="clip_threshold"):
            Adafactor([p], lr=1e-3, clip_threshold=bad)
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="beta1"):
            Adafactor([p], lr=1e-3, beta1=bad)
    with pytest.raises(AozoraError, match="3 dimensions"):
        Adafactor([torch.nn.Parameter(torch.zeros(2, 3, 4, dtype=torch.bfloat16))], lr=1e-3)
    with pytest.raises(AozoraError, match="kernel"):
        Adafactor([torch.nn.Parameter(torch.zeros(2, 3, 2, 2, dtype=torch.bfloat16))], lr=1e-3)
    q = torch.zeros(4, 4, dtype=torch.bfloat16)
    if hasattr(q, "grad_dtype"):
        q.grad_dtype = None                                                   # let torch attach a gradient of another dtype at all
    q.grad = torch.zeros(4, 4, dtype=torch.float32)
    with pytest.raises(AozoraError, match="bf16 gradients"):
        Adafactor([q], lr=1e-3)
    with pytest.raises(AozoraError, match="no CPU fallback"):
        Adafactor([p], lr=1e-3)                                               # valid options, but no device: never a quiet fallback


# ---- the entry point's own refusals: host-side, before any launch, so they need no device -------------------------------------------------
def test_entry_point_refuses_bad_arguments_before_any_launch():
    import ctypes
    from aozora_sdxl_training_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = L.lib()
    step, geo = lib._fn["az_adafactor_step"], lib._fn["az_adafactor_geometry"]
    W = geo(0)
    assert W == 24 and geo(1) > 0 and geo(99) <= -1000
    hyper = (ctypes.c_double * 16)(0.0, 1e-3, 1e-30, 1e-3, 1.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    hp = ctypes.cast(hyper, ctypes.c_void_p)
    buf = (ctypes.c_double * 64)()                       # 16-byte aligned host memory standing in for device buffers: never dereferenced
    a = ctypes.addressof(buf)
    a += (-a) % 16
    vp = ctypes.c_void_p
    assert step(0, None, None, None, 0, None, 0, None, 0, None, None, hp, None) == 0            # zero tensors: a successful no-op
    assert step(-1, None, None, None, 0, None, 0, None, 0, None, None, hp, None) <= -1000       # negative count
    assert step(0, None, None, None, -1, None, 0, None, 0, None, None, hp, None) <= -1000
    assert step(0, None, None, None, 0, None, 0, None, 0, None, None, None, None) <= -1000      # no hyper-parameters

    def row(**kw):
        r = dict(cls=1, flags=0, p=a, g=a, nb0=1, nb1=1, sb0=0, sb1=0, R=4, sr=8, C=8, sc=1, strow=0, stcol=64, stm=-1, first=0, nwg=1,
                 first2=0, n2=2, scr=0, fac=0, sr0=0, numel=32, spare=0)
        r.update(kw)
        return (ctypes.c_long * W)(*r.values())

    def call(desc, state_numel=128, **over):
        args = dict(n=1, dh=vp(ctypes.addressof(desc)), dd=vp(a), state=vp(a), sn=state_numel, scr=vp(a), scn=64, fac=vp(a), fn=64,
                    partials=vp(a), tsc=vp(a), hyper=hp, stream=None)
        args.update(over)
        return step(*args.values())

    # every refusal below comes from the host-side check of the table; a table that passed would launch, which this test never does
    assert call(row(cls=3)) <= -1000 and call(row(cls=-1)) <= -1000                              # unsupported class
    assert call(row(p=0)) <= -1000 and call(row(g=a + 1)) <= -1000                               # null, misaligned
    assert call(row(R=-4)) <= -1000 and call(row(C=0)) <= -1000                                  # negative / empty extents
    assert call(row(flags=1, C=12, sr=12, numel=48)) <= -1000                                    # 16-byte path needs C % 8 == 0
    assert call(row(flags=1, p=a + 2)) <= -1000                                                  # ... and 16-byte aligned storage
    assert call(row(cls=2, R=2, C=2, nb0=2, nb1=2, numel=16, n2=0)) <= -1000                     # a 2 x 2 kernel
    assert call(row(nwg=2)) <= -1000 and call(row(first=1)) <= -1000                             # a numbering that does not add up
    assert call(row(), state_numel=66) <= -1000                                                  # the column state would end outside
    assert call(row(scr=60)) <= -1000 and call(row(fac=56)) <= -1000                             # partials / factors outside
    assert call(row(), state=vp(a + 4)) <= -1000 and call(row(), dd=None) <= -1000               # misaligned / null buffers
