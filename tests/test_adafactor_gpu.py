"""optimizers.Adafactor on the GPU, on loose tensors and on hand-built slots of a ParamStore, against the float64 restatement
(tests/adafactor_ref.py) with the bounds of tests/test_adafactor_ref_cpu.py: every shape class in ONE descriptor table, a matrix of
several row stripes with a ragged last one, rows off the 16-byte boundary, a stored convolution with channel padding between
sentinels, the clip on both sides of its bend, beta1 / weight decay / scale_parameter, lr = 0, bit reproducibility, the state round
trip and stochastic rounding."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import adafactor_ref as R  # noqa: E402

DEV = "cuda:0"
BASE_SHAPES = [(1,), (7,), (320,), (16, 1), (1, 16), (3, 5), (64, 64), (130, 257), (4, 1280), (1280, 4), (4, 5, 3, 3), (8, 4, 1, 1), (16, 24, 3, 3)]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd._lib import lib
    return int(lib()._fn["az_adafactor_geometry"](1))            # the stripe height of the matrix kernels


@pytest.fixture(scope="module")
def data(gpu):
    """The shapes (the placeholder (520, 72) replaced by a matrix of three row stripes with a ragged last one, and one of 16-byte rows
    that spans stripes and column chunks), bf16 parameters and three bf16 gradients of scales 1e-1, 1e-2, 1e-3: made once, never changed."""
    shapes = BASE_SHAPES + [(2 * gpu + 40, 72), (gpu + 3, 2056)]
    gen = torch.Generator().manual_seed(4242)
    p0 = [(torch.randn(s, generator=gen) * 0.05).bfloat16() for s in shapes]
    grads = [[(torch.randn(s, generator=gen) * sc).bfloat16() for s in shapes] for sc in R.GRAD_SCALES]
    return shapes, p0, grads


def make(p0, grads0=None, **kw):
    from aozora_sdxl_training_amd.optimizers import Adafactor
    params = [p.clone().to(DEV) for p in p0]
    for p in params:
        p.grad = torch.zeros_like(p)
    if kw.get("lr", 0) is None:
        kw["lr"] = 0.0
    return params, Adafactor(params, **kw)


def run(shapes, p0, grads, **kw):
    """-> (p_after[step][tensor], state_after[step][tensor], the optimizer) on the host."""
    params, opt = make(p0, **kw)
    p_after, states = [], []
    for g in grads:
        for p, gi in zip(params, g):
            p.grad.copy_(gi)
        opt.step()
        st = opt.save_cpu_state()
        p_after.append([p.detach().cpu() for p in params])
        states.append([st["state"][f"param.{i}"] for i in range(len(params))])
    return p_after, states, opt


@pytest.mark.parametrize("si", range(len(R.OPTION_SETS)))
def test_every_class_in_one_table_against_float64(data, si):
    shapes, p0, grads = data
    opt = R.OPTION_SETS[si]
    p_after, states, o = run(shapes, p0, grads, **opt)
    assert len({e["cls"] for e in o.entries}) == 3 and any(e["nwg"] >= 3 and e["R"] % o.stripe_rows for e in o.entries)
    assert any(int(f) == 1 for f in o.desc_host[:, 1]) and any(e["cls"] == 1 and int(o.desc_host[i, 1]) == 0 for i, e in enumerate(o.entries))
    worst = R.check_run(shapes, opt, p0, grads, p_after, states)
    print("excess over the bounds (<= 1 passes):", worst)
    assert worst["state"] <= 1.0 and worst["param"] <= 1.0 and worst["exp_avg"] <= 1.0, worst
    assert o.state_bytes == 4 * sum(math.prod(R.state_shape(k, s)) for s in shapes for k in R.state_names(s, opt))


@pytest.mark.parametrize("clip", [0.5, 2.0])
def test_clip_on_both_sides_of_its_bend(data, clip):
    """At the first step |u| is near 1 in every tensor (RMS(u) between 0.5 and 2): clip_threshold 0.5 bends every tensor, 2 none."""
    shapes, p0, grads = data
    opt = R.options(lr=1e-2, clip_threshold=clip)
    p_after, states, o = run(shapes, p0, grads[:1], **opt)
    worst = R.check_run(shapes, opt, p0, grads[:1], p_after, states)
    assert worst["state"] <= 1.0 and worst["param"] <= 1.0, worst
    den = o.tsc.cpu().view(-1, 4)[:len(shapes), 0]
    assert bool((den > 1.0).all()) if clip == 0.5 else bool((den == 1.0).all())


@pytest.mark.parametrize("kw", [dict(lr=1e-2, beta1=0.9), dict(lr=1e-2, weight_decay=0.1), dict(lr=1e-2, beta1=0.5, weight_decay=0.1, clip_threshold=0.5),
                                dict(lr=1e-2, clip_threshold=2.0)], ids=["beta1", "decay", "both-bent", "neither-unbent"])
def test_beta1_and_weight_decay_on_and_off(data, kw):
    shapes, p0, grads = data
    opt = R.options(**kw)
    p_after, states, _ = run(shapes, p0, grads, **opt)
    worst = R.check_run(shapes, opt, p0, grads, p_after, states)
    print("excess over the bounds (<= 1 passes):", worst)
    assert worst["state"] <= 1.0 and worst["param"] <= 1.0 and worst["exp_avg"] <= 1.0, worst


def test_scale_parameter_below_eps2(data):
    """RMS(p) < eps2: lr_t = eps2 * lr."""
    shapes, p0, grads = data
    small = [(p.float() * 1e-3).bfloat16() for p in p0]
    assert all(R.rms(p.double()) < 1e-3 for p in small)
    opt = R.options(lr=1e-2, scale_parameter=True)
    p_after, states, o = run(shapes, small, grads[:2], **opt)
    worst = R.check_run(shapes, opt, small, grads[:2], p_after, states)
    assert worst["state"] <= 1.0 and worst["param"] <= 1.0, worst
    lr_t = o.tsc.cpu().view(-1, 4)[:len(shapes), 1]
    assert bool((lr_t == torch.tensor(1e-3 * 1e-2, dtype=torch.float32)).all())


def test_stored_convolution_between_sentinels(gpu):
    """Hand-built slots: conv_in [8][3][3][8] with logical I = 4, a matrix whose slot does not fill its 64 elements, a vector, a frozen
    matrix.  Padding channels, slot padding and the frozen slot hold NaN sentinels in p and g: they come back bit-identical and move no
    state, no RMS."""
    from aozora_sdxl_training_amd.params import ParamStore
    from aozora_sdxl_training_amd.optimizers import Adafactor
    table = [("conv_in.weight", (8, 4, 3, 3)), ("a.weight", (5, 7)), ("a.bias", (7,)), ("frozen.weight", (6, 10)), ("b.weight", (8, 4, 1, 1))]
    store = ParamStore(None, table, len(table), DEV)
    store._params["frozen.weight"].requires_grad = False
    assert store._slots["conv_in.weight"][1] == (8, 3, 3, 8)
    SENT_P, SENT_G = 0x7FC1, 0x7FC2                                 # quiet NaNs with distinct payloads
    store.pflat.view(torch.int16).fill_(SENT_P)
    store.gflat.view(torch.int16).fill_(SENT_G)
    gen = torch.Generator().manual_seed(9)
    names = [n for n, _ in table if n != "frozen.weight"]
    shapes = [s for n, s in table if n != "frozen.weight"]
    p0 = [(torch.randn(s, generator=gen) * 0.05).bfloat16() for s in shapes]
    grads = [[(torch.randn(s, generator=gen) * sc).bfloat16() for s in shapes] for sc in (1e-1, 1e-2)]
    logical = torch.zeros(store.flat_numel, dtype=torch.bool, device=DEV)
    with torch.no_grad():
        for n, p in zip(names, p0):
            store._params[n].copy_(p.to(DEV))
            o, st, shape = store._slots[n]
            v = logical[o:o + math.prod(st)].view(st)
            (v.permute(0, 3, 1, 2)[:, :shape[1]] if len(st) == 4 else v).fill_(True)
    opt_kw = R.options(lr=1e-2, scale_parameter=True, weight_decay=0.01, beta1=0.9, clip_threshold=0.5)
    opt = Adafactor(list(store.parameters()), **opt_kw)
    store._wt_dirty = False
    assert [e["name"] for e in opt.entries] == ["a.weight", "conv_in.weight", "a.bias", "b.weight"]
    p_after, states = [], []
    for g in grads:
        with torch.no_grad():
            for n, gi in zip(names, g):
                store._gviews[n].copy_(gi.to(DEV))
        opt.step()
        st = opt.save_cpu_state()
        p_after.append([store._params[n].detach().cpu().clone() for n in names])
        states.append([st["state"][n] for n in names])
    torch.cuda.synchronize()
    pb, gb = store.pflat.view(torch.int16), store.gflat.view(torch.int16)
    assert bool((pb[~logical] == SENT_P).all()) and bool((gb[~logical] == SENT_G).all())
    assert not bool(torch.isnan(store.pflat[logical].float()).any())
    worst = R.check_run(shapes, opt_kw, p0, grads, p_after, states)                 # NaN anywhere in a state or an RMS would show here
    print("excess over the bounds (<= 1 passes):", worst)
    assert worst["state"] <= 1.0 and worst["param"] <= 1.0 and worst["exp_avg"] <= 1.0, worst
    assert store._wt_dirty


@pytest.mark.parametrize("sr", [False, True], ids=["nearest", "stochastic"])
def test_lr_zero_moves_state_only(data, sr):
    shapes, p0, grads = data
    p_after, states, _ = run(shapes, p0, grads[:1], lr=0.0, stochastic_rounding=sr, sr_seed=3)
    for a, b, st in zip(p_after[0], p0, states[0]):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        assert all(float(t.min()) > 0.0 for t in st.values())


def test_two_runs_are_bitwise_equal_and_state_round_trips(data):
    shapes, p0, grads = data
    kw = dict(lr=1e-2, beta1=0.9, weight_decay=0.01, scale_parameter=True, stochastic_rounding=True, sr_seed=11)
    pa, sa, _ = run(shapes, p0, grads, **kw)
    pb, sb, _ = run(shapes, p0, grads, **kw)
    for k in range(3):
        for x, y, s, t in zip(pa[k], pb[k], sa[k], sb[k]):
            assert torch.equal(x.view(torch.int16), y.view(torch.int16))
            assert all(torch.equal(s[n], t[n]) for n in s)
    # save after step 1 -> a fresh optimizer on the parameters of step 1 -> steps 2 and 3 equal the uninterrupted run bit for bit
    params, first = make(p0, **kw)
    for p, gi in zip(params, grads[0]):
        p.grad.copy_(gi)
    first.step()
    saved = first.save_cpu_state()
    assert saved["step"] == 1 and saved["version"] == "aozora-adafactor-1"
    params2, second = make([p.detach().cpu() for p in params], **kw)
    second.load_cpu_state(saved)
    for k in (1, 2):
        for p, gi in zip(params2, grads[k]):
            p.grad.copy_(gi)
        second.step()
        st = second.save_cpu_state()
        for i, p in enumerate(params2):
            assert torch.equal(p.detach().cpu().view(torch.int16), pa[k][i].view(torch.int16))
            assert all(torch.equal(st["state"][f"param.{i}"][n], sa[k][i][n]) for n in sa[k][i])
    # a state of other tensors is refused
    _, other = make(p0[:-1], **kw)
    with pytest.raises(ValueError, match="freeze mask"):
        other.load_cpu_state(saved)


def test_stochastic_rounding(gpu):
    """n = 65536 elements whose update is below a quarter of the bf16 spacing: round-to-nearest cannot move them, stochastic rounding
    moves each with probability |lr u| / spacing to the neighbour on the update's side, without bias."""
    n, shape = 65536, (256, 256)
    gen = torch.Generator().manual_seed(31)
    sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0)
    p0 = ((0.035 + 0.02 * torch.rand(shape, generator=gen)) * sign).bfloat16()          # one binade: spacing 2^-12 everywhere
    g = ((0.5 + 0.5 * torch.rand(shape, generator=gen)) * 1e-2).bfloat16()              # one sign: round-to-nearest errs one way
    sp = 2.0 ** -12
    assert bool((R.bf16_spacing(p0.double()) == sp).all())
    _, unit = R.step(p0.double(), g.double(), R.new_state(shape, R.options(lr=1.0)), 1, R.options(lr=1.0))
    lr = 0.24 * sp / float(unit.abs().max())
    opt = R.options(lr=lr)
    x, u = R.step(p0.double(), g.double(), R.new_state(shape, opt), 1, opt)
    assert float(u.abs().max()) < sp / 4
    nearest, _, _ = run([shape], [p0], [[g]], lr=lr)
    assert torch.equal(nearest[0][0].view(torch.int16), p0.view(torch.int16))            # round to nearest: nothing moves
    sr, _, _ = run([shape], [p0], [[g]], lr=lr, stochastic_rounding=True, sr_seed=5)
    got = sr[0][0].double()
    slack = 2 * (256 + 256 + 32) * R.U * u.abs() + 4 * R.U * p0.double().abs()
    lo, hi = torch.floor((x - slack) / sp) * sp, torch.ceil((x + slack) / sp) * sp
    assert bool(((got >= lo) & (got <= hi)).all())                                        # one of the two bf16 neighbours of x
    q = u.abs() / sp
    moved = (got != p0.double())
    sd = math.sqrt(float((q * (1 - q)).sum())) / n
    share, want = float(moved.double().mean()), float(q.mean())
    print(f"moved {share:.5f}, expected {want:.5f} +- {sd:.5f}; bias sum {float(((got - x) / sp).sum()):.1f} (bound {2.5 * math.sqrt(n):.0f})")
    assert abs(share - want) <= 5 * sd
    assert abs(float(((got - x) / sp).sum())) <= 2.5 * math.sqrt(n)
    assert abs(float(((nearest[0][0].double() - x) / sp).sum())) > 10 * 2.5 * math.sqrt(n)          # round to nearest fails it tenfold
    again, _, _ = run([shape], [p0], [[g]], lr=lr, stochastic_rounding=True, sr_seed=5)
    assert torch.equal(again[0][0].view(torch.int16), sr[0][0].view(torch.int16))         # same seed, same step: same bits
    other_seed, _, _ = run([shape], [p0], [[g]], lr=lr, stochastic_rounding=True, sr_seed=6)
    assert not torch.equal(other_seed[0][0].view(torch.int16), sr[0][0].view(torch.int16))
    # another optimizer step draws other bits: a fresh optimizer told that one step lies behind it
    params, o = make([p0], lr=lr, stochastic_rounding=True, sr_seed=5)
    st = o.save_cpu_state()
    st["step"] = 1
    o.load_cpu_state(st)
    params[0].grad.copy_(g)
    o.step()
    assert o.optimizer_step == 2
    moved2 = params[0].detach().cpu().double() != p0.double()
    assert int((moved2 != moved).sum()) > 100
