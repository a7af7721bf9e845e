"""TrainStep(..., noise=...) on the mini UNet (16 x 16 latents, B = 2; the fixture of tests/test_loss_step_gpu.py): the step's noisy
latents and target are, bit for bit, what az_noise_shape + az_noise_target_ex give when called on their own on the step's inputs;
eager issue, Python tape replay, the native tape and the captured graph agree bit for bit under
pyramid:levels=2,offset=0.05,perturb=0.1; with noise="normal" the recorded tape is the one recorded without the argument; draws the
spec cannot use, or missing ones, are refused before anything runs."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_loss_step_gpu as LS        # noqa: E402
from test_loss_step_gpu import unet     # noqa: E402,F401  (the module-scoped mini UNet fixture)
from aozora_sdxl_training_amd import noise as nz      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = LS.DEV
BF16, F32 = torch.bfloat16, torch.float32
B, H, W = LS.B, LS.H, LS.W
bits = LS.bits
SPEC = "pyramid:levels=2,offset=0.05,perturb=0.1"


def _aux(spec, micro_step=1):
    return nz.draw_aux(nz.parse_noise_mode(spec), (B, 4, H, W), 42, micro_step)


@pytest.mark.parametrize("mode,spec", [("v_prediction", SPEC), ("epsilon", "offset"), ("rectified_flow", "normal:perturb=0.2"),
                                       ("epsilon", "pyramid"), ("rectified_flow", SPEC)])
def test_step_noise_launches_equal_the_kernels_called_on_their_own(unet, mode, spec):
    from aozora_sdxl_training_amd import ops
    from aozora_sdxl_training_amd.train_step import MODES, TrainStep
    ns = nz.parse_noise_mode(spec)
    args, ts, jit = LS._args(unet)
    aux = _aux(spec)
    step = TrainStep(unet, mode=mode, grad_accum=2, use_graph=False, noise=spec)
    unet.zero_grad()
    loss = step.micro_step(*args, noise_aux=aux)
    step.synchronize()
    torch.cuda.synchronize()
    bk = step.last_bucket
    assert (bk.n_o is not None) == (ns.offset > 0) and (bk.n_fields is not None) == (ns.levels > 0) == (bk.n_table is not None)
    assert (bk.n_xi is not None) == (ns.perturb > 0) and (bk.n_part is not None) == ns.normalises
    noise = args[1]
    u = noise.clone()
    C = 4
    part = None
    if ns.needs_shape:
        rows, total = nz.level_table(B, C, H, W, ns)
        part = torch.zeros(B, ops.noise_partial_blocks(H * W), 2, dtype=F32, device=DEV) if ns.normalises else None
        ops.noise_shape(u, aux.o.to(DEV) if ns.offset > 0 else None, ns.offset, aux.packed().to(DEV) if ns.levels else None,
                        nz.table_tensor(rows).to(DEV) if ns.levels else None, rows, part)
        assert not torch.equal(u, noise)
        assert bool((bits(bk.noise) == bits(u)).all()), "the step's shaped noise differs from az_noise_shape on its own"
    else:
        assert bool((bits(bk.noise) == bits(noise)).all())
    x8 = torch.zeros(B, H, W, 8, dtype=BF16, device=DEV)
    tg = torch.empty(B, C, H, W, dtype=F32, device=DEV)
    ops.noise_target_ex(MODES[mode], args[0], u, bk.dev[0], bk.dev[1], part, aux.xi.to(DEV) if ns.perturb > 0 else None, ns.perturb, x8, tg)
    torch.cuda.synchronize()
    assert bool((bits(bk.x8) == bits(x8)).all()) and bool((bits(bk.target) == bits(tg)).all()) and bool((bits(x8[..., C:]) == 0).all())
    # ... and it is not what plain noise gives
    x0 = torch.zeros(B, H, W, 8, dtype=BF16, device=DEV)
    t0 = torch.empty(B, C, H, W, dtype=F32, device=DEV)
    ops.noise_target(MODES[mode], args[0], noise, bk.dev[0], bk.dev[1], x0, t0)
    torch.cuda.synchronize()
    assert not torch.equal(x0, x8)
    if ns.needs_shape:
        assert not torch.equal(t0, tg)
        if ns.normalises:           # per-sample unit variance (the normalised noise is the epsilon target; any mode: bk.noise * r_b)
            s1, s2 = part[:, :, 0].sum(1).double(), part[:, :, 1].sum(1).double()
            n = C * H * W
            std = ((s2 - s1 * s1 / n) / (n - 1)).sqrt()
            assert bool(((std - u.double().reshape(B, -1).std(dim=1)).abs() <= 1e-5 * std).all())
    else:
        assert torch.equal(t0, tg)      # perturbation alone leaves the target alone
    assert float(loss) > 0 and float(unet.gflat.float().abs().max()) > 0


def test_eager_python_replay_native_tape_and_graph_agree_under_a_noise_mode(unet):
    from aozora_sdxl_training_amd.train_step import TrainStep
    args, _, _ = LS._args(unet)
    aux = [_aux(SPEC, 1), _aux(SPEC, 2)]

    def window(step):
        unet.zero_grad()
        losses = [step.micro_step(*args, noise_aux=aux[i]).item() for i in range(2)]
        step.synchronize()
        return losses, unet.gflat.clone()
    ref = None
    for native in (False, True):
        step = TrainStep(unet, mode="v_prediction", grad_accum=2, use_graph=False, noise=SPEC)
        step.native_tape = native
        for l, g in [window(step) for _ in range(3)]:          # window 1: eager issue and the recording; 2, 3: replay
            if ref is None:
                ref = (l, g)
            assert l == ref[0] and torch.equal(g, ref[1])
        bk = step.last_bucket
        assert bk.tape is not None
        names = [op.name for op in bk.tape if hasattr(op, "name")]
        assert names.count("az_noise_shape") == 1 and names.count("az_noise_target_ex") == 1 and "az_noise_target" not in names
        assert names.index("az_noise_shape") < names.index("az_noise_target_ex")
        if native:
            assert bk.ntape is not None and bk.ntape.n == len(bk.tape)
    graphed = TrainStep(unet, mode="v_prediction", grad_accum=2, use_graph=True, noise=SPEC)
    for i in range(2):                                       # window 1: eager run, then capture + replay; window 2: replays
        l, g = window(graphed)
        assert l == ref[0] and torch.equal(g, ref[1]), f"graph window {i} differs from eager"
    assert graphed.last_bucket.graph is not None
    assert ref[0][0] > 0 and ref[0][0] != ref[0][1] and float(ref[1].float().abs().max()) > 0
    # perturbation alone: no shaping launch
    step = TrainStep(unet, mode="epsilon", grad_accum=2, use_graph=False, noise="normal:perturb=0.2")
    a = _aux("normal:perturb=0.2")
    unet.zero_grad()
    for _ in range(2):
        step.micro_step(*args, noise_aux=a)
    step.synchronize()
    names = [op.name for op in step.last_bucket.tape if hasattr(op, "name")]
    assert "az_noise_shape" not in names and names.count("az_noise_target_ex") == 1 and "az_noise_target" not in names


def test_with_normal_noise_the_tape_is_the_one_recorded_without_the_argument(unet):
    base, l0, shape0, g0 = LS._tape_of(unet)
    for spelling in ("normal", "NORMAL", None, "", nz.parse_noise_mode("normal"), "offset:offset=0"):
        t, l, shape, g = LS._tape_of(unet, noise=spelling)
        assert shape == shape0
        assert [x[:2] for x in t] == [x[:2] for x in base]
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(t, base)) if a != b]
        assert not diff, diff[:3]
        assert l == l0 and torch.equal(g, g0)
    names = [x[1] for x in base]
    assert names.count("az_noise_target") == 1 and "az_noise_shape" not in names and "az_noise_target_ex" not in names


def test_draws_are_required_or_refused_before_anything_runs(unet):
    from aozora_sdxl_training_amd._lib import AozoraError
    from aozora_sdxl_training_amd.train_step import TrainStep
    args, _, _ = LS._args(unet)
    step = TrainStep(unet, mode="epsilon", grad_accum=2, use_graph=False, noise=SPEC)
    aux = _aux(SPEC)
    for bad in (None, aux._replace(o=None), aux._replace(z=aux.z[:1]), aux.rows(slice(0, 1)), aux._replace(xi=aux.xi.double())):
        with pytest.raises(AozoraError, match="noise_aux"):
            step.micro_step(*args, noise_aux=bad)
    assert not step._buckets and step.last_bucket is None          # nothing was allocated, staged or launched
    plain = TrainStep(unet, mode="epsilon", grad_accum=2, use_graph=False)
    with pytest.raises(AozoraError, match="noise_aux"):
        plain.micro_step(*args, noise_aux=aux)
    assert not plain._buckets
    with pytest.raises(ValueError, match="NOISE_MODE"):
        TrainStep(unet, mode="epsilon", noise="pyramyd")
