"""optimizers.Adafactor on the mini UNet of test_master_optim_gpu.make_unet (conv1 / conv2 frozen): the gradients of one real
micro-step, then Adafactor.step(), against the float64 restatement applied to named_parameters() and the logical gradient views with
the bounds of tests/test_adafactor_ref_cpu.py; frozen ranges and all padding stay bit for bit; state_bytes is the sum over logical
shapes; the next forward refreshes the W^T mirror; a state of another freeze mask is refused."""
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
OPT = R.options(lr=1e-2, weight_decay=0.01, beta1=0.9, scale_parameter=True, clip_threshold=0.5)


def _micro_step(u):
    from aozora_sdxl_training_amd.train_step import TrainStep
    from test_model_gpu import _inputs
    lat, noise, ctx, pooled, tid, ts, jit = _inputs(2, 8, 8, u.cfg, seed=3)
    step = TrainStep(u, mode="epsilon", grad_accum=1, use_graph=False)
    step.micro_step(lat.to(DEV), noise.to(DEV), ts, ctx.to(DEV), pooled.to(DEV), tid.to(DEV), jit)
    step.synchronize()
    return step


@pytest.fixture(scope="module")
def stepped():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_master_optim_gpu import make_unet
    from aozora_sdxl_training_amd.optimizers import Adafactor
    u = make_unet()
    u.zero_grad()
    step = _micro_step(u)
    u.expose_grads()
    torch.cuda.synchronize()
    names = [n for n, p in u.named_parameters() if p.requires_grad]
    p0 = {n: p.detach().cpu().clone() for n, p in u.named_parameters() if p.requires_grad}
    g0 = {n: p.grad.detach().cpu().clone() for n, p in u.named_parameters() if p.requires_grad}
    pflat0, gflat0 = u.pflat.clone(), u.gflat.clone()
    opt = Adafactor([p for p in u.parameters()], **OPT)          # frozen parameters are handed over too: they own no state
    opt.step()
    torch.cuda.synchronize()
    return dict(u=u, opt=opt, names=names, p0=p0, g0=g0, pflat0=pflat0, gflat0=gflat0, step=step)


def test_one_step_against_float64(stepped):
    u, opt, names = stepped["u"], stepped["opt"], stepped["names"]
    assert sorted(e["name"] for e in opt.entries) == sorted(names) and len({e["cls"] for e in opt.entries}) == 3
    shapes = [tuple(stepped["p0"][n].shape) for n in names]
    st = opt.save_cpu_state()
    got_p = dict(u.named_parameters())
    worst = R.check_run(shapes, OPT, [stepped["p0"][n] for n in names], [[stepped["g0"][n] for n in names]],
                        [[got_p[n].detach().cpu() for n in names]], [[st["state"][n] for n in names]])
    print("excess over the bounds (<= 1 passes):", worst)
    assert worst["state"] <= 1.0 and worst["param"] <= 1.0 and worst["exp_avg"] <= 1.0, worst
    assert any(float(stepped["g0"][n].float().abs().max()) > 0 for n in names)
    assert opt.state_bytes == 4 * sum(math.prod(R.state_shape(k, s)) for s in shapes for k in R.state_names(s, OPT))
    assert st["step"] == 1 and sorted(st["state"]) == sorted(names)


def test_frozen_ranges_and_padding_are_untouched(stepped):
    u = stepped["u"]
    moved = torch.zeros(u.flat_numel, dtype=torch.bool, device=DEV)            # where a trainable LOGICAL element lives
    train = {n: p.requires_grad for n, p in u.named_parameters()}
    for n, (o, st, shape) in u._slots.items():
        if not train[n]:
            continue
        v = moved[o:o + math.prod(st)].view(st)
        (v.permute(0, 3, 1, 2)[:, :shape[1]] if len(st) == 4 else v).fill_(True)
    assert bool((~moved).any()) and not all(train.values())
    a, b = u.pflat.view(torch.int16), stepped["pflat0"].view(torch.int16)
    assert torch.equal(a[~moved], b[~moved])
    assert int((a[moved] != b[moved]).sum()) > 0
    assert torch.equal(u.gflat.view(torch.int16), stepped["gflat0"].view(torch.int16))          # gradients are read, never written


def test_the_next_forward_refreshes_the_transposed_mirror(stepped):
    u = stepped["u"]
    assert u.params._wt_dirty
    u.zero_grad()
    _micro_step(u)
    torch.cuda.synchronize()
    stale = [o for o, r, c in u._wt_jobs if not torch.equal(u.wtflat[o:o + r * c].view(c, r), u.pflat[o:o + r * c].view(r, c).t())]
    stale += [o for o, co, ci in u._wt_conv_jobs
              if not torch.equal(u.wtflat[o:o + co * 9 * ci].view(ci, 9, co), u.pflat[o:o + co * 9 * ci].view(co, 9, ci).permute(2, 1, 0))]
    assert u._wt_jobs and not stale


def test_a_state_of_another_freeze_mask_is_refused(stepped):
    from test_master_optim_gpu import make_unet
    from aozora_sdxl_training_amd.optimizers import Adafactor
    saved = stepped["opt"].save_cpu_state()
    other = make_unet(exclude=("conv1",))
    opt = Adafactor([p for p in other.parameters() if p.requires_grad], **OPT)
    with pytest.raises(ValueError, match="freeze mask"):
        opt.load_cpu_state(saved)
    same = make_unet()
    opt2 = Adafactor([p for p in same.parameters() if p.requires_grad], **OPT)
    opt2.load_cpu_state(saved)
    assert opt2.optimizer_step == 1
    with pytest.raises(ValueError, match="beta1"):
        Adafactor([p for p in same.parameters() if p.requires_grad], **{**OPT, "beta1": None}).load_cpu_state(saved)
