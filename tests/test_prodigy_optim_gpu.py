"""optimizers.Prodigy on a mini UNet with conv1 / conv2 frozen (several flat ranges) and synthetic gradients that are zero on the channel
padding, as in test_master_optim_gpu.py: frozen ranges and padding never move, pflat stays bf16(master), the state round-trips bit for bit
and refuses another freeze mask, resync_master() picks up parameters written from outside; and on plain tensors the toy problem of the
contract's motivation finds its step size on the device."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = "cuda:0"
STEPS = 3
HP = dict(lr=1.0, d0=1e-5, weight_decay=0.01, use_bias_correction=True)
TENSORS = ("w", "p0", "m", "v", "s")


@pytest.fixture(scope="module")
def model():
    """Mini UNet with conv1 / conv2 frozen, its initial flat parameters, the mask of real (non-padding) elements and three synthetic
    gradients of scale 1e-2 that are zero on the channel padding of 4-D weights, as a backward leaves it."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_master_optim_gpu import make_unet
    u = make_unet()
    g = torch.Generator().manual_seed(5)
    real = torch.zeros(u.flat_numel, dtype=torch.bfloat16, device=DEV)
    for name, (o, st, shape) in u._slots.items():
        k = 1
        for d in st:
            k *= d
        v = real[o:o + k].view(st)
        (v.permute(0, 3, 1, 2)[:, :shape[1]] if len(st) == 4 else v).fill_(1.0)
    grads = [(torch.randn(u.flat_numel, generator=g) * 1e-2).to(torch.bfloat16).to(DEV) * real for _ in range(STEPS)]
    torch.cuda.synchronize()
    return u, u.pflat.clone(), grads, real.bool()


def fresh(model):
    from aozora_sdxl_training_amd.optimizers import Prodigy
    u, start, _, _ = model
    torch.cuda.synchronize()
    u.pflat.copy_(start)
    u.mark_params_dirty()
    return Prodigy([p for p in u.parameters() if p.requires_grad], **HP)


def advance(model, opt, which):
    u, _, grads, _ = model
    for i in which:
        opt.zero_grad()
        u.gflat.copy_(grads[i])
        opt.step()
    torch.cuda.synchronize()


def scattered(opt, k="w"):
    """State tensor k scattered to flat offsets (NaN where the optimizer owns nothing)."""
    out = torch.full((opt.owner.flat_numel,), float("nan"), dtype=torch.float32, device=DEV)
    for (_, a, b), o in zip(opt.ranges, opt.range_off):
        out[a:b] = getattr(opt, k + "_dev")[o:o + (b - a)]
    return out


@pytest.fixture(scope="module")
def three(model):
    opt = fresh(model)
    advance(model, opt, range(STEPS))
    return dict(opt=opt, pflat=model[0].pflat.clone(), state={k: scattered(opt, k) for k in TENSORS}, scalars=opt.scalars())


def test_ranges_follow_the_freeze_mask(model, three):
    u, opt = model[0], three["opt"]
    assert [(a, b) for _, a, b in opt.ranges] == list(u.trainable_ranges()) and len(opt.ranges) > 1
    assert all(o % 64 == 0 for o in opt.range_off)
    n = sum(b - a for a, b in u.trainable_ranges())
    assert opt.state_bytes == 20 * n and n < u.flat_numel                 # frozen parameters own no state
    assert three["scalars"]["k"] == float(STEPS) and three["scalars"]["d"] >= HP["d0"]


def test_frozen_ranges_and_padding_never_move_and_pflat_is_the_bf16_image_of_the_master(model, three):
    u, start, _, real = model
    own = ~three["state"]["w"].isnan()
    assert torch.equal(own, ~three["state"]["p0"].isnan()) and 0 < int(own.sum()) < u.flat_numel
    last, w = three["pflat"], three["state"]["w"]
    assert torch.equal(last[~own], start[~own])                           # frozen: untouched
    pad = own & ~real
    assert int(pad.sum()) > 0 and torch.equal(last[pad], start[pad]) and torch.equal(w[pad], start[pad].float())
    assert torch.equal(w[own].bfloat16(), last[own])                      # round to nearest even
    assert not torch.equal(w[own], last[own].float())                     # ... of a master that holds more than bf16
    moved = own & real
    assert int((last[moved] != start[moved]).sum()) > 0
    assert torch.equal(three["state"]["p0"][own], start[own].float())


def test_save_and_load_after_step_two_equals_three_uninterrupted_steps(model, three):
    from aozora_sdxl_training_amd.optimizers import Prodigy
    from aozora_sdxl_training_amd.optimizers.prodigy import STATE_VERSION
    u = model[0]
    a = fresh(model)
    advance(model, a, range(2))
    st, p2 = a.save_cpu_state(), u.pflat.clone()
    n = sum(b - x for _, x, b in a.ranges)
    assert st["version"] == STATE_VERSION and set(st) == {"version", "options", "scalars", "ranges", *TENSORS}
    assert set(st["scalars"]) == {"d", "d_max", "d_numerator", "d_denom", "d_hat", "k", "d0"} and all(isinstance(v, float) for v in st["scalars"].values())
    assert st["ranges"] == [tuple(r) for r in a.ranges] and st["options"]["weight_decay"] == 0.01
    assert all(st[k].dtype == torch.float32 and not st[k].is_cuda and st[k].numel() == n for k in TENSORS)
    b = fresh(model)
    u.pflat.copy_(p2)
    u.mark_params_dirty()
    b.load_cpu_state(st)
    advance(model, b, [2])
    assert torch.equal(u.pflat, three["pflat"])
    for k in TENSORS:
        assert torch.equal(scattered(b, k).view(torch.int32), three["state"][k].view(torch.int32)), k
    assert b.scalars() == three["scalars"]
    assert b.d_value() == three["scalars"]["d"]


def test_another_freeze_mask_and_a_foreign_state_are_refused(model):
    from test_master_optim_gpu import make_unet
    from aozora_sdxl_training_amd.optimizers import Prodigy
    a = fresh(model)
    advance(model, a, [0])
    st = a.save_cpu_state()
    other = make_unet(exclude=("conv1",))
    c = Prodigy([p for p in other.parameters() if p.requires_grad], **HP)
    assert c.ranges != a.ranges
    with pytest.raises(ValueError, match="freeze mask"):
        c.load_cpu_state(st)
    with pytest.raises(ValueError, match="version tag"):
        a.load_cpu_state({"_momentum_dtype": torch.bfloat16})
    with pytest.raises(ValueError, match="fp32 tensor"):
        a.load_cpu_state({**st, "m": st["m"][:-8]})


def test_resync_master_takes_parameters_written_from_outside(model):
    u, start, _, _ = model
    opt = fresh(model)
    advance(model, opt, range(2))
    own = ~scattered(opt).isnan()
    assert not torch.equal(scattered(opt)[own], start[own].float())
    u.pflat.copy_(start)                       # as unet.load_state_dict / ema.copy_to would
    u.mark_params_dirty()
    opt.resync_master()
    assert torch.equal(scattered(opt)[own].view(torch.int32), start[own].float().view(torch.int32))
    assert torch.equal(scattered(opt, "p0")[own], start[own].float())


def test_constructor_refusals(model):
    from aozora_sdxl_training_amd._lib import AozoraError
    from aozora_sdxl_training_amd.optimizers import Prodigy
    u = model[0]
    ps = [p for p in u.parameters() if p.requires_grad]
    with pytest.raises(AozoraError, match="one param group"):
        Prodigy([{"params": ps[:2]}, {"params": ps[2:4]}])
    with pytest.raises(AozoraError, match="contiguous bf16 device tensors"):
        Prodigy([torch.zeros(8, device=DEV, requires_grad=True)])
    with pytest.raises(AozoraError, match="contiguous bf16 device tensors"):
        Prodigy([torch.zeros(8, dtype=torch.bfloat16, requires_grad=True)])          # a CPU tensor: there is no CPU fallback
    for kw, match in ((dict(eps=0.0), "eps must be > 0"), (dict(d0=0.0), "d0 must be > 0"), (dict(betas=(0.9, 1.0)), "betas must lie")):
        with pytest.raises(ValueError, match=match):
            Prodigy(ps, **kw)


@pytest.fixture(scope="module")
def toy():
    """The toy problem through the class on one plain bf16 tensor, with bf16 and with fp32 gradients of the same values."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_prodigy_ref_cpu import toy_parameters, toy_problem
    from aozora_sdxl_training_amd.optimizers import Prodigy
    out = {}
    for tag, gdt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        p = toy_parameters().to(DEV).requires_grad_(True)
        if gdt != p.dtype and hasattr(p, "grad_dtype"):
            p.grad_dtype = gdt                     # (torch checks a gradient's dtype against this attribute where it has one)
        opt = Prodigy([p])

        def step(gr):
            p.grad = gr.to(gdt).to(DEV)
            opt.step()
            return opt.w_dev[:p.numel()].cpu()

        first, last = toy_problem(step, toy_parameters())
        out[tag] = dict(first=first, last=last, sc=opt.scalars(), p=p.detach().cpu(), w=opt.w_dev[:p.numel()].cpu())
    return out


def test_toy_problem_finds_its_step_size_on_the_device(toy):
    t = toy["bf16"]
    print(f"toy problem on the device: d / d0 = {t['sc']['d'] / t['sc']['d0']:.3e}, loss ratio = {t['last'] / t['first']:.3e}")
    assert t["sc"]["d0"] == 1e-6 and t["sc"]["k"] == 80.0
    assert t["sc"]["d"] >= 1e3 * t["sc"]["d0"]
    assert t["last"] <= 1e-2 * t["first"]
    assert torch.equal(t["p"], t["w"].bfloat16())


def test_fp32_gradients_of_the_same_values_give_the_same_bits(toy):
    a, b = toy["bf16"], toy["fp32"]
    assert torch.equal(a["w"].view(torch.int32), b["w"].view(torch.int32)) and a["sc"] == b["sc"]


def test_lr_zero_launches_nothing_and_a_missing_gradient_is_refused():
    from aozora_sdxl_training_amd._lib import AozoraError, lib
    from aozora_sdxl_training_amd.optimizers import Prodigy
    p = torch.ones(100, dtype=torch.bfloat16, device=DEV).requires_grad_(True)
    opt = Prodigy([p], lr=0.0)
    p.grad = torch.ones_like(p)
    L = lib()
    L.recorder = []
    try:
        opt.step()
        assert L.recorder == [] and opt.w_dev is None
        opt.param_groups[0]["lr"] = 1.0
        opt.step()
        assert [c.name for c in L.recorder] == ["az_prodigy_begin", "az_prodigy_moments", "az_prodigy_finish", "az_prodigy_apply"]      # 2 R + 2, R = 1
    finally:
        L.recorder = None
    torch.cuda.synchronize()
    assert opt.scalars()["k"] == 1.0 and bool((opt.w_dev[:100] < 1.0).all())      # (the first update, 3e-6, is below a bf16 ulp of p)
    opt.zero_grad()
    with pytest.raises(AozoraError, match="needs a gradient"):
        opt.step()
