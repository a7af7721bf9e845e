"""master_weights=True through dist.ShardedRaven (one region; three regions with the overlapped and the plain schedule) and
dist.ShardedTitan on a mini UNet with a freeze mask: the first step is the default's bit for bit, pflat stays bf16(master), the region
layouts agree bit for bit, frozen ranges own no master memory and never move, the state round-trips and refuses another freeze mask,
resync_master() picks up parameters written from outside."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, debias_strength=0.3, momentum_dtype=torch.bfloat16)
STEPS = 3


def make_unet(exclude=("conv1", "conv2")):
    from aozora_sdxl_training_amd.schedule import trainable_mask
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import mini_config
    u = AozoraUNet(mini_config(), DEV)
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for n, p in u.named_parameters():
            if "norm" in n:
                p.fill_(1.0 if n.endswith("weight") else 0.0)
            else:
                p.copy_((torch.randn(p.shape, generator=g) * 0.05).bfloat16())
    names = [n for n, _ in u.named_parameters()]
    for (n, p), m in zip(u.named_parameters(), trainable_mask(names, list(exclude))):
        p.requires_grad = m
    assert any(not p.requires_grad for p in u.parameters()) and any(p.requires_grad for p in u.parameters())
    return u


@pytest.fixture(scope="module")
def model():
    """Mini UNet with conv1 / conv2 frozen, its initial flat parameters and three synthetic gradients of scale 1e-2 (zero on the channel
    padding of 4-D weights, as a backward leaves it: the reference's per-parameter state layout of save_cpu_state has no room for it)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
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
    return u, u.pflat.clone(), grads


def settle(u):
    u.wait_tail_params()
    torch.cuda.synchronize()


def master_flat(opt):
    """The master copy scattered to flat offsets through ranges / range_off (NaN where this optimizer owns nothing)."""
    out = torch.full((opt.unet.flat_numel,), float("nan"), dtype=torch.float32, device=DEV)
    for rs, offs in zip(opt.ranges, opt.range_off):
        for (a, b), o in zip(rs, offs):
            out[a:b] = opt.w_dev[o:o + (b - a)]
    return out


def run(model, titan=False, steps=STEPS, **kw):
    """-> (optimizer, pflat after step 1, pflat after `steps`).  clip_grad_norm = 0: the clip coefficient is exactly 1 (the sum of squares
    is accumulated range by range, so its last bit may depend on where the regions cut the ranges; the kernel test covers a coefficient)."""
    from aozora_sdxl_training_amd.dist import ShardedRaven, ShardedTitan
    u, start, grads = model
    settle(u)
    u.pflat.copy_(start)
    u.mark_params_dirty()
    opt = (ShardedTitan if titan else ShardedRaven)(u, clip_grad_norm=0, force_local=True, **HP, **kw)
    first = None
    for g in grads[:steps]:
        opt.zero_grad()
        settle(u)                                       # the clear may run on the background stream
        u.gflat.copy_(g)
        if titan:
            opt.accumulate()
        opt.step()
        if first is None:
            settle(u)
            first = u.pflat.clone()
    settle(u)
    assert opt.step_count == steps
    return opt, first, u.pflat.clone()


def owned_mask(opt):
    m = torch.zeros(opt.unet.flat_numel, dtype=torch.bool, device=DEV)
    for rs in opt.ranges:
        for a, b in rs:
            m[a:b] = True
    return m


@pytest.fixture(scope="module")
def runs(model):
    r = {}
    for tag, kw in (("off", dict(regions=1)), ("m1", dict(regions=1, master_weights=True)),
                    ("m3_overlap", dict(regions=3, overlap=True, master_weights=True)), ("m3_plain", dict(regions=3, overlap=False, master_weights=True)),
                    ("titan_off", dict(titan=True)), ("titan_m", dict(titan=True, master_weights=True))):
        opt, first, last = run(model, **kw)
        r[tag] = dict(opt=opt, first=first, last=last, w=master_flat(opt) if opt.w_dev is not None else None)
    assert r["m3_overlap"]["opt"].update_overlap and len(r["m3_overlap"]["opt"].regions) == 3
    assert not r["m3_plain"]["opt"].update_overlap and len(r["m3_plain"]["opt"].regions) == 3 and len(r["m1"]["opt"].regions) == 1
    return r


@pytest.mark.parametrize("on,off", [("m1", "off"), ("m3_overlap", "off"), ("m3_plain", "off"), ("titan_m", "titan_off")])
def test_first_step_is_the_default_and_later_steps_are_not(runs, on, off):
    assert torch.equal(runs[on]["first"], runs[off]["first"]), "the first step must be the default's bit for bit"
    differ = int((runs[on]["last"] != runs[off]["last"]).sum())
    assert differ > 0, "after three steps the master must have kept something the bf16 write-back discards"


@pytest.mark.parametrize("tag", ["m1", "m3_overlap", "m3_plain", "titan_m"])
def test_pflat_is_the_bf16_image_of_the_master_and_frozen_ranges_never_move(model, runs, tag):
    u, start, _ = model
    r = runs[tag]
    opt, own = r["opt"], owned_mask(r["opt"])
    assert opt.w_dev.dtype == torch.float32 and opt.w_dev.numel() == opt.shard == sum(b - a for a, b in u.trainable_ranges())
    assert opt.shard < u.flat_numel                                                    # frozen parameters own no master memory
    assert not bool(r["w"][own].isnan().any()) and bool(r["w"][~own].isnan().all())
    assert torch.equal(r["w"][own].bfloat16(), r["last"][own])                         # round to nearest even
    assert not torch.equal(r["w"][own], r["last"][own].float())                        # ... of a master that holds more than bf16
    assert torch.equal(r["last"][~own], start[~own])                                   # frozen: untouched


def test_region_layouts_agree_bit_for_bit(runs):
    for other in ("m3_overlap", "m3_plain"):
        assert torch.equal(runs["m1"]["last"], runs[other]["last"]), other
        assert torch.equal(runs["m1"]["w"].view(torch.int32), runs[other]["w"].view(torch.int32)), other


def test_flag_off_keeps_no_master_and_the_combination_with_stochastic_rounding_raises(model, runs):
    from aozora_sdxl_training_amd.dist import ShardedRaven, ShardedTitan
    assert runs["off"]["opt"].w_dev is None and runs["titan_off"]["opt"].w_dev is None
    opt, _, last = run(model, regions=1, master_weights=False)
    assert opt.w_dev is None and torch.equal(last, runs["off"]["last"])
    for fn in (opt.resync_master, opt.save_master_state, lambda: opt.load_master_state({})):
        with pytest.raises(ValueError, match="no fp32 master weights"):
            fn()
    u = model[0]
    for cls in (ShardedRaven, ShardedTitan):
        with pytest.raises(ValueError, match="do not combine"):
            cls(u, force_local=True, master_weights=True, stochastic_rounding=True, **HP)


def test_state_round_trips_and_refuses_another_layout(model, runs):
    """Two steps, save, a fresh optimizer loads master and moments, third step: bitwise the uninterrupted run."""
    u, start, grads = model
    a, _, _ = run(model, steps=2, regions=3, master_weights=True)
    st, cpu, p2 = a.save_master_state(), a.save_cpu_state(), u.pflat.clone()
    assert set(st) == {"world", "rank", "ranges", "master"} and (st["world"], st["rank"]) == (1, 0)
    assert st["master"].dtype == torch.float32 and not st["master"].is_cuda and st["master"].numel() == a.shard
    assert st["ranges"] == [list(map(tuple, rs)) for rs in a.ranges]
    from aozora_sdxl_training_amd.dist import ShardedRaven
    settle(u)
    u.pflat.copy_(p2)
    u.mark_params_dirty()
    b = ShardedRaven(u, clip_grad_norm=0, force_local=True, regions=3, master_weights=True, **HP)
    assert torch.equal(b.w_dev, master_flat(b)[owned_mask(b)]) and torch.equal(master_flat(b)[owned_mask(b)], p2[owned_mask(b)].float())
    b.load_cpu_state(cpu)
    b.load_master_state(st)
    assert torch.equal(b.w_dev.cpu().view(torch.int32), st["master"].view(torch.int32))
    b.zero_grad(); settle(u)
    u.gflat.copy_(grads[2])
    b.step(); settle(u)
    assert torch.equal(u.pflat, runs["m1"]["last"])
    assert torch.equal(master_flat(b).view(torch.int32), runs["m1"]["w"].view(torch.int32))
    # refusals: another region layout, world size, rank, element count -- each names the mismatch
    one = ShardedRaven(u, force_local=True, regions=1, master_weights=True, **HP)
    with pytest.raises(ValueError, match="region"):
        one.load_master_state(st)
    with pytest.raises(ValueError, match="world"):
        b.load_master_state({**st, "world": 2})
    with pytest.raises(ValueError, match="rank"):
        b.load_master_state({**st, "rank": 1})
    with pytest.raises(ValueError, match="elements"):
        b.load_master_state({**st, "master": st["master"][:-8]})
    # ... and a changed freeze mask
    other = make_unet(exclude=("conv1",))
    c = ShardedRaven(other, force_local=True, regions=3, master_weights=True, **HP)
    assert c.shard != a.shard
    with pytest.raises(ValueError, match="freeze mask"):
        c.load_master_state(st)


def test_resync_master_takes_parameters_written_from_outside(model):
    u, start, grads = model
    opt, _, last = run(model, steps=2, regions=3, master_weights=True)
    own = owned_mask(opt)
    assert not torch.equal(master_flat(opt)[own], u.pflat[own].float())
    u.pflat.copy_(start)                       # as unet.load_state_dict / ema.copy_to would
    u.mark_params_dirty()
    opt.resync_master()
    assert torch.equal(master_flat(opt)[own].view(torch.int32), start[own].float().view(torch.int32))
    assert torch.equal(opt.w_dev, master_flat(opt)[own])
