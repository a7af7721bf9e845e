"""Parameter groups through the optimizer classes, on the reduced-width UNet: dist.ShardedRaven / ShardedTitan with groups= (ONE launch
per contiguous range, az_adamw_flat_seg) against the per-group launches of the parent commit -- optimizers.RavenAdamW / TitanAdamW given the
equivalent torch param_groups, and, for fp32 master weights (which the drop-in classes do not keep), the ungrouped optimizer with every
ops.adamw_range call cut into one single-group launch per segment.  Parameters and moments bit for bit after 3 steps with the learning
rate changed between steps; the neutral list equals no groups; the number of update launches does not change; the trainer's torch groups
for the 8-bit optimizer equal hand-built ones."""
import gc
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import elem_ref as R                # noqa: E402
import groups_ref as G              # noqa: E402

DEV = "cuda:0"
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, debias_strength=0.3, momentum_dtype=torch.bfloat16)
LRS = (1e-3, 7e-4, 2.5e-4)          # the scheduler's value before each of the three steps
RULES = [{"match": "bias, norm", "weight_decay": 0.0}, {"match": ["down_blocks.0.*", "conv_in"], "lr_scale": 0.25},
         {"match": "mid_block", "lr_scale": 0.0, "weight_decay": 0.0}]
NEUTRAL = [{"match": "bias, norm", "weight_decay": 0.01}, {"match": "conv_in", "lr_scale": 1.0}]
SR = dict(stochastic_rounding=True, sr_seed=42)


@pytest.fixture(autouse=True)
def _collect_cycles():
    """Optimizers and UNets sit in reference cycles that hold device objects: they are collected here, when the test that made them
    ends, not by whichever later test happens to trigger the collector."""
    yield
    gc.collect()


@pytest.fixture(scope="module")
def model():
    """Mini UNet, its initial flat parameters, three synthetic gradients (zero on the channel padding of 4-D weights)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
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
    real = torch.zeros(u.flat_numel, dtype=torch.bfloat16, device=DEV)
    for name, (o, st, shape) in u._slots.items():
        k = int(np.prod(st))
        v = real[o:o + k].view(st)
        (v.permute(0, 3, 1, 2)[:, :shape[1]] if len(st) == 4 else v).fill_(1.0)
    grads = [(torch.randn(u.flat_numel, generator=g) * 1e-2).to(torch.bfloat16).to(DEV) * real for _ in LRS]
    torch.cuda.synchronize()
    return u, u.pflat.clone(), grads


def resolved(u, rules):
    from aozora_sdxl_training_amd import param_groups as PG
    for p in u.parameters():
        p.requires_grad = True
    return PG.resolve_unet(u, PG.parse_rules(rules, HP["weight_decay"]), HP["weight_decay"])


def _reset(u, start):
    u.wait_tail_params()
    torch.cuda.synchronize()
    u.pflat.copy_(start)
    u.mark_params_dirty()
    for p in u.parameters():
        p.requires_grad = True


def flat_moments(opt):
    """(m, v) of a flat optimizer at flat offsets (zero where it owns nothing), plus the master copy when it keeps one."""
    n = opt.unet.flat_numel
    out = [torch.zeros(n, dtype=opt.m_dev.dtype, device=DEV), torch.zeros(n, dtype=opt.m_dev.dtype, device=DEV)]
    w = torch.zeros(n, dtype=torch.float32, device=DEV) if opt.w_dev is not None else None
    for a, b, o in opt._owned():
        out[0][a:b] = opt.m_dev[o:o + (b - a)]
        out[1][a:b] = opt.v_dev[o:o + (b - a)]
        if w is not None:
            w[a:b] = opt.w_dev[o:o + (b - a)]
    return out[0], out[1], w


def sharded(model, titan=False, groups=None, patch=None, **kw):
    """3 steps of dist.ShardedRaven / ShardedTitan -> (pflat, m, v, w) at flat offsets.  patch(opt): called before the first step."""
    from aozora_sdxl_training_amd.dist import ShardedRaven, ShardedTitan
    u, start, grads = model
    _reset(u, start)
    opt = (ShardedTitan if titan else ShardedRaven)(u, clip_grad_norm=0, force_local=True, **HP, **kw, **({} if groups is None else dict(groups=groups)))
    if patch is not None:
        patch(opt)
    for lr, g in zip(LRS, grads):
        opt.param_groups[0]["lr"] = lr                     # what the scheduler writes: the base group, unscaled
        opt.zero_grad()
        u.wait_tail_params(); torch.cuda.synchronize()
        u.gflat.copy_(g)
        if titan:
            opt.accumulate()
        opt.step()
    u.wait_tail_params(); torch.cuda.synchronize()
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["lr"] == LRS[-1]
    return (u.pflat.clone(),) + flat_moments(opt)


def dropin(model, res, titan=False, **kw):
    """3 steps of optimizers.RavenAdamW / TitanAdamW with the equivalent torch param_groups: the parent's launches, one per stretch of
    parameters whose hyper-parameters agree."""
    from aozora_sdxl_training_amd.optimizers import RavenAdamW, TitanAdamW
    u, start, grads = model
    _reset(u, start)
    members = [[] for _ in res.groups]
    for name, p in u.named_parameters():
        members[res.param_gid[name]].append(p)
    tg = [{"params": ps, "lr_scale": s, "weight_decay": wd} for ps, (s, wd) in zip(members, res.groups) if ps]
    opt = (TitanAdamW if titan else RavenAdamW)(tg, **HP, **({} if titan else dict(state_on_device=True)), **kw)
    try:
        for lr, g in zip(LRS, grads):
            for grp in opt.param_groups:
                grp["lr"] = lr * grp.get("lr_scale", 1.0)              # schedule.CustomCurveLRScheduler._update_lr
            opt.zero_grad(set_to_none=True)
            u.gflat.copy_(g)
            if titan:
                opt.offload_flat(u)
            else:
                u.expose_grads()
            opt.step()
        torch.cuda.synchronize()
        hs = opt._host[u]
        return u.pflat.clone(), hs.m.to(DEV).clone(), hs.v.to(DEV).clone()
    finally:
        if titan:
            opt.close()


def per_segment_launches(res):
    """patch for sharded(): every ops.adamw_range call of an UNGROUPED optimizer becomes one single-group call per segment, with that
    group's hyper vector formed as the optimizer forms its own (elem_ref.adamw_hyper)."""
    from aozora_sdxl_training_amd import dist as D

    def patch(opt):
        real = D.ops.adamw_range
        base = opt.unet.pflat.data_ptr()
        keep = []

        def hyper_vectors():
            g0 = opt.param_groups[0]
            rows = [R.adamw_hyper(lr=g0["lr"] * s, betas=g0["betas"], wd=wd, eps=g0["eps"], debias=g0["debias_strength"], step=opt.step_count)
                    for s, wd in res.groups]
            keep.append(torch.from_numpy(np.stack(rows)).to(DEV))
            return keep[-1]

        def split(n, p, g, gdtype, m, v, mdtype, hyper, coef, stream, *, master=None, sr=None, host_pipeline=None, groups=None):
            assert groups is None and host_pipeline is None
            hs, a0 = hyper_vectors(), (p - base) // 2
            gsz, esz = (2, 4)[gdtype], torch.empty(0, dtype=mdtype).element_size()
            for a, b, s in G.segments_in(res.seg_end, a0, n):
                real(b - a, p + 2 * a, g + gsz * a, gdtype, m + esz * a, v + esz * a, mdtype, hs[res.seg_gid[s]].data_ptr(), coef, stream,
                     master=None if master is None else master + 4 * a, sr=None if sr is None else (sr[0], sr[1], sr[2], sr[3] + a))
        opt._restore = lambda: setattr(D.ops, "adamw_range", real)
        D.ops.adamw_range = split
    return patch


def equal(a, b, what):
    for x, y, nm in zip(a, b, ("p", "m", "v", "w")):
        if x is None or y is None:
            continue
        assert x.dtype == y.dtype and torch.equal(x, y), f"{nm} differs: {what} ({int((x != y).sum())} elements)"


@pytest.fixture(scope="module")
def plain_runs(model):
    u = model[0]
    res = resolved(u, RULES)
    assert len(res.groups) == 4 and len(res.seg_end) > 20
    return res, sharded(model, regions=1), sharded(model, regions=1, groups=res)


def test_raven_with_groups_equals_the_dropin_per_group_launches(model, plain_runs):
    res, off, on = plain_runs
    equal(on, dropin(model, res), "ShardedRaven(groups) against RavenAdamW(param_groups)")
    equal(on, sharded(model, regions=3, groups=res), "three regions against one")
    assert not torch.equal(on[0], off[0])                                   # the option selects results
    u, start, _ = model
    frozen = torch.zeros(u.flat_numel, dtype=torch.bool, device=DEV)
    for n in res.param_gid:
        if "mid_block" in n and not ("bias" in n or "norm" in n):
            o, st, _ = u._slots[n]
            frozen[o:o + int(np.prod(st))] = True
    assert bool(frozen.any()) and torch.equal(on[0][frozen], start[frozen])          # lr_scale 0, weight_decay 0: bit-unchanged
    assert not torch.equal(off[0][frozen], start[frozen])


def test_raven_with_groups_and_stochastic_rounding(model, plain_runs):
    res = plain_runs[0]
    on = sharded(model, regions=1, groups=res, **SR)
    equal(on, dropin(model, res, **SR), "stochastic rounding: ShardedRaven(groups) against RavenAdamW(param_groups)")
    equal(on, sharded(model, regions=3, groups=res, **SR), "stochastic rounding: three regions against one")
    assert not torch.equal(on[0], plain_runs[2][0])


@pytest.mark.parametrize("titan", [False, True])
def test_master_weights_with_groups_equal_one_launch_per_segment(model, plain_runs, titan):
    res = plain_runs[0]
    on = sharded(model, titan=titan, regions=1, groups=res, master_weights=True)
    from aozora_sdxl_training_amd import dist as D
    real = D.ops.adamw_range
    try:
        cut = sharded(model, titan=titan, regions=1, master_weights=True, patch=per_segment_launches(res))
    finally:
        D.ops.adamw_range = real
    assert on[3] is not None
    equal(on, cut, "master weights: one segmented launch against one launch per segment")
    assert torch.equal(on[3].bfloat16()[on[3] != 0], on[0][on[3] != 0])


def test_titan_with_groups_equals_the_dropin_per_group_launches(model, plain_runs):
    res = plain_runs[0]
    on = sharded(model, titan=True, groups=res)
    equal(on, dropin(model, res, titan=True), "ShardedTitan(groups) against TitanAdamW(param_groups)")
    equal(sharded(model, titan=True, groups=res, **SR), dropin(model, res, titan=True, **SR), "Titan, stochastic rounding")


def test_neutral_groups_equal_no_groups(model, plain_runs):
    u = model[0]
    res = resolved(u, NEUTRAL)
    assert res.groups == [(1.0, 0.01)] and res.seg_gid == [0]
    equal(sharded(model, regions=1, groups=res), plain_runs[1], "neutral list against no groups")
    equal(sharded(model, regions=1, groups=res, **SR), sharded(model, regions=1, **SR), "neutral list against no groups, stochastic rounding")
    equal(sharded(model, regions=1, groups=res, master_weights=True), sharded(model, regions=1, master_weights=True), "neutral, master weights")


def test_the_number_of_update_launches_does_not_change(model, plain_runs):
    """Counted at ops.adamw_range, the one caller of the az_adamw_flat* entry points; without groups the keyword is not passed at all."""
    from aozora_sdxl_training_amd import dist as D
    res = plain_runs[0]
    real = D.ops.adamw_range
    calls = []

    def counting(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)
    counts = {}
    try:
        D.ops.adamw_range = counting
        for tag, kw in (("off", {}), ("on", dict(groups=res))):
            for regions in (1, 3):
                calls.clear()
                sharded(model, regions=regions, **kw)
                counts[tag, regions] = len(calls)
                assert all(("groups" in c) == (tag == "on") for c in calls)
    finally:
        D.ops.adamw_range = real
    assert counts["on", 1] == counts["off", 1] == len(LRS) * 1 and counts["on", 3] == counts["off", 3] and counts["on", 3] >= counts["on", 1]


def test_refusals_of_the_constructor(model):
    from aozora_sdxl_training_amd.dist import ShardedRaven
    from aozora_sdxl_training_amd._lib import AozoraError
    u = model[0]
    res = resolved(u, RULES)
    with pytest.raises(ValueError, match="pinned-host"):
        ShardedRaven(u, force_local=True, state_on_host=True, groups=res, **HP)
    with pytest.raises(ValueError, match="base group"):
        ShardedRaven(u, force_local=True, groups=res, **{**HP, "weight_decay": 0.02})
    with pytest.raises(AozoraError):
        ShardedRaven(u, force_local=True, groups=res._replace(seg_end=res.seg_end[:-1] + [res.seg_end[-2]]), **HP)


def test_8bit_trainer_groups_equal_hand_built_groups(model):
    from aozora_sdxl_training_amd.optimizers import PagedAdamW8bit
    from aozora_sdxl_training_amd.trainer import _optimizer_8bit
    u, start, grads = model
    res = resolved(u, RULES)
    hp8 = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    cfg = types.SimpleNamespace(LR_CUSTOM_CURVE=[], LEARNING_RATE=1e-3, PAGED_ADAMW_8BIT_PARAMS=dict(hp8, param_groups=RULES))

    def run(make):
        _reset(u, start)
        opt = make([p for p in u.parameters()])
        for lr, g in zip(LRS, grads):
            for grp in opt.param_groups:
                grp["lr"] = lr * grp.get("lr_scale", 1.0)
            opt.zero_grad(set_to_none=True)
            u.gflat.copy_(g)
            u.expose_grads()
            opt.step()
        torch.cuda.synchronize()
        return opt, u.pflat.clone()

    def by_hand(params):
        name = {id(p): n for n, p in u.named_parameters()}
        sets = {"nodecay": [], "slow": [], "frozen": [], "base": []}
        for p in params:
            n = name[id(p)]
            key = ("nodecay" if ("bias" in n or "norm" in n) else "slow" if (n.startswith("down_blocks.0.") or "conv_in" in n) else
                   "frozen" if "mid_block" in n else "base")
            sets[key].append(p)
        return PagedAdamW8bit([{"params": sets["nodecay"], "lr_scale": 1.0, "weight_decay": 0.0}, {"params": sets["slow"], "lr_scale": 0.25},
                               {"params": sets["frozen"], "lr_scale": 0.0, "weight_decay": 0.0}, {"params": sets["base"], "lr_scale": 1.0}],
                              lr=1e-3, min_8bit_size=4096, **hp8)

    opt_t, p_t = run(lambda ps: _optimizer_8bit(cfg, ps, res))
    opt_h, p_h = run(by_hand)
    assert [(len(g["params"]), g["lr_scale"], g["weight_decay"]) for g in opt_t.param_groups] == \
           [(len(g["params"]), g["lr_scale"], g["weight_decay"]) for g in opt_h.param_groups]
    assert opt_t.param_groups[-1]["lr_scale"] == 1.0 and opt_t.param_groups[-1]["lr"] == LRS[-1]        # the base group last: the reported lr
    assert torch.equal(p_t, p_h)
    _, p_off = run(lambda ps: _optimizer_8bit(types.SimpleNamespace(LR_CUSTOM_CURVE=[], LEARNING_RATE=1e-3, PAGED_ADAMW_8BIT_PARAMS=hp8), ps))
    assert not torch.equal(p_t, p_off)
