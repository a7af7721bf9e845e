"""ema.EmaWeights on a mini UNet with a freeze mask, driven by the optimizers themselves: random gradients in gflat (no forward
needed), three optimizer steps, and after each step the EMA must equal -- bit for bit -- tests/ema_ref.py replayed over snapshots of
the parameters.  ShardedRaven runs its default overlapped update here (regions 1 and 2 on the parameter-gradient stream): an EMA
launch that ran ahead of the update it follows would read the old parameters and fail (a)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ema_ref as E        # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DECAY, STEPS, LR = 0.9, 3, 1e-3           # warm-up: d_k = 2/11, 3/12, 4/13 -- three different omd


def make_unet(exclude=("conv1", "conv2")):
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import mini_config
    from aozora_sdxl_training_amd.schedule import trainable_mask
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
def grads():
    """One random bf16 gradient buffer per step, shared by every test (host copies, never modified)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = make_unet().flat_numel
    g = torch.Generator().manual_seed(5)
    return [(torch.randn(n, generator=g) * 1e-3).bfloat16() for _ in range(STEPS)]


def snapshot(u):
    return {n: t.detach().clone().cpu() for n, t in u.state_dict().items()}


def same(got, want, what):
    got = got.detach().cpu().contiguous().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    ok = (got.view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} elements differ"


def run(kind, grads, with_ema=True):
    """-> (unet, ema, snapshots [initial, after step 1, ...], EMA state dicts after each step)."""
    from aozora_sdxl_training_amd.dist import ShardedRaven, ShardedTitan
    from aozora_sdxl_training_amd.ema import EmaWeights
    from aozora_sdxl_training_amd.optimizers import RavenAdamW
    u = make_unet()
    spec = dict(decay=DECAY) if with_ema else None
    if kind == "raven":
        opt = ShardedRaven(u, lr=LR, clip_grad_norm=1.0, force_local=True, ema=spec)
        assert opt.update_overlap and len(opt.regions) == 3
        ema = opt.ema
    elif kind == "titan":                                              # an EmaWeights of the caller's: whole trainable ranges, cut by the regions
        opt = ShardedTitan(u, lr=LR, clip_grad_norm=1.0, force_local=True, ema=EmaWeights(u, DECAY) if with_ema else None)
        ema = opt.ema
        assert ema is None or ema.ranges == [tuple(r) for r in u.trainable_ranges()]
    else:
        opt = RavenAdamW([{"params": [p for p in u.parameters() if p.requires_grad], "lr_scale": 1.0}], lr=LR, betas=(0.9, 0.999),
                         weight_decay=0.01, debias_strength=0.3)
        ema = EmaWeights(u, DECAY) if with_ema else None
    if with_ema:
        assert ema.numel == sum(b - a for a, b in u.trainable_ranges()) and ema.nbytes == 4 * ema.numel and ema.k == 0
    snaps, emas = [snapshot(u)], []
    for s in range(STEPS):
        u.gflat.copy_(grads[s].to(DEV))
        if kind == "titan":
            opt.accumulate()
        if kind == "module":
            u.expose_grads()
            opt.step()
            if ema is not None:
                ema.update()
        else:
            opt.step()
            opt.synchronize_params()
        snaps.append(snapshot(u))
        if ema is not None:
            emas.append({n: t.clone() for n, t in ema.state_dict().items()})
            assert ema.k == s + 1
    torch.cuda.synchronize()
    return u, ema, snaps, emas


@pytest.mark.parametrize("kind", ["raven", "titan", "module"])
def test_ema_follows_the_parameters_bit_for_bit(grads, kind):
    """(a), (b), (c), (e): ShardedRaven (overlapped update), ShardedTitan, RavenAdamW + ema.update()."""
    u, ema, snaps, emas = run(kind, grads)
    want = E.replay(snaps, DECAY, True)
    trainable = {n for n, p in u.named_parameters() if p.requires_grad}
    moved = 0
    for s in range(STEPS):
        assert list(emas[s]) == [n for n, _ in u.named_parameters()]
        for n, t in emas[s].items():
            assert tuple(t.shape) == tuple(snaps[0][n].shape)
            if n in trainable:
                same(t, want[s][n], f"{kind} step {s + 1} {n}")
                if "norm" not in n:                                    # (norm weights sit at 1.0, where a step of LR is below half a bf16 ulp)
                    assert not torch.equal(snaps[s + 1][n], snaps[s][n]), f"{kind} step {s + 1}: {n} did not move"
                    moved += 1
            else:                                                       # (c) frozen: float32(p), exactly, and p never moved
                assert torch.equal(snaps[s + 1][n], snaps[0][n])
                same(t, E.torch_bf16_to_f32(snaps[0][n]), f"{kind} frozen {n}")
    assert moved >= STEPS                                               # the optimizer really moved what the EMA follows
    # the EMA is not the parameters: it lags them
    assert any(not np.array_equal(emas[-1][n].cpu().numpy(), E.torch_bf16_to_f32(snaps[-1][n])) for n in trainable)
    # (e) copy_to: every parameter becomes bf16(ema), round to nearest even
    final = {n: t.clone() for n, t in ema.state_dict().items()}
    ema.copy_to(u)
    assert u.params._wt_dirty
    for n, p in u.state_dict().items():
        assert torch.equal(p.detach(), final[n].bfloat16()), n
    with pytest.raises(ValueError):                                     # a range must lie inside a tracked one (refused before any launch)
        ema.update_range(u.trainable_ranges()[0][0], u.flat_numel + 64, torch.cuda.current_stream())


@pytest.mark.parametrize("kind", ["raven", "titan"])
def test_ema_only_reads_the_parameters(grads, kind):
    """(d): pflat after three steps is bit-identical with and without an EMA attached."""
    u1, _, _, _ = run(kind, grads, with_ema=True)
    u0, ema0, _, _ = run(kind, grads, with_ema=False)
    assert ema0 is None
    assert torch.equal(u1.pflat, u0.pflat)


def test_state_round_trip_and_mismatches(grads):
    """save_state -> a fresh object -> load_state continues bit for bit; (f) a state taken under another freeze mask is refused."""
    from aozora_sdxl_training_amd.ema import EmaWeights
    u = make_unet()
    ema = EmaWeights(u, DECAY)
    ema.update()
    st = ema.save_state()
    assert set(st) == {"k", "decay", "warmup", "world", "rank", "ranges", "ema"}
    assert st["k"] == 1 and st["world"] == 1 and st["rank"] == 0 and st["ema"].dtype == torch.float32 and st["ema"].device.type == "cpu"
    assert st["ema"].numel() == ema.numel and st["ranges"] == [tuple(r) for r in u.trainable_ranges()]
    ema2 = EmaWeights(u, DECAY)
    ema2.load_state(st)
    assert ema2.k == 1
    u.pflat.copy_((u.pflat.float() * 1.5).bfloat16())
    ema.update(); ema2.update()
    assert torch.equal(ema.full().view(torch.int32), ema2.full().view(torch.int32))
    other = EmaWeights(make_unet(exclude=("conv1",)), DECAY)
    with pytest.raises(ValueError, match="ranges"):
        other.load_state(st)
    with pytest.raises(ValueError, match="ranges"):
        ema.load_state(other.save_state())
    with pytest.raises(ValueError, match="world"):
        ema.load_state({**st, "world": 2})
    with pytest.raises(ValueError, match="rank"):
        ema.load_state({**st, "rank": 1})
    with pytest.raises(ValueError, match="numel"):
        ema.load_state({**st, "ema": st["ema"][:-64]})
    # an optimizer refuses an EMA that tracks something else than its owned trainable elements
    from aozora_sdxl_training_amd.dist import ShardedRaven
    with pytest.raises(ValueError, match="does not track"):
        ShardedRaven(u, lr=LR, force_local=True, ema=other)
