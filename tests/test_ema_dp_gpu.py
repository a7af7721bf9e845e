"""The EMA of the weights under data parallel: 2 ranks (sharing the single GPU of the test box, gloo backend, spawned as
tests/test_dp_gpu.py spawns them) run dist.ShardedRaven(..., ema=...) in its overlapped three-region schedule.  Each rank keeps the
fp32 EMA of its own shard only; state_dict() gathers; a per-rank save / load round trip continues bit for bit."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECAY, LR = 0.9, 1e-3


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import numpy as np
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dev = "cuda:0"
    import ema_ref as E
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import mini_config
    from aozora_sdxl_training_amd.dist import ShardedRaven
    from aozora_sdxl_training_amd.schedule import trainable_mask
    pc = mini_config()

    def make_unet():
        u = AozoraUNet(pc, dev)
        gg = torch.Generator().manual_seed(77)
        with torch.no_grad():
            for n, p in u.named_parameters():
                if "norm" in n:
                    p.fill_(1.0 if n.endswith("weight") else 0.0)
                else:
                    p.copy_((torch.randn(p.shape, generator=gg) * 0.05).bfloat16())
        names = [n for n, _ in u.named_parameters()]
        for (n, p), m in zip(u.named_parameters(), trainable_mask(names, ["conv1", "conv2"])):
            p.requires_grad = m
        return u

    u = make_unet()
    g = torch.Generator().manual_seed(100 + rank)                      # every rank its own gradients: the reduce-scatter sums them
    grads = [(torch.randn(u.flat_numel, generator=g) * 1e-3).bfloat16() for _ in range(3)]
    opt = ShardedRaven(u, lr=LR, clip_grad_norm=1.0, ema=dict(decay=DECAY))
    ema = opt.ema
    res = dict(overlap=bool(opt.overlap), shard=opt.shard, ema_numel=ema.numel, ema_buf=ema.ema.numel(), world=ema.world, ema_rank=ema.rank,
               trainable=sum(b - a for a, b in u.trainable_ranges()))

    def snapshot(un):
        return {n: t.detach().clone().cpu() for n, t in un.state_dict().items()}

    def one_step(o, un, s):
        un.gflat.copy_(grads[s].to(dev))
        o.step()
        o.synchronize_params()

    snaps, emas = [snapshot(u)], []
    for s in range(2):
        one_step(opt, u, s)
        snaps.append(snapshot(u))
        emas.append({n: t.clone().cpu() for n, t in ema.state_dict().items()})       # every rank: the gather is a collective
    # bit for bit against the restatement replayed over THIS rank's parameter snapshots
    want = E.replay(snaps, DECAY, True)
    bad = 0
    for s in range(2):
        for n, t in emas[s].items():
            a, b = t.contiguous().numpy(), np.ascontiguousarray(want[s][n])
            bad += int((~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))).sum())
    res["mismatches"] = bad
    res["moved"] = sum(int(not torch.equal(snaps[2][n], snaps[0][n])) for n in snaps[0])
    res["lags"] = any(not np.array_equal(emas[1][n].numpy(), E.torch_bf16_to_f32(snaps[2][n])) for n in snaps[0])
    # per-rank save -> fresh objects -> load, one more step: equals the uninterrupted run
    p2 = u.pflat.clone()
    ost, est = opt.save_cpu_state(), ema.save_state()
    res["state_keys"] = sorted(est)
    res["state_ok"] = bool(est["k"] == 2 and est["world"] == world and est["rank"] == rank and est["ema"].numel() == opt.shard
                           and [tuple(r) for r in est["ranges"]] == [tuple(r) for rs in opt.ranges for r in rs])
    one_step(opt, u, 2)
    full_a = ema.full()
    u2 = make_unet()
    u2.pflat.copy_(p2)
    u2.mark_params_dirty()
    opt2 = ShardedRaven(u2, lr=LR, clip_grad_norm=1.0, ema=dict(decay=DECAY))
    opt2.load_cpu_state(ost)
    opt2.ema.load_state(est)
    one_step(opt2, u2, 2)
    full_b = opt2.ema.full()
    torch.cuda.synchronize()
    res["resumed_params_equal"] = bool(torch.equal(u.pflat, u2.pflat))
    res["resumed_ema_equal"] = bool(torch.equal(full_a.view(torch.int32), full_b.view(torch.int32))
                                    and torch.equal(ema.ema.view(torch.int32), opt2.ema.ema.view(torch.int32)) and opt2.ema.k == ema.k == 3)
    # another rank's state is refused
    try:
        opt2.ema.load_state({**est, "rank": 1 - rank})
        res["foreign_rank_refused"] = False
    except ValueError:
        res["foreign_rank_refused"] = True
    out[rank] = res
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_keep_sharded_ema():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    r0, r1 = dict(out[0]), dict(out[1])
    for r in (r0, r1):
        assert r["overlap"] and r["world"] == 2, r
        assert r["ema_numel"] == r["shard"] and r["ema_buf"] == max(r["shard"], 1), r      # frozen parameters and other ranks' elements own no EMA memory
        assert set(r["state_keys"]) == {"decay", "ema", "k", "rank", "ranges", "warmup", "world"} and r["state_ok"], r
        assert r["resumed_params_equal"] and r["resumed_ema_equal"] and r["foreign_rank_refused"], r
    assert (r0["ema_rank"], r1["ema_rank"]) == (0, 1)
    assert r0["shard"] + r1["shard"] == r0["trainable"] and 0 < r0["shard"] < r0["trainable"], (r0, r1)
    assert r0["mismatches"] == 0 and r0["moved"] > 0 and r0["lags"], r0
    assert r1["mismatches"] == 0, r1
