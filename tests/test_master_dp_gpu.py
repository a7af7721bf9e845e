"""fp32 master weights under data parallel: 2 ranks (sharing the single GPU of the test box, gloo backend) each keep the master of
their shards of the three regions.  The gathered parameters are bit-identical on both ranks AND equal to a single-process run on the
same (summed) gradients; so is the master: every rank's w_dev scattered to flat offsets through its ranges / range_off, the union
of the ranks.  The same comparison with the flag off is the control.  (The harness of tests/test_sr_dp_gpu.py.)"""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 2


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dev = "cuda:0"
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import mini_config
    from aozora_sdxl_training_amd.dist import ShardedRaven
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
        return u

    def run(scale, **kw):
        """STEPS optimizer steps on synthetic gradients scale * g (the same on every rank).  clip_grad_norm = 0: the clip coefficient
        is exactly 1, and the exchange leaves the exact sum world * g (a power of two times a bf16 value)."""
        u = make_unet()
        g = torch.Generator().manual_seed(5)
        opt = ShardedRaven(u, lr=1e-3, clip_grad_norm=0, **kw)
        for _ in range(STEPS):
            u.wait_tail_params(); torch.cuda.synchronize()
            u.gflat.copy_(((torch.randn(u.flat_numel, generator=g) * 1e-2).to(torch.bfloat16) * scale).to(dev))
            opt.step()
        u.wait_tail_params(); torch.cuda.synchronize()
        return opt, u.pflat.cpu()

    def master_flat(opt):
        """(fp32 values at flat offsets, mask of the elements this optimizer owns)"""
        w = torch.zeros(opt.unet.flat_numel, dtype=torch.float32)
        own = torch.zeros(opt.unet.flat_numel, dtype=torch.bool)
        wd = opt.w_dev.cpu()
        for rs, offs in zip(opt.ranges, opt.range_off):
            for (a, b), o in zip(rs, offs):
                w[a:b] = wd[o:o + (b - a)]
                own[a:b] = True
        return w, own

    res = {}
    for tag, kw in (("off", {}), ("on", dict(master_weights=True))):
        opt, pf = run(1.0, **kw)
        assert opt.exchange and opt.overlap and len(opt.regions) == 3 and opt.world == world
        gathered = [None] * world
        dist.all_gather_object(gathered, pf)
        res[f"ranks_agree_{tag}"] = bool(all(torch.equal(gathered[0], t) for t in gathered))
        opt1, p1 = run(float(world), force_local=True, **kw)           # single process on the summed gradients
        res[f"equals_single_{tag}"] = bool(torch.equal(pf, p1))
        res[f"p_{tag}"] = pf
        if tag == "on":
            w, own = master_flat(opt)
            w1, own1 = master_flat(opt1)
            res["shard_is_its_share"] = opt.w_dev.numel() == opt.shard == int(own.sum()) and opt1.w_dev.numel() == opt1.shard == int(own1.sum())
            res["master_equals_single_on_owned"] = bool(torch.equal(w[own].view(torch.int32), w1[own].view(torch.int32)))
            res["pflat_is_bf16_of_master"] = bool(torch.equal(w[own].bfloat16(), pf[own]))
            parts = [None] * world
            dist.all_gather_object(parts, (w, own))
            cover = sum(o.int() for _, o in parts)
            union = torch.zeros_like(w1)
            for x, o in parts:
                union[o] = x[o]
            res["ranks_partition_the_single_ranges"] = bool(torch.equal(cover, own1.int()))       # disjoint, and together what one process owns
            res["union_equals_single"] = bool(torch.equal(union.view(torch.int32), w1.view(torch.int32)))
        else:
            res["off_keeps_no_master"] = opt.w_dev is None
    res["on_differs_from_off"] = int((res.pop("p_on") != res.pop("p_off")).sum())
    out[rank] = res
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_keep_the_master_of_one_process():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    for r in (out[0], out[1]):
        assert r["ranks_agree_off"] and r["equals_single_off"] and r["off_keeps_no_master"], r          # the control
        assert r["ranks_agree_on"], r
        assert r["equals_single_on"], r
        assert r["shard_is_its_share"] and r["pflat_is_bf16_of_master"], r
        assert r["master_equals_single_on_owned"] and r["ranks_partition_the_single_ranges"] and r["union_equals_single"], r
        assert r["on_differs_from_off"] > 0, r
