"""Stochastic rounding under data parallel: 2 ranks (sharing the single GPU of the test box, gloo backend) each update their shards
of the three regions; the random bits are keyed by the offset in the flat buffer, so the gathered parameters are bit-identical on
both ranks AND equal to a single-process run on the same (summed) gradients.  The same comparison with the flag off is the control."""
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

    res = {}
    for tag, kw in (("off", {}), ("on", dict(stochastic_rounding=True, sr_seed=42))):
        opt, pf = run(1.0, **kw)
        assert opt.exchange and opt.overlap and len(opt.regions) == 3 and opt.world == world
        gathered = [None] * world
        dist.all_gather_object(gathered, pf)
        res[f"ranks_agree_{tag}"] = bool(all(torch.equal(gathered[0], t) for t in gathered))
        _, p1 = run(float(world), force_local=True, **kw)           # single process on the summed gradients
        res[f"equals_single_{tag}"] = bool(torch.equal(pf, p1))
        res[f"p_{tag}"] = pf
    res["on_differs_from_off"] = float((res.pop("p_on") != res.pop("p_off")).float().mean())
    out[rank] = res
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_draw_the_bits_of_one_process():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    r0, r1 = out[0], out[1]
    for r in (r0, r1):
        assert r["ranks_agree_off"] and r["equals_single_off"], r          # the control: round-to-nearest
        assert r["ranks_agree_on"], r
        assert r["equals_single_on"], r
        assert 0.2 < r["on_differs_from_off"] < 0.8, r
