"""Parameter groups under data parallel: the whole exchange schedule over RCCL in a group of one rank (ShardedRaven / ShardedTitan with
force_exchange=True: three regions, reduce-scatter, the shards of regions 1 and 2 updated on the communication stream, all-gathers) must
leave the parameters and moments of the local optimizer bit for bit -- with one rank every collective is the identity, so what is compared
is that each region's launch finds its groups through the global offset it passes as elem0.  Plain, stochastic rounding, master weights."""
import gc
import os
import socket
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
STEPS = 3
LRS = (1e-3, 7e-4, 2.5e-4)
RULES = [{"match": "bias, norm", "weight_decay": 0.0}, {"match": ["down_blocks.0.*", "conv_in"], "lr_scale": 0.25},
         {"match": "mid_block", "lr_scale": 0.0, "weight_decay": 0.0}]


@pytest.fixture(autouse=True)
def _collect_cycles():
    """Optimizers and UNets sit in reference cycles that hold device objects: they are collected here, when the test that made them
    ends, not by whichever later test happens to trigger the collector."""
    yield
    gc.collect()


def test_exchange_schedule_at_world_one_equals_the_local_optimizer():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import torch.distributed as dist
    from aozora_sdxl_training_amd import param_groups as PG
    from aozora_sdxl_training_amd.dist import ShardedRaven, ShardedTitan
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import mini_config
    if dist.is_initialized():
        pytest.skip("process group already initialised")
    u = AozoraUNet(mini_config(), DEV)
    gg = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for n, p in u.named_parameters():
            if "norm" in n:
                p.fill_(1.0 if n.endswith("weight") else 0.0)
            else:
                p.copy_((torch.randn(p.shape, generator=gg) * 0.05).bfloat16())
    start = u.pflat.clone()
    grads = [(torch.randn(u.flat_numel, generator=gg) * 1e-2).to(torch.bfloat16).to(DEV) for _ in range(STEPS)]
    res = PG.resolve_unet(u, PG.parse_rules(RULES, 0.01), 0.01)

    def run(cls, **kw):
        u.wait_tail_params(); torch.cuda.synchronize()
        u.pflat.copy_(start)
        u.mark_params_dirty()
        opt = cls(u, lr=1e-3, weight_decay=0.01, clip_grad_norm=0, groups=res, **kw)
        for lr, g in zip(LRS, grads):
            opt.param_groups[0]["lr"] = lr
            opt.zero_grad()
            u.wait_tail_params(); torch.cuda.synchronize()
            u.gflat.copy_(g)
            if cls is ShardedTitan:
                opt.accumulate()
            opt.step()
        u.wait_tail_params(); torch.cuda.synchronize()
        return opt, u.pflat.clone(), opt.m_dev.clone(), opt.v_dev.clone(), (opt.w_dev.clone() if opt.w_dev is not None else None)

    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        for cls, kw in ((ShardedRaven, {}), (ShardedRaven, dict(stochastic_rounding=True, sr_seed=42)), (ShardedRaven, dict(master_weights=True)),
                        (ShardedTitan, {})):
            o_x, p_x, m_x, v_x, w_x = run(cls, force_exchange=True, **kw)
            assert o_x.exchange and len(o_x.regions) == 3 and o_x.world == 1 and (cls is ShardedTitan or o_x.overlap)
            o_l, p_l, m_l, v_l, w_l = run(cls, force_local=True, regions=3, **kw)
            assert not o_l.exchange and o_l.ranges == o_x.ranges
            what = f"{cls.__name__} {kw}"
            assert torch.equal(p_x, p_l) and torch.equal(m_x, m_l) and torch.equal(v_x, v_l), what
            assert (w_x is None) == (w_l is None) and (w_x is None or torch.equal(w_x, w_l)), what
            assert not torch.equal(p_x, start)
    finally:
        dist.destroy_process_group()
