"""paged_adamw_8bit on the device: the HIP kernel against the CPU restatement (tests/adamw8bit_ref.py) bit for bit, the optimizer as
a drop-in on a mini-UNet with a state_dict round trip, and the trainer end to end with a bitwise resume."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
DEV = "cuda:0"

import adamw8bit_ref as R        # noqa: E402


def _bits(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16).reshape(-1).copy()


def _grad32(t):
    return t.detach().float().contiguous().cpu().numpy().reshape(-1).copy()


def _check_state(opt, ref, params):
    for p, st in zip(params, ref.state):
        mine = opt.state[p]
        if "m" in st:
            assert mine["state1"].dtype == torch.float32
            assert torch.equal(mine["state1"].cpu().reshape(-1), torch.from_numpy(st["m"]))
            assert torch.equal(mine["state2"].cpu().reshape(-1), torch.from_numpy(st["v"]))
        else:
            assert mine["state1"].dtype == torch.uint8
            assert torch.equal(mine["state1"].cpu().reshape(-1), torch.from_numpy(st["c1"]))
            assert torch.equal(mine["state2"].cpu().reshape(-1), torch.from_numpy(st["c2"]))
            assert torch.equal(mine["absmax1"].cpu(), torch.from_numpy(st["a1"]))
            assert torch.equal(mine["absmax2"].cpu(), torch.from_numpy(st["a2"]))


def _mini_unet(seed):
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import mini_config
    unet = AozoraUNet(mini_config(), DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    unet.pflat.copy_((torch.randn(unet.flat_numel, generator=g, device=DEV) * 0.05).bfloat16())
    return unet


def test_kernel_matches_restatement_bitwise():
    from aozora_sdxl_training_amd.optimizers import PagedAdamW8bit
    torch.manual_seed(0)
    unet = _mini_unet(1)
    named = dict(unet.named_parameters())
    conv = named["down_blocks.0.resnets.0.conv1.weight"]
    conv_in = named["conv_in.weight"]
    assert conv.dim() == 4 and conv.shape[2:] == (3, 3) and conv_in.shape[1] == 4      # permuted and padded storage
    plain = [(torch.randn(n, device=DEV) * 0.1).bfloat16() for n in (1000, 4096, 5000)]
    plain.append((torch.randn(96, 64, device=DEV) * 0.1).bfloat16())                 # a 2-D linear weight
    params = plain + [conv, conv_in]
    opt = PagedAdamW8bit(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    ref = R.RefAdamW8bit([p.numel() for p in params], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    unet.expose_grads()
    pads_before = unet.pflat.clone()
    p_host = [_bits(p) for p in params]
    nan_at = 17
    nan_elem = p_host[1][nan_at]
    for t in range(5):
        for p in plain:
            p.grad = (torch.randn(p.shape, device=DEV) * 10 ** (-t)).bfloat16()
        plain[1].grad.view(-1)[nan_at] = float("nan")                                  # this element never moves
        unet.gflat.copy_((torch.randn(unet.flat_numel, device=DEV) * 0.01).bfloat16())
        grads = [_grad32(p.grad) for p in params]
        lr = 1e-3 * (1.0 - 0.15 * t)
        opt.param_groups[0]["lr"] = lr
        ref.lr = lr
        coef = 0.7
        opt.clip_coef = torch.tensor([coef], dtype=torch.float32, device=DEV)
        opt.step()
        torch.cuda.synchronize()
        p_host = ref.step(p_host, grads, coef=coef)
        for p, want in zip(params, p_host):
            assert np.array_equal(_bits(p), want)
        _check_state(opt, ref, params)
    # the NaN-gradient element kept its initial value through all five steps
    assert _bits(plain[1])[nan_at] == nan_elem and torch.isfinite(plain[1].float()).all()
    # storage outside the two parameters (other slots, conv_in's input-channel pad) is untouched
    sl = []
    for name in ("down_blocks.0.resnets.0.conv1.weight", "conv_in.weight"):
        off, st, lshape = unet._slots[name]
        n = int(np.prod(st))
        view = unet.pflat[off:off + n].view(st)
        if name == "conv_in.weight":
            assert torch.equal(view[..., lshape[1]:], pads_before[off:off + n].view(st)[..., lshape[1]:])
        sl.append((off, off + n))
    keep = torch.ones(unet.flat_numel, dtype=torch.bool, device=DEV)
    for a, b in sl:
        keep[a:b] = False
    assert torch.equal(unet.pflat[keep], pads_before[keep])


def test_nan_gradient_element_is_unchanged():
    from aozora_sdxl_training_amd.optimizers import PagedAdamW8bit
    p = (torch.randn(4096, device=DEV) * 0.1).bfloat16()
    before = p.clone()
    opt = PagedAdamW8bit([p], lr=1e-2, weight_decay=0.1)
    for _ in range(3):
        p.grad = torch.randn(4096, device=DEV).bfloat16()
        p.grad[5] = float("nan")
        p.grad[6] = float("inf")
        opt.step()
    torch.cuda.synchronize()
    assert p[5].item() == before[5].item() and p[6].item() == before[6].item()
    assert not torch.equal(p[7:], before[7:])


def _inputs(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    B, h, w = 2, 16, 16
    return (torch.randn(B, 4, h, w, generator=g).bfloat16().to(DEV), torch.randn(B, 4, h, w, generator=g).to(DEV),
            torch.tensor([37, 911]), torch.randn(B, 77, cfg.cross_attention_dim, generator=g).bfloat16().to(DEV),
            torch.randn(B, cfg.pooled_dim, generator=g).bfloat16().to(DEV),
            torch.tensor([[128, 128, 0, 0, 128, 128]] * B, dtype=torch.bfloat16).to(DEV))


def test_drop_in_on_mini_unet_and_state_dict_round_trip():
    from aozora_sdxl_training_amd.clip import clip_grad_norm_
    from aozora_sdxl_training_amd.optimizers import PagedAdamW8bit
    from aozora_sdxl_training_amd.train_step import TrainStep
    from aozora_sdxl_training_amd.unet_spec import mini_config
    unet = _mini_unet(2)
    params = list(unet.parameters())
    opt = PagedAdamW8bit(params, lr=1e-4, weight_decay=0.01)
    ref = R.RefAdamW8bit([p.numel() for p in params], lr=1e-4, weight_decay=0.01)
    step = TrainStep(unet, mode="epsilon", grad_accum=1, use_graph=False)
    p_host = [_bits(p) for p in params]
    cfg = mini_config()

    def one_step(k):
        opt.zero_grad(set_to_none=True)
        loss = step.micro_step(*_inputs(cfg, k))
        unet.expose_grads()
        clip_grad_norm_(unet, 1.0)
        grads = [_grad32(p.grad) for p in params]
        opt.step()
        torch.cuda.synchronize()
        assert torch.isfinite(loss).all()
        return grads

    for k in range(3):
        grads = one_step(k)
        p_host = ref.step(p_host, grads)
        for p, want in zip(params, p_host):
            assert np.array_equal(_bits(p), want)
    _check_state(opt, ref, params)
    assert sum("absmax1" in opt.state[p] for p in params) > 0 and sum("absmax1" not in opt.state[p] for p in params) > 0

    # state_dict -> fresh optimizer -> load_state_dict -> one more step == the uninterrupted run
    sd = opt.state_dict()
    assert all(v["state1"].device.type == "cpu" for v in sd["state"].values())
    p_snap = unet.pflat.clone()
    opt.zero_grad(set_to_none=True)
    step.micro_step(*_inputs(cfg, 3))
    unet.expose_grads()
    clip_grad_norm_(unet, 1.0)
    g_snap = unet.gflat.clone()
    opt.step()
    torch.cuda.synchronize()
    want_p = unet.pflat.clone()
    want_state = [{k: v.clone() for k, v in opt.state[p].items() if torch.is_tensor(v)} for p in params]

    unet.pflat.copy_(p_snap)
    unet.gflat.copy_(g_snap)
    opt2 = PagedAdamW8bit(params, lr=1e-4, weight_decay=0.01)
    opt2.load_state_dict(sd)
    assert all(opt2.state[p]["absmax1"].dtype == torch.float32 for p in params if "absmax1" in opt2.state[p])
    opt2.step()
    torch.cuda.synchronize()
    assert torch.equal(unet.pflat, want_p)
    for p, ws in zip(params, want_state):
        for k, v in ws.items():
            assert torch.equal(opt2.state[p][k], v), k

    # a file whose tensors carry differing maps is refused
    bad = opt.state_dict()
    i8 = [i for i, v in bad["state"].items() if "qmap1" in v]
    bad["state"][i8[1]]["qmap1"] = bad["state"][i8[1]]["qmap1"].clone()
    bad["state"][i8[1]]["qmap1"][3] += 1e-3
    from aozora_sdxl_training_amd._lib import AozoraError
    with pytest.raises(AozoraError, match="differing"):
        PagedAdamW8bit(params).load_state_dict(bad)


def test_trainer_end_to_end_and_bitwise_resume(tmp_path):
    from aozora_sdxl_training_amd import checkpoint as C
    from aozora_sdxl_training_amd.trainer import train
    from aozora_sdxl_training_amd.telemetry import Reporter
    from aozora_sdxl_training_amd.unet_spec import mini_config
    from tests.test_trainer_gpu import _base_checkpoint, _config
    model = mini_config(ctx_dim=64, pooled=32)
    tmp = str(tmp_path)
    over = dict(OPTIMIZER_TYPE="paged_adamw_8bit", PAGED_ADAMW_8BIT_PARAMS={"betas": [0.9, 0.999], "eps": 1e-8, "weight_decay": 0.01})
    cfg = _config(tmp, "v_prediction", **over)
    _base_checkpoint(cfg.SINGLE_FILE_CHECKPOINT_PATH, model)
    with contextlib.redirect_stdout(io.StringIO()):
        unet = C.load_unet(cfg.SINGLE_FILE_CHECKPOINT_PATH, DEV, model)
        h = train(cfg, unet=unet, device=DEV, reporter=Reporter(cfg.MAX_TRAIN_STEPS, asynchronous=False))
    torch.cuda.synchronize()
    assert h["micro_step"] == 8 and h["optimizer_step"] == 4 and len(h["losses"]) == 8
    assert all(l == l and 0.0 < l < 10.0 for l in h["losses"])
    final = unet.pflat.clone()

    st = torch.load(os.path.join(cfg.OUTPUT_DIR, "mini_run_training_state_step_2.pt"), map_location="cpu", weights_only=False)
    osd = st["optimizer_state"]
    assert set(osd) == {"state", "param_groups"}
    eight = [v for v in osd["state"].values() if "qmap1" in v]
    small = [v for v in osd["state"].values() if "qmap1" not in v]
    assert eight and small
    for v in eight:
        assert set(v) == {"step", "state1", "state2", "qmap1", "qmap2", "absmax1", "absmax2"}
        assert v["state1"].dtype == torch.uint8 and v["state2"].dtype == torch.uint8 and v["absmax1"].dtype == torch.float32
        assert v["step"] == 2
    for v in small:
        assert set(v) == {"step", "state1", "state2"} and v["state1"].dtype == torch.float32

    cfg2 = _config(tmp, "v_prediction", RESUME_TRAINING=True, SAVE_EVERY_N_STEPS=0,
                   RESUME_MODEL_PATH=os.path.join(cfg.OUTPUT_DIR, "mini_run_step_2.safetensors"),
                   RESUME_STATE_PATH=os.path.join(cfg.OUTPUT_DIR, "mini_run_training_state_step_2.pt"), **over)
    with contextlib.redirect_stdout(io.StringIO()):
        unet2 = C.load_unet(cfg2.RESUME_MODEL_PATH, DEV, model)
        h2 = train(cfg2, unet=unet2, device=DEV, reporter=Reporter(cfg2.MAX_TRAIN_STEPS, asynchronous=False))
    torch.cuda.synchronize()
    assert h2["micro_step"] == 8 and h2["optimizer_step"] == 4
    assert h2["losses"] == h["losses"][4:] and h2["grad_norms"] == h["grad_norms"][2:]
    assert torch.equal(unet2.pflat, final)
