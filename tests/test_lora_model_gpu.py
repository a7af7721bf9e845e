"""AozoraUNet(lora=LoraSpec(...)) at the mini configuration (latent 8x8, B = 2, a 77-token context): the B = 0 identity against an
un-adapted UNet, parity of prediction, loss and adapter gradients with tests/lora_ref.LoraRefUNet in fp32 under the bounds of
tests/test_model_gpu.py, bitwise replay of the recorded step, gradient accumulation, a second resolution bucket in the same arena, a
narrowed target list (fused groups with adapters on some of their parts), and the adapter state dict."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import lora_ref as LR                                     # noqa: E402
from test_model_gpu import _mini, _inputs, _rel           # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, H, W = 2, 8, 8
RANK, ALPHA = 4, 8.0


def _freeze_base(unet):
    for n, p in unet.named_parameters():
        p.requires_grad = ".lora_" in n


def _gauss_b(unet, seed=5, sigma=0.02):
    g = torch.Generator().manual_seed(seed)
    sd = {n: t.float().cpu() for n, t in unet.lora_state_dict().items()}
    for n in sd:
        if n.endswith(".lora_B.weight"):
            sd[n] = (sigma * torch.randn(sd[n].shape, generator=g)).bfloat16().float()
    unet.load_lora_state_dict(sd)
    return sd


@pytest.fixture(scope="module")
def setup():
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    from oracle.unet_ref import init_params
    pc, oc = _mini()
    params = {k: v.bfloat16().float() for k, v in init_params(oc, seed=1234).items()}
    base = AozoraUNet(pc, DEV).load_state_dict(params)
    spec = LoraSpec(RANK, ALPHA)
    unet = AozoraUNet(pc, DEV, lora=spec).load_state_dict(params)
    unet.init_lora(42)
    _freeze_base(unet)
    return pc, oc, params, base, unet, spec


def _args(pc, h=H, w=W, seed=7):
    lat, noise, ctx, pooled, tid, ts, jit = _inputs(B, h, w, pc, seed=seed)
    return (lat, noise, ts, ctx, pooled, tid, jit), (lat.to(DEV), noise.to(DEV), ts, ctx.to(DEV), pooled.to(DEV), tid.to(DEV), jit)


def _micro(unet, dev_args, **kw):
    from aozora_sdxl_training_amd.train_step import TrainStep
    unet.zero_grad()
    step = TrainStep(unet, mode="epsilon", grad_accum=1, use_graph=False, **kw)
    loss = step.micro_step(*dev_args)
    step.synchronize()
    return loss.item(), step.last_pred_nhwc.clone(), step


def test_table_layout(setup):
    pc, oc, params, base, unet, spec = setup
    names = [n for n, _ in unet.named_parameters()]
    nb = len(base._table)
    assert names[:nb] == [n for n, _ in base._table] and names[nb - 1] == "conv_out.bias"
    assert all(".lora_" in n for n in names[nb:]) and len(names) - nb == 2 * 8 * 17         # 17 transformer blocks, 8 projections each
    assert all(unet._slots[n] == base._slots[n] for n, _ in base._table)                # the base slots keep their offsets
    assert set(unet.state_dict()) == set(base.state_dict()) and set(unet.lora_state_dict()) == set(names[nb:])
    tr = unet.trainable_ranges()
    assert len(tr) == 1 and tr[0][0] == unet._slots[names[nb]][0]                       # one contiguous trainable range: the adapters
    assert unet.region_bounds()[:2] == base.region_bounds()[:2]


def test_zero_up_matrices_are_the_identity(setup):
    pc, oc, params, base, unet, spec = setup
    _, dev = _args(pc)
    unet.init_lora(42)
    l0, p0, _ = _micro(base, dev)
    l1, p1, _ = _micro(unet, dev)
    assert torch.equal(p1, p0) and l1 == l0
    unet.expose_grads()
    nb = len(base._table)
    lo = unet._slots["conv_out.bias"][0] + 64
    assert not bool(unet.gflat[:lo].any()), "a frozen base parameter received a gradient"
    some_db = False
    for i, (n, p) in enumerate(unet.named_parameters()):
        if i < nb:
            assert p.grad is None, n
        elif n.endswith(".lora_A.weight"):
            assert not bool(p.grad.any()), n + ": dA must be zero while B = 0"
        else:
            some_db |= bool(p.grad.any())
    assert some_db


def _oracle_parity(unet, spec, params, oc, pc, h=H, w=W):
    """Prediction, loss and adapter-gradient vector of one micro-step against LoraRefUNet in fp32, under the bounds of
    tests/test_model_gpu.py: 1.5e-2 relative, 3e-3, max(1.5e-2, 1.5 x the bf16 oracle's own deviation)."""
    from oracle.step_ref import RefTrainer
    cpu, dev = _args(pc, h=h, w=w)
    lsd = _gauss_b(unet)
    allp = dict(params); allp.update(lsd)
    out = {}
    for bf16 in (False, True):
        ref = RefTrainer(oc, allp, mode="epsilon", bf16=bf16, ga=1, clip=1.0, frozen=tuple(params))
        ref.net = LR.LoraRefUNet(oc, ref.params, spec.scale)
        out[bf16] = (ref.micro_step(*cpu), ref.grads(), ref.last_pred)
    (l_ref, g_ref, p_ref), (l_b, g_b, p_b) = out[False], out[True]
    assert set(g_ref) == set(lsd)
    loss, pred_dev, _ = _micro(unet, dev)
    unet.expose_grads()
    pred = pred_dev.view(B, h, w, 4).permute(0, 3, 1, 2).float().cpu()
    sq_r = sq_d = sq_db = 0.0
    for n, p in unet.named_parameters():
        if ".lora_" not in n:
            continue
        gh, gr = p.grad.float().cpu(), g_ref[n].float()
        sq_r += gr.double().pow(2).sum().item()
        sq_d += (gh - gr).double().pow(2).sum().item()
        sq_db += (g_b[n].float() - gr).double().pow(2).sum().item()
    rep = dict(pred_rel=_rel(pred, p_ref), loss_hip=loss, loss_fp32=l_ref, grad_vector_rel=math.sqrt(sq_d / sq_r),
               grad_vector_rel_bf16_oracle=math.sqrt(sq_db / sq_r), pred_rel_bf16_oracle=_rel(p_b, p_ref))
    print(rep)
    assert sq_r > 0
    assert rep["pred_rel"] <= 1.5e-2, rep
    assert abs(loss - l_ref) <= 3e-3 * abs(l_ref), rep
    assert rep["grad_vector_rel"] <= max(1.5e-2, 1.5 * rep["grad_vector_rel_bf16_oracle"]), rep
    return loss, pred_dev, dev


def test_matches_the_oracle_with_adapters(setup):
    pc, oc, params, base, unet, spec = setup
    _oracle_parity(unet, spec, params, oc, pc)


@pytest.mark.parametrize("rank, low", [(16, False), (64, True)], ids=["rank16", "rank64-lowered-thresholds"])
def test_unit_scale_takes_the_general_product_where_it_is_faster(setup, rank, low):
    """alpha = rank (s = 1) at latent 48x48 (1152 rows at the first attention level, 288 at the second, 154 of context): the products
    that tools/lora_time.py found faster as az_gemm_bf16 are issued there (lora_exec.LoraRoutes.down / up / tall), the rest as
    az_lora_*.  rank 16: the shipped thresholds -- every tall reduction and the many-row single projections go to the general product.
    rank 64 with the row thresholds lowered to what a 48x48 latent reaches: the stacked down product and the fused accumulates too.
    Same contract, same bounds; the recorded step replays bit for bit."""
    from aozora_sdxl_training_amd._lib import lib
    from aozora_sdxl_training_amd.train_step import TrainStep
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    pc, oc, params, base, _, _ = setup
    spec = LoraSpec(rank, float(rank))
    unet = AozoraUNet(pc, DEV, lora=spec).load_state_dict(params)
    unet.init_lora(3)
    _freeze_base(unet)
    if low:
        unet.adapters.routes.DOWN_GEMM_ROWS, unet.adapters.routes.UP_FEW_ROWS = 1000, 100
    L = lib()
    L.recorder = []
    try:
        loss, pred, dev = _oracle_parity(unet, spec, params, oc, pc, h=48, w=48)
    finally:
        names, L.recorder = [getattr(op, "name", None) for op in L.recorder], None
    assert "az_lora_down_bf16" in names and "az_lora_wgrad_bf16" not in names
    assert ("az_lora_up_bf16" in names) == (not low)          # rank 16: the few-row inputs and the fused q|k|v groups
    g1 = unet.gflat.clone()
    step = TrainStep(unet, mode="epsilon", grad_accum=1, use_graph=True)
    for i in range(3):
        unet.zero_grad()
        l = step.micro_step(*dev).item()
        step.synchronize()
        assert l == loss and torch.equal(unet.gflat, g1), f"replay {i} differs from the eager step"


def test_replay_is_bitwise_and_accumulation_doubles(setup):
    from aozora_sdxl_training_amd.train_step import TrainStep
    pc, oc, params, base, unet, spec = setup
    _, dev = _args(pc, seed=11)
    _gauss_b(unet)
    unet.zero_grad()
    eager = TrainStep(unet, mode="epsilon", grad_accum=2, use_graph=False)
    l0 = eager.micro_step(*dev).item()
    eager.synchronize()
    g1 = unet.gflat.clone()
    eager.micro_step(*dev); eager.synchronize()
    g2 = unet.gflat.clone()
    assert bool(g1.any()) and _rel(g2, 2 * g1.float()) < 8e-3
    graphed = TrainStep(unet, mode="epsilon", grad_accum=2, use_graph=True)
    for i in range(3):                 # run 0 eager (allocates), runs 1 and 2 replay the recorded step
        unet.zero_grad()
        l = graphed.micro_step(*dev).item()
        graphed.synchronize()
        assert torch.equal(unet.gflat, g1), f"replay {i} differs from the eager step"
        assert l == l0


def test_second_bucket_shares_the_arena(setup):
    from aozora_sdxl_training_amd.unet import AozoraUNet
    pc, oc, params, base, unet0, spec = setup
    unet = AozoraUNet(pc, DEV, lora=spec).load_state_dict(params)
    unet.load_lora_state_dict(unet0.lora_state_dict())
    _freeze_base(unet)
    from aozora_sdxl_training_amd.train_step import TrainStep
    step = TrainStep(unet, mode="epsilon", grad_accum=1, use_graph=False)
    big, small = _args(pc)[1], _args(pc, h=4, w=8, seed=9)[1]
    res = []
    for a in (big, small, big, small):
        unet.zero_grad()
        l = step.micro_step(*a).item(); step.synchronize()
        res.append((l, unet.gflat.clone()))
    ab = unet.activation_bytes()
    assert ab["generation"] == 1, ab
    assert res[2][0] == res[0][0] and torch.equal(res[2][1], res[0][1]) and res[3][0] == res[1][0] and torch.equal(res[3][1], res[1][1])


def test_narrowed_targets_and_state_dict_round_trip(setup):
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    pc, oc, params, base, _, _ = setup
    spec = LoraSpec(16, 8.0, "to_q, to_v")               # attn1: parts 0 and 2 of the fused q|k|v; attn2: to_q and part 1 of k|v
    unet = AozoraUNet(pc, DEV, lora=spec).load_state_dict(params)
    unet.init_lora(1)
    _freeze_base(unet)
    lsd = _gauss_b(unet)
    assert all(".to_q." in n or ".to_v." in n for n in lsd) and len(lsd) == 2 * 4 * (2 * 1 + 2 * 2 + 3 * 2 + 3 * 1 + 2)
    loss, pred, dev = _oracle_parity(unet, spec, params, oc, pc)      # (draws the Gaussian up matrices again: same seed, same values)
    # the adapters of one UNet loaded into a fresh one reproduce the prediction bit for bit
    other = AozoraUNet(pc, DEV, lora=spec).load_state_dict(params)
    other.load_lora_state_dict({k: v.clone() for k, v in unet.lora_state_dict().items()})
    _freeze_base(other)
    l2, pred2, _ = _micro(other, dev)
    assert l2 == loss and torch.equal(pred2, pred)
    with pytest.raises(KeyError):
        other.load_lora_state_dict({k: v for k, v in list(lsd.items())[1:]})


def test_spec_refusals():
    from aozora_sdxl_training_amd.unet_spec import LoraSpec, lora_modules, SDXL_BASE
    assert len(lora_modules(SDXL_BASE, LoraSpec(16, 16.0))) == 560
    for bad in (dict(rank=5), dict(rank=128), dict(alpha=0.0), dict(alpha=-1.0)):
        with pytest.raises(ValueError):
            LoraSpec(**bad)
    for targets, why in (("proj_in", "out of scope"), ("ff.net.2", "out of scope"), ("no_such_layer", "selects no")):
        with pytest.raises(ValueError, match=why):
            lora_modules(SDXL_BASE, LoraSpec(16, 16.0, targets))
