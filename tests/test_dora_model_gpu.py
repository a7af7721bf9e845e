"""AozoraUNet(lora=LoraSpec(..., dora=True)) at the mini configuration (latent 8x8, B = 2), scopes "attention" and "transformer", also
with targets narrowed to "to_q, to_v" (a partly adapted fused group): prediction, loss and the gradient vector over A, B and dora_scale
against tests/dora_ref.DoraRefUNet (its adapted linears in float64 inside the fp32 oracle) under the bounds of
tests/test_lora_model_gpu.py -- 1.5e-2 on the prediction, 3e-3 on the loss, max(1.5e-2, 1.5 x the rounded oracle's own deviation) on
the gradient; the init identity; accumulation; new gains after load_lora_state_dict; the replayed tape against the eager step; and with
dora=False the parent's launch list and activation_bytes()."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import dora_ref as D                                                                   # noqa: E402
from test_model_gpu import _mini, _rel                                                 # noqa: E402
from test_lora_model_gpu import _args, _micro, B, H, W                                 # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RANK, ALPHA = 4, 8.0
SPECS = {"attention": ("", "attention"), "transformer": ("", "transformer"), "q-and-v": ("to_q, to_v", "attention")}


def _freeze_base(unet):
    adapters = set(unet.lora_state_dict())
    for n, p in unet.named_parameters():
        p.requires_grad = n in adapters


def _perturb(unet, seed=5):
    """Gaussian up matrices and magnitudes 10 % off the row norms: every gain differs from 1.  -> the loaded state (float32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    sd = {n: t.float().cpu() for n, t in unet.lora_state_dict().items()}
    for n in sd:
        if n.endswith(".lora_B.weight"):
            sd[n] = (0.02 * torch.randn(sd[n].shape, generator=g)).bfloat16().float()
        elif n.endswith(".dora_scale"):
            sd[n] = (sd[n] * (1.0 + 0.1 * torch.randn(sd[n].shape, generator=g))).bfloat16().float()
    unet.load_lora_state_dict(sd)
    return sd


@pytest.fixture(scope="module")
def setup():
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from oracle.unet_ref import init_params
    pc, oc = _mini()
    params = {k: v.bfloat16().float() for k, v in init_params(oc, seed=1234).items()}
    base = AozoraUNet(pc, DEV).load_state_dict(params)
    return pc, oc, params, base, {}


def _unet(setup, key, seed=42):
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    pc, oc, params, base, cache = setup
    if key not in cache:
        spec = LoraSpec(RANK, ALPHA, *SPECS[key], dora=True)
        unet = AozoraUNet(pc, DEV, lora=spec).load_state_dict(params)
        unet.init_lora(seed)
        _freeze_base(unet)
        cache[key] = (unet, spec)
    return cache[key]


def _oracle(setup, spec, lsd):
    """(loss, gradients, prediction) of the fp32 oracle and of the bf16 one for the adapter state lsd."""
    from oracle.step_ref import RefTrainer
    pc, oc, params, _, _ = setup
    cpu, dev = _args(pc)
    allp = dict(params); allp.update(lsd)
    out = {}
    for bf16 in (False, True):
        ref = RefTrainer(oc, allp, mode="epsilon", bf16=bf16, ga=1, clip=1.0, frozen=tuple(params))
        ref.net = D.DoraRefUNet(oc, ref.params, spec.scale)
        out[bf16] = (ref.micro_step(*cpu), ref.grads(), ref.last_pred)
    return out, dev


def _parity(setup, unet, spec, lsd):
    out, dev = _oracle(setup, spec, lsd)
    (l_ref, g_ref, p_ref), (l_b, g_b, p_b) = out[False], out[True]
    assert set(g_ref) == set(lsd)
    loss, pred_dev, _ = _micro(unet, dev)
    unet.expose_grads()
    pred = pred_dev.view(B, H, W, 4).permute(0, 3, 1, 2).float().cpu()
    sq_r = sq_d = sq_db = 0.0
    sq_m = sq_md = 0.0
    for n, p in unet.named_parameters():
        if n not in lsd:
            continue
        gh, gr = p.grad.float().cpu(), g_ref[n].float()
        sq_r += gr.double().pow(2).sum().item()
        sq_d += (gh - gr).double().pow(2).sum().item()
        sq_db += (g_b[n].float() - gr).double().pow(2).sum().item()
        if n.endswith(".dora_scale"):
            sq_m += gr.double().pow(2).sum().item()
            sq_md += (gh - gr).double().pow(2).sum().item()
    rep = dict(pred_rel=_rel(pred, p_ref), loss_hip=loss, loss_fp32=l_ref, grad_vector_rel=math.sqrt(sq_d / sq_r),
               grad_vector_rel_bf16_oracle=math.sqrt(sq_db / sq_r), pred_rel_bf16_oracle=_rel(p_b, p_ref),
               dora_scale_grad_rel=math.sqrt(sq_md / sq_m))
    print(rep)
    assert sq_r > 0 and sq_m > 0
    assert rep["pred_rel"] <= 1.5e-2, rep
    assert abs(loss - l_ref) <= 3e-3 * abs(l_ref), rep
    assert rep["grad_vector_rel"] <= max(1.5e-2, 1.5 * rep["grad_vector_rel_bf16_oracle"]), rep
    return dev


def test_table_and_init(setup):
    """The magnitudes are ordinary trainable entries behind conv_out.bias, one contiguous range; after init_lora m = bf16(row norm), so
    every gain is within 2^-8 of 1 (not exactly 1) and the prediction stays within that of the base model's."""
    pc, oc, params, base, _ = setup
    unet, spec = _unet(setup, "transformer")
    unet.init_lora(42)
    names = [n for n, _ in unet.named_parameters()]
    nb = len(base._table)
    assert names[:nb] == [n for n, _ in base._table] and len(names) - nb == 3 * 192
    assert all(unet._slots[n] == base._slots[n] for n, _ in base._table)
    assert set(unet.lora_state_dict()) == set(names[nb:]) and sum(n.endswith(".dora_scale") for n in names) == 192
    tr = unet.trainable_ranges()
    assert len(tr) == 1 and tr[0][0] == unet._slots[names[nb]][0]
    g = unet.dora.g.cpu()
    assert float((g - 1.0).abs().max()) <= 2.0 ** -8 + 2.0 ** -22 and bool((g != 1.0).any())
    for n, p in unet.named_parameters():
        if n.endswith(".dora_scale"):
            Wt = params[n[:-len(".dora_scale")] + ".weight"].double()
            assert torch.equal(p.detach().cpu(), Wt.norm(dim=1).float().bfloat16()) or \
                float((p.detach().float().cpu().double() / Wt.norm(dim=1) - 1).abs().max()) <= 2.0 ** -8, n
    _, dev = _args(pc)
    l0, p0, _ = _micro(base, dev)
    l1, p1, _ = _micro(unet, dev)
    assert _rel(p1.float().cpu(), p0.float().cpu()) <= 1.5e-2 and abs(l1 - l0) <= 3e-3 * abs(l0)
    unet.expose_grads()
    lo = unet._slots["conv_out.bias"][0] + 64
    assert not bool(unet.gflat[:lo].any()), "a frozen base parameter received a gradient"
    gp = dict(unet.named_parameters())
    assert all(not bool(gp[n].grad.any()) for n in names[nb:] if n.endswith(".lora_A.weight"))          # dA = 0 while B = 0
    assert any(bool(gp[n].grad.any()) for n in names[nb:] if n.endswith(".dora_scale"))


@pytest.mark.parametrize("key", list(SPECS))
def test_matches_the_oracle(setup, key):
    unet, spec = _unet(setup, key)
    lsd = _perturb(unet)
    _parity(setup, unet, spec, lsd)
    n_mod = sum(n.endswith(".dora_scale") for n in lsd)
    assert len(lsd) == 3 * n_mod and n_mod == {"attention": 136, "transformer": 192, "q-and-v": 68}[key]


def test_new_gains_follow_load_lora_state_dict(setup):
    """Changed A, B and m: the next forward reads gains of the new values (one pass per load), checked against the oracle."""
    unet, spec = _unet(setup, "attention")
    _perturb(unet, seed=5)
    before = unet.dora.g.clone()
    n0 = unet.dora.launches
    g = torch.Generator().manual_seed(77)
    sd = {n: t.float().cpu() for n, t in unet.lora_state_dict().items()}
    for n in sd:
        if n.endswith(".lora_A.weight"):
            sd[n] = (sd[n] * 1.5).bfloat16().float()
        elif n.endswith(".lora_B.weight"):
            sd[n] = (0.05 * torch.randn(sd[n].shape, generator=g)).bfloat16().float()
        else:
            sd[n] = (sd[n] * (1.0 + 0.3 * torch.rand(sd[n].shape, generator=g))).bfloat16().float()
    unet.load_lora_state_dict(sd)
    assert unet.dora.launches == n0 + 1 and not torch.equal(unet.dora.g, before)
    _parity(setup, unet, spec, sd)


@pytest.mark.parametrize("key", ["transformer", "q-and-v"])
def test_replay_is_bitwise_and_accumulation_doubles(setup, key):
    from aozora_sdxl_training_amd.train_step import TrainStep
    pc = setup[0]
    unet, spec = _unet(setup, key)
    _, dev = _args(pc, seed=11)
    _perturb(unet)
    passes = unet.dora.launches
    unet.zero_grad()
    eager = TrainStep(unet, mode="epsilon", grad_accum=2, use_graph=False)
    l0 = eager.micro_step(*dev).item()
    eager.synchronize()
    g1 = unet.gflat.clone()
    eager.micro_step(*dev); eager.synchronize()
    g2 = unet.gflat.clone()
    assert bool(g1.any()) and _rel(g2, 2 * g1.float()) < 8e-3
    scales = [unet._slots[n][0] for n, _ in unet.named_parameters() if n.endswith(".dora_scale")]
    idx = torch.tensor(scales, device=DEV)
    assert bool(g1[idx].any()) and _rel(g2[idx], 2 * g1[idx].float()) < 8e-3
    graphed = TrainStep(unet, mode="epsilon", grad_accum=2, use_graph=True)
    for i in range(3):                 # run 0 eager (allocates), runs 1 and 2 replay the recorded step
        unet.zero_grad()
        l = graphed.micro_step(*dev).item()
        graphed.synchronize()
        assert torch.equal(unet.gflat, g1), f"replay {i} differs from the eager step"
        assert l == l0
    assert unet.dora.launches == passes, "a micro-step issued the norm pass"


def _recorded(unet, dev):
    from aozora_sdxl_training_amd._lib import lib
    L = lib()
    L.recorder = []
    try:
        loss, pred, _ = _micro(unet, dev)
    finally:
        names, L.recorder = [getattr(op, "name", None) for op in L.recorder], None
    return names, loss, pred


def test_without_dora_nothing_changes(setup):
    """LoraSpec(dora=False) against a spec built without the field: the same launch list, the same activation_bytes(), the same bits, no
    DoRA state; and with DoRA the fused GEGLU kernels are not issued."""
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    pc, oc, params, base, _ = setup
    dev = _args(pc)[1]
    runs = []
    for spec in (LoraSpec(RANK, ALPHA, "", "transformer"), LoraSpec(RANK, ALPHA, "", "transformer", dora=False)):
        unet = AozoraUNet(pc, DEV, lora=spec).load_state_dict(params)
        unet.init_lora(42)
        for n, p in unet.named_parameters():
            p.requires_grad = ".lora_" in n
        assert unet.dora is None and unet.adapters.dora is None
        names, loss, pred = _recorded(unet, dev)
        runs.append((names, loss, pred, unet.activation_bytes(), unet.gflat.clone()))
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2]) and a[3] == b[3] and torch.equal(a[4], b[4])
    assert not any(n is not None and n.startswith("az_dora") for n in a[0])
    unet, _ = _unet(setup, "transformer")
    names, _, _ = _recorded(unet, dev)
    assert names.count("az_lora_up_geglu_bf16") == 0 and names.count("az_gemm_geglu_fwd_bf16") == 0 and names.count("az_geglu_fwd") == 17
    assert names.count("az_dora_norm_bf16") == 0 and names.count("az_dora_scale_bf16") > 0 and names.count("az_dora_bwd_bf16") > 0
    print("activation_bytes: LoRA", a[3], "DoRA", unet.activation_bytes())
