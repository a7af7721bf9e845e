"""LoRA dropout through AozoraUNet and TrainStep at the mini configuration (latent 8x8, B = 2, a 77-token context; scope "unet",
rank 4, conv_rank 8, the three dropouts at 0.5): prediction, loss and every adapter gradient against
tests/lora_dropout_ref.LoraDropoutRefUNet in fp32 under the bounds of tests/test_lora_model_gpu._oracle_parity and
tests/test_lora_conv_model_gpu.py (1.5e-2 relative, 3e-3, max(1.5e-2, 1.5 x the bf16 oracle's own deviation)), exact-zero gradients of
dropped modules, bitwise replay under the native tape and the captured graph with the step word rewritten, two accumulated micro-steps,
the launch sequence with dropout off, and the lora_step / __call__ refusals with the no-grad (eval) equality."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import lora_dropout_ref as D                                                     # noqa: E402
from test_model_gpu import _mini, _rel                                           # noqa: E402
from test_lora_model_gpu import _args, _gauss_b                                  # noqa: E402
from test_lora_conv_model_gpu import _unet, _recorded                            # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, H, W = 2, 8, 8
SEED = 42
RANK, ALPHA, CONV_RANK, CONV_ALPHA = 4, 8.0, 8, 4.0
ENTRY = "az_lora_dropout_bf16"


@pytest.fixture(scope="module")
def setup():
    """(pc, oc, params, unet with dropout, its spec, the adapters as CPU tensors, the reference's results).  The reference runs once:
    an accumulation window of two micro-steps (lora_step 1, then 2) in fp32 and in the bf16 oracle; its first half is the single step."""
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    from oracle.unet_ref import init_params
    from oracle.step_ref import RefTrainer
    pc, oc = _mini()
    params = {k: v.bfloat16().float() for k, v in init_params(oc, seed=1234).items()}
    spec = LoraSpec(RANK, ALPHA, "", "unet", CONV_RANK, CONV_ALPHA, 0.5, 0.5, 0.5)
    unet = _unet((pc, oc, params, None), spec)
    unet.set_lora_dropout_seed(SEED)
    lsd = _gauss_b(unet)
    cpu, _ = _args(pc)
    allp = dict(params); allp.update(lsd)
    ref = {}
    for bf16 in (False, True):
        tr = RefTrainer(oc, allp, mode="epsilon", bf16=bf16, ga=2, clip=1.0, frozen=tuple(params))
        tr.net = D.LoraDropoutRefUNet(oc, tr.params, spec, D.module_ids(pc), SEED, step=1)
        l1 = tr.micro_step(*cpu)
        g1 = {k: 2.0 * g.detach().float().clone() for k, g in tr.grads().items()}          # ga = 2 halves the seed: exact
        p1, seen1 = tr.last_pred.detach().clone(), dict(tr.net.seen)
        tr.net.step = 2
        l2 = tr.micro_step(*cpu)
        g12 = {k: g.detach().float().clone() for k, g in tr.grads().items()}
        ref[bf16] = dict(l1=float(l1), g1=g1, p1=p1, seen1=seen1, l2=float(l2), g12=g12, p2=tr.last_pred.detach().clone())
    assert set(ref[False]["g1"]) == set(lsd)
    return pc, oc, params, unet, spec, lsd, ref


def _step(unet, **kw):
    from aozora_sdxl_training_amd.train_step import TrainStep
    return TrainStep(unet, mode="epsilon", use_graph=False, **kw)


def _grad_rel(unet, g_ref, g_b):
    """(relative error of the adapter-gradient vector, the bf16 oracle's own) against the fp32 reference."""
    unet.expose_grads()
    sq_r = sq_d = sq_b = 0.0
    for n, p in unet.named_parameters():
        if ".lora_" not in n:
            continue
        gh, gr = p.grad.float().cpu(), g_ref[n]
        sq_r += gr.double().pow(2).sum().item()
        sq_d += (gh - gr).double().pow(2).sum().item()
        sq_b += (g_b[n] - gr).double().pow(2).sum().item()
    assert sq_r > 0
    return math.sqrt(sq_d / sq_r), math.sqrt(sq_b / sq_r)


def _nchw(pred_dev):
    return pred_dev.view(B, H, W, 4).permute(0, 3, 1, 2).float().cpu()


def test_matches_the_reference_and_dropped_modules_get_exact_zeros(setup):
    pc, oc, params, unet, spec, lsd, ref = setup
    _, dev = _args(pc)
    r32, r16 = ref[False], ref[True]
    seen = r32["seen1"]
    dropped, kept = [m for m, k in seen.items() if not k], [m for m, k in seen.items() if k]
    assert len(seen) == len(lsd) // 2 and dropped and kept, (len(dropped), len(kept))
    assert any("conv1" in m for m in dropped + kept) and any(".to_k" in m for m in dropped) and any(".to_k" in m for m in kept)
    unet.zero_grad()
    step = _step(unet, grad_accum=1)
    loss = step.micro_step(*dev, lora_step=1).item()
    step.synchronize()
    g, g_bf = _grad_rel(unet, r32["g1"], r16["g1"])
    rep = dict(pred_rel=_rel(_nchw(step.last_pred_nhwc), r32["p1"]), loss_hip=loss, loss_fp32=r32["l1"], grad_vector_rel=g,
               grad_vector_rel_bf16_oracle=g_bf, pred_rel_bf16_oracle=_rel(r16["p1"], r32["p1"]), dropped=len(dropped), kept=len(kept))
    print(rep)
    assert rep["pred_rel"] <= 1.5e-2, rep
    assert abs(loss - r32["l1"]) <= 3e-3 * abs(r32["l1"]), rep
    assert g <= max(1.5e-2, 1.5 * g_bf), rep
    prm = dict(unet.named_parameters())
    for m in dropped:       # u and du are selected to +0: the products add exact zeros, the gradients stay all-zero bits
        for leaf in (".lora_A.weight", ".lora_B.weight"):
            assert not bool(prm[m + leaf].grad.view(torch.int16).any()), m + leaf
            assert not bool(r32["g1"][m + leaf].any()), m + leaf
    assert sum(bool(prm[m + ".lora_B.weight"].grad.any()) for m in kept) >= len(kept) // 2


@pytest.mark.parametrize("use_graph", [False, True], ids=["native-tape", "graph"])
def test_replay_is_bitwise_and_follows_the_step_word(setup, use_graph):
    from aozora_sdxl_training_amd.train_step import TrainStep
    pc, oc, params, unet, spec, lsd, ref = setup
    _, dev = _args(pc)
    step = TrainStep(unet, mode="epsilon", grad_accum=1, use_graph=use_graph)
    outs = []
    for i, ls in enumerate((1, 1, 1, 2, 1)):          # run 0 allocates, run 1 is recorded / captured, runs 2.. are replays
        unet.zero_grad()
        loss = step.micro_step(*dev, lora_step=ls).item()
        step.synchronize()
        outs.append((loss, step.last_pred_nhwc.clone(), unet.gflat.clone()))
    bk = step.last_bucket
    assert (bk.graph is not None) if use_graph else (getattr(bk, "tape", None) is not None)
    for i in (1, 2, 4):
        assert outs[i][0] == outs[0][0] and torch.equal(outs[i][1], outs[0][1]) and torch.equal(outs[i][2], outs[0][2]), f"run {i} differs from run 0"
    assert not torch.equal(outs[3][1], outs[0][1]) and not torch.equal(outs[3][2], outs[0][2])      # another lora_step: other masks
    assert _rel(_nchw(outs[3][1]), ref[False]["p2"]) <= 1.5e-2


def test_two_accumulated_micro_steps_match_the_reference(setup):
    pc, oc, params, unet, spec, lsd, ref = setup
    _, dev = _args(pc)
    unet.zero_grad()
    step = _step(unet, grad_accum=2)
    l1 = step.micro_step(*dev, lora_step=1).item()
    l2 = step.micro_step(*dev, lora_step=2).item()
    step.synchronize()
    g, g_bf = _grad_rel(unet, ref[False]["g12"], ref[True]["g12"])
    rep = dict(l1=l1, l1_ref=ref[False]["l1"], l2=l2, l2_ref=ref[False]["l2"], grad_vector_rel=g, grad_vector_rel_bf16_oracle=g_bf)
    print(rep)
    assert abs(l1 - ref[False]["l1"]) <= 3e-3 * abs(ref[False]["l1"]) and abs(l2 - ref[False]["l2"]) <= 3e-3 * abs(ref[False]["l2"]), rep
    assert g <= max(1.5e-2, 1.5 * g_bf), rep


def test_dropout_off_issues_todays_launch_sequence(setup):
    """The three at 0: not one new launch.  With dropout: two more launches per adapter group and nothing else."""
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    pc, oc, params, unet, spec, lsd, ref = setup
    _, dev = _args(pc)
    plain_spec = LoraSpec(RANK, ALPHA, "", "unet", CONV_RANK, CONV_ALPHA, 0.0, 0.0, 0.0)
    assert plain_spec == LoraSpec(RANK, ALPHA, "", "unet", CONV_RANK, CONV_ALPHA) and not plain_spec.has_dropout
    plain = _unet((pc, oc, params, None), plain_spec)
    plain.load_lora_state_dict(lsd)

    def run(u, **kw):
        u.zero_grad()
        s = _step(u, grad_accum=1)
        s.micro_step(*dev, **kw)
        s.synchronize()
    run(plain)                     # a UNet's first TrainStep probes its stream pair: not part of a micro-step
    today, _ = _recorded(lambda: run(plain))
    mine, _ = _recorded(lambda: run(unet, lora_step=1))
    assert ENTRY not in today and len(today) > 1000
    groups = sum(1 for g in unet.adapters._groups.values() if g is not None)
    assert mine.count(ENTRY) == 2 * groups and groups == sum(1 for g in plain.adapters._groups.values() if g is not None) > 100
    assert [n for n in mine if n != ENTRY] == today


def test_refusals_and_eval_equality(setup):
    from aozora_sdxl_training_amd._lib import AozoraError
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    pc, oc, params, unet, spec, lsd, ref = setup
    cpu, dev = _args(pc)
    plain = _unet((pc, oc, params, None), LoraSpec(RANK, ALPHA, "", "unet", CONV_RANK, CONV_ALPHA))
    plain.load_lora_state_dict(lsd)
    with pytest.raises(AozoraError, match="lora_step"):
        _step(unet).micro_step(*dev)
    for bad in (True, 1.5, -1, 2 ** 31):
        with pytest.raises(AozoraError, match="lora_step"):
            _step(unet).micro_step(*dev, lora_step=bad)
    with pytest.raises(AozoraError, match="lora_step"):
        _step(plain).micro_step(*dev, lora_step=1)
    with pytest.raises(AozoraError, match="lora_step"):
        _step(AozoraUNet(pc, DEV).load_state_dict(params)).micro_step(*dev, lora_step=1)
    lat, noise, ts, ctx, pooled, tid, jit = cpu
    kw = dict(added_cond_kwargs={"text_embeds": pooled.to(DEV), "time_ids": tid.to(DEV)})
    with pytest.raises(AozoraError, match="TrainStep"):
        unet(lat.to(DEV), ts, ctx.to(DEV), **kw)
    with torch.no_grad():
        names, (a, b) = _recorded(lambda: [u(lat.to(DEV), ts, ctx.to(DEV), **kw).sample for u in (unet, plain)])
    torch.cuda.synchronize()
    assert ENTRY not in names and len(names) > 100          # eval: no masks
    assert torch.equal(a, b) and bool(a.float().abs().sum() > 0)
