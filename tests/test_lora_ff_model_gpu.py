"""AozoraUNet(lora=LoraSpec(..., scope="transformer")) at the mini configuration (latent 8x8, B = 2: 8 and 32 token rows, H = 512 /
1024 at the GEGLU): adapters on proj_in, the eight attention projections, ff.net.0.proj, ff.net.2 and proj_out.  The table layout,
the B = 0 identity, parity with tests/lora_ref.LoraRefUNet under the bounds of tests/test_lora_model_gpu._oracle_parity (1.5e-2,
3e-3, max(1.5e-2, 1.5 x the bf16 oracle's own deviation)) at two ranks, which launches carry the adapted GEGLU projection under the
default policy / geglu_fuse=False / narrowed targets, the fused az_lora_up_geglu_bf16 against the two-launch form bit for bit,
replay and accumulation, and the adapter file round trip."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from test_model_gpu import _mini, _rel                                                           # noqa: E402
from test_lora_model_gpu import _args, _freeze_base, _gauss_b, _micro, _oracle_parity            # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RANK, ALPHA = 4, 8.0
BLOCKS, TRANSFORMERS = 17, 11   # BasicTransformerBlocks and Transformer2DModels of the mini configuration
FUSED, FUSED_GEMM = "az_lora_up_geglu_bf16", "az_gemm_geglu_fwd_bf16"


def _unet(setup, spec, policy=None, seed=42):
    from aozora_sdxl_training_amd.unet import AozoraUNet
    pc, oc, params, base = setup[:4]
    unet = AozoraUNet(pc, DEV, policy=policy, lora=spec).load_state_dict(params)
    unet.init_lora(seed)
    _freeze_base(unet)
    return unet


@pytest.fixture(scope="module")
def setup():
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    from oracle.unet_ref import init_params
    pc, oc = _mini()
    params = {k: v.bfloat16().float() for k, v in init_params(oc, seed=1234).items()}
    base = AozoraUNet(pc, DEV).load_state_dict(params)
    spec = LoraSpec(RANK, ALPHA, "", "transformer")
    s = (pc, oc, params, base)
    return s + (_unet(s, spec), spec)


def _recorded(unet, dev):
    """The entry-point names one eager micro-step issues -> (names, loss, prediction)."""
    from aozora_sdxl_training_amd._lib import lib
    L = lib()
    L.recorder = []
    try:
        loss, pred, _ = _micro(unet, dev)
    finally:
        names, L.recorder = [getattr(op, "name", None) for op in L.recorder], None
    return names, loss, pred


def test_table_layout(setup):
    pc, oc, params, base, unet, spec = setup
    names = [n for n, _ in unet.named_parameters()]
    nb = len(base._table)
    assert names[:nb] == [n for n, _ in base._table] and names[nb - 1] == "conv_out.bias"
    assert all(".lora_" in n for n in names[nb:]) and len(names) - nb == 384            # 2 x (17 blocks x 10 linears + 11 x 2)
    assert names[nb].endswith(".proj_in.lora_A.weight") and names[-1].endswith(".proj_out.lora_B.weight")
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
    moved = set()
    for i, (n, p) in enumerate(unet.named_parameters()):
        if i < nb:
            assert p.grad is None, n
        elif n.endswith(".lora_A.weight"):
            assert not bool(p.grad.any()), n + ": dA must be zero while B = 0"
        elif bool(p.grad.any()):
            moved.update(k for k in ("ff.net.0.proj", "ff.net.2", "proj_in", "proj_out") if n.endswith(k + ".lora_B.weight"))
    assert moved == {"ff.net.0.proj", "ff.net.2", "proj_in", "proj_out"}, moved


@pytest.mark.parametrize("rank, alpha", [(4, 8.0), (16, 16.0)], ids=["rank4-alpha8", "rank16-alpha16"])
def test_matches_the_oracle_with_adapters(setup, rank, alpha):
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    pc, oc, params, base, unet0, spec0 = setup
    spec = LoraSpec(rank, alpha, "", "transformer")
    unet = unet0 if spec == spec0 else _unet(setup, spec, seed=3)
    _oracle_parity(unet, spec, params, oc, pc)         # asserts that the oracle's gradient set is the adapter set
    assert len(unet.lora_state_dict()) == 384


def test_default_policy_issues_the_fused_kernel_once_per_block(setup):
    pc, oc, params, base, unet, spec = setup
    _gauss_b(unet)
    names, _, _ = _recorded(unet, _args(pc)[1])
    assert names.count(FUSED) == BLOCKS and names.count(FUSED_GEMM) == 0


def test_unfused_policy_and_narrowed_targets_keep_their_launches(setup):
    from aozora_sdxl_training_amd.unet import ExecPolicy
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    pc, oc, params, base, _, spec = setup
    dev = _args(pc)[1]
    names, _, _ = _recorded(_unet(setup, spec, policy=ExecPolicy(geglu_fuse=False)), dev)
    assert names.count(FUSED) == 0 and names.count(FUSED_GEMM) == 0 and names.count("az_geglu_fwd") == BLOCKS
    narrowed = _unet(setup, LoraSpec(RANK, ALPHA, "ff.net.2, proj_out", "transformer"))
    lsd = narrowed.lora_state_dict()
    assert len(lsd) == 2 * (BLOCKS + TRANSFORMERS) and all(".ff.net.2.lora_" in n or ".proj_out.lora_" in n for n in lsd)
    names, _, _ = _recorded(narrowed, dev)
    assert names.count(FUSED) == 0 and names.count(FUSED_GEMM) == BLOCKS


def test_unit_scale_takes_the_two_launch_form_where_the_general_product_is_faster(setup):
    """rank 16, alpha 16 (s = 1): at the mini configuration's 32 and 128 rows the up product is az_lora_up_bf16's and the fused kernel
    carries it (the parity test above runs that side).  With the few-row threshold lowered below them the rule of
    lora_exec.LoraRoutes.up_geglu sends the up product to the general product, as at the model's 4096 and 16384 rows, and az_geglu_fwd
    follows: same contract, same bounds."""
    from aozora_sdxl_training_amd._lib import lib
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    pc, oc, params, base, _, _ = setup
    spec = LoraSpec(16, 16.0, "", "transformer")
    unet = _unet(setup, spec, seed=3)
    names, _, _ = _recorded(unet, _args(pc)[1])
    assert names.count(FUSED) == BLOCKS and names.count("az_geglu_fwd") == 0
    unet.adapters.routes.UP_FEW_ROWS = 0
    L = lib()
    L.recorder = []
    try:
        _oracle_parity(unet, spec, params, oc, pc)
    finally:
        names, L.recorder = [getattr(op, "name", None) for op in L.recorder], None
    assert names.count(FUSED) == 0 and names.count(FUSED_GEMM) == 0 and names.count("az_geglu_fwd") == BLOCKS


def test_fused_equals_the_two_launch_form(setup):
    """rank 4, alpha 8 (s = 2): both sides take az_lora_up_bf16's arithmetic for the up product of ff.net.0.proj, so the fused kernel and
    az_lora_up_bf16 + az_geglu_fwd must agree on every bit of the prediction, the loss and every adapter gradient."""
    from aozora_sdxl_training_amd.unet import ExecPolicy
    pc, oc, params, base, unet, spec = setup
    dev = _args(pc, seed=13)[1]
    lsd = _gauss_b(unet)
    other = _unet(setup, spec, policy=ExecPolicy(geglu_fuse=False))
    other.load_lora_state_dict(lsd)
    la, pa, _ = _micro(unet, dev)
    lb, pb, _ = _micro(other, dev)
    assert la == lb and torch.equal(pa, pb)
    unet.expose_grads(); other.expose_grads()
    ga, gb = dict(unet.named_parameters()), dict(other.named_parameters())
    for n in lsd:
        assert torch.equal(ga[n].grad, gb[n].grad), n
    assert all(bool(ga[n].grad.any()) for n in lsd if ".ff.net.0.proj." in n)


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


def test_adapter_file_round_trip(setup, tmp_path):
    from safetensors import safe_open
    from aozora_sdxl_training_amd import lora
    pc, oc, params, base, unet, spec = setup
    lsd = {k: v.clone() for k, v in _gauss_b(unet, seed=9).items()}
    path = lora.save_lora_file(tmp_path / "ff.safetensors", unet)
    with safe_open(str(path), framework="pt", device="cpu") as f:
        keys = set(f.keys())
    assert len(keys) == 3 * 192 and sum(k.endswith("_ff_net_0_proj.lora_up.weight") for k in keys) == BLOCKS
    assert sum(k.endswith("_proj_in.alpha") for k in keys) == TRANSFORMERS and sum(k.endswith("_ff_net_2.lora_down.weight") for k in keys) == BLOCKS
    fresh = _unet(setup, spec, seed=1)
    fresh.load_lora_state_dict(lora.read_lora_file(path, fresh))
    got = fresh.lora_state_dict()
    assert set(got) == set(lsd) and all(torch.equal(got[n].float().cpu(), lsd[n]) for n in lsd)
    assert torch.equal(fresh.pflat, unet.pflat)
