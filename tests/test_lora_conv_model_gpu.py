"""AozoraUNet(lora=LoraSpec(..., scope="unet")) at the mini configuration (latent 8x8, B = 2: 128, 32 and 8 pixels on the three levels):
adapters on conv1, conv2 and conv_shortcut of every ResnetBlock2D beside those of scope "transformer".  The table layout, the B = 0
identity, that every adapter receives a gradient, parity with tests/lora_conv_ref.LoraConvRefUNet under the bounds of
tests/test_lora_model_gpu._oracle_parity (1.5e-2, 3e-3, max(1.5e-2, 1.5 x the bf16 oracle's own deviation)) with conv_rank equal to
and different from rank, the same at the odd latent 5x7 (35, 12 and 4 pixels per image: 3x4 and 2x2 grids on the lower levels), which
entry points an eager micro-step records under the shipped thresholds / with them moved to the other side / under scope
"transformer", replay and accumulation, and the adapter file round trip."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import lora_ref as LR                                                                            # noqa: E402
import lora_conv_ref as CR                                                                       # noqa: E402
from test_model_gpu import _mini, _rel                                                           # noqa: E402
from test_lora_model_gpu import _args, _freeze_base, _gauss_b, _micro, _oracle_parity            # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RANK, ALPHA, CONV_RANK, CONV_ALPHA = 4, 8.0, 8, 4.0
RESNETS, SHORTCUTS, LINEARS = 17, 11, 192      # of the mini configuration (tests/test_lora_conv_ref_cpu.py derives them)
CONV_ENTRIES = ("az_lora_conv_down_bf16", "az_lora_conv_dgrad_bf16", "az_lora_conv_wgrad_bf16")


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
    spec = LoraSpec(RANK, ALPHA, "", "unet", CONV_RANK, CONV_ALPHA)
    s = (pc, oc, params, base)
    return s + (_unet(s, spec), spec)


def _parity(monkeypatch, unet, spec, params, oc, pc, **kw):
    """_oracle_parity with the oracle that carries the convolutions' adapters too (each module at its own alpha / rank); at a latent
    size that is no multiple of 4, the one with tests/oddsize_ref.py's size-targeted upsamples."""
    ref = CR.LoraConvRefUNet if kw.get("h", 8) % 4 == 0 and kw.get("w", 8) % 4 == 0 else CR.LoraConvOddRefUNet
    monkeypatch.setattr(LR, "LoraRefUNet", lambda cfg, p, scale: ref(cfg, p, spec))
    return _oracle_parity(unet, spec, params, oc, pc, **kw)


def _recorded(fn):
    """The entry-point names fn() issues -> (names, fn's result)."""
    from aozora_sdxl_training_amd._lib import lib
    L = lib()
    L.recorder = []
    try:
        out = fn()
    finally:
        names, L.recorder = [getattr(op, "name", None) for op in L.recorder], None
    return names, out


def test_table_layout(setup):
    pc, oc, params, base, unet, spec = setup
    names = [n for n, _ in unet.named_parameters()]
    nb = len(base._table)
    assert names[:nb] == [n for n, _ in base._table] and names[nb - 1] == "conv_out.bias"
    assert all(".lora_" in n for n in names[nb:]) and len(names) - nb == 2 * (LINEARS + 2 * RESNETS + SHORTCUTS)
    assert names[nb] == "down_blocks.0.resnets.0.conv1.lora_A.weight" and names[-1] == "mid_block.resnets.1.conv2.lora_B.weight"
    assert all(unet._slots[n] == base._slots[n] for n, _ in base._table)                # the base slots keep their offsets
    assert set(unet.state_dict()) == set(base.state_dict()) and set(unet.lora_state_dict()) == set(names[nb:])
    tr = unet.trainable_ranges()
    assert len(tr) == 1 and tr[0][0] == unet._slots[names[nb]][0]                       # one contiguous trainable range: the adapters
    assert unet.region_bounds()[:2] == base.region_bounds()[:2]
    prm = dict(unet.named_parameters())
    a1, b1 = prm["down_blocks.1.resnets.0.conv1.lora_A.weight"], prm["down_blocks.1.resnets.0.conv1.lora_B.weight"]
    assert tuple(a1.shape) == (CONV_RANK, 64, 3, 3) and a1.stride() == (9 * 64, 1, 3 * 64, 64) and tuple(b1.shape) == (128, CONV_RANK)
    assert tuple(prm["down_blocks.1.resnets.0.conv_shortcut.lora_A.weight"].shape) == (RANK, 64)
    assert tuple(prm["down_blocks.1.attentions.0.proj_in.lora_A.weight"].shape) == (RANK, 128)


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
            moved.update(k for k in ("conv1", "conv2", "conv_shortcut", "proj_in") if n.endswith(k + ".lora_B.weight"))
    assert moved == {"conv1", "conv2", "conv_shortcut", "proj_in"}, moved


def test_every_adapter_receives_a_gradient(setup):
    pc, oc, params, base, unet, spec = setup
    _, dev = _args(pc, seed=5)
    _gauss_b(unet)
    _micro(unet, dev)
    unet.expose_grads()
    still = [n for n, p in unet.named_parameters() if ".lora_" in n and not bool(p.grad.any())]
    assert not still, f"adapters without a gradient: {still[:6]}"
    lo = unet._slots["conv_out.bias"][0] + 64
    assert not bool(unet.gflat[:lo].any()), "a frozen base parameter received a gradient"


@pytest.mark.parametrize("rank, alpha, conv_rank, conv_alpha", [(RANK, ALPHA, CONV_RANK, CONV_ALPHA), (16, 16.0, 16, None), (8, 8.0, 64, 16.0)],
                         ids=["rank4-conv8", "rank16-conv-default", "rank8-conv64"])
def test_matches_the_oracle_with_adapters(setup, monkeypatch, rank, alpha, conv_rank, conv_alpha):
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    pc, oc, params, base, unet0, spec0 = setup
    spec = LoraSpec(rank, alpha, "", "unet", conv_rank, conv_alpha)
    unet = unet0 if spec == spec0 else _unet(setup, spec, seed=3)
    names, _ = _recorded(lambda: _parity(monkeypatch, unet, spec, params, oc, pc))        # asserts that the oracle's gradient set is the adapter set
    assert len(unet.lora_state_dict()) == 2 * (LINEARS + 2 * RESNETS + SHORTCUTS)
    assert all(names.count(e) == 2 * RESNETS for e in CONV_ENTRIES)


def test_matches_the_oracle_at_an_odd_latent_size(setup, monkeypatch):
    pc, oc, params, base, unet, spec = setup
    _parity(monkeypatch, unet, spec, params, oc, pc, h=5, w=7)


def test_general_convolution_side_matches_the_oracle_and_is_recorded(setup, monkeypatch):
    """The thresholds moved so that all three gathered products go to az_conv2d_bf16 (Cout = conv_rank 8, s = 1): no az_lora_conv_*
    launch, 3 x 2 x 17 more launches of the general kernel, the same contract and the same bounds."""
    pc, oc, params, base, unet0, spec = setup
    dev = _args(pc)[1]
    _gauss_b(unet0)
    ours, _ = _recorded(lambda: _micro(unet0, dev))
    unet = _unet(setup, spec)
    unet.adapters.routes.CONV_DOWN_GEMM = unet.adapters.routes.CONV_DGRAD_GEMM = unet.adapters.routes.CONV_WGRAD_GEMM = ((0, 0),)
    names, _ = _recorded(lambda: _parity(monkeypatch, unet, spec, params, oc, pc))
    assert all(ours.count(e) == 2 * RESNETS and names.count(e) == 0 for e in CONV_ENTRIES)
    assert names.count("az_conv2d_bf16") == ours.count("az_conv2d_bf16") + 3 * 2 * RESNETS
    one = _unet(setup, spec)
    one.adapters.routes.CONV_DGRAD_GEMM = ((0, 0),)          # each rule moves its own product only
    names, _ = _recorded(lambda: _micro(one, dev))
    assert [names.count(e) for e in CONV_ENTRIES] == [2 * RESNETS, 0, 2 * RESNETS]
    one.adapters.routes.CONV_DGRAD_GEMM = ((0, 16),)         # ... from its rank on: conv_rank 8 stays with the adapter kernel
    names, _ = _recorded(lambda: _micro(one, dev))
    assert [names.count(e) for e in CONV_ENTRIES] == [2 * RESNETS] * 3


def test_rank_4_stays_with_the_adapter_kernels(setup):
    """The general kernel cannot take Cout = 4: whatever the thresholds say, conv_rank 4 is az_lora_conv_*."""
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    pc, oc, params, base, _, _ = setup
    unet = _unet(setup, LoraSpec(8, 8.0, "resnets", "unet", 4, 4.0))
    unet.adapters.routes.CONV_DOWN_GEMM = unet.adapters.routes.CONV_DGRAD_GEMM = unet.adapters.routes.CONV_WGRAD_GEMM = ((0, 0),)
    _gauss_b(unet)
    names, _ = _recorded(lambda: _micro(unet, _args(pc)[1]))
    assert all(names.count(e) == 2 * RESNETS for e in CONV_ENTRIES)
    unet.expose_grads()
    assert all(bool(p.grad.any()) for n, p in unet.named_parameters() if ".lora_" in n)


def test_scope_transformer_records_nothing_new(setup):
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    pc, oc, params, base, unet, spec = setup
    dev = _args(pc)[1]
    tr = _unet(setup, LoraSpec(RANK, ALPHA, "", "transformer"))
    _gauss_b(tr)
    names, _ = _recorded(lambda: _micro(tr, dev))
    assert not any(e in names for e in CONV_ENTRIES)
    _gauss_b(unet)
    mine, _ = _recorded(lambda: _micro(unet, dev))
    for e in ("az_conv2d_bf16", "az_gemm_bf16", "az_groupnorm_fwd", "az_groupnorm_bwd_ex", "az_attn_fwd", "az_attn_bwd", "az_lora_up_geglu_bf16"):
        assert mine.count(e) == names.count(e), e          # s = 2, rank 4: every adapter product of both scopes is an az_lora_* launch
    assert all(mine.count(e) == 2 * RESNETS for e in CONV_ENTRIES)
    assert tr._pool.count() < unet._pool.count()      # u and du of 34 convolutions and 11 shortcuts


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
    path = lora.save_lora_file(tmp_path / "conv.safetensors", unet)
    n_mod = LINEARS + 2 * RESNETS + SHORTCUTS
    with safe_open(str(path), framework="pt", device="cpu") as f:
        keys = set(f.keys())
        assert len(keys) == 3 * n_mod and sum(k.endswith("_in_layers_2.lora_down.weight") for k in keys) == RESNETS
        assert sum(k.endswith("_out_layers_3.lora_up.weight") for k in keys) == RESNETS and sum(k.endswith("_skip_connection.alpha") for k in keys) == SHORTCUTS
        k = lora.file_key("down_blocks.1.resnets.0.conv1")
        down = f.get_tensor(k + ".lora_down.weight")
        assert tuple(down.shape) == (CONV_RANK, 64, 3, 3) and tuple(f.get_tensor(k + ".lora_up.weight").shape) == (128, CONV_RANK, 1, 1)
        assert torch.equal(down.float(), lsd["down_blocks.1.resnets.0.conv1.lora_A.weight"]) and float(f.get_tensor(k + ".alpha")) == CONV_ALPHA
        assert float(f.get_tensor(lora.file_key("down_blocks.1.resnets.0.conv_shortcut") + ".alpha")) == ALPHA
    fresh = _unet(setup, spec, seed=1)
    fresh.load_lora_state_dict(lora.read_lora_file(path, fresh))
    got = fresh.lora_state_dict()
    assert set(got) == set(lsd) and all(torch.equal(got[n].float().cpu(), lsd[n]) for n in lsd)
    assert torch.equal(fresh.pflat, unet.pflat)
