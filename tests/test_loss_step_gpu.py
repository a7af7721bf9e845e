"""TrainStep(..., loss=...) on the mini UNet (16 x 16 latents, B = 2): the robust-loss launch of the step gives, bit for bit, what
az_robust_loss_fwd_bwd gives when called on its own on the step's prediction and target, with the widths c_b that loss.loss_widths
states, in all three prediction types; eager issue, Python tape replay and the native tape agree bit for bit; and with loss="MSE" the
recorded launch tape is the one the step records without the argument."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
B, H, W = 2, 16, 16


@pytest.fixture(scope="module")
def unet():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import mini_config, param_table
    cfg = mini_config()
    g = torch.Generator().manual_seed(1234)
    sd = {}
    for n, s in param_table(cfg):
        if "norm" in n:
            sd[n] = (1 + 0.1 * torch.randn(*s, generator=g)) if n.endswith("weight") else 0.1 * torch.randn(*s, generator=g)
        else:
            sd[n] = torch.randn(*s, generator=g) * 0.05
    u = AozoraUNet(cfg, DEV)
    u.load_state_dict(sd)
    return u


def _args(unet, seed=7):
    g = torch.Generator().manual_seed(seed)
    cfg = unet.cfg
    lat = torch.randn(B, 4, H, W, generator=g).bfloat16()
    noise = torch.randn(B, 4, H, W, generator=g)
    ctx = torch.randn(B, 77, cfg.cross_attention_dim, generator=g).bfloat16()
    pooled = torch.randn(B, cfg.pooled_dim, generator=g).bfloat16()
    tid = torch.tensor([[H * 8, W * 8, 0, 0, H * 8, W * 8]] * B, dtype=BF16)
    ts = torch.tensor([37, 911])
    jit = torch.rand(B, generator=g)
    return (lat.to(DEV), noise.to(DEV), ts, ctx.to(DEV), pooled.to(DEV), tid.to(DEV), jit), ts, jit


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("mode,loss", [("epsilon", "huber:c=0.3"), ("v_prediction", "huber:c=0.3"), ("rectified_flow", "huber:c=0.3"),
                                       ("epsilon", "smooth_l1:c=0.2,schedule=exponential"), ("v_prediction", "l1")])
def test_step_loss_launch_equals_the_kernel_called_on_its_own(unet, mode, loss):
    from aozora_sdxl_training_amd import ops
    from aozora_sdxl_training_amd.loss import loss_widths, parse_loss_type
    from aozora_sdxl_training_amd.train_step import TrainStep
    spec = parse_loss_type(loss, mode)
    args, ts, jit = _args(unet)
    curve = torch.linspace(0.5, 1.5, 1000)
    step = TrainStep(unet, mode=mode, grad_accum=2, use_graph=False, loss_curve=curve, loss=loss)
    unet.zero_grad()
    out = step.micro_step(*args)
    step.synchronize()
    torch.cuda.synchronize()
    bk = step.last_bucket
    assert bk.dev.shape[0] == (5 if spec.needs_c else 4)
    if spec.needs_c:
        want_c = loss_widths(spec, mode, ts, jit)
        assert torch.equal(bk.dev[4].cpu(), want_c) and bool((want_c[0] != want_c[1]).item())
    assert torch.equal(bk.dev[3].cpu(), curve[ts])
    C = bk.lat.shape[1]
    loss2 = torch.full((1,), -1.0, dtype=F32, device=DEV)
    per2 = torch.zeros(B, dtype=F32, device=DEV)
    dp2 = torch.zeros(B, H, W, 8, dtype=BF16, device=DEV)
    ops.robust_loss_fwd_bwd(spec.kind, bk.pred.view(B, H, W, C), bk.target, bk.dev[3], bk.dev[4] if spec.needs_c else None, 1.0 / 2, loss2, per2, dp2)
    torch.cuda.synchronize()
    assert out is bk.loss and float(loss2) > 0.0
    assert bool((bits(bk.loss) == bits(loss2)).all()) and bool((bits(bk.per_sample) == bits(per2)).all())
    assert bool((bits(bk.dpred8) == bits(dp2)).all()) and bool((bits(bk.dpred8[..., C:]) == 0).all()) and float(dp2.float().abs().max()) > 0
    # ... and it is not the squared error
    loss3, per3 = torch.zeros(1, dtype=F32, device=DEV), torch.zeros(B, dtype=F32, device=DEV)
    ops.mse_loss_fwd_bwd(bk.pred.view(B, H, W, C), bk.target, bk.dev[3], 1.0 / 2, loss3, per3, None)
    assert abs(float(loss3) - float(loss2)) > 1e-3 * float(loss3)
    assert float(unet.gflat.float().abs().max()) > 0


def test_eager_python_replay_and_native_tape_agree_under_a_robust_loss(unet):
    """As test_native_launch_tape_equals_python_replay_and_eager (tests/test_model_gpu.py), with loss="huber": loss and the whole
    gradient buffer bit-identical between eager issue (window 1), Python replay and native replay (windows 2-3)."""
    from aozora_sdxl_training_amd.train_step import TrainStep
    args, _, _ = _args(unet)

    def window(step):
        unet.zero_grad()
        losses = [step.micro_step(*args).item() for _ in range(2)]
        step.synchronize()
        return losses, unet.gflat.clone()
    ref = None
    for native in (False, True):
        step = TrainStep(unet, mode="v_prediction", grad_accum=2, use_graph=False, loss="huber:c=0.3")
        step.native_tape = native
        outs = [window(step) for _ in range(3)]
        for l, g in outs:
            if ref is None:
                ref = (l, g)
            assert l == ref[0] and torch.equal(g, ref[1])
        bk = step.last_bucket
        assert bk.tape is not None
        names = [op.name for op in bk.tape if hasattr(op, "name")]
        assert names.count("az_robust_loss_fwd_bwd") == 1 and "az_mse_loss_fwd_bwd" not in names
        if native:
            nt = bk.ntape
            assert nt is not None and nt.n == len(bk.tape) and nt.n_calls > 100 and len(nt.callbacks) < 20
    assert ref[0][0] > 0 and float(ref[1].float().abs().max()) > 0


def _tape_of(unet, **kw):
    """The recorded tape of a fresh TrainStep (second run of its bucket) -> [(kind, name, words)], with the addresses of the bucket's
    own buffers (fresh allocations of every TrainStep) replaced by (buffer name, offset)."""
    from aozora_sdxl_training_amd._lib import Call
    from aozora_sdxl_training_amd.train_step import TrainStep
    args, _, _ = _args(unet)
    step = TrainStep(unet, mode="epsilon", grad_accum=2, use_graph=False, **kw)
    unet.zero_grad()
    losses = [step.micro_step(*args).item() for _ in range(2)]
    step.synchronize()
    bk = step.last_bucket
    assert bk.tape is not None
    own = {k: v for k, v in vars(bk).items() if isinstance(v, torch.Tensor) and v.is_cuda}
    assert {"lat", "noise", "ctx", "pooled", "dev", "x8", "target", "dpred8", "loss", "per_sample", "tids"} <= set(own)

    def word(a):
        a = getattr(a, "value", a)
        if a is None:
            return 0
        if isinstance(a, int):
            for k, t in own.items():
                if t.data_ptr() <= a < t.data_ptr() + max(1, t.numel() * t.element_size()):
                    return (k, a - t.data_ptr())
        return a
    out = []
    for op in bk.tape:
        if isinstance(op, Call) and op.name in ("az_set_launch_stop_event", "az_event_record", "az_stream_wait_event"):
            out.append(("call", op.name, tuple(bool(word(a)) for a in op.args)))     # event handles: armed or cleared, not which event
        elif isinstance(op, Call):
            out.append(("call", op.name, tuple(word(a) for a in op.args)))
        else:
            out.append((type(op).__name__, None, ()))
    return out, losses, tuple(bk.dev.shape), unet.gflat.clone()


def test_with_mse_the_tape_is_the_one_recorded_without_the_argument(unet):
    base, l0, shape0, g0 = _tape_of(unet)
    for spelling in ("MSE", "mse", None):
        t, l, shape, g = _tape_of(unet, loss=spelling)
        assert shape == shape0 == (4, B)                     # no fifth coefficient row
        assert [x[:2] for x in t] == [x[:2] for x in base]   # the same operations and entry names in the same order ...
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(t, base)) if a != b]
        assert not diff, diff[:3]                            # ... with the same arguments
        assert l == l0 and torch.equal(g, g0)
    names = [x[1] for x in base]
    assert names.count("az_mse_loss_fwd_bwd") == 1 and "az_robust_loss_fwd_bwd" not in names
    # min-SNR is folded into the curve by the caller: the step's launches stay the MSE ones
    t, _, shape, _ = _tape_of(unet, loss="MSE:min_snr_gamma=5")
    assert shape == (4, B) and t == base
