"""lora_norm.LoraMaxNorm on AozoraUNet(lora=LoraSpec(..., scope="unet")) at the mini configuration with rank != conv_rank and random up
matrices: after apply() every module's float64 || s B A || is within the limit up to a derived bound, modules under the limit are
bitwise unchanged, the landed statistics agree with float64, and a forward + backward after the pass is bitwise that of a fresh UNet
loaded with the scaled adapters -- the W^T mirror was refreshed behind the pass."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import lora_maxnorm_ref as N                                              # noqa: E402
from test_model_gpu import _mini                                          # noqa: E402
from test_lora_model_gpu import _args, _freeze_base, _gauss_b, _micro     # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RANK, ALPHA, CONV_RANK, CONV_ALPHA = 4, 8.0, 16, 4.0


def _mats(lsd, spec):
    """{module: (A float64 [r][K], B float64 [out][r], s)} of an adapter state dict."""
    out = {}
    for n, t in lsd.items():
        if n.endswith(".lora_A.weight"):
            m = n[:-len(".lora_A.weight")]
            A = t.double().cpu().numpy()
            out[m] = (A.reshape(A.shape[0], -1), lsd[m + ".lora_B.weight"].double().cpu().numpy(), spec.scale_of(m))
    return out


@pytest.fixture(scope="module")
def world():
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    from aozora_sdxl_training_amd.lora_norm import LoraMaxNorm
    from oracle.unet_ref import init_params
    pc, oc = _mini()
    params = {k: v.bfloat16().float() for k, v in init_params(oc, seed=1234).items()}
    spec = LoraSpec(RANK, ALPHA, "", "unet", CONV_RANK, CONV_ALPHA)
    unet = AozoraUNet(pc, DEV, lora=spec).load_state_dict(params)
    unet.init_lora(42)
    _freeze_base(unet)
    _gauss_b(unet, sigma=0.05)
    _, dev = _args(pc)
    _micro(unet, dev)                                   # the W^T mirror now holds the copies of the UNSCALED adapters and is clean
    before = {n: t.clone() for n, t in unet.lora_state_dict().items()}
    mats = _mats(before, spec)
    norms = np.sort([np.sqrt(N.n2_gram(A, B, s)) for A, B, s in mats.values()])
    # the limit sits in the widest relative gap between neighbouring norms of the middle third: between a third and two thirds of the
    # modules are above it, and none sits where the decision could go either way (asserted below, a condition on these inputs)
    lo3, hi3 = len(norms) // 3, 2 * len(norms) // 3
    k = lo3 + int(np.argmax(norms[lo3 + 1:hi3 + 1] / norms[lo3:hi3]))
    limit = float(np.sqrt(norms[k] * norms[k + 1]))
    mn = LoraMaxNorm(unet, limit)
    slot = mn.apply()
    torch.cuda.synchronize()
    return dict(pc=pc, params=params, spec=spec, unet=unet, dev=dev, before=before, mats=mats, limit=limit, mn=mn, slot=slot)


def test_every_module_is_within_the_limit(world):
    spec, unet, limit, mn = world["spec"], world["unet"], world["limit"], world["mn"]
    after = _mats(unet.lora_state_dict(), spec)
    stats = mn.landed(world["slot"]).numpy()
    assert mn.modules == list(world["mats"]) and len(mn.modules) == 192 + 2 * 17 + 11
    ranks = {A.shape[0] for A, _, _ in after.values()}
    assert ranks == {RANK, CONV_RANK}
    n_over = 0
    for i, m in enumerate(mn.modules):
        A0, B0, s = world["mats"][m]
        n0 = np.sqrt(N.n2_gram(A0, B0, s))
        bq = N.q_bound(A0, B0, s)
        # a condition on the inputs: no module sits where the decision could go either way
        assert abs(n0 / limit - 1.0) >= 10.0 * (N.n2_bound(A0, B0, s) / n0 ** 2 / 2.0 + N.U), m
        assert abs(float(stats[i, 0]) / n0 - 1.0) <= N.n2_bound(A0, B0, s) / n0 ** 2 / 2.0 * 1.01 + 2.0 * N.U, m
        A1, B1, _ = after[m]
        n1 = np.sqrt(N.n2_gram(A1, B1, s))
        # q is within bound_q of sqrt(limit / norm); A and B each carry one bf16 rounding per element (relative 2^-9 each, 2 * 2^-9 on a
        # term of the product B A, hence on its norm)
        assert n1 <= limit * (1.0 + 2.0 ** -8 + bq), (m, n1, limit)
        if n0 > limit:
            n_over += 1
            assert stats[i, 1] != 1.0 and abs(float(stats[i, 1]) / np.sqrt(limit / n0) - 1.0) <= bq, m
            assert n1 >= limit * (1.0 - 2.0 ** -8 - bq), m          # scaled TO the limit, not below it
        else:
            assert stats[i, 1] == 1.0
            for sfx in (".lora_A.weight", ".lora_B.weight"):
                assert torch.equal(unet.lora_state_dict()[m + sfx], world["before"][m + sfx]), m
    assert len(mn.modules) // 3 <= n_over <= 2 * len(mn.modules) // 3 + 1
    k, avg, mx = mn.summary(world["slot"])
    assert k == n_over and mx == pytest.approx(limit, rel=1e-6) and 0.0 < avg < limit
    lo = unet._slots["conv_out.bias"][0] + 64
    fresh_base = type(unet)(world["pc"], DEV).load_state_dict(world["params"])
    assert torch.equal(unet.pflat[:lo], fresh_base.pflat[:lo]), "a base parameter changed"


def test_step_after_the_pass_is_that_of_a_fresh_unet(world):
    from aozora_sdxl_training_amd.unet import AozoraUNet
    unet, dev = world["unet"], world["dev"]
    fresh = AozoraUNet(world["pc"], DEV, lora=world["spec"]).load_state_dict(world["params"])
    fresh.load_lora_state_dict({n: t.float().cpu() for n, t in unet.lora_state_dict().items()})
    _freeze_base(fresh)
    assert torch.equal(fresh.pflat, unet.pflat)
    l0, p0, _ = _micro(fresh, dev)
    l1, p1, _ = _micro(unet, dev)
    assert l0 == l1 and torch.equal(p0, p1)
    assert torch.equal(fresh.gflat, unet.gflat), "the backward read stale transposed copies of the scaled adapters"
    assert torch.equal(fresh.wtflat, unet.wtflat)
