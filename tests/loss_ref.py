"""Restatement of the robust losses (csrc/az_elem.hip robust_loss_kernel: l1, huber, smooth_l1) with per-element error bounds, in the
manner of tests/elem_ref.py, whose bound / excess / half_ulp_bf16 it uses.  The product never imports this file;
tests/test_loss_gpu.py compares the HIP kernel against it and tests/test_loss_ref_cpu.py checks it (and derives the constants K
below) without a GPU.  Plain torch on the CPU.

Per element x = fp32(pred) - target and c = c_b of the sample:
    l1          l = |x|                                 l' = sign(x), +0 at 0
    huber       l = 2c x^2 / (sqrt(x^2 + c^2) + c)      l' = 2c x / sqrt(x^2 + c^2)
    smooth_l1   l = 2  x^2 / (sqrt(x^2 + c^2) + c)      l' = 2  x / sqrt(x^2 + c^2)
per_b = mean over (C, HW) of l, loss = (1/B) sum_b w_b per_b, dpred = k_b l'(x) with k_b = gscale w_b / (C HW B).  The float64
restatement uses the same cancellation-free spelling: in float64 it is exact to ~2^-52 for every input of the tests (c^2 + x^2 holds
both terms at c = 2^20), whereas 2c (sqrt(x^2 + c^2) - c) would lose x^2 / c^2 of its bits even there.

K: as elem_ref's -- the kernel's own formula in float32 torch (robust_f32: the operations of robust_elem one by one, the kernel's
summation order) against float64 over the test inputs, 4 x measured rounded up to a power of two, never below 1, the measured value
in brackets; tests/test_loss_ref_cpu.py requires K >= 4 x measured.  robust_f32(naive=True) is the difference spelling the kernel
must NOT use: the same file shows it outside the robust_mean bound on the tiny-residual and the huge-c inputs."""
import torch

import elem_ref as R

KINDS = {"l1": 1, "huber": 2, "smooth_l1": 3}

K = {
    "robust_dpred": 32.0,   # [4.06]  k (three fp32 operations), the difference, x^2, c^2, their sum, sqrt, the product and the quotient rounded
    "robust_mean": 16.0,    # [3.58]  l (the same operations) summed over HW * C terms: thread, block, sample
    "robust_loss": 16.0,    # [3.40]
}

# (B, C, HW, ldp, cpad): one pixel; both sides of a 256-thread block; more than one sweep (64 blocks x 256 threads); ldp != cpad != C
SHAPES = [(1, 4, 1, 4, 4), (3, 4, 255, 8, 8), (2, 4, 257, 4, 8), (2, 4, 16384 + 300, 8, 8)]
VARIANTS = ("unit", "tiny", "zero", "huge_c")
WEIGHTS = (1.3, 0.0, 0.7)                   # a zero weight among them
WIDTHS = (0.1, 0.37, 0.03)                  # per-sample c that differ
WIDTHS_HUGE = (2.0 ** 20, 0.1, 0.03)        # ... and one sample at which the pseudo-Huber loss is the squared error to 2^-42
GSCALE = 0.5


def bound(ref, S, k, rounding=None):
    return (R.half_ulp_bf16(ref) if rounding is None else rounding) + K[k] * R.U_F32 * S


def inputs(variant, B, C, HW, ldp):
    """-> pred [B][HW][ldp] bf16, target [B][C][HW] fp32, w [B] fp32, c [B] fp32.
    unit: Gaussian prediction and target; tiny: target = fp32(pred) + 2^-12 randn; zero: target = fp32(pred) exactly;
    huge_c: the unit data with c_0 = 2^20."""
    pred = R.gauss_bf16((B, HW, ldp), seed=HW)
    own = pred[..., :C].float().permute(0, 2, 1).contiguous()
    noise = torch.randn(B, C, HW, generator=R.gen(HW + 1))
    target = {"unit": noise, "huge_c": noise, "tiny": own + 2.0 ** -12 * noise, "zero": own}[variant]
    w = torch.tensor(WEIGHTS[:B])
    c = torch.tensor((WIDTHS_HUGE if variant == "huge_c" else WIDTHS)[:B], dtype=torch.float32)
    return pred, target.contiguous(), w, c


def elem(kind, x, c, naive=False):
    """(l, l') of residuals x with widths c (broadcastable) in the dtype of x -- float64: the restatement; float32: robust_elem's
    operations one by one (torch's float32 product, sum, quotient and sqrt are correctly rounded, as the kernel's are).
    naive: 2c (sqrt(x^2 + c^2) - c), the spelling that cancels."""
    if kind == "l1":
        return x.abs(), torch.sign(x)
    c = c.to(x.dtype)
    c2 = 2.0 * c if kind == "huber" else torch.full_like(c, 2.0)
    t = x * x
    r = torch.sqrt(t + c * c)
    l = c2 * (r - c) if naive else (c2 * t) / (r + c)
    return l, (c2 * x) / r


def robust_ref(kind, pred, target, w, c, gscale):
    """-> dict(dpred [B][HW][C], S_dpred, mean [B], S_mean, loss, S_loss) in float64 (as elem_ref.mse_ref)."""
    B, C, HW = target.shape
    x = pred[..., :C].double() - target.double().permute(0, 2, 1)
    l, dl = elem(kind, x, c.double()[:, None, None])
    k = gscale * w.double() / (C * HW * B)
    mean = l.sum((1, 2)) / (C * HW)
    # every term is a product / quotient of rounded values: relative to its own magnitude; the sums have positive terms only
    return dict(dpred=k[:, None, None] * dl, S_dpred=(k[:, None, None] * dl).abs(), mean=mean, S_mean=mean,
                loss=(mean * w.double()).sum() / B, S_loss=(mean * w.double().abs()).sum() / B)


def robust_f32(kind, pred, target, w, c, gscale, naive=False):
    """robust_loss_kernel / mse_finalize_kernel in float32 in their own order (as elem_ref.mse_f32): a thread's pixels and channels
    one after the other, the block, the sample's blocks one after the other."""
    B, C, HW = target.shape
    gx = min((HW + 255) // 256, 64)
    x = pred[..., :C].float() - target.permute(0, 2, 1)
    l, dl = elem(kind, x, c.float()[:, None, None], naive)
    k = (torch.tensor(gscale, dtype=torch.float32) * w) / (torch.tensor(float(C)) * float(HW) * float(B))
    sweep = gx * 256
    nsw = (HW + sweep - 1) // sweep
    ll = torch.zeros(B, nsw * sweep, C)
    ll[:, :HW] = l
    acc = torch.zeros(B, sweep)
    for s in range(nsw):
        for ch in range(C):
            acc = acc + ll[:, s * sweep:(s + 1) * sweep, ch]
    blocks = acc.reshape(B, gx, 256).sum(2)
    ps = torch.zeros(B)
    for j in range(gx):
        ps = ps + blocks[:, j]
    mean = ps / (torch.tensor(float(C)) * float(HW))
    loss = torch.zeros(())
    for b in range(B):
        loss = loss + mean[b] * w[b]
    return k[:, None, None] * dl, mean, loss / float(B)
