"""weighted_sdxl_mse_loss -- the loss seam of the reference loop (train.py:2408-2416, called at train.py:2763) as a callable
on the HIP path, for callers that keep the reference's loop body verbatim:

    pred = unet(...).sample                       # (B,C,H,W) bf16, AozoraUNet.__call__
    loss = weighted_sdxl_mse_loss(pred, target, timesteps, timestep_loss_weights)
    (loss / GA).backward()

Forward and d(loss)/d(pred) come from ONE launch of az_mse_loss_fwd_bwd (the per-sample mean over (C,H,W) does not depend on
the element order, so the NCHW tensors are handed to the kernel as [B][1 channel][C*H*W]); backward scales the saved bf16
gradient by the incoming scalar with az_scale_bf16 (device-resident coefficient: no host sync).  TrainStep uses the same
kernel directly on the NHWC prediction; this wrapper exists for the drop-in seam.

LOSS_TYPE (an option outside the reference, whose presets carry the key and whose GUI offers "MSE" only): parse_loss_type reads
`kind[:key=value[,key=value...]]` -- kinds mse, l1, huber, smooth_l1; keys c, schedule, min_snr_gamma -- into a LossSpec, the one
parser of the trainer, TrainStep and weighted_sdxl_loss.  loss_widths is the per-sample width c_b of the pseudo-Huber kinds,
min_snr_factors / fold_min_snr the min-SNR-gamma factor of the 1000-entry loss-weight curve; the element math is az_robust_loss_fwd_bwd's
(INTEGRATION.md "Loss types")."""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple, Optional

import torch

from . import ops
from ._lib import lib
from .schedule import ddpm_alphas_cumprod

KINDS = ("mse", "l1", "huber", "smooth_l1")
SCHEDULES = ("snr", "constant", "exponential")
PREDICTION_TYPES = ("epsilon", "v_prediction", "rectified_flow")


class LossSpec(NamedTuple):
    kind: str                          # one of KINDS
    c: Optional[float]                 # width of huber / smooth_l1 (None for mse and l1)
    schedule: Optional[str]            # how c_b follows the timestep (None for mse and l1)
    min_snr_gamma: Optional[float]     # None: off

    @property
    def needs_c(self):
        return self.kind in ("huber", "smooth_l1")

    def describe(self):
        s = {"mse": "MSE", "l1": "L1", "huber": "pseudo-Huber", "smooth_l1": "smooth-L1"}[self.kind]
        if self.needs_c:
            s += f" (c = {self.c:g}, schedule {self.schedule})"
        return s + (f", min-SNR gamma = {self.min_snr_gamma:g}" if self.min_snr_gamma is not None else ", no min-SNR weighting")


def _positive(key, text):
    try:
        v = float(text)
    except ValueError:
        raise ValueError(f"LOSS_TYPE: {key}={text!r} is not a number") from None
    if not math.isfinite(v) or v <= 0.0:
        raise ValueError(f"LOSS_TYPE: {key} must be a finite number above 0, got {text!r}")
    return v


def parse_loss_type(s, prediction_type) -> LossSpec:
    """`kind[:key=value[,key=value...]]`, kind and keys in any letter case; None, "" and "MSE" are the squared error.  ValueError for
    an unknown kind or key, c or schedule on mse / l1, c <= 0 or not finite, and min_snr_gamma with rectified_flow."""
    if isinstance(s, LossSpec):
        spec = s
    else:
        text = "mse" if s is None or not str(s).strip() else str(s).strip()
        kind, _, rest = text.partition(":")
        kind = kind.strip().lower()
        if kind not in KINDS:
            raise ValueError(f"LOSS_TYPE: unknown loss {kind!r} (known: {', '.join(KINDS)})")
        opts = {}
        for item in (rest.split(",") if rest.strip() else []):
            key, eq, val = item.partition("=")
            key, val = key.strip().lower(), val.strip()
            if not eq or key not in ("c", "schedule", "min_snr_gamma") or key in opts:
                raise ValueError(f"LOSS_TYPE: cannot read {item.strip()!r} (keys: c, schedule, min_snr_gamma, each once, as key=value)")
            opts[key] = val
        wide = kind in ("huber", "smooth_l1")
        for key in ("c", "schedule"):
            if key in opts and not wide:
                raise ValueError(f"LOSS_TYPE: {key} belongs to huber and smooth_l1, not to {kind}")
        sched = opts.get("schedule", "snr").lower() if wide else None
        if wide and sched not in SCHEDULES:
            raise ValueError(f"LOSS_TYPE: unknown schedule {sched!r} (known: {', '.join(SCHEDULES)})")
        spec = LossSpec(kind, _positive("c", opts.get("c", "0.1")) if wide else None, sched,
                        _positive("min_snr_gamma", opts["min_snr_gamma"]) if "min_snr_gamma" in opts else None)
    if spec.min_snr_gamma is not None and prediction_type not in ("epsilon", "v_prediction"):
        raise ValueError(f"LOSS_TYPE: min_snr_gamma is defined for epsilon and v_prediction, not for {prediction_type!r}")
    return spec


def _snr_table():
    """SNR_t = abar_t / (1 - abar_t) of the 1000 DDPM timesteps, float64."""
    ac = ddpm_alphas_cumprod().double()
    return ac / (1.0 - ac)


def loss_widths(spec: LossSpec, prediction_type, timesteps, jitter=None):
    """c_b of every sample, float64 on the host and rounded to fp32 once -> fp32 [B] (CPU).  tau_b = t_b / 1000 for the DDPM modes,
    clamp((t_b + jitter_b) / 1000, 0, 1) for rectified flow.  constant: c; exponential: exp(ln(c) tau); snr: (1 - c) / (1 + sigma)^2 + c
    with sigma = sqrt((1 - abar_t) / abar_t) (DDPM) or tau / (1 - tau) (rectified flow; tau = 1 gives c)."""
    if not spec.needs_c:
        raise ValueError(f"the {spec.kind} loss has no width")
    t = torch.as_tensor(timesteps).detach().cpu().double()
    c = float(spec.c)
    if spec.schedule == "constant":
        return torch.full(t.shape, c, dtype=torch.float64).float()
    rf = prediction_type == "rectified_flow"
    if rf:
        if jitter is None:
            raise ValueError("rectified_flow needs the jitter tensor (train.py:2744-2745)")
        tau = ((t + torch.as_tensor(jitter).detach().cpu().double()) / 1000.0).clamp(0.0, 1.0)
    else:
        tau = t / 1000.0
    if spec.schedule == "exponential":
        return torch.exp(math.log(c) * tau).float()
    if rf:
        inv = (1.0 - tau) ** 2                                # 1 / (1 + sigma)^2 = (1 - tau)^2, 0 at tau = 1
    else:
        snr = _snr_table()[t.long().clamp(0, 999)]
        inv = 1.0 / (1.0 + torch.sqrt(1.0 / snr)) ** 2
    return ((1.0 - c) * inv + c).float()


def min_snr_factors(gamma, prediction_type):
    """m_t of the 1000 timesteps, float64: min(SNR_t, gamma) / SNR_t for epsilon, min(SNR_t, gamma) / (SNR_t + 1) for v_prediction."""
    if prediction_type not in ("epsilon", "v_prediction"):
        raise ValueError(f"min_snr_gamma is defined for epsilon and v_prediction, not for {prediction_type!r}")
    snr = _snr_table()
    return snr.clamp(max=float(gamma)) / (snr if prediction_type == "epsilon" else snr + 1.0)


def fold_min_snr(curve, spec: LossSpec, prediction_type):
    """The per-timestep loss weights (fp32 [1000]) times m_t when the spec asks for min-SNR weighting (the product in float64,
    rounded to fp32 once); the curve itself otherwise."""
    if spec.min_snr_gamma is None:
        return curve
    return (curve.double().cpu() * min_snr_factors(spec.min_snr_gamma, prediction_type)).float()


class _WeightedMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, w):
        B = pred.shape[0]
        n = pred[0].numel()
        dev = pred.device
        p2 = pred.contiguous().view(B, 1, n, 1)                    # "NHWC" with H*W = C*H*W rows of one channel
        t2 = target.contiguous().view(B, 1, 1, n)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        per = torch.empty(B, dtype=torch.float32, device=dev)
        dpred = torch.empty(B, 1, n, 1, dtype=torch.bfloat16, device=dev)
        ops.mse_loss_fwd_bwd(p2, t2, w, 1.0, loss, per, dpred)
        ctx.save_for_backward(dpred)
        ctx.shape = pred.shape
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        out = dpred.clone()
        coef = g.detach().to(torch.float32).reshape(1).contiguous()
        lib().call("az_scale_bf16", out.numel(), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(coef.data_ptr()),
                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        return out.view(ctx.shape), None, None


def weighted_sdxl_mse_loss(pred, target, timesteps, timestep_loss_weights=None):
    """train.py:2408-2416.  pred (B,C,H,W) bf16 on the HIP device (differentiable), target (B,C,H,W) any float dtype,
    timesteps (B,) integer, timestep_loss_weights None or a 1-D curve indexed by clamp(timestep, 0, len-1).  Returns the 0-d
    fp32 loss: mean over the batch of weight * mean over (C,H,W) of the squared error (fp32 accumulation)."""
    if not pred.is_cuda or pred.dtype != torch.bfloat16:
        raise ops.AozoraError("weighted_sdxl_mse_loss (HIP) needs the bf16 prediction on the device; there is no CPU fallback")
    B = pred.shape[0]
    dev = pred.device
    if timestep_loss_weights is None:
        w = torch.ones(B, dtype=torch.float32, device=dev)
    else:
        curve = timestep_loss_weights.to(device=dev, dtype=torch.float32)
        w = curve[timesteps.to(dev).long().clamp(0, curve.shape[0] - 1)].contiguous()
    return _WeightedMSE.apply(pred, target.to(device=dev, dtype=torch.float32), w)


class _WeightedRobust(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, w, c, kind):
        B = pred.shape[0]
        n = pred[0].numel()
        dev = pred.device
        p2 = pred.contiguous().view(B, 1, n, 1)                    # as _WeightedMSE: one channel of C*H*W "pixels"
        t2 = target.contiguous().view(B, 1, 1, n)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        per = torch.empty(B, dtype=torch.float32, device=dev)
        dpred = torch.empty(B, 1, n, 1, dtype=torch.bfloat16, device=dev)
        ops.robust_loss_fwd_bwd(kind, p2, t2, w, c, 1.0, loss, per, dpred)
        ctx.save_for_backward(dpred)
        ctx.shape = pred.shape
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        out = dpred.clone()
        coef = g.detach().to(torch.float32).reshape(1).contiguous()
        lib().call("az_scale_bf16", out.numel(), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(coef.data_ptr()),
                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        return out.view(ctx.shape), None, None, None, None


def weighted_sdxl_loss(pred, target, timesteps, timestep_loss_weights=None, *, loss_type="MSE", c=None):
    """weighted_sdxl_mse_loss with the per-element function chosen by loss_type (a LOSS_TYPE string or a LossSpec): "MSE" IS
    weighted_sdxl_mse_loss; l1 / huber / smooth_l1 run az_robust_loss_fwd_bwd.  c: the per-sample widths (B,) of huber / smooth_l1
    (loss_widths gives the scheduled ones), or None for the spec's constant c.  The seam knows no prediction type: min-SNR weights
    belong in timestep_loss_weights (fold_min_snr), and a loss_type that carries min_snr_gamma is refused here."""
    spec = parse_loss_type(loss_type, "epsilon")
    if spec.min_snr_gamma is not None:
        raise ValueError("weighted_sdxl_loss: fold min_snr_gamma into timestep_loss_weights (loss.fold_min_snr); the seam does not know the prediction type")
    if c is not None and not spec.needs_c:
        raise ValueError(f"weighted_sdxl_loss: the {spec.kind} loss takes no width c")
    if spec.kind == "mse":
        return weighted_sdxl_mse_loss(pred, target, timesteps, timestep_loss_weights)
    if not pred.is_cuda or pred.dtype != torch.bfloat16:
        raise ops.AozoraError("weighted_sdxl_loss (HIP) needs the bf16 prediction on the device; there is no CPU fallback")
    B = pred.shape[0]
    dev = pred.device
    if timestep_loss_weights is None:
        w = torch.ones(B, dtype=torch.float32, device=dev)
    else:
        curve = timestep_loss_weights.to(device=dev, dtype=torch.float32)
        w = curve[timesteps.to(dev).long().clamp(0, curve.shape[0] - 1)].contiguous()
    cw = None
    if spec.needs_c:
        cw = (torch.full((B,), float(spec.c), dtype=torch.float32, device=dev) if c is None
              else torch.as_tensor(c).to(device=dev, dtype=torch.float32).reshape(-1).contiguous())
        if cw.numel() != B:
            raise ValueError(f"weighted_sdxl_loss: c holds {cw.numel()} widths for a batch of {B}")
    return _WeightedRobust.apply(pred, target.to(device=dev, dtype=torch.float32), w, cw, spec.kind)
