"""Prodigy -- Mishchenko & Defazio, "Prodigy: An Expeditiously Adaptive Parameter-Free Learner" (arXiv 2306.06101) -- on the HIP path:
AdamW-shaped moments scaled by a step size d that the device estimates itself, so `lr` is a multiplier near 1 and not a searched
scale.  The reference has no such optimizer; it stands where `optimizer.step()` does (train.py:2783).

Arithmetic (the project's contract; INTEGRATION.md "The Prodigy optimizer" states it in full, tests/prodigy_ref.py restates it on the
CPU).  It follows the authors' published implementation (the `prodigyopt` package) as far as its form is known and is UNPINNED against
it: `prodigyopt` is not part of this project.
  * tensor state per trainable element, all fp32: w (master), p0 (the starting point), m, v, s; w = p0 = float(p) at the first step, and
    the bf16 parameter is always the round-to-nearest image of w (it is written, never read);
  * scalar state on the device, fp64: d, d_max, d_numerator, d_denom, d_hat, k, d0; initially d = d_max = d0, the rest 0;
  * one step with lr > 0 (lr == 0: nothing is launched, nothing changes) is 2 R + 2 launches for R contiguous ranges on the current
    stream -- az_prodigy_begin, az_prodigy_moments per range, az_prodigy_finish, az_prodigy_apply per range -- with no copy to the host
    and no synchronisation: the two sums over all elements, the new d and the constants derived from it never leave the device;
  * both sums are accumulated in fp64 in a fixed order (per thread, per block, then one workgroup over all partials): no floating-point
    atomics, a step is bit-reproducible;
  * when d_denom == 0 (all-zero gradients) the step ends after the moments pass: no parameter update, k unchanged.

It takes AozoraUNet parameters (mapped to merged ranges of the owner's flat buffers, frozen slots skipped, as clip._grad_ranges does)
and plain contiguous bf16 device tensors with bf16 or fp32 gradients (one range each); one param group, one device.

save_cpu_state() / load_cpu_state() are the hooks checkpoint.save_training_state / resume_optimizer look for; the schema is the
project's own (version tag, options, the seven scalars as Python floats, the range list, w / p0 / m / v / s as fp32 host tensors in the
storage order of those ranges).  A state whose ranges differ from the optimizer's -- another freeze mask -- is refused.
"""
from __future__ import annotations

import ctypes
import math
from typing import List

import torch
from torch.optim import Optimizer

from .._lib import lib, AozoraError

STATE_VERSION = "aozora-prodigy-1"
SCALARS = ("d", "d_max", "d_numerator", "d_denom", "d_hat", "k", "d0")
TENSORS = ("w", "p0", "m", "v", "s")
_ALIGN = 64          # state offset of a range in the packed fp32 buffers: a multiple of 64 elements (256 bytes)
STATE_BYTES_PER_ELEMENT = 4 * len(TENSORS)


def check_options(betas, beta3, eps, d0):
    """The value refusals of the constructor (and of trainer's reading of PRODIGY_PARAMS): ValueError."""
    if not (len(betas) == 2 and 0.0 <= float(betas[0]) < 1.0 and 0.0 <= float(betas[1]) < 1.0):
        raise ValueError(f"Prodigy: betas must lie in [0, 1), got {tuple(betas)}")
    if beta3 is not None and not 0.0 <= float(beta3) < 1.0:
        raise ValueError(f"Prodigy: beta3 must lie in [0, 1), got {beta3}")
    if not float(eps) > 0.0:
        raise ValueError(f"Prodigy: eps must be > 0, got {eps}: on channel padding and wherever a gradient is zero the update is "
                         "0 / (0 + d * eps), which eps = 0 turns into NaN")
    if not (float(d0) > 0.0 and math.isfinite(float(d0))):
        raise ValueError(f"Prodigy: d0 must be > 0, got {d0}")


def _vp(x):
    return ctypes.c_void_p(x)


class Prodigy(Optimizer):
    def __init__(self, params, lr: float = 1.0, betas=(0.9, 0.999), beta3=None, eps: float = 1e-8, weight_decay: float = 0.0,
                 use_bias_correction: bool = False, safeguard_warmup: bool = False, d0: float = 1e-6, d_coef: float = 1.0,
                 growth_rate: float = float("inf")):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        check_options(betas, beta3, eps, d0)
        super().__init__(params, dict(lr=lr, betas=(float(betas[0]), float(betas[1])), beta3=None if beta3 is None else float(beta3),
                                      eps=float(eps), weight_decay=float(weight_decay), use_bias_correction=bool(use_bias_correction),
                                      safeguard_warmup=bool(safeguard_warmup), d0=float(d0), d_coef=float(d_coef),
                                      growth_rate=float(growth_rate)))
        if len(self.param_groups) != 1:
            raise AozoraError("Prodigy (HIP) takes one param group: d is estimated over all trainable elements together")
        owner, spans, loose, dev = None, [], [], None
        for p in self.param_groups[0]["params"]:
            if dev is None:
                dev = p.device
            if p.device != dev:
                raise AozoraError("Prodigy (HIP): all parameters must be on one device")
            o = getattr(p, "_az_owner", None)
            if o is None:
                if p.dtype != torch.bfloat16 or not p.is_cuda or not p.is_contiguous():
                    raise AozoraError("Prodigy (HIP) updates contiguous bf16 device tensors or AozoraUNet parameters")
                loose.append(p)
                continue
            if owner is not None and o is not owner:
                raise AozoraError("Prodigy (HIP): parameters of two different AozoraUNet objects in one optimizer")
            owner = o
            if not p.requires_grad:
                continue                                    # a frozen slot owns no state and never moves
            off, st, _ = o._slots[p._az_name]
            spans.append((off, off + ((math.prod(st) + 63) // 64) * 64))
        if dev is None or dev.type != "cuda":
            raise AozoraError("Prodigy (HIP) needs parameters on a HIP device; there is no CPU fallback")
        self.param_device, self.owner, self._loose = dev, owner, loose
        spans.sort()
        merged: List[List[int]] = []
        for a, b in spans:
            if merged and merged[-1][1] == a:
                merged[-1][1] = b
            else:
                merged.append([a, b])
        # the range list: ("flat", start, end) in the owner's flat buffers, then ("tensor", index among the plain tensors, numel)
        self.ranges = [("flat", a, b) for a, b in merged] + [("tensor", i, p.numel()) for i, p in enumerate(loose)]
        self.range_off, n = [], 0
        for r in self.ranges:
            self.range_off.append(n)
            n += (self._len(r) + _ALIGN - 1) // _ALIGN * _ALIGN
        self._numel = sum(self._len(r) for r in self.ranges)
        with torch.cuda.device(dev):
            self._npairs = [int(lib()._fn["az_prodigy_partials"](self._len(r))) for r in self.ranges]
        if any(k < 0 for k in self._npairs):
            raise AozoraError(f"az_prodigy_partials failed with code {min(self._npairs)}")
        self._state_numel = n
        for k in TENSORS:
            setattr(self, k + "_dev", None)
        self.dstate = torch.zeros(8, dtype=torch.float64, device=dev)
        self.dstate[0] = self.dstate[1] = self.dstate[6] = float(d0)
        self.consts = torch.zeros(16, dtype=torch.float64, device=dev)          # 128 bytes: fp32[16] then fp64[8] (include/aozora_hip.h)
        self.partials = torch.zeros(max(1, 2 * sum(self._npairs)), dtype=torch.float64, device=dev)
        self._hyper = (ctypes.c_double * 16)()
        self.clip_coef = None      # optional device fp32[1]; multiplies grads inside the moments pass (as PagedAdamW8bit.clip_coef)

    # -------------------------------------------------------------------------------------------
    @staticmethod
    def _len(r):
        return r[2] - r[1] if r[0] == "flat" else r[2]

    @property
    def state_bytes(self) -> int:
        """Bytes of fp32 tensor state this optimizer holds once it has stepped (w, p0, m, v, s)."""
        return self._numel * STATE_BYTES_PER_ELEMENT

    def _param_of(self, r) -> torch.Tensor:
        """The bf16 storage of range r as a flat tensor."""
        return self.owner.pflat[r[1]:r[2]] if r[0] == "flat" else self._loose[r[1]].detach().view(-1)

    def _fill(self, names):
        for r, o in zip(self.ranges, self.range_off):
            src = self._param_of(r)
            for k in names:
                getattr(self, k + "_dev")[o:o + src.numel()].copy_(src)

    def _init_state(self):
        if self.w_dev is not None:
            return
        for k in TENSORS:
            setattr(self, k + "_dev", torch.zeros(self._state_numel, dtype=torch.float32, device=self.param_device))
        self._fill(("w", "p0"))

    def resync_master(self):
        """w <- float32(p) over every range: for whoever writes parameters from outside (unet.load_state_dict, ema.copy_to) -- the
        next step would otherwise overwrite them with bf16(old master + update).  p0, the point d is measured from, stays."""
        self._init_state()
        self._fill(("w",))
        torch.cuda.synchronize(self.param_device)

    def master_address(self, off: int, numel: int) -> int:
        """Address of the master copy w of flat [off, off + numel) of the owner's buffers, which must lie inside one range (for
        lora_norm.LoraMaxNorm: it scales w and leaves the starting point p0 and every other state alone)."""
        self._init_state()
        for r, o in zip(self.ranges, self.range_off):
            if r[0] == "flat" and r[1] <= off and off + numel <= r[2]:
                return self.w_dev.data_ptr() + 4 * (o + off - r[1])
        raise ValueError(f"flat [{off}, {off + numel}) lies inside none of this optimizer's ranges")

    def zero_grad(self, set_to_none: bool = True):
        """As PagedAdamW8bit.zero_grad: AozoraUNet gradients accumulate in the owner's flat buffer, so the buffer itself is cleared."""
        if self.owner is not None:
            for a, b in self.owner.trainable_ranges():
                self.owner.gflat[a:b].zero_()
        super().zero_grad(set_to_none)

    def _grad_of(self, r):
        """-> (address, gdtype) of the gradient of range r."""
        if r[0] == "flat":
            return self.owner.gflat.data_ptr() + r[1] * 2, 0
        g = self._loose[r[1]].grad
        if g is None:
            raise AozoraError("Prodigy (HIP): every parameter needs a gradient at step() -- d is estimated over all of them")
        if g.dtype not in (torch.bfloat16, torch.float32) or not g.is_contiguous() or g.device != self.param_device or g.numel() != r[2]:
            raise AozoraError("Prodigy (HIP) needs contiguous bf16 or fp32 device gradients")
        return g.data_ptr(), 0 if g.dtype == torch.bfloat16 else 1

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        lr = float(group["lr"])
        coef, self.clip_coef = self.clip_coef, None
        if lr == 0.0 or not self.ranges:
            return loss
        grads = [self._grad_of(r) for r in self.ranges]
        self._init_state()
        b1, b2 = group["betas"]
        h = self._hyper
        h[0], h[1], h[2] = lr, b1, b2
        h[3] = math.sqrt(b2) if group["beta3"] is None else group["beta3"]
        h[4], h[5], h[6], h[7] = group["eps"], group["weight_decay"], group["d_coef"], group["growth_rate"]
        h[8], h[9] = float(group["use_bias_correction"]), float(group["safeguard_warmup"])
        L = lib()
        st = _vp(torch.cuda.current_stream(self.param_device).cuda_stream)
        ds, cs, cf = _vp(self.dstate.data_ptr()), _vp(self.consts.data_ptr()), _vp(coef.data_ptr() if coef is not None else 0)
        addr = {k: getattr(self, k + "_dev").data_ptr() for k in TENSORS}
        L.call("az_prodigy_begin", ds, ctypes.cast(h, ctypes.c_void_p), cs, st)
        pair = 0
        for r, o, (gptr, gdt), npair in zip(self.ranges, self.range_off, grads, self._npairs):
            L.call("az_prodigy_moments", self._len(r), _vp(addr["w"] + o * 4), _vp(addr["p0"] + o * 4), _vp(gptr), gdt, _vp(addr["m"] + o * 4),
                   _vp(addr["v"] + o * 4), _vp(addr["s"] + o * 4), cs, cf, _vp(self.partials.data_ptr() + pair * 16), st)
            pair += npair
        L.call("az_prodigy_finish", pair, _vp(self.partials.data_ptr()), ds, cs, st)
        for r, o in zip(self.ranges, self.range_off):
            L.call("az_prodigy_apply", self._len(r), _vp(self._param_of(r).data_ptr()), _vp(addr["w"] + o * 4), _vp(addr["m"] + o * 4),
                   _vp(addr["v"] + o * 4), cs, st)
        if self.owner is not None:
            self.owner.mark_params_dirty()
        return loss

    def d_value(self) -> float:
        """The current step size d, read back from the device: the only member that synchronises; step() never calls it."""
        return float(self.dstate[0].item())

    def scalars(self) -> dict:
        """The seven scalars as Python floats (synchronises, like d_value)."""
        vals = self.dstate.cpu().tolist()
        return {k: vals[i] for i, k in enumerate(SCALARS)}

    # -------------------------------------------------------------------------------------------
    def _packed(self, k) -> torch.Tensor:
        """State tensor k without the alignment gaps between ranges, on the host."""
        buf = getattr(self, k + "_dev")
        return torch.cat([buf[o:o + self._len(r)] for r, o in zip(self.ranges, self.range_off)]).cpu() if self.ranges else torch.zeros(0)

    def save_cpu_state(self):
        self._init_state()
        torch.cuda.synchronize(self.param_device)
        g = self.param_groups[0]
        return {"version": STATE_VERSION, "options": {k: (list(v) if isinstance(v, tuple) else v) for k, v in g.items() if k != "params"},
                "scalars": self.scalars(), "ranges": [tuple(r) for r in self.ranges], **{k: self._packed(k) for k in TENSORS}}

    def load_cpu_state(self, st):
        if not isinstance(st, dict) or st.get("version") != STATE_VERSION:
            raise ValueError(f"not a Prodigy optimizer state of this project (version tag {STATE_VERSION!r} expected, found "
                             f"{st.get('version') if isinstance(st, dict) else type(st).__name__!r})")
        if [tuple(r) for r in st.get("ranges", [])] != [tuple(r) for r in self.ranges]:
            raise ValueError("Prodigy state covers other trainable ranges than this optimizer: the freeze mask (or the parameter list) changed")
        for k in TENSORS:
            t = st.get(k)
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.numel() != self._numel:
                raise ValueError(f"Prodigy state: {k!r} must be an fp32 tensor of {self._numel} elements")
        sc = st["scalars"]
        if not (float(sc["d0"]) > 0.0 and float(sc["d"]) > 0.0):
            raise ValueError("Prodigy state: d and d0 must be > 0")
        self._init_state()
        for k in TENSORS:
            buf, src, off = getattr(self, k + "_dev"), st[k].reshape(-1), 0
            for r, o in zip(self.ranges, self.range_off):
                n = self._len(r)
                buf[o:o + n].copy_(src[off:off + n])
                off += n
        self.dstate.copy_(torch.tensor([float(sc[k]) for k in SCALARS] + [0.0], dtype=torch.float64))
        torch.cuda.synchronize(self.param_device)
