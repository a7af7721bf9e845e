"""Adafactor -- Shazeer & Stern, "Adafactor: Adaptive Learning Rates with Sublinear Memory Cost" (arXiv 1804.04235) -- on the HIP path:
factored second moments (one row and one column vector per matrix) in place of a per-element one, the update clipped per tensor by its
own RMS.  The reference has no such optimizer; it stands where `optimizer.step()` does (train.py:2783).

Arithmetic (INTEGRATION.md "The Adafactor optimizer" states it in full, tests/adafactor_ref.py restates it in float64): that of
`transformers.optimization.Adafactor.step` on LOGICAL tensor shapes, PINNED against transformers 5.15.0 by
tests/golden/adafactor_golden.pt.  A 2-D weight [R][C] has a row vector [R] and a column vector [C]; a 4-D weight (O, I, kh, kw) is a
batch of O*I little kh x kw matrices (row (O, I, kh), col (O, I, kw)); a 1-D tensor keeps a full second moment.  Channel padding of the
stored convolutions and the padding between slots belong to no tensor: never read, never written.

One step is one call of az_adafactor_step -- five launches whatever the number of tensors, dealt from a descriptor table with one row
per trainable tensor that is built once here -- with no copy to the host and no synchronisation; every sum has a fixed order, a step is
bit-reproducible.  The one extension beyond the package is `stochastic_rounding` of the single bf16 write (Philox bits keyed by
sr_seed, the optimizer step and the element's flat offset, the convention of az_adamw_flat_sr).

It takes AozoraUNet parameters (frozen ones own no state and never move) and plain contiguous bf16 device tensors of 1, 2 or 4
dimensions with bf16 gradients; one param group, one device.

save_cpu_state() / load_cpu_state() are the hooks checkpoint.save_training_state / resume_optimizer look for: a version tag, the
options, `step`, and one entry per tensor by parameter name, in logical shapes, under the package's names (exp_avg_sq_row,
exp_avg_sq_col, exp_avg_sq, exp_avg).  A state whose names or shapes differ from the optimizer's -- another freeze mask -- is refused.
"""
from __future__ import annotations

import ctypes
import math

import torch
from torch.optim import Optimizer

from .._lib import lib, AozoraError

STATE_VERSION = "aozora-adafactor-1"
SR_DOMAIN = 0x0ADF          # Philox counter word 3 of the stochastic-rounding draws of this optimizer
_ALIGN = 64                 # offsets into the fp32 buffers: multiples of 64 elements (256 bytes)
CLS_VEC, CLS_MAT, CLS_BATCH = 0, 1, 2
(W_CLS, W_FLAGS, W_P, W_G, W_NB0, W_NB1, W_SB0, W_SB1, W_R, W_SR, W_C, W_SC, W_STROW, W_STCOL, W_STM, W_FIRST, W_NWG, W_FIRST2, W_N2, W_SCR,
 W_FAC, W_SR0, W_NUMEL, W_SPARE) = range(24)


def check_options(eps, clip_threshold, decay_rate, beta1, weight_decay, scale_parameter, relative_step, warmup_init):
    """The value refusals of the constructor (and of trainer's reading of ADAFACTOR_PARAMS): ValueError.  Needs no device."""
    if not (len(eps) == 2 and float(eps[0]) >= 0.0 and float(eps[1]) >= 0.0):
        raise ValueError(f"Adafactor: eps must be two values >= 0 (eps1 joins g*g, eps2 bounds RMS(p) from below), got {eps}")
    if warmup_init and not relative_step:
        raise ValueError("Adafactor: warmup_init=True needs relative_step=True: it shapes the relative step and nothing else")
    if not float(clip_threshold) > 0.0:
        raise ValueError(f"Adafactor: clip_threshold must be > 0, got {clip_threshold}")
    if beta1 is not None and not 0.0 <= float(beta1) < 1.0:
        raise ValueError(f"Adafactor: beta1 must lie in [0, 1) or be None, got {beta1}")
    if not math.isfinite(float(decay_rate)) or float(decay_rate) > 0.0:
        raise ValueError(f"Adafactor: decay_rate must be <= 0 (beta2t = 1 - step ** decay_rate), got {decay_rate}")
    if not float(weight_decay) >= 0.0:
        raise ValueError(f"Adafactor: weight_decay must be >= 0, got {weight_decay}")


def state_shapes(shape, beta1):
    """Logical shape -> {package state name: shape} (what save_cpu_state writes for a tensor of that shape)."""
    shape = tuple(shape)
    out = {"exp_avg_sq_row": shape[:-1], "exp_avg_sq_col": shape[:-2] + shape[-1:]} if len(shape) >= 2 else {"exp_avg_sq": shape}
    if beta1 is not None:
        out["exp_avg"] = shape
    return out


def _vp(x):
    return ctypes.c_void_p(x)


def _up(n, a=_ALIGN):
    return (n + a - 1) // a * a


class Adafactor(Optimizer):
    def __init__(self, params, lr, eps=(1e-30, 1e-3), clip_threshold: float = 1.0, decay_rate: float = -0.8, beta1=None,
                 weight_decay: float = 0.0, scale_parameter: bool = False, relative_step: bool = False, warmup_init: bool = False,
                 stochastic_rounding: bool = False, sr_seed: int = 0):
        if lr is None:              # the package's spelling under relative_step, where the group's lr is ignored
            lr = 0.0
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        check_options(eps, clip_threshold, decay_rate, beta1, weight_decay, scale_parameter, relative_step, warmup_init)
        if int(sr_seed) < 0:
            raise ValueError(f"Adafactor: sr_seed must be >= 0, got {sr_seed}")
        super().__init__(params, dict(lr=float(lr), eps=(float(eps[0]), float(eps[1])), clip_threshold=float(clip_threshold),
                                      decay_rate=float(decay_rate), beta1=None if beta1 is None else float(beta1),
                                      weight_decay=float(weight_decay), scale_parameter=bool(scale_parameter),
                                      relative_step=bool(relative_step), warmup_init=bool(warmup_init),
                                      stochastic_rounding=bool(stochastic_rounding), sr_seed=int(sr_seed)))
        if len(self.param_groups) != 1:
            raise AozoraError("Adafactor (HIP) takes one param group")
        owner, dev, entries, loose_off = None, None, [], 0
        for idx, p in enumerate(self.param_groups[0]["params"]):
            if dev is None:
                dev = p.device
            if p.device != dev:
                raise AozoraError("Adafactor (HIP): all parameters must be on one device")
            o = getattr(p, "_az_owner", None)
            if o is None:
                if p.dtype != torch.bfloat16 or not p.is_contiguous():
                    raise AozoraError("Adafactor (HIP) updates contiguous bf16 device tensors or AozoraUNet parameters")
                if p.grad is not None and p.grad.dtype != torch.bfloat16:
                    raise AozoraError(f"Adafactor (HIP) reads bf16 gradients; parameter {idx} has a {p.grad.dtype} one")
                shape, name = tuple(p.shape), f"param.{idx}"
                geom = self._geometry(name, shape, shape, loose=True)
                entries.append(dict(name=name, shape=shape, param=p, sr0=loose_off, **geom))
                loose_off += _up(p.numel())
                continue
            if owner is not None and o is not owner:
                raise AozoraError("Adafactor (HIP): parameters of two different AozoraUNet objects in one optimizer")
            owner = o
            if not p.requires_grad:
                continue                                    # a frozen slot owns no state and never moves
            off, st, shape = o._slots[p._az_name]
            entries.append(dict(name=p._az_name, shape=tuple(shape), param=None, off=off, sr0=off, **self._geometry(p._az_name, shape, st, loose=False)))
        if dev is None or dev.type != "cuda":
            raise AozoraError("Adafactor (HIP) needs parameters on a HIP device; there is no CPU fallback")
        self.param_device, self.owner = dev, owner
        entries.sort(key=lambda e: e["cls"] != CLS_MAT)     # stable: matrices first, as the kernels' numbering wants
        self.entries = entries
        self._step = 0
        self._has_m = beta1 is not None
        L = lib()
        geo = lambda w: int(L._fn["az_adafactor_geometry"](w))
        if geo(0) != 24:
            raise AozoraError("az_adafactor_geometry: the library's descriptor row is not the 24 words this module writes")
        self.stripe_rows, self._vec_item, self._batch_item, self._col_item = geo(1), geo(2), geo(3), geo(4)
        # offsets: state (row | v, col, exp_avg), column partials, factors; the work-item numbering
        so = sc = fo = first = first2 = 0
        for e in entries:
            n = math.prod(e["shape"])
            e["numel"] = n
            if e["cls"] == CLS_MAT:
                e["nwg"], e["n2"] = -(-e["R"] // self.stripe_rows), -(-e["C"] // self._col_item) + 1
                nrow, ncol = e["R"], e["C"]
                e["scr"], sc = sc, sc + _up(e["nwg"] * e["C"])
                e["fac"], fo = fo, fo + _up(e["R"] + e["C"])
            elif e["cls"] == CLS_VEC:
                e["nwg"], e["n2"], nrow, ncol, e["scr"], e["fac"] = -(-n // self._vec_item), 0, n, 0, 0, 0
            else:
                nb = e["nb0"] * e["nb1"]
                e["nwg"], e["n2"], nrow, ncol, e["scr"], e["fac"] = -(-nb // self._batch_item), 0, nb * e["R"], nb * e["C"], 0, 0
            e["st_row"], so = so, so + _up(nrow)
            e["st_col"], so = so, so + _up(ncol)
            e["st_m"] = so if self._has_m else -1
            so += _up(n) if self._has_m else 0
            e["first"], e["first2"] = first, first2
            first, first2 = first + e["nwg"], first2 + e["n2"]
        self._state_numel, self._scratch_numel, self._fac_numel, self._nwg = so, sc, fo, first
        self._state_elems = sum(sum(math.prod(s) for s in state_shapes(e["shape"], beta1).values()) for e in entries)
        self.state = self.scratch = self.fac = self.partials = self.tsc = self.desc_dev = self.desc_host = None
        self._hyper = (ctypes.c_double * 16)()

    # -------------------------------------------------------------------------------------------
    @staticmethod
    def _geometry(name, shape, st, loose):
        """Class, extents and strides (in elements of the storage) of a tensor of logical `shape` stored as `st`."""
        if math.prod(shape) == 0:
            raise AozoraError(f"Adafactor (HIP): {name} is empty")
        if len(shape) == 1:
            return dict(cls=CLS_VEC, nb0=1, nb1=1, sb0=0, sb1=0, R=1, sr=0, C=shape[0], sc=1)
        if len(shape) == 2:
            return dict(cls=CLS_MAT, nb0=1, nb1=1, sb0=0, sb1=0, R=shape[0], sr=shape[1], C=shape[1], sc=1)
        if len(shape) == 4:
            O, I, kh, kw = shape
            if (kh, kw) not in ((1, 1), (3, 3)):
                raise AozoraError(f"Adafactor (HIP): {name} has a {kh} x {kw} kernel; the batched kernels cover 1 x 1 and 3 x 3")
            if loose:
                return dict(cls=CLS_BATCH, nb0=O, nb1=I, sb0=I * kh * kw, sb1=kh * kw, R=kh, sr=kw, C=kw, sc=1)
            ipad = st[3]                                     # stored [O][kh][kw][Ipad]
            return dict(cls=CLS_BATCH, nb0=O, nb1=I, sb0=kh * kw * ipad, sb1=1, R=kh, sr=kw * ipad, C=kw, sc=ipad)
        raise AozoraError(f"Adafactor (HIP): {name} has {len(shape)} dimensions; tensors of 1, 2 or 4 are taken (a 3-D tensor would be a "
                          "batch of matrices of arbitrary size, which no kernel here covers)")

    @property
    def state_bytes(self) -> int:
        """Bytes of fp32 optimizer state over the logical shapes (row and column vectors, full moments of vectors, exp_avg with beta1)."""
        return 4 * self._state_elems

    @property
    def optimizer_step(self) -> int:
        return self._step

    def _init_state(self):
        if self.state is not None:
            return
        dev = self.param_device
        self.state = torch.zeros(max(4, self._state_numel), dtype=torch.float32, device=dev)
        self.scratch = torch.zeros(max(4, self._scratch_numel), dtype=torch.float32, device=dev)
        self.fac = torch.zeros(max(4, self._fac_numel), dtype=torch.float32, device=dev)
        self.partials = torch.zeros(max(2, 2 * self._nwg), dtype=torch.float64, device=dev)
        self.tsc = torch.zeros(max(4, 4 * len(self.entries)), dtype=torch.float32, device=dev)
        self.desc_host = torch.zeros((max(1, len(self.entries)), 24), dtype=torch.int64)
        for i, e in enumerate(self.entries):
            if e["param"] is None:
                pa, ga = self.owner.pflat.data_ptr() + 2 * e["off"], self.owner.gflat.data_ptr() + 2 * e["off"]
            else:
                pa, ga = e["param"].data_ptr(), 0
            wide = (e["cls"] == CLS_MAT and pa % 16 == 0 and e["C"] % 8 == 0 and e["sr0"] % 8 == 0)
            e["wide_ok"] = wide
            row = self.desc_host[i]
            for w, v in ((W_CLS, e["cls"]), (W_FLAGS, 0), (W_P, pa), (W_G, ga), (W_NB0, e["nb0"]), (W_NB1, e["nb1"]), (W_SB0, e["sb0"]),
                         (W_SB1, e["sb1"]), (W_R, e["R"]), (W_SR, e["sr"]), (W_C, e["C"]), (W_SC, e["sc"]), (W_STROW, e["st_row"]),
                         (W_STCOL, e["st_col"]), (W_STM, e["st_m"]), (W_FIRST, e["first"]), (W_NWG, e["nwg"]), (W_FIRST2, e["first2"]),
                         (W_N2, e["n2"]), (W_SCR, e["scr"]), (W_FAC, e["fac"]), (W_SR0, e["sr0"]), (W_NUMEL, e["numel"])):
                row[w] = v
        self.desc_dev = torch.zeros_like(self.desc_host, device=dev)
        self._desc_stale = True

    def _bind_grads(self):
        """Gradient addresses (and with them the 16-byte flag) into the table; the device copy is refreshed only when one moved --
        never for AozoraUNet parameters, whose flat buffers stay where they are."""
        for i, e in enumerate(self.entries):
            if e["param"] is None:
                ga = int(self.desc_host[i, W_G])
            else:
                g = e["param"].grad
                if g is None:
                    raise AozoraError(f"Adafactor (HIP): {e['name']} has no gradient at step()")
                if g.dtype != torch.bfloat16 or not g.is_contiguous() or g.device != self.param_device or g.shape != e["param"].shape:
                    raise AozoraError(f"Adafactor (HIP) reads contiguous bf16 device gradients; {e['name']} has {g.dtype} {tuple(g.shape)}")
                ga = g.data_ptr()
            flags = 1 if (e["wide_ok"] and ga % 16 == 0) else 0
            if int(self.desc_host[i, W_G]) != ga or int(self.desc_host[i, W_FLAGS]) != flags:
                self.desc_host[i, W_G], self.desc_host[i, W_FLAGS] = ga, flags
                self._desc_stale = True
        if self._desc_stale:
            self.desc_dev.copy_(self.desc_host)
            self._desc_stale = False

    def zero_grad(self, set_to_none: bool = True):
        """As Prodigy.zero_grad: AozoraUNet gradients accumulate in the owner's flat buffer, so the buffer itself is cleared."""
        if self.owner is not None:
            for a, b in self.owner.trainable_ranges():
                self.owner.gflat[a:b].zero_()
        super().zero_grad(set_to_none)

    def step_lr(self, step: int) -> float:
        """The learning rate of optimizer step `step` before scale_parameter: the relative step, or the group's lr."""
        g = self.param_groups[0]
        if g["relative_step"]:
            return min(1e-6 * step if g["warmup_init"] else 1e-2, 1.0 / math.sqrt(step))
        return float(g["lr"])

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not self.entries:
            return loss
        self._init_state()
        self._bind_grads()
        g = self.param_groups[0]
        self._step += 1
        step = self._step
        h = self._hyper
        h[0] = 1.0 - math.pow(step, g["decay_rate"])
        h[1] = self.step_lr(step)
        h[2], h[3] = g["eps"]
        h[4] = g["clip_threshold"]
        h[5] = -1.0 if g["beta1"] is None else g["beta1"]
        h[6] = g["weight_decay"]
        h[7], h[8] = float(g["scale_parameter"]), float(g["stochastic_rounding"])
        h[9], h[10], h[11] = float(g["sr_seed"]), float(step), float(SR_DOMAIN)
        st = _vp(torch.cuda.current_stream(self.param_device).cuda_stream)
        lib().call("az_adafactor_step", len(self.entries), _vp(self.desc_host.data_ptr()), _vp(self.desc_dev.data_ptr()),
                   _vp(self.state.data_ptr()), self.state.numel(), _vp(self.scratch.data_ptr()), self.scratch.numel(),
                   _vp(self.fac.data_ptr()), self.fac.numel(), _vp(self.partials.data_ptr()), _vp(self.tsc.data_ptr()),
                   ctypes.cast(h, ctypes.c_void_p), st)
        if self.owner is not None:
            self.owner.mark_params_dirty()
        return loss

    # -------------------------------------------------------------------------------------------
    def _views(self, e):
        """{package state name: view of the fp32 state buffer in its logical shape}."""
        out = {}
        for k, shape in state_shapes(e["shape"], self.param_groups[0]["beta1"]).items():
            o = {"exp_avg_sq_row": e["st_row"], "exp_avg_sq": e["st_row"], "exp_avg_sq_col": e["st_col"], "exp_avg": e["st_m"]}[k]
            out[k] = self.state[o:o + math.prod(shape)].view(shape)
        return out

    def save_cpu_state(self):
        self._init_state()
        torch.cuda.synchronize(self.param_device)
        g = self.param_groups[0]
        return {"version": STATE_VERSION, "options": {k: (list(v) if isinstance(v, tuple) else v) for k, v in g.items() if k != "params"},
                "step": self._step, "state": {e["name"]: {k: v.cpu().clone() for k, v in self._views(e).items()} for e in self.entries}}

    def load_cpu_state(self, st):
        if not isinstance(st, dict) or st.get("version") != STATE_VERSION:
            raise ValueError(f"not an Adafactor optimizer state of this project (version tag {STATE_VERSION!r} expected, found "
                             f"{st.get('version') if isinstance(st, dict) else type(st).__name__!r})")
        check_state(st, [(e["name"], e["shape"]) for e in self.entries], self.param_groups[0]["beta1"])
        self._init_state()
        for e in self.entries:
            for k, v in self._views(e).items():
                v.copy_(st["state"][e["name"]][k])
        self._step = int(st["step"])
        torch.cuda.synchronize(self.param_device)


def check_state(st, named_shapes, beta1):
    """Refuse a saved state whose names or shapes differ from `named_shapes` [(parameter name, logical shape)]: ValueError."""
    saved = st.get("state")
    if not isinstance(saved, dict) or sorted(saved) != sorted(n for n, _ in named_shapes):
        raise ValueError("Adafactor state covers other tensors than this optimizer: the freeze mask (or the parameter list) changed")
    if not isinstance(st.get("step"), int) or st["step"] < 0:
        raise ValueError("Adafactor state: step must be an integer >= 0")
    for name, shape in named_shapes:
        want = state_shapes(shape, beta1)
        got = saved[name]
        if not isinstance(got, dict) or sorted(got) != sorted(want):
            raise ValueError(f"Adafactor state of {name}: entries {sorted(got) if isinstance(got, dict) else got!r}, expected {sorted(want)} "
                             "(beta1 switched on or off, or another shape class)")
        for k, s in want.items():
            t = got[k]
            if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != tuple(s):
                raise ValueError(f"Adafactor state of {name}: {k} must be an fp32 tensor of shape {tuple(s)}")
