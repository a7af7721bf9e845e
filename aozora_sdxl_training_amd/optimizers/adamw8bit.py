"""PagedAdamW8bit -- the reference's `paged_adamw_8bit` optimizer (train.py:2271-2288: bitsandbytes' PagedAdamW8bit with
optim_bits=8, blockwise, percentile_clipping=100, min_8bit_size=4096) on the HIP path: one multi-tensor launch of
`az_adamw8bit_step` per step.

Arithmetic (the project's contract; INTEGRATION.md section 5 states it in full, tests/adamw8bit_ref.py restates it on the CPU).
It follows bitsandbytes' blockwise kernel as far as its published form is known and is UNPINNED against bitsandbytes, which is
not part of this project:
  * a tensor with numel < min_8bit_size keeps fp32 state1 / state2 (m / v); every other tensor keeps uint8 codes plus one fp32
    absmax per 256-element block of its LOGICAL flat order (p.view(-1) of the reference's parameter, whatever this project's
    storage order is); the last block may be short;
  * codes index two 256-entry maps built as create_dynamic_map(signed, 7, 8): signed for m, unsigned for v;
  * per step t (shared by all tensors): b1, b2, 1-b1, 1-b2, step_size = -lr*sqrt(1-b2^t)/(1-b1^t), eps*sqrt(1-b2^t) and
    1-lr*wd in float64 on the host, rounded to fp32 once; lr is param_groups[g]["lr"] at call time;
  * per element, fp32 with one rounding per operation: g (times the optional clip coefficient, rounded to bf16), decode with the
    OLD absmax, v = v*b2 + ((1-b2)*g)*g, m = m*b1 + (1-b1)*g (fp32 path: v*b2 + (1-b2)*(g*g)), new absmax = max |.| over the
    block (NaN ignored), p = bf16(p + step_size*(m/(sqrt(v)+eps_c))) then p = bf16(p*(1-lr*wd)) if wd > 0 -- only where g is
    finite; re-encode to the nearest map entry (ties to the lower), absmax 0 -> the code of 0.0, bitsandbytes' sign rule on m.
  * stated deviation: division is correctly rounded (bitsandbytes uses __fdividef).

"Paged" in bitsandbytes means CUDA managed memory that the driver evicts under memory pressure.  It has no arithmetic effect, and
on a 288 GB part the state (5.1 GB for SDXL-base) simply stays in device memory: no managed memory, nothing that needs XNACK.

state_dict() / load_state_dict() use bitsandbytes' per-parameter schema: step, state1, state2 (uint8 in logical order, or fp32 on
the 32-bit path) and, on the 8-bit path, qmap1, qmap2, absmax1, absmax2.  There is deliberately no save_cpu_state():
checkpoint.save_training_state then writes state_dict(), as the reference does for this optimizer (train.py:2522).
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Tuple

import torch
from torch.optim import Optimizer

from .._lib import lib, AozoraError

BLOCK = 256
_F_8BIT, _F_PERM, _F_VEC = 1, 2, 4
_ZERO1, _ZERO2 = 127, 0          # index of 0.0 in the signed / unsigned map (the kernel's code for an all-zero block)


def create_dynamic_map(signed: bool = True, max_exponent_bits: int = 7, total_bits: int = 8) -> torch.Tensor:
    """bitsandbytes' create_dynamic_map for (7, 8): 2^i (signed) or 2^(i+1) (unsigned) interval means of linspace(0.1, 1),
    scaled by 10^(i-6), the negatives too when signed, then 0 and 1.0; sorted, fp32."""
    assert (max_exponent_bits, total_bits) == (7, 8)
    data: List[float] = []
    for i in range(max_exponent_bits):
        k = 2 ** i if signed else 2 ** (i + 1)
        b = torch.linspace(0.1, 1, k + 1)
        means = (b[:-1] + b[1:]) / 2.0
        data += ((10 ** (i - 6)) * means).tolist()
        if signed:
            data += (-(10 ** (i - 6)) * means).tolist()
    data += [0, 1.0]
    data.sort()
    q = torch.tensor(data, dtype=torch.float32)
    _check_map(q, signed)
    return q


def _check_map(q: torch.Tensor, signed: bool):
    q = q.detach().float().cpu().reshape(-1)
    ok = (q.numel() == 256 and bool((q[1:] > q[:-1]).all()) and float(q.max()) == 1.0 and int((q == 0).sum()) == 1
          and float(q[_ZERO1 if signed else _ZERO2]) == 0.0)
    if not ok:
        raise AozoraError("PagedAdamW8bit: a quantisation map must hold 256 sorted fp32 entries, max 1.0, one zero "
                          f"(at index {_ZERO1 if signed else _ZERO2})")


def _geometry(p: torch.Tensor):
    """-> (p_ptr, g_ptr or None, flags, kh*kw, I, I_pad, owner) of a parameter: AozoraUNet slots (storage (O, kh, kw, I_pad) for
    4-D weights) or a plain contiguous bf16 device tensor."""
    owner = getattr(p, "_az_owner", None)
    if owner is not None:
        off, sshape, lshape = owner._slots[p._az_name]
        pptr, gptr = owner.pflat.data_ptr() + off * 2, owner.gflat.data_ptr() + off * 2
        if p.grad is None:
            gptr = None
        if len(sshape) == 4:
            O, I, kh, kw = lshape
            if kh * kw > 1 or sshape[3] != I:
                return pptr, gptr, _F_PERM, kh * kw, I, sshape[3], owner
        return pptr, gptr, 0, 1, 1, 1, owner
    if p.dtype != torch.bfloat16 or not p.is_cuda or not p.is_contiguous():
        raise AozoraError("PagedAdamW8bit (HIP) updates contiguous bf16 device tensors or AozoraUNet parameters")
    gptr = None
    if p.grad is not None:
        g = p.grad
        if g.dtype != torch.bfloat16 or not g.is_contiguous() or g.device != p.device:
            raise AozoraError("PagedAdamW8bit (HIP) needs contiguous bf16 device gradients")
        gptr = g.data_ptr()
    return p.data_ptr(), gptr, 0, 1, 1, 1, None


class PagedAdamW8bit(Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 min_8bit_size: int = 4096):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid betas: {betas}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self.min_8bit_size = int(min_8bit_size)
        self.param_device = None
        for group in self.param_groups:
            for p in group["params"]:
                if self.param_device is None:
                    self.param_device = p.device
                if p.device != self.param_device:
                    raise AozoraError("PagedAdamW8bit (HIP): all parameters must be on one device")
                _geometry(p)      # refuses other dtypes / layouts up front
        if self.param_device is None or self.param_device.type != "cuda":
            raise AozoraError("PagedAdamW8bit (HIP) needs parameters on a HIP device; there is no CPU fallback")
        self._t = 0
        self.qmap1 = create_dynamic_map(True).to(self.param_device)
        self.qmap2 = create_dynamic_map(False).to(self.param_device)
        self._qmaps = torch.cat([self.qmap1, self.qmap2])
        self._table_key = None
        self._desc = None
        self._nblocks = 0
        self._ntensors = 0
        self._hyper_host = None
        self._hyper_dev = None
        self._hyper_ev = None
        self.clip_coef = None      # optional device fp32[1]; multiplies grads inside the kernel (as RavenAdamW.clip_coef)

    # -------------------------------------------------------------------------------------------
    def _is_8bit(self, p) -> bool:
        return p.numel() >= self.min_8bit_size

    def _init_state(self, p):
        st = self.state[p]
        if "state1" in st:
            return st
        dev = self.param_device
        st["step"] = 0
        if self._is_8bit(p):
            nb = (p.numel() + BLOCK - 1) // BLOCK
            st["state1"] = torch.zeros(p.shape, dtype=torch.uint8, device=dev)
            st["state2"] = torch.zeros(p.shape, dtype=torch.uint8, device=dev)
            st["qmap1"], st["qmap2"] = self.qmap1, self.qmap2
            st["absmax1"] = torch.zeros(nb, dtype=torch.float32, device=dev)
            st["absmax2"] = torch.zeros(nb, dtype=torch.float32, device=dev)
        else:
            st["state1"] = torch.zeros(p.shape, dtype=torch.float32, device=dev)
            st["state2"] = torch.zeros(p.shape, dtype=torch.float32, device=dev)
        return st

    def zero_grad(self, set_to_none: bool = True):
        """As RavenAdamW.zero_grad: AozoraUNet gradients accumulate in the owner's flat buffer, so the buffer itself is cleared."""
        owners = []
        for g in self.param_groups:
            for p in g["params"]:
                o = getattr(p, "_az_owner", None)
                if o is not None and all(o is not q for q in owners):
                    owners.append(o)
        for o in owners:
            for a, b in o.trainable_ranges():
                o.gflat[a:b].zero_()
        super().zero_grad(set_to_none)

    def _build_table(self, work: List[Tuple[int, torch.Tensor, tuple]]):
        """Descriptor records (12 int64 words each, see include/aozora_hip.h) plus the first-block prefix table, on the device."""
        rows, first, nb = [], [], 0
        for gi, p, (pptr, gptr, flags, ks, I, Ipad, _) in work:
            st = self.state[p]
            n = p.numel()
            if n >= 2 ** 31 or ks > 32:
                raise AozoraError("PagedAdamW8bit (HIP): tensors need numel < 2^31 and kh*kw <= 32")
            eight = self._is_8bit(p)
            s1, s2 = st["state1"].data_ptr(), st["state2"].data_ptr()
            a1 = st["absmax1"].data_ptr() if eight else 0
            a2 = st["absmax2"].data_ptr() if eight else 0
            fl = flags | (_F_8BIT if eight else 0)
            if not flags & _F_PERM and pptr % 8 == 0 and gptr % 8 == 0 and (not eight or (s1 % 4 == 0 and s2 % 4 == 0)):
                fl |= _F_VEC
            rows.append([pptr, gptr, s1, s2, a1, a2, n, nb, fl, ks, I | (Ipad << 32), gi])
            first.append(nb)
            nb += (n + BLOCK - 1) // BLOCK
        first.append(nb)
        flat = [w for r in rows for w in r] + first
        host = torch.tensor([w - (1 << 64) if w >= (1 << 63) else w for w in flat], dtype=torch.int64)
        self._desc = host.to(self.param_device)
        self._nblocks, self._ntensors = nb, len(rows)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work, owners = [], []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                geo = _geometry(p)
                if geo[1] is None:
                    continue
                self._init_state(p)
                work.append((gi, p, geo))
                if geo[6] is not None and all(geo[6] is not o for o in owners):
                    owners.append(geo[6])
        if not work:
            return loss
        self._t += 1
        t = self._t
        key = tuple((gi, id(p), geo[0], geo[1], self.state[p]["state1"].data_ptr()) for gi, p, geo in work)
        if key != self._table_key:
            self._build_table(work)
            self._table_key = key
        ng = len(self.param_groups)
        if self._hyper_host is None or self._hyper_host.shape[0] < ng:
            self._hyper_host = torch.zeros(ng, 8, dtype=torch.float32).pin_memory()
            self._hyper_dev = torch.zeros(ng, 8, dtype=torch.float32, device=self.param_device)
        if self._hyper_ev is not None:
            self._hyper_ev.synchronize()      # the previous step's copy out of the pinned buffer has completed
        for gi, group in enumerate(self.param_groups):
            lr, (b1, b2), eps, wd = float(group["lr"]), group["betas"], float(group["eps"]), float(group["weight_decay"])
            b1, b2 = float(b1), float(b2)
            c1, c2 = 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)
            self._hyper_host[gi] = torch.tensor([b1, b2, 1.0 - b1, 1.0 - b2, -lr * c2 / c1, eps * c2, 1.0 - lr * wd,
                                                 1.0 if wd > 0 else 0.0], dtype=torch.float64).float()
        self._hyper_dev[:ng].copy_(self._hyper_host[:ng], non_blocking=True)
        sc = torch.cuda.current_stream(self.param_device)
        self._hyper_ev = torch.cuda.Event()
        self._hyper_ev.record(sc)
        coef = self.clip_coef
        lib().call("az_adamw8bit_step", self._ntensors, ctypes.c_void_p(self._desc.data_ptr()), self._nblocks,
                   ctypes.c_void_p(self._hyper_dev.data_ptr()), ctypes.c_void_p(self._qmaps.data_ptr()),
                   ctypes.c_void_p(coef.data_ptr() if coef is not None else 0), ctypes.c_void_p(sc.cuda_stream))
        self.clip_coef = None
        for _, p, _ in work:
            self.state[p]["step"] = t
        for o in owners:
            o.mark_params_dirty()
        return loss

    # -------------------------------------------------------------------------------------------
    def state_dict(self):
        """torch's layout ({"state": {index: ...}, "param_groups": [...]}) with bitsandbytes' per-parameter keys; host tensors."""
        torch.cuda.synchronize(self.param_device)
        sd = super().state_dict()
        sd["state"] = {i: {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in st.items()}
                       for i, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """Restores the schema of state_dict() without torch's cast of floating state to the parameter dtype (which would turn
        absmax into bf16).  The file's maps are used for decoding; a file whose tensors carry differing maps is refused."""
        groups = state_dict["param_groups"]
        if len(groups) != len(self.param_groups) or any(len(a["params"]) != len(b["params"]) for a, b in zip(groups, self.param_groups)):
            raise ValueError("loaded state dict does not match the optimizer's parameter groups")
        index: Dict[int, torch.Tensor] = {}
        for saved, mine in zip(groups, self.param_groups):
            for i, p in zip(saved["params"], mine["params"]):
                index[i] = p
            for k, v in saved.items():
                if k != "params":
                    mine[k] = tuple(v) if k == "betas" else v
        q1 = q2 = None
        steps = set()
        for i, st in state_dict["state"].items():
            if "qmap1" in st:
                if q1 is None:
                    q1, q2 = st["qmap1"].detach().float().cpu(), st["qmap2"].detach().float().cpu()
                elif not (torch.equal(q1, st["qmap1"].detach().float().cpu()) and torch.equal(q2, st["qmap2"].detach().float().cpu())):
                    raise AozoraError("PagedAdamW8bit.load_state_dict: the tensors of this file carry differing quantisation maps")
        if q1 is not None:
            _check_map(q1, True)
            _check_map(q2, False)
            self.qmap1.copy_(q1)
            self.qmap2.copy_(q2)
            self._qmaps.copy_(torch.cat([q1, q2]))
        for i, st in state_dict["state"].items():
            p = index[i]
            mine = self._init_state(p)
            eight = self._is_8bit(p)
            if ("qmap1" in st) != eight or st["state1"].numel() != p.numel():
                raise AozoraError(f"PagedAdamW8bit.load_state_dict: state {i} does not match its parameter ({tuple(p.shape)}, "
                                  f"{'8-bit' if eight else '32-bit'} path)")
            for k in ("state1", "state2") + (("absmax1", "absmax2") if eight else ()):
                src = st[k]
                if src.dtype != mine[k].dtype or src.numel() != mine[k].numel():
                    raise AozoraError(f"PagedAdamW8bit.load_state_dict: state {i}.{k} is {src.dtype} x {src.numel()}, "
                                      f"expected {mine[k].dtype} x {mine[k].numel()}")
                mine[k].copy_(src.reshape(mine[k].shape))
            step = st.get("step", 0)
            step = int(step.item()) if torch.is_tensor(step) else int(step)
            mine["step"] = step
            steps.add(step)
        if len(steps) > 1:
            raise AozoraError(f"PagedAdamW8bit.load_state_dict: parameters saved at different steps {sorted(steps)}")
        self._t = steps.pop() if steps else 0
        torch.cuda.synchronize(self.param_device)
