"""LoRA max-norm regularisation (INTEGRATION.md "LoRA max-norm"; kohya-ss scale_weight_norms; not in the reference, whose train.py is
full fine-tuning only): after every optimizer step the effective update (alpha / rank) B A of each adapted module has its Frobenius
norm measured, and where it exceeds the limit A and B are both scaled by sqrt(limit / norm).  Host-side placement only: the arithmetic
is az_lora_max_norm_bf16 (csrc/az_lora.hip), ONE launch over a job table built once from the flat parameter store -- no product B A,
no per-module read-back.  The rule is written from kohya-ss's apply_max_norm_regularization as understood and is unpinned against the
package, like the rest of LoRA.

Ordering is the caller's: apply(stream) goes behind the update of the adapters' range on the stream that issued it, ahead of the W^T
refresh of that range and ahead of any reader.  The flat optimizers (dist.ShardedRaven / ShardedTitan) issue it themselves inside
step() (`optimizer.lora_norm`); a module optimizer's step() is followed by apply() and unet.mark_params_dirty() in the loop.  The pass
is a function of the parameters alone: nothing of it goes into a training state.
"""
from __future__ import annotations

import math
import struct
from typing import Callable, List, Optional, Tuple

import torch

from . import ops
from ._lib import AozoraError
from .unet_spec import LORA_RANKS


def check_max_norm(max_norm) -> float:
    """A positive finite real number (bool, str, None and the rest are refused): ValueError otherwise."""
    if isinstance(max_norm, bool) or not isinstance(max_norm, (int, float)) or not math.isfinite(max_norm) or not max_norm > 0.0:
        raise ValueError(f"LoRA max_norm must be a positive finite real number, got {max_norm!r}")
    return float(max_norm)


def s_bits(s: float) -> int:
    """The fp32 bits of a module's scale, as the job table carries them."""
    return struct.unpack("<I", struct.pack("<f", float(s)))[0]


def check_row(row, what="row"):
    """One row of the job table against the rules of az_lora_max_norm_bf16 (the kernel skips a row that breaks one; the builder
    refuses it): AozoraError."""
    a, b, r, K, out, _, ma, mb = row
    if r not in LORA_RANKS or K <= 0 or out <= 0 or K % 8 or out % 8 or K > (1 << 24) or out > (1 << 24):
        raise AozoraError(f"lora max-norm: {what} has rank {r}, K {K}, out {out}: rank one of {LORA_RANKS}, K and out positive multiples of 8")
    if not a or not b or (a | b | ma | mb) % 16:
        raise AozoraError(f"lora max-norm: {what} has a null or misaligned address (16 bytes)")


def job_rows(unet, master: Optional[Callable[[int, int], int]] = None) -> Tuple[List[List[int]], List[str]]:
    """-> (rows of the job table, module names), one row per adapted module in the order of the adapter table: [address of A, address
    of B, r, K, out, fp32 bits of alpha_of / rank_of, address of the fp32 master of A, of B (0 = none)].  A [r][K] and B [out][r] are the
    dense slots of pflat (a 3x3 convolution's [r][3][3][Cin]: K = 9 Cin).  master(flat offset, numel) -> the address of the fp32 master
    copy of that slot, or 0."""
    spec = unet.lora
    if spec is None:
        raise AozoraError("lora max-norm needs a UNet with adapters (AozoraUNet(lora=spec))")
    p0 = unet.pflat.data_ptr()
    rows, modules = [], []
    for name, _ in unet._table:
        if not name.endswith(".lora_A.weight"):
            continue
        m = name[:-len(".lora_A.weight")]
        oa, sta, _ = unet._slots[name]
        ob, stb, _ = unet._slots[m + ".lora_B.weight"]
        r, K, out = sta[0], math.prod(sta[1:]), stb[0]
        if stb[1] != r:
            raise AozoraError(f"lora max-norm: {m} has A {sta} but B {stb}")
        ma = master(oa, r * K) if master is not None else 0
        mb = master(ob, out * r) if master is not None else 0
        row = [p0 + 2 * oa, p0 + 2 * ob, r, K, out, s_bits(spec.scale_of(m)), int(ma or 0), int(mb or 0)]
        check_row(row, m)
        rows.append(row)
        modules.append(m)
    if not rows:
        raise AozoraError("lora max-norm: this UNet carries no adapter")
    return rows, modules


class LoraMaxNorm:
    """The max-norm pass of one AozoraUNet.  master: None, or a callable (flat offset, numel) -> address of the fp32 master copy of that
    slot (dist.ShardedRaven.master_address with "master_weights", optimizers.Prodigy.master_address always): the kernel then scales the
    master and writes bf16(master), so the master's extra bits survive (resync_master() would throw them away).

    apply(stream) issues the launch and a non-blocking copy of the per-module (norm, q) into one of RING pinned slots behind an event,
    and returns the slot; summary(slot) waits for THAT event only and reduces on the host -- the trainer reads it with the closing
    micro-step's record, never by draining the queue.  At most RING applies may be unread at once."""
    RING = 4

    def __init__(self, unet, max_norm, master: Optional[Callable[[int, int], int]] = None):
        self.max_norm = check_max_norm(max_norm)
        self.unet = unet
        rows, self.modules = job_rows(unet, master)
        self.n = len(rows)
        self.has_master = any(row[6] or row[7] for row in rows)
        self.table = torch.tensor(rows, dtype=torch.int64, device=unet.device)
        self.stats = torch.zeros(self.n, 2, dtype=torch.float32, device=unet.device)
        self._host = torch.zeros(self.RING, self.n, 2, dtype=torch.float32).pin_memory()
        self._events = [None] * self.RING
        self._count = 0

    def apply(self, stream=None) -> int:
        stream = stream if stream is not None else torch.cuda.current_stream(self.unet.device)
        ops.lora_max_norm(self.table, self.max_norm, self.stats, stream)
        self.unet.mark_params_dirty()             # the W^T copies of the adapters are stale until the next refresh (a flat optimizer's step()
        k = self._count % self.RING               # refreshes them right behind this and clears the flag again)
        self._count += 1
        with torch.cuda.stream(stream):
            self._host[k].copy_(self.stats, non_blocking=True)
        self._events[k] = torch.cuda.Event()
        self._events[k].record(stream)
        return k

    @property
    def last(self) -> Optional[int]:
        """The slot of the latest apply(), or None before the first."""
        return (self._count - 1) % self.RING if self._count else None

    def landed(self, slot=None) -> torch.Tensor:
        """The host copy [n][2] of (norm before scaling, q) of apply() number `slot` (default: the latest), once it has landed."""
        slot = self.last if slot is None else slot
        if slot is None or self._events[slot] is None:
            raise RuntimeError("LoraMaxNorm: nothing applied yet")
        self._events[slot].synchronize()
        return self._host[slot]

    def summary(self, slot=None) -> Tuple[int, float, float]:
        """(keys_scaled, mean_norm, max_norm) over the modules, kohya-ss's three numbers: a module counts as scaled when q != 1, and its
        reported norm is min(norm, limit) (kohya-ss's norm * ratio)."""
        st = self.landed(slot).double()
        norms = torch.minimum(st[:, 0], torch.tensor(self.max_norm, dtype=torch.float64))
        return int((st[:, 1] != 1.0).sum()), float(norms.mean()), float(norms.max())
