"""fp32 exponential moving average (EMA) of the trainable weights, updated by az_ema_flat (csrc/az_optim.hip) directly on the flat
storage-order parameter buffer.  Not in the reference (an fp32 shadow of SDXL-base is 10.3 GB; its cards have 12-24), off by default
(trainer: "ema_decay" in the active optimizer's dictionary); INTEGRATION.md "EMA of the weights".

The rule is diffusers' EMAModel.step without its "power" warm-up: e <- e - omd * (e - float(p)), omd = fp32(1 - d_k),
d_k = min(decay, (1 + k) / (10 + k)) for update k = 1, 2, ... (warm-up) or d_k = decay.  The EMA starts as float32(p), which makes
diffusers' zero-decay first step redundant.  It smooths the minibatch noise of the trajectory; it does not undo the bf16 rounding of
the parameter write-back.

The flat optimizers (dist.ShardedRaven / ShardedTitan) own the schedule: they hand over their owned trainable ranges and issue
update_range() on the stream that just updated a range, so the launches of 97 % of the elements stay off the main stream.  The
module optimizers are followed by one update() on the current stream.
"""
from __future__ import annotations

import bisect
import math
import struct
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops


def check_decay(decay) -> float:
    """0 < decay < 1, a real number (bool, str, None and the rest are refused): ValueError otherwise."""
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not math.isfinite(decay) or not 0.0 < decay < 1.0:
        raise ValueError(f"ema decay must be a real number with 0 < decay < 1, got {decay!r}")
    return float(decay)


def one_minus_decay(decay: float, k: int, warmup: bool = True) -> float:
    """omd of update number k (k = 1, 2, ...): float64 on the host, rounded to fp32 once."""
    d = min(decay, (1.0 + k) / (10.0 + k)) if warmup else decay
    return struct.unpack("f", struct.pack("f", 1.0 - d))[0]


def read_options(params) -> Tuple[Optional[float], bool]:
    """("ema_decay", "ema_warmup") of an optimizer's parameter dictionary (RAVEN_PARAMS / TITAN_PARAMS / PAGED_ADAMW_8BIT_PARAMS) ->
    (decay or None when the key is absent, warm-up flag, default true).  An invalid decay is a ValueError."""
    params = params or {}
    if "ema_decay" not in params:
        return None, True
    w = params.get("ema_warmup", True)
    w = w.strip().lower() in ("true", "1", "t", "y", "yes") if isinstance(w, str) else bool(w)      # config.coerce_types' reading of a bool
    return check_decay(params["ema_decay"]), w


def logical_views(unet, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
    """{diffusers name: logical-shape view} over any flat_numel buffer in the storage order of unet.pflat: 4-D weights are stored
    [Cout][kh][kw][Cin padded] and read (Cout, Cin, kh, kw) -- the views ParamStore._layout lays over pflat."""
    out = {}
    for name, _ in unet._table:
        o, st, shape = unet._slots[name]
        v = flat[o:o + math.prod(st)].view(st)
        out[name] = v.permute(0, 3, 1, 2)[:, :shape[1]] if len(st) == 4 else v
    return out


class EmaWeights:
    """fp32 EMA of flat ranges of unet.pflat.

    ranges / offsets: ascending, disjoint flat ranges [(a, b), ...] and the offset of each in the EMA buffer; default: every trainable
    range (unet.trainable_ranges()), packed back to back.  A flat optimizer passes its own owned trainable ranges (the concatenation of
    ShardedRaven.ranges / range_off), which exist only once it is built -- so dist.ShardedRaven / ShardedTitan also accept
    ema=dict(decay=, warmup=) and build the shard themselves (`optimizer.ema`).  With ranges given and torch.distributed initialised
    the other ranks of process_group hold the rest and full() gathers; force_local (ShardedRaven's flag of that name) keeps an object
    inside an initialised group local.

    The launches of a flat optimizer run on its background / exchange streams and READ pflat under the next forward.  full(),
    state_dict(), copy_to() and save_state() wait for them; anything else that WRITES parameters from outside (unet.load_state_dict,
    a copy into pflat) must call synchronize() -- or the optimizer's synchronize_state() -- first: synchronize_params() covers the
    parameter updates only."""

    def __init__(self, unet, decay, warmup=True, ranges: Optional[Sequence] = None, offsets: Optional[Sequence] = None, process_group=None,
                 force_local=False):
        import torch.distributed as dist
        self.decay = check_decay(decay)
        self.warmup = bool(warmup)
        self.unet = unet
        self.dist = dist if (ranges is not None and not force_local and dist.is_available() and dist.is_initialized()) else None
        self.pg = process_group
        self.world = self.dist.get_world_size(self.pg) if self.dist else 1
        self.rank = self.dist.get_rank(self.pg) if self.dist else 0
        self.ranges = [(int(a), int(b)) for a, b in (unet.trainable_ranges() if ranges is None else ranges)]
        self.numel = sum(b - a for a, b in self.ranges)
        if offsets is None:
            self.offsets = [sum(b - a for a, b in self.ranges[:i]) for i in range(len(self.ranges))]
        else:
            self.offsets = [int(o) for o in offsets]
        if len(self.offsets) != len(self.ranges):
            raise ValueError("ema: ranges and offsets differ in length")
        for i, (a, b) in enumerate(self.ranges):
            if not (0 <= a < b <= unet.flat_numel) or (i and a < self.ranges[i - 1][1]):
                raise ValueError(f"ema: tracked ranges must be non-empty, ascending and disjoint inside the flat buffer, got {self.ranges}")
        ends = self.offsets[1:] + [self.numel]
        if any(o < 0 or o + (b - a) > e for (a, b), o, e in zip(self.ranges, self.offsets, ends)):
            raise ValueError("ema: offsets do not pack the tracked ranges back to back")
        self._starts = [a for a, _ in self.ranges]
        self.ema = torch.empty(max(self.numel, 1), dtype=torch.float32, device=unet.device)
        self.k = 0
        self.omd = None
        self._streams: Dict[int, torch.cuda.Stream] = {}      # streams with EMA launches nobody has waited for yet
        self._tracked_all = None
        unet.wait_tail_params()
        self._from_params()

    def _from_params(self):
        """ema = float32(p) of the tracked elements, exact (a widening copy)."""
        p = self.unet.pflat
        for (a, b), o in zip(self.ranges, self.offsets):
            self.ema[o:o + (b - a)].copy_(p[a:b])

    @property
    def nbytes(self) -> int:
        return 4 * self.numel

    # ---- the update ------------------------------------------------------------------------------------------------------------
    def begin_update(self):
        """Advance the update counter and fix omd for this optimizer step."""
        self.k += 1
        self.omd = one_minus_decay(self.decay, self.k, self.warmup)

    def offset_of(self, a: int, b: int) -> int:
        """Offset in the EMA buffer of flat [a, b), which must be one of the tracked ranges or lie inside one (ValueError)."""
        i = bisect.bisect_right(self._starts, a) - 1
        if b <= a or i < 0 or b > self.ranges[i][1]:
            raise ValueError(f"ema: [{a}, {b}) lies inside none of the tracked ranges")
        return self.offsets[i] + (a - self.ranges[i][0])

    def update_range(self, a: int, b: int, stream):
        """One az_ema_flat over flat [a, b) on `stream`, which must be the stream that updated the parameters of that range (or be
        ordered behind it).  [a, b) is one of the tracked ranges or lies inside one."""
        if self.omd is None:
            raise RuntimeError("EmaWeights.update_range() before begin_update()")
        off = self.offset_of(a, b)
        ops.ema_flat(self.unet.pflat[a:b], self.ema[off:off + (b - a)], self.omd, stream)
        self._streams[stream.cuda_stream] = stream

    def update(self, stream=None):
        """begin_update(), then every tracked range on `stream` (default: the current one) -- behind a module optimizer's step()."""
        stream = stream if stream is not None else torch.cuda.current_stream(self.unet.device)
        self.begin_update()
        for a, b in self.ranges:
            self.update_range(a, b, stream)

    def _join(self):
        """The current stream waits for every EMA launch in flight."""
        cur = torch.cuda.current_stream(self.unet.device)
        for s in self._streams.values():
            if s.cuda_stream != cur.cuda_stream:
                ev = torch.cuda.Event(); ev.record(s); cur.wait_event(ev)
        self._streams.clear()

    def synchronize(self):
        """The host waits for every EMA launch in flight."""
        for s in self._streams.values():
            s.synchronize()
        self._streams.clear()

    # ---- reading it ------------------------------------------------------------------------------------------------------------
    def _all_tracked(self) -> List[Tuple[int, int]]:
        """Tracked ranges of all ranks (exchanged once)."""
        if self._tracked_all is None:
            if self.world > 1:
                box = [None] * self.world
                self.dist.all_gather_object(box, list(self.ranges), group=self.pg)
                self._tracked_all = sorted(tuple(r) for rs in box for r in rs)
            else:
                self._tracked_all = list(self.ranges)
        return self._tracked_all

    def full(self) -> torch.Tensor:
        """flat_numel fp32 on the device, in storage order: tracked elements from the EMA (other ranks' through one all-reduce of a
        zero-filled buffer -- summed as integers, so every bit pattern arrives as it is), everything else float32(pflat).  Every rank of
        the group must call it."""
        u = self.unet
        self._join()
        u.wait_tail_params()
        out = u.pflat.float()
        if self.world > 1:
            from .dist import all_reduce_flat
            tmp = torch.zeros(u.flat_numel, dtype=torch.float32, device=u.device)
            for (a, b), o in zip(self.ranges, self.offsets):
                tmp[a:b].copy_(self.ema[o:o + (b - a)])
            all_reduce_flat(self.dist, tmp.view(torch.int32), self.pg)
            for a, b in self._all_tracked():
                out[a:b].copy_(tmp[a:b])
        else:
            for (a, b), o in zip(self.ranges, self.offsets):
                out[a:b].copy_(self.ema[o:o + (b - a)])
        return out

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """{diffusers name: fp32 tensor of the logical shape}, views of one full() buffer."""
        return logical_views(self.unet, self.full())

    def copy_to(self, unet=None):
        """Every tracked parameter <- bf16(ema), round to nearest even (az_f32_to_bf16).  One way: restoring is the caller's business."""
        unet = unet if unet is not None else self.unet
        if unet.flat_numel != self.unet.flat_numel:
            raise ValueError("ema: copy_to() needs a UNet of the same layout")
        f = self.full()
        unet.wait_tail_params()
        for a, b in self._all_tracked():
            ops.f32_to_bf16(f[a:b], unet.pflat[a:b])
        unet.mark_params_dirty()

    # ---- checkpoints -----------------------------------------------------------------------------------------------------------
    def save_state(self):
        self._join()
        return {"k": self.k, "decay": self.decay, "warmup": self.warmup, "world": self.world, "rank": self.rank,
                "ranges": [tuple(r) for r in self.ranges], "ema": self.ema[:self.numel].cpu()}

    def load_state(self, st):
        for key, mine in (("world", self.world), ("rank", self.rank)):
            if st[key] != mine:
                raise ValueError(f"ema state does not match this run: {key} {st[key]} in the file, {mine} here")
        if [tuple(r) for r in st["ranges"]] != [tuple(r) for r in self.ranges]:
            raise ValueError("ema state does not match this run: the tracked ranges differ (freeze mask / region layout)")
        if st["ema"].numel() != self.numel:
            raise ValueError(f"ema state does not match this run: numel {st['ema'].numel()} in the file, {self.numel} here")
        self._join()
        self.ema[:self.numel].copy_(st["ema"].to(torch.float32))
        torch.cuda.synchronize(self.unet.device)
        self.k = int(st["k"])
        self.omd = None
