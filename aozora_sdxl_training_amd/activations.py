"""ActivationStore -- the activation store of an AozoraUNet, buildable on any torch device:
  * the replay-stable pools (`_Pool`, one per bucket key) over the shared arenas (`_Arena`, one per parity) and the arena life cycle:
    which arena a key uses, when it is replaced, who has to let go of its addresses first, the generation count;
  * the readers a micro-step left running (deferred weight-gradient work, parity -> events) and the clients that hold recorded addresses;
  * the gradient-buffer rules of the backward: when a contribution is written in place, out of place, or aliases a layer's dY.
The only launch issued here is the ops.add_rows of give_grad; the only stream operation the wait of wait_free."""
from __future__ import annotations

import math
import weakref
from typing import Dict, List, Optional

import torch

from . import ops
from ._lib import AozoraError

BF16 = torch.bfloat16


class Act:
    """An activation [rows][C] (2-D view, unit inner stride) and its gradient buffer."""
    __slots__ = ("t", "g", "need_grad", "ready", "g_alias")

    def __init__(self, t: torch.Tensor, need_grad: bool = True):
        self.t = t
        self.g: Optional[torch.Tensor] = None
        self.need_grad = need_grad
        self.ready = None     # event: g is being WRITTEN on the side stream (wait before READING g on main)
        self.g_alias = False  # g IS some layer's dY (given by give_grad): the parameter-gradient branch may read it at any later
                              # time, so it is never written again -- the next contribution goes to a fresh buffer (g_new = g + ...)


POOL_ALIGN = 256  # bytes: every pool buffer starts on a multiple of it inside the arena (the kernels need 16)


class _Arena:
    """ONE device allocation that all activation pools of a parity carve their buffers from.  Nothing in a pool lives across
    micro-steps (every buffer is rewritten on every run), so the buckets of a run can share the memory of the largest one
    instead of each holding its own.  A pool that needs more than the arena holds keeps the excess in buffers of its own for
    that run and leaves the size it wants; grow() then REPLACES the arena by one of exactly that size -- the old one is
    released first, so old and new never coexist -- and counts a generation: every address handed out before is dead."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.buf: Optional[torch.Tensor] = None
        self.wanted = 0          # bytes the largest pool seen so far needs
        self.generation = 0      # allocations so far; pools and launch tapes made under another value are stale

    @property
    def capacity(self) -> int:
        return 0 if self.buf is None else self.buf.numel()

    def want(self, nbytes: int):
        self.wanted = max(self.wanted, int(nbytes))

    def pending(self) -> bool:
        return self.wanted > self.capacity

    def view(self, off: int, nbytes: int, shape, dtype):
        return self.buf[off:off + nbytes].view(dtype).view(shape)

    def grow(self):
        """The caller has synchronised the device and dropped every view of the old arena."""
        self.buf = None
        if self.device.type == "cuda":
            torch.cuda.empty_cache()     # back to the driver before the new one is taken: the peak is not old + new
        self.buf = torch.empty(self.wanted, dtype=torch.uint8, device=self.device)
        self.generation += 1


class _Pool:
    """Static buffer pool: the n-th allocation of a step always returns the same tensor, so the
    launch sequence (including addresses) repeats exactly and can be replayed from a hipGraph.
    The buffers are views of the shared arena at bump-assigned offsets (allocation order, POOL_ALIGN-aligned); whatever
    does not fit the arena as it stands is a tensor of its own until the arena has grown (_Arena)."""

    def __init__(self, device, arena: Optional[_Arena] = None):
        self.device = device
        self.arena = arena if arena is not None else _Arena(device)
        self.bufs: List[torch.Tensor] = []
        self.offsets: List[int] = []
        self.top = 0             # bytes assigned so far == offset of the next buffer
        self.cursor = 0
        self._gen = self.arena.generation
        self._need, self._count = 0, 0     # need and buffer count of the last table that was dropped

    def drop(self):
        """Forget the offset table and every view (the arena was replaced): the next run assigns them again."""
        if self.bufs:
            self._need, self._count = self.top, len(self.bufs)
        self.bufs, self.offsets, self.top, self.cursor = [], [], 0, 0
        self._gen = self.arena.generation

    def reset(self):
        if self._gen != self.arena.generation:
            self.drop()
        self.cursor = 0

    def get(self, shape, dtype=BF16):
        if self.cursor < len(self.bufs):
            t = self.bufs[self.cursor]
            if tuple(t.shape) != tuple(shape) or t.dtype != dtype:
                raise AozoraError("activation pool replay mismatch (topology changed between steps)")
        else:
            nb = math.prod(shape) * dtype.itemsize
            off, a = self.top, self.arena
            self.top = off + (nb + POOL_ALIGN - 1) // POOL_ALIGN * POOL_ALIGN
            if nb > 0 and off + nb <= a.capacity:
                t = a.view(off, nb, shape, dtype)
            else:
                t = torch.empty(shape, dtype=dtype, device=self.device)
            if self.top > a.capacity:
                a.want(self.top)
            self.bufs.append(t)
            self.offsets.append(off)
        self.cursor += 1
        return t

    def nbytes(self):
        """What this bucket needs of the arena: the sum of its buffers, each rounded up to POOL_ALIGN."""
        return self.top if self.bufs else self._need

    def count(self):
        """Buffers of this bucket (of its last complete table while the offsets wait to be assigned again)."""
        return len(self.bufs) if self.bufs else self._count


class ActivationStore:
    def __init__(self, device, on_replace=None):
        """on_replace(arena): called while `arena` is being replaced, after its pools were dropped and before it is released -- the
        executor lets go of its own per-step state and tells the clients (settle)."""
        self.device = torch.device(device)
        self.on_replace = on_replace
        self.pools: Dict[tuple, _Pool] = {}
        self.pool: Optional[_Pool] = None       # the current step's
        self.arenas: Dict[int, _Arena] = {}     # parity -> the arena its pools share (survives pools.clear())
        self.generation = 0                     # arena allocations so far, all parities (activation_bytes)
        self.clients = weakref.WeakSet()        # TrainStep objects: they hold launch tapes / graphs / views made of arena addresses
        self.deferred = {}                      # parity -> events of the weight-gradient work that still reads that parity's pool

    def add_client(self, obj):
        self.clients.add(obj)

    # ------------------------------------------------------------------ arena life cycle ---------
    def arena_of(self, parity) -> _Arena:
        """The arena of a pool key's last component: 0 / 1 (TrainStep, two under double_buffer); everything else -- the "call" key
        of the autograd bridge among them -- shares parity 0's."""
        k = parity if parity in (0, 1) else 0
        if k not in self.arenas:
            self.arenas[k] = _Arena(self.device)
        return self.arenas[k]

    def settle(self, arena: _Arena):
        """Between micro-steps: if some pool of `arena` wanted more than it holds, replace it.  Order matters -- the device is
        synchronised first (deferred weight-gradient work, a launched hipGraph and the C-side tape player may still use the old
        addresses), then every holder of those addresses lets go (pools, parked jobs, the launch tapes / graphs of the
        TrainStep objects), then the old arena goes back to the driver, then the new one is taken."""
        if not arena.pending():
            return
        torch.cuda.synchronize(self.device)
        self.deferred.clear()
        for pool in self.pools.values():
            if pool.arena is arena:
                pool.drop()
        self.pool = None
        if self.on_replace is not None:
            self.on_replace(arena)
        arena.grow()
        self.generation += 1

    def prepare(self, parity) -> int:
        """Called by TrainStep before a micro-step on `parity` issues anything: grows the arena if the previous micro-step asked
        for it.  -> the arena's generation; whatever recorded addresses under another value must be rebuilt."""
        arena = self.arena_of(parity)
        self.settle(arena)
        return arena.generation

    def begin(self, key, recording: bool):
        """A step on the pool of `key` begins: its arena settled (never under a running recording, whose launches already hold
        addresses), the pool made if this is the key's first visit, current, and rewound to its first buffer."""
        arena = self.arena_of(key[-1])
        if not recording:
            self.settle(arena)
        if key not in self.pools:
            self.pools[key] = _Pool(self.device, arena)
        self.pool = self.pools[key]
        self.pool.reset()

    def activation_bytes(self) -> dict:
        """{"arena": {parity: bytes held}, "need": {pool key: bytes that bucket needs}, "generation": arena allocations so far}.
        All buckets of a parity share one arena, sized for the largest of them: after any sequence of buckets
        arena <= max need + 256 B x (buffers of that bucket).  An arena that is too small is replaced, which counts a generation
        and makes every bucket of that parity rebuild its launch tape / graph on its next visit.
        Because the buckets overwrite each other's activations, `TrainStep.last_pred_nhwc`, `bk.pred` and `bk.per_sample` of a
        bucket are valid until the next micro-step of ANY bucket of the same parity (not, as with one pool per bucket, until the
        next visit of the same bucket): read them before that."""
        return {"arena": {k: a.capacity for k, a in self.arenas.items()},
                "need": {k: p.nbytes() for k, p in self.pools.items()},
                "generation": self.generation}

    # ------------------------------------------------------------------ deferred readers ---------
    def leave_readers(self, parity, events):
        """A micro-step ends without joining its parameter-gradient branch: `events` complete what still reads pool `parity`."""
        self.deferred[parity] = events

    def clear_readers(self):
        self.deferred.clear()

    def wait_free(self, parity):
        """Before a micro-step writes into activation pool `parity`: the deferred weight-gradient work that still reads it."""
        for ev in self.deferred.pop(parity, []):
            torch.cuda.current_stream().wait_event(ev)

    def has_deferred(self):
        return bool(self.deferred)

    # ------------------------------------------------------------------ gradient buffers ---------
    def new(self, rows, C, need_grad=True, dtype=BF16) -> Act:
        return Act(self.pool.get((rows, C), dtype), need_grad)

    def gbuf(self, a: Act):
        """-> (dst, add) for writing a contribution to a's gradient: add is None (dst is overwritten), dst itself (accumulate in
        place) or another tensor (dst = add + contribution, out of place).  Out of place exactly when the current gradient
        storage is some layer's dY (g_alias): that layer's weight-gradient product, queued on the parameter-gradient branch,
        reads it at an unspecified later time, and never having to wait for it is what lets the branch lag and its forks be
        batched (one event per block instead of one per layer: the event packets cost the data-gradient stream 5-10 us each,
        ~5 ms per micro-step, tools/trace_gaps.py)."""
        if a.g is None:
            a.g = self.pool.get(tuple(a.t.shape), BF16)
            a.g_alias = False
            return a.g, None
        if a.g_alias:
            old = a.g
            a.g = self.pool.get(tuple(a.t.shape), BF16)
            a.g_alias = False
            return a.g, old
        return a.g, a.g

    def gbuf_single(self, a: Act, what: str):
        """Gradient buffer of an activation that must have exactly one consumer (no accumulation form in the kernel)."""
        dst, add = self.gbuf(a)
        if add is not None:
            raise AozoraError(what + " must have a single consumer")
        return dst

    def give_grad(self, a: Act, dy: torch.Tensor, alias=True):
        """a.g += dy, aliasing dy's storage when a has no gradient yet (dy is dead afterwards for the data-gradient chain).
        alias=True: dy is a layer's dY that the parameter-gradient branch still reads (see gbuf)."""
        if not a.need_grad:
            return
        if a.g is None:
            a.g = dy
            a.g_alias = alias
        elif a.g_alias:
            old = a.g
            a.g = self.pool.get(tuple(a.t.shape), BF16)
            a.g_alias = False
            ops.add_rows(old, dy, a.g)
        else:
            ops.add_rows(a.g, dy, a.g)
