"""GradBranch -- the parameter-gradient branch of an AozoraUNet's backward, buildable on any torch device:
  * the queue of weight / bias gradient launches (`defer`) and its batches: `flush` issues what is queued on a branch stream behind ONE
    fork event (`fork`, round-robin over the streams the UNet hands in, each with its own workspace slot) and keeps the completion
    event of the last batch;
  * what the layers park until a block or a parameter region ends -- LayerNorm partial sums, linear weight gradients, the weight
    gradients of the hoisted context projections -- and the pointer tables of the grouped launches they go out as;
  * the pool of fork / join events, and the join (or the deferred join) at the end of a backward.
Nothing here touches the device before the first fork: with `sides=[]` the queueing rules run on the CPU (tests/test_branch_cpu.py)."""
from __future__ import annotations

from typing import List

import torch

from . import ops
from ._lib import ForkEvent, record_event, wait_event, run_live


def _tiles(jobs) -> int:
    """128x128 output tiles of parked linear weight gradients (dY [K][N], X [K][M], ...)."""
    return sum(((dy.shape[1] + 127) // 128) * ((x.shape[1] + 127) // 128) for dy, x, *_ in jobs)


class _Side:
    """with branch.fork(): ... launches go to the side stream (own workspace) and are joined on exit."""

    def __init__(self, b):
        self.b = b

    def __enter__(self):
        b = self.b
        self.main = torch.cuda.current_stream()
        if not b.concurrent:
            return self
        k = b.rr % len(b.sides)
        b.rr += 1
        self.stream = b.sides[k]
        ev = b.event(); record_event(ev, self.main); wait_event(self.stream, ev)
        b.used = True
        self.ctx = torch.cuda.stream(self.stream); self.ctx.__enter__()
        ops.set_workspace_slot(1 + k)
        return self

    def __exit__(self, *a):
        b = self.b
        if not b.concurrent:
            return False
        ops.set_workspace_slot(0)
        self.ctx.__exit__(*a)
        self.done = b.event(); record_event(self.done, self.stream)
        return False

    done = None

    def join(self):
        if self.b.concurrent and self.done is not None:
            wait_event(self.main, self.done)


class GradBranch:
    def __init__(self, policy, acts, sides, device):
        """policy: the UNet's ExecPolicy (read at every use: tests and tools change it between steps); acts: its ActivationStore (the
        readers a deferred join leaves); sides: the branch streams, made by the UNet."""
        self.policy, self.acts, self.sides, self.device = policy, acts, sides, torch.device(device)
        # backward concurrency: each layer's wgrad (+ bias grad) runs on a forked stream beside its dgrad
        self.concurrent = True
        self.ln_tables, self.tn_tables = {}, {}
        self.events: list = []         # pool of fork / join events (ForkEvent, or torch.cuda.Event with policy.fork_events off)
        self.defer_join, self.parity = False, 0      # how this micro-step's backward ends (enter, _end_join)
        self.begin()

    def begin(self):
        """A step begins."""
        self.ev_cursor = 0
        self.rr = 0
        self.used = False
        self.done = None               # completion event of the last batch issued to the branch
        self.drop()

    def drop(self):
        """An arena is being replaced: the holders of its addresses let go."""
        self.q: List = []              # queued parameter-gradient launches (see defer / flush)
        self.ln_jobs: List = []        # parked LayerNorm partial sums (part, dgamma, dbeta, nblk, C)
        self.tn_jobs: List = []        # parked linear weight gradients of the current block (dY, X, dW, bias gradient)
        self.xkv_jobs: List = []       # parked weight gradients of the hoisted context projections of the current parameter region
        # the pointer tables (ln_tables, tn_tables; the UNet's _group_tables) stay: recorded launches of the OTHER parity's buckets hold
        # their raw addresses, and their keys carry everything a record holds, so an entry made of dead addresses can only be found
        # again by a launch that means exactly those addresses and shapes

    def enter(self, parity, defer_join):
        """A micro-step on activation pool `parity` begins; defer_join: its backward leaves the branch running (_end_join)."""
        self.defer_join, self.parity = bool(defer_join), parity

    # ------------------------------------------------------------------ fork / join ---------------
    def event(self):
        if self.ev_cursor == len(self.events):
            self.events.append(ForkEvent() if self.policy.fork_events else torch.cuda.Event())
        ev = self.events[self.ev_cursor]
        self.ev_cursor += 1
        return ev

    def reset_events(self):
        """Destroy the pooled events (a ForkEvent holds a HIP event of its own) and start an empty pool."""
        for ev in self.events:
            if isinstance(ev, ForkEvent):
                ev.destroy()
        del self.events[:]
        self.ev_cursor = 0

    def fork(self):
        return _Side(self)

    def _end_join(self):
        """End of a backward.  Default: the data chain waits for the parameter-gradient stream(s).  With
        `defer_join` (TrainStep(double_buffer=True), a non-final micro-step of an accumulation window) the branch is NOT
        joined: its remaining weight-gradient products keep running under the next micro-step's forward, whose launches
        write into the other activation pool; only an event is left for the next user of THIS pool."""
        main = torch.cuda.current_stream()
        evs = []
        for sd in self.sides:
            ev = torch.cuda.Event(); ev.record(sd); evs.append(ev)
        if self.defer_join:
            self.acts.leave_readers(self.parity, evs)
        else:
            for ev in evs:
                main.wait_event(ev)
            self.acts.clear_readers()     # the in-order side stream(s) are fully drained now

    def join(self):
        """The backward has issued everything: join the branch streams (or let them run on), if anything was forked."""
        if self.concurrent and self.used:
            run_live(self._end_join)
            self.used = False

    # ------------------------------------------------------------------ the queue -----------------
    def defer(self, fn):
        if not self.concurrent:
            fn()
        else:
            self.q.append(fn)
            if len(self.q) >= self.policy.side_batch:
                self.flush()

    def flush(self):
        """Issue the queued parameter-gradient launches on the side stream behind ONE fork event; -> the completion event of
        everything issued to the branch so far (the branch is one in-order stream per fork target; with an empty queue that is
        the previous flush's event, which defer may just have produced)."""
        if not self.q:
            return self.done
        q, self.q = self.q, []
        side = self.fork()
        with side:
            for fn in q:
                fn()
        self.done = side.done
        return side.done

    # ------------------------------------------------------------------ parked work ---------------
    def park_ln(self, job):
        self.ln_jobs.append(job)

    def park_tn(self, job):
        """Parked until the parked products add up to a chip-filling grid (attn2.to_out + attn2.to_q; attn1.to_out + to_q|k|v; the
        feed-forward ones are that large on their own), then ONE grouped launch, every product over its whole k-range."""
        self.tn_jobs.append(job)
        if _tiles(self.tn_jobs) >= self.policy.tn_group:
            self.finish_tn()

    def park_xkv(self, job):
        self.xkv_jobs.append(job)

    def finish_ln(self):
        """Queue ONE finish launch for the parked LayerNorm partial sums (layernorm.bwd) on the parameter-gradient branch."""
        jobs, self.ln_jobs = self.ln_jobs, []
        if not jobs:
            return
        # keyed by everything a record holds: pools of different buckets hand out the same arena addresses for other shapes
        key = tuple((p.data_ptr(), gw.data_ptr() if gw is not None else 0, gb.data_ptr() if gb is not None else 0, nblk, C)
                    for p, gw, gb, nblk, C in jobs)
        tab = self.ln_tables.get(key)
        if tab is None:
            rows_, blocks = [], 0
            for part, gw, gb, nblk, C in jobs:
                rows_.append([part.data_ptr(), gw.data_ptr() if gw is not None else 0, gb.data_ptr() if gb is not None else 0, nblk, C, blocks])
                blocks += (C + 31) // 32
            tab = (torch.tensor(rows_, dtype=torch.int64, device=self.device), len(rows_), blocks)
            self.ln_tables[key] = tab
        self.defer(lambda: ops.ln_param_finish_multi(tab[0], tab[1], tab[2]))

    @staticmethod
    def _linear_wgrad(dy, x, dW, bias_grad):
        """dW += dY^T . X of a linear layer; the bias gradient (column sums of dY) rides on the same pass over dY."""
        ops.gemm(dy, x, dW, trans_a=True, trans_b=False, accumulate=True, split_k=0, bias_grad=bias_grad)

    def queue_wgrads(self, jobs, grouped, tag=()):
        """Queue parked linear weight gradients (dY, X, dW, bias gradient) on the parameter-gradient branch: as ONE grouped launch
        whose job table is built once per operand set (`tag` keeps the keys of different callers apart), or one product each."""
        if not grouped:
            for job in jobs:
                self.defer(lambda job=job: self._linear_wgrad(*job))
            return
        key = tag + tuple((dy.data_ptr(), xt.data_ptr(), GW.data_ptr(), bg.data_ptr() if bg is not None else 0, tuple(dy.shape), dy.stride(0),
                           tuple(xt.shape), xt.stride(0), bg.numel() if bg is not None else 0) for dy, xt, GW, bg in jobs)
        tab = self.tn_tables.get(key)
        if tab is None:
            tab = self.tn_tables[key] = ops.tn_group_table(jobs, self.device)
        self.defer(lambda: ops.gemm_tn_grouped(*tab))

    def finish_tn(self):
        """Queue the parked linear weight gradients on the parameter-gradient branch: as ONE grouped launch (every product over its
        whole k-range on 128x128 tiles -- no fp32 slabs, no reduce launches, the tiles of all products fill the chip together) when
        they add up to a chip-filling grid, else one split-K product each as before.  dY / X stay valid until the step ends: the
        activation pool never re-uses a buffer inside a step and a buffer that is some layer's dY is never written again (acts.gbuf)."""
        jobs, self.tn_jobs = self.tn_jobs, []
        if jobs:
            self.queue_wgrads(jobs, _tiles(jobs) >= self.policy.tn_group)

    def finish_xkv(self):
        """The parked K / V projection weight gradients of a parameter region as ONE grouped launch on the branch (policy.xkv_group)."""
        jobs, self.xkv_jobs = self.xkv_jobs, []
        if jobs:
            self.queue_wgrads(jobs, len(jobs) > 1, ("xkv",))

    def region_end(self):
        """A parameter region's backward is through: everything parked for the parameter-gradient branch goes out."""
        self.finish_ln()
        self.finish_tn()
        self.finish_xkv()
        self.flush()

    def block_end(self):
        """Tape entry placed at the START of a block's forward (so it runs AFTER the block's backward): the block's parked
        parameter-gradient work goes out."""
        self.finish_tn()
        self.flush()
