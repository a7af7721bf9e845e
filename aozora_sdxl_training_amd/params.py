"""ParamStore -- the flat parameter store of an AozoraUNet, buildable on any torch device from a parameter table
(the base table followed by the adapter entries):
  * layout: every parameter is a slot (a multiple of ALIGN elements) of ONE flat bf16 buffer `pflat`, its gradient the same slot of
    `gflat`; each diffusers-named torch.nn.Parameter is a view of its slot (conv weights are stored [Cout][kh][kw][Cin] and exposed with
    logical shape (Cout,Cin,kh,kw)); to_q/to_k/to_v are adjacent so the projections run as one N=3C (self) / N=2C (cross k,v) GEMM;
  * regions: three contiguous ranges of the flat buffers with 4096-aligned cuts, the units of the data-parallel overlap;
  * the W^T mirror `wtflat`: transposed copies of the linear / 1x1 / 3x3 weights at the same offsets, refreshed per region by the only two
    kernels issued here (az_transpose_multi_bf16, az_transpose_bf16), and the freshness protocol around it (dirty flag, region events of
    in-flight all-gathers, the ready event of a refresh on another stream);
  * the state-dict family.
Everything but the refresh launches runs without a device or the library; the stream operations go through _stream()."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Tuple

import torch

from ._lib import lib, AozoraError
from .lora_exec import wt_jobs

BF16 = torch.bfloat16
ALIGN = 64  # elements


class ParamStore:
    def __init__(self, cfg, table, n_base, device, owner=None):
        self.cfg, self.device, self.owner = cfg, torch.device(device), owner if owner is not None else self
        self._table, self._base_table = table, table[:n_base]
        self._layout()
        # data-parallel overlap state (see region_bounds, wait_region_params)
        self._regions = None
        self._region_events = {}
        self._wt_region_pending = set()
        self._wt_ready = None
        self._grads_busy = None

    def _stream(self):
        """The seam of the stream operations (wait_event, the handle launches take): the current stream."""
        return torch.cuda.current_stream()

    def _storage_shape(self, name, shape):
        if len(shape) == 4:
            O, I, kh, kw = shape
            if name == "conv_in.weight":
                I = ((I + 7) // 8) * 8
            return (O, kh, kw, I)
        return tuple(shape)

    def _layout(self):
        off = 0
        self._slots: Dict[str, Tuple[int, tuple, tuple]] = {}
        for name, shape in self._table:
            st = self._storage_shape(name, shape)
            n = math.prod(st)
            self._slots[name] = (off, st, tuple(shape))
            off += ((n + ALIGN - 1) // ALIGN) * ALIGN
        off = ((off + 4095) // 4096) * 4096     # equal shards for 1/2/4/8-way in-place reduce-scatter / all-gather
        self.flat_numel = off
        self.pflat = torch.zeros(off, dtype=BF16, device=self.device)
        self.gflat = torch.zeros(off, dtype=BF16, device=self.device)
        self._w: Dict[str, torch.Tensor] = {}      # storage-shaped views (what kernels read)
        self._gw: Dict[str, torch.Tensor] = {}
        self._params: Dict[str, torch.nn.Parameter] = {}
        self._gviews: Dict[str, torch.Tensor] = {}  # logical-shaped grad views (what .grad exposes)
        for name, (o, st, shape) in self._slots.items():
            n = math.prod(st)
            w = self.pflat[o:o + n].view(st)
            g = self.gflat[o:o + n].view(st)
            self._w[name], self._gw[name] = w, g
            if len(st) == 4:
                lv = w.permute(0, 3, 1, 2)[:, :shape[1]]
                gv = g.permute(0, 3, 1, 2)[:, :shape[1]]
            else:
                lv, gv = w, g
            prm = torch.nn.Parameter(lv, requires_grad=True)
            prm._az_owner, prm._az_name = self.owner, name
            self._params[name] = prm
            self._gviews[name] = gv

        # transposed copies W^T of every 2-D (linear / 1x1-conv) weight, same offsets in a parallel flat buffer: the
        # data-gradient product dX = dY . W then runs in the k-contiguous (NT) form.  Fused projections
        # (to_q|to_k|to_v, to_k|to_v) are transposed as one [sum(out)][in] matrix.
        self.wtflat = torch.zeros(self.flat_numel, dtype=BF16, device=self.device)
        self._wt_tables = {}
        self._wt_jobs: List[Tuple[int, int, int]] = []       # (offset, rows N, cols K) of the stored [N][K] matrix
        names = [n for n, _ in self._table]
        skip = set()
        for name in names:
            o, st, shape = self._slots[name]
            if not name.endswith(".weight") or name in skip or ".lora_" in name:
                continue
            if len(st) == 2:
                rows, cols = st
            elif len(st) == 4 and st[1] == 1 and st[2] == 1:
                rows, cols = st[0], st[3]
            else:
                continue
            if name.endswith("attn1.to_q.weight"):
                rows *= 3
                skip.update({name.replace("to_q", "to_k"), name.replace("to_q", "to_v")})
            elif name.endswith("attn2.to_k.weight"):
                rows *= 2
                skip.add(name.replace("to_k", "to_v"))
            self._wt_jobs.append((o, rows, cols))
        # adapters (lora_exec.wt_jobs): their linear jobs behind the base linear jobs, their 3x3 jobs in front of the base 3x3 jobs
        lin, self._wt_conv_jobs = wt_jobs(self._table[len(self._base_table):], self._slots)      # (offset, Cout, Cin)
        self._wt_jobs += lin
        # 3x3 conv weights [Cout][9][Cin] -> W'[Cin][9][Cout] (nine strided transposes) for the NT-form conv dgrad
        for name in names:
            o, st, shape = self._slots[name]
            if name.endswith(".weight") and len(st) == 4 and st[1] == 3 and st[0] % 8 == 0 and name != "conv_in.weight" and ".lora_" not in name:
                self._wt_conv_jobs.append((o, st[0], st[3]))
        self._wt_dirty = True
        self._wt_version = -1

    # ------------------------------------------------------------------ views ----------------------
    def _wt(self, W: torch.Tensor) -> torch.Tensor:
        """transposed copy [K][N] of a stored [N][K] weight view of pflat."""
        o = (W.data_ptr() - self.pflat.data_ptr()) // 2
        N, K = W.shape
        return self.wtflat[o:o + N * K].view(K, N)

    def _fused_w(self, names: List[str]):
        """storage of adjacent parameters as one [sum(out)][in] matrix (to_q|to_k|to_v)."""
        o0, st0, _ = self._slots[names[0]]
        rows, cols = 0, st0[1]
        off = o0
        for n in names:
            o, st, _ = self._slots[n]
            if o != off or st[1] != cols or math.prod(st) % ALIGN:
                raise AozoraError(f"parameters {names} are not adjacent in the flat buffer")
            rows += st[0]
            off += math.prod(st)
        W = self.pflat[o0:off].view(rows, cols)
        G = self.gflat[o0:off].view(rows, cols)
        return W, G, any(self.trainable(n) for n in names)

    def trainable(self, name):
        return self._params[name].requires_grad

    def trainable_ranges(self) -> List[Tuple[int, int]]:
        """Merged [start, end) element ranges of the flat buffers that belong to trainable params."""
        out: List[List[int]] = []
        for name, (o, st, _) in self._slots.items():
            if not self._params[name].requires_grad:
                continue
            n = ((math.prod(st) + ALIGN - 1) // ALIGN) * ALIGN
            if out and out[-1][1] == o:
                out[-1][1] = o + n
            else:
                out.append([o, o + n])
        return [(a, b) for a, b in out]

    def expose_grads(self):
        """Make .grad of every trainable Parameter a view of the flat gradient buffer."""
        for name, p in self._params.items():
            p.grad = self._gviews[name] if p.requires_grad else None

    def grads_busy_until(self, ev):
        """dist.ShardedRaven: an optimizer update on another stream reads the gradients until `ev` (None: no longer): zero_grad goes behind it."""
        self._grads_busy = ev

    def zero_grad(self, set_to_none=True):
        ev, self._grads_busy = self._grads_busy, None
        if ev is not None:            # an optimizer update that runs on another stream under the next forward (dist.ShardedRaven, one rank) is
            self._stream().wait_event(ev)      # still reading the gradients: clear them behind it
        self.gflat.zero_()
        if set_to_none:
            for p in self._params.values():
                p.grad = None

    def requires_grad_(self, flag=True):
        for p in self._params.values():
            p.requires_grad = flag
        return self.owner

    # ------------------------------------------------------------------ regions --------------------
    def tail_offset(self) -> int:
        """Flat offset (multiple of 4096) from which every parameter belongs to up_blocks / mid_block / the output head:
        their gradients are complete once the backward has passed the mid block, and the forward does not read them
        before the mid block -- the hook points of the data-parallel overlap (dist.ShardedRaven)."""
        return self.region_bounds()[-1][0]

    def region_bounds(self):
        """Three contiguous ranges of the flat buffers (cuts are multiples of 4096) ordered as the forward first needs them
        and as the backward finishes them last-to-first -- the units of the data-parallel overlap (dist.ShardedRaven):
          0: conv_in, embeddings, down_blocks.0 .. n-2      read first by the forward, gradients complete last
          1: the last (widest) down block                     (SDXL: 757 M of the 830 M "head" parameters)
          2: up_blocks, mid_block, output head                read from the mid block on, gradients complete first"""
        if self._regions is None:
            last = len(self.cfg.block_out_channels) - 1
            up4 = lambda o: ((o + 4095) // 4096) * 4096
            c1 = up4(min(o for n, (o, _, _) in self._slots.items() if n.startswith(f"down_blocks.{last}.")))
            c2 = up4(min(o for n, (o, _, _) in self._slots.items() if n.startswith("up_blocks.")))
            self._regions = [(0, c1), (c1, c2), (c2, self.flat_numel)]
        return self._regions

    # ------------------------------------------------------------------ the W^T mirror -------------
    def mark_params_dirty(self):
        """Call after parameters were modified behind torch's back (the HIP optimizers do)."""
        self._wt_dirty = True

    def _refresh_table(self, lo, hi):
        """Job table (device int64 [njobs][8], see az_transpose_multi_bf16) of the W^T copies whose LAST element lies in [lo, hi),
        built once per (lo, hi): the flat buffers never move."""
        key = (lo, hi)
        tab = self._wt_tables.get(key)
        if tab is not None:
            return tab
        rows_, tiles, loose = [], 0, []
        p0, t0 = self.pflat.data_ptr(), self.wtflat.data_ptr()

        def add(src_off, dst_off, R, C, ld_src, ld_dst):
            nonlocal tiles
            if (R | C | ld_src | ld_dst) & 7 or (p0 + 2 * src_off) & 15 or (t0 + 2 * dst_off) & 15:
                loose.append((src_off, dst_off, R, C, ld_src, ld_dst))      # odd shapes (test configurations): one launch each
                return
            tc = (C + 63) // 64
            rows_.append([p0 + 2 * src_off, t0 + 2 * dst_off, R, C, ld_src, ld_dst, tiles, tc])
            tiles += tc * ((R + 63) // 64)
        for o, rows, cols in self._wt_jobs:                 # [N][K] -> [K][N]
            n = rows * cols
            if lo <= o + n - 1 < hi:
                add(o, o, rows, cols, cols, rows)
        for o, co, ci in self._wt_conv_jobs:                # [Cout][9][Cin] -> [Cin][9][Cout], one job per tap
            n = co * 9 * ci
            if lo <= o + n - 1 < hi:
                for tap in range(9):
                    add(o + tap * ci, o + tap * co, co, ci, 9 * ci, 9 * co)
        tab = (torch.tensor(rows_, dtype=torch.int64, device=self.device) if rows_ else None, len(rows_), tiles, loose)
        self._wt_tables[key] = tab
        return tab

    def refresh_region(self, lo, hi):
        """W^T copies of the weights whose LAST element lies in [lo, hi), in ONE launch.  Region cuts are 4096-aligned, not
        parameter-aligned: a weight straddling a cut is complete only once the later region has been all-gathered, so it
        belongs to that region's refresh."""
        tab, njobs, tiles, loose = self._refresh_table(lo, hi)
        st = ctypes.c_void_p(self._stream().cuda_stream)
        if njobs:
            lib().call("az_transpose_multi_bf16", ctypes.c_void_p(tab.data_ptr()), njobs, tiles, st)
        p0, t0 = self.pflat.data_ptr(), self.wtflat.data_ptr()
        for so, do, R, C, ls, ld in loose:
            lib().call("az_transpose_bf16", R, C, ctypes.c_void_p(p0 + 2 * so), ls, ctypes.c_void_p(t0 + 2 * do), ld, st)

    def refresh_transposed(self):
        """Refresh the W^T copies if the parameters changed.  Regions whose all-gather is still in flight
        (set_region_params_event) are skipped; wait_region_params() refreshes them when they have landed."""
        if not self._wt_dirty and self._wt_version == self.pflat._version:
            return
        ev, pend = self._region_events, self._wt_region_pending
        for k, (lo, hi) in enumerate(self.region_bounds()):
            if k in ev:
                pend.add(k)
            else:
                self.refresh_region(lo, hi)
        self._wt_dirty = False
        self._wt_version = self.pflat._version

    def refresh_transposed_async(self, side):
        """The W^T copies are only read by the BACKWARD (data-gradient products): refresh them on the parameter-gradient
        stream `side` while the forward runs; the backward waits for the event (_wait_wt_ready)."""
        if not self._wt_dirty and self._wt_version == self.pflat._version:
            return
        ev = torch.cuda.Event(); ev.record(self._stream()); side.wait_event(ev)
        with torch.cuda.stream(side):
            self.refresh_transposed()
        self.wt_refreshed_on(side)

    def wt_refreshed_on(self, stream):
        """The W^T copies (or whatever else the next backward must wait for) are being written on `stream`: record the ready event there."""
        self._wt_ready = torch.cuda.Event(); self._wt_ready.record(stream)

    def _wait_wt_ready(self):
        ev = self._wt_ready
        if ev is not None:
            self._stream().wait_event(ev)
            self._wt_ready = None

    def transposed_refreshed_externally(self):
        """dist.ShardedRaven refreshed every region's W^T copies itself (on its communication stream, ordered behind the
        all-gathers and ahead of the region events): nothing left to do at the next micro-step."""
        self._wt_dirty = False
        self._wt_version = self.pflat._version
        self._wt_region_pending.clear()

    def set_region_params_event(self, k, ev):
        """dist.ShardedRaven: the parameters of region k are being all-gathered on another stream; `ev` fires when they
        have landed.  Nothing may read them before wait_region_params(k)."""
        self._region_events[k] = ev

    def wait_region_params(self, k):
        ev = self._region_events.pop(k, None)
        if ev is not None:
            self._stream().wait_event(ev)
        pend = self._wt_region_pending
        if k in pend:
            lo, hi = self.region_bounds()[k]
            self.refresh_region(lo, hi)
            pend.discard(k)

    def wait_tail_params(self):
        """Wait for every in-flight parameter all-gather (name kept from the two-region form)."""
        for k in (0, 1, 2):
            self.wait_region_params(k)

    # ------------------------------------------------------------------ state dicts ----------------
    def named_parameters(self):
        for name, _ in self._table:
            yield name, self._params[name]

    def parameters(self):
        for name, _ in self._table:
            yield self._params[name]

    def state_dict(self):
        """The BASE model's tensors (adapters: lora_state_dict)."""
        self.wait_tail_params()
        return {name: self._params[name].detach() for name, _ in self._base_table}

    def lora_state_dict(self):
        self.wait_tail_params()
        return {name: self._params[name].detach() for name, _ in self._table[len(self._base_table):]}

    def load_lora_state_dict(self, sd: Dict[str, torch.Tensor]):
        names = [name for name, _ in self._table[len(self._base_table):]]
        if set(sd) != set(names):
            raise KeyError(f"adapter tensors do not match this UNet's LoraSpec: {sorted(set(sd) ^ set(names))[:4]} ...")
        with torch.no_grad():
            for name in names:
                if tuple(sd[name].shape) != tuple(self._params[name].shape):
                    raise ValueError(f"{name}: shape {tuple(sd[name].shape)} != {tuple(self._params[name].shape)}")
                self._params[name].copy_(sd[name].to(device=self.device, dtype=BF16))
        self._wt_dirty = True
        return self.owner

    def init_lora(self, seed: int):
        """B = 0; A ~ U(-1/sqrt(K), 1/sqrt(K)) (K = the fan-in: 9 Cin for a 3x3 convolution) drawn on the CPU from one generator seeded with `seed`, in table order.
        A DoRA magnitude is written as 0 here; AozoraUNet.init_lora sets it to the row norms behind this (dora.DoraState.refresh(init=True))."""
        g = torch.Generator().manual_seed(int(seed))
        sd = {}
        for name, shape in self._table[len(self._base_table):]:
            if name.endswith(".lora_A.weight"):
                sd[name] = (torch.rand(shape, generator=g) * 2.0 - 1.0) / math.sqrt(math.prod(shape[1:]))
            else:
                sd[name] = torch.zeros(shape)
        return self.load_lora_state_dict(sd)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict=True):
        with torch.no_grad():
            for name, _ in self._base_table:
                if name not in sd:
                    if strict:
                        raise KeyError(name)
                    continue
                self._params[name].copy_(sd[name].to(device=self.device, dtype=BF16))
        self._wt_dirty = True
        return self.owner
