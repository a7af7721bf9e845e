"""DoRA, weight-decomposed LoRA (INTEGRATION.md "DoRA"; Liu et al., arXiv 2402.09353; not in the reference, whose train.py is full
fine-tuning only): the derived state of the magnitudes.  Every adapted linear W [N][K] with adapters A, B and the trainable magnitude
m = `<module>.dora_scale` has two fp32 vectors, inv[o] = 1 / || (W + s B A)[o][:] || and the gain g[o] = float(m[o]) inv[o].  They are
a pure function of (W, A, B, m) -- derived state like the W^T copies, not parameters -- and are written by az_dora_norm_bf16
(csrc/az_lora.hip) in ONE launch over a job table built once from the flat parameter store.  Host-side placement only.

Unlike the W^T copies the gains are read by the FORWARD: refresh() goes behind whatever changed W, A, B or m, on the stream that
changed them, ahead of the next forward (recorded, replayed or eager).  AozoraUNet issues it behind init_lora (with init: m = the row
norms), load_lora_state_dict and -- once adapters have been loaded or drawn: the gains mean nothing before -- load_state_dict; the
flat optimizers (dist.ShardedRaven / ShardedTitan, `optimizer.dora`) issue it inside step() behind the update of the adapters' range; a module optimizer's step() is followed by refresh() in the loop.  Whoever
writes parameters through torch calls refresh() too.  Exactly one launch per optimizer step, none per micro-step; nothing of it goes into
a training state.
"""
from __future__ import annotations

from typing import List, Tuple

import torch

from . import ops
from ._lib import AozoraError
from .lora_norm import s_bits
from .unet_spec import LORA_RANKS

SUFFIX = ".dora_scale"
TILE_ROWS = 64          # output rows a workgroup of az_dora_norm_bf16 owns


def check_row(row, what="row"):
    """One row of the job table against the rules of az_dora_norm_bf16 (the kernel skips a row that breaks one; the builder refuses
    it): AozoraError."""
    w, a, b, m, g, inv, r, K, N = row[:9]
    if r not in LORA_RANKS or K <= 0 or N <= 0 or K % 8 or N % 8 or K > (1 << 24) or N > (1 << 24):
        raise AozoraError(f"dora norm: {what} has rank {r}, K {K}, N {N}: rank one of {LORA_RANKS}, K and N positive multiples of 8")
    if not (w and a and b and m and g and inv) or (w | a | b) % 16 or m % 2 or (g | inv) % 4:
        raise AozoraError(f"dora norm: {what} has a null or misaligned address")


def job_rows(unet, g_ptr: int, inv_ptr: int) -> Tuple[List[List[int]], List[str], List[int], int]:
    """-> (rows of the job table, module names, the offset of every module in the gain vectors, tiles), one row per magnitude in the
    order of the adapter table: [address of W, A, B, m, g, inv, r, K, N, fp32 bits of alpha / rank, first tile, 0].  The gains of the
    modules lie side by side in table order, so those of a fused group are one contiguous vector in its part order."""
    spec = unet.lora
    p0 = unet.pflat.data_ptr()
    rows, modules, offs, off, tiles = [], [], [], 0, 0
    for name, _ in unet._table:
        if not name.endswith(SUFFIX):
            continue
        m = name[:-len(SUFFIX)]
        ow, stw, _ = unet._slots[m + ".weight"]
        oa, sta, _ = unet._slots[m + ".lora_A.weight"]
        ob, stb, _ = unet._slots[m + ".lora_B.weight"]
        om, stm, _ = unet._slots[name]
        if len(stw) != 2 or len(sta) != 2:
            raise AozoraError(f"dora norm: {m} is no Linear (weight {stw}): DoRA on the convolutions is a follow-up")
        (N, K), r = stw, sta[0]
        if sta != (r, K) or stb != (N, r) or stm != (N,):
            raise AozoraError(f"dora norm: {m} has W {stw}, A {sta}, B {stb}, magnitude {stm}")
        row = [p0 + 2 * ow, p0 + 2 * oa, p0 + 2 * ob, p0 + 2 * om, g_ptr + 4 * off, inv_ptr + 4 * off, r, K, N, s_bits(spec.scale_of(m)), tiles, 0]
        check_row(row, m)
        rows.append(row); modules.append(m); offs.append(off)
        off += N
        tiles += (N + TILE_ROWS - 1) // TILE_ROWS
    if not rows:
        raise AozoraError("dora norm: this UNet carries no magnitude (LoraSpec(dora=True))")
    return rows, modules, offs, tiles


class DoraState:
    """The gains of one AozoraUNet: two fp32 device vectors at fixed addresses and the job table, built once.  `launches` counts the
    passes issued."""

    def __init__(self, unet):
        if unet.lora is None or not unet.lora.dora:
            raise AozoraError("DoraState needs a UNet with LoraSpec(dora=True)")
        self.unet = unet
        total = sum(shape[0] for name, shape in unet._table if name.endswith(SUFFIX))
        self.g = torch.zeros(total, dtype=torch.float32, device=unet.device)
        self.inv = torch.zeros(total, dtype=torch.float32, device=unet.device)
        rows, self.modules, offs, self.tiles = job_rows(unet, self.g.data_ptr(), self.inv.data_ptr())
        self.offset = dict(zip(self.modules, offs))
        self.width = {m: row[8] for m, row in zip(self.modules, rows)}
        self.n = len(rows)
        self.table = torch.tensor(rows, dtype=torch.int64, device=unet.device)
        # the gain of a part of a fused group that carries no adapter (targets narrowed to "to_q, to_v"): fmaf(1, v, 0) = v
        self.ones = torch.ones(max(self.width.values()), dtype=torch.float32, device=unet.device)
        self.launches = 0

    def refresh(self, stream=None, init=False):
        """One launch: g and inv of every module from the current W, A, B, m; init: m = bf16(row norm) first (the magnitudes' initial value)."""
        ops.dora_norm(self.table, self.tiles, init, stream)
        self.launches += 1

    def gains(self, modules: List[str]):
        """(g, inv) of adjacent modules as one vector each."""
        o = self.offset[modules[0]]
        n = 0
        for m in modules:
            if self.offset[m] != o + n:
                raise AozoraError(f"dora: the gains of {modules} are not adjacent")
            n += self.width[m]
        return self.g[o:o + n], self.inv[o:o + n]
