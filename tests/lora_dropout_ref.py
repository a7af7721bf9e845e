"""Numpy / torch restatement of LoRA dropout (include/aozora_hip.h az_lora_dropout_bf16, INTEGRATION.md "LoRA dropout"): the three masks
on tests/sr_ref.sr_bits16, the masked inner activation u' bit for bit, and a LoraDropoutRefUNet that applies the same masks to the
adapters of the oracle.  The product never imports this file.

For a module with id `mid` (the index of `<module>.weight` in unet_spec.param_table), rank r and rows = B * rows_per_sample:
    keep_net[row][j]   16 bits of e = (mid << 35) + row r + j, domain 0x10A1, >= t_net
    keep_rank[b][j]    16 bits of e = (mid << 35) + b r + j,   domain 0x10A2, >= t_rank        b = row // rows_per_sample
    keep_mod           16 bits of e = mid << 35,               domain 0x10A3, >= t_mod
    u'[row][j] = bf16(fp32(u) * inv) where all three keep, else +0.0; inv = float32(1 / ((1 - p_net)(1 - p_rank)))
t = clamp(int(p 65536 + 0.5), 1, 65535) for p > 0; p = 0: t = 0, nothing drawn, nothing multiplied."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import elem_ref as R            # noqa: E402
import sr_ref as S              # noqa: E402
import lora_conv_ref as CR      # noqa: E402

DOM_NET, DOM_RANK, DOM_MOD = 0x10A1, 0x10A2, 0x10A3


def threshold(p):
    if p <= 0.0:
        return 0
    return min(65535, max(1, int(p * 65536 + 0.5)))


def thresholds(p_net, p_rank, p_mod):
    return threshold(p_net), threshold(p_rank), threshold(p_mod)


def inv_of(p_net, p_rank):
    return np.float32(1.0 / ((1.0 - p_net) * (1.0 - p_rank)))


def keep_net(seed, step, mid, rows, r, t):
    """-> bool [rows][r]"""
    if t == 0:
        return np.ones((rows, r), dtype=bool)
    e = (np.int64(mid) << 35) + np.arange(rows * r, dtype=np.int64)
    return (S.sr_bits16(seed, step, DOM_NET, e) >= t).reshape(rows, r)


def keep_rank(seed, step, mid, nsamples, r, t):
    """-> bool [nsamples][r]"""
    if t == 0:
        return np.ones((nsamples, r), dtype=bool)
    e = (np.int64(mid) << 35) + np.arange(nsamples * r, dtype=np.int64)
    return (S.sr_bits16(seed, step, DOM_RANK, e) >= t).reshape(nsamples, r)


def keep_mod(seed, step, mid, t):
    if t == 0:
        return True
    return bool(S.sr_bits16(seed, step, DOM_MOD, np.array([np.int64(mid) << 35], dtype=np.int64))[0] >= t)


def mask(seed, step, mid, rows, rows_per_sample, r, ts):
    """The product of the three masks of one module -> bool [rows][r]."""
    assert rows % rows_per_sample == 0
    t_net, t_rank, t_mod = ts
    m = keep_net(seed, step, mid, rows, r, t_net)
    m = m & np.repeat(keep_rank(seed, step, mid, rows // rows_per_sample, r, t_rank), rows_per_sample, axis=0)
    return m & keep_mod(seed, step, mid, t_mod)


def group_mask(seed, step, mids, rows, rows_per_sample, r, ts):
    """The parts of a fused group side by side -> bool [rows][len(mids) r]."""
    return np.concatenate([mask(seed, step, mid, rows, rows_per_sample, r, ts) for mid in mids], axis=1)


def apply_bits(u_bits, r, rows_per_sample, mids, ts, inv, seed, step):
    """az_lora_dropout_bf16 on uint16 bf16 bits [rows][len(mids) r] -> uint16 bits.  inv is applied iff t_net or t_rank is on."""
    u_bits = np.asarray(u_bits, dtype=np.uint16)
    rows = u_bits.shape[0]
    assert u_bits.shape[1] == len(mids) * r
    m = group_mask(seed, step, mids, rows, rows_per_sample, r, ts)
    if ts[0] or ts[1]:
        x = (u_bits.astype(np.uint32) << 16).view(np.float32)
        with np.errstate(all="ignore"):
            kept = R.bf16_bits_np(x * np.float32(inv)).reshape(u_bits.shape)
    else:
        kept = u_bits
    return np.where(m, kept, np.uint16(0)).astype(np.uint16)


def module_ids(cfg):
    """{module: index of <module>.weight in unet_spec.param_table(cfg)}"""
    from aozora_sdxl_training_amd.unet_spec import param_table
    return {n[:-len(".weight")]: i for i, (n, _) in enumerate(param_table(cfg)) if n.endswith(".weight")}


class LoraDropoutRefUNet(CR.LoraConvRefUNet):
    """LoraConvRefUNet whose adapters carry the dropout masks of (seed, self.step) on their inner activation: u' = m u inv, so that
    autograd gives du' = m du inv, dA = du'^T x, dB = s dy^T u', dx += du' A.  self.step None = no masks (eval).  `mids`: module_ids of
    the product's configuration."""

    def __init__(self, cfg, params, spec, mids, seed, step=None):
        super().__init__(cfg, params, spec)
        self.mids, self.seed, self.step = mids, seed, step
        self.ts = thresholds(spec.dropout, spec.rank_dropout, spec.module_dropout)
        self.inv = float(inv_of(spec.dropout, spec.rank_dropout))
        self.seen = {}          # module -> keep_mod of the last forward

    def _m(self, name, rows, rows_per_sample, r):
        self.seen[name] = keep_mod(self.seed, self.step, self.mids[name], self.ts[2])
        return torch.from_numpy(mask(self.seed, self.step, self.mids[name], rows, rows_per_sample, r, self.ts))

    def _lin(self, x, name, bias=True):
        A = self.p.get(name + ".lora_A.weight")
        if A is None or self.step is None:
            return super()._lin(x, name, bias)
        y = F.linear(x, self.p[name + ".weight"], self.p[name + ".bias"] if bias else None)
        u = F.linear(x, A)                                   # [B][T][r]: row = b T + t
        Bn, T, r = u.shape
        m = self._m(name, Bn * T, T, r).reshape(Bn, T, r).to(u.dtype)
        u = torch.where(m > 0, u * self.inv, torch.zeros_like(u))
        return y + self.spec.scale_of(name) * F.linear(u, self.p[name + ".lora_B.weight"])

    def _conv(self, x, name, stride=1, pad=1):
        A = self.p.get(name + ".lora_A.weight")
        if A is None or self.step is None:
            return super()._conv(x, name, stride, pad)
        y = F.conv2d(x, self.p[name + ".weight"], self.p[name + ".bias"], stride=stride, padding=pad)
        u = F.conv2d(x, A, padding=1) if A.dim() == 4 else F.conv2d(x, A[:, :, None, None])       # [B][r][H][W]: row = (b H + h) W + w
        Bn, r, H, W = u.shape
        m = self._m(name, Bn * H * W, H * W, r).reshape(Bn, H, W, r).permute(0, 3, 1, 2).to(u.dtype)
        u = torch.where(m > 0, u * self.inv, torch.zeros_like(u))
        return y + self.spec.scale_of(name) * F.conv2d(u, self.p[name + ".lora_B.weight"][:, :, None, None])
