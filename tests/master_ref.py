"""Numpy restatement of az_adamw_flat_master (csrc/az_optim.hip): elem_ref.adamw_bits' arithmetic with the fp32 master w as the
parameter operand instead of float(p).  The kernel writes w = pp and p = bf16(pp), round to nearest even; p is never read."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import elem_ref as R        # noqa: E402


def adamw_master_bits(w, g, m, v, hyper, coef=None):
    """w fp32, g bf16 | fp32, m / v bf16 | fp32 | fp16 torch CPU tensors, hyper a float32 numpy vector (elem_ref.adamw_hyper), coef None
    or a float -> (p bf16, w fp32, m, v) new tensors.  One fused multiply-add (exp_avg); every other product, quotient, sqrt and sum
    rounded to fp32; a bf16 gradient times the coefficient is rounded to bf16 again."""
    mdtype = {torch.bfloat16: 0, torch.float32: 1, torch.float16: 2}[m.dtype]
    f = np.float32
    b1, b2, eps, wdf, step, sbc2 = (f(hyper[i]) for i in range(1, 7))
    omb1, omb2 = f(1.0) - b1, f(1.0) - b2
    with np.errstate(all="ignore"):
        gr = g.float().numpy() * (f(coef) if coef is not None else f(1.0))
        if g.dtype == torch.bfloat16:
            gr = R.bf16_round_np(gr)
        mm = R.fma32(gr, np.full_like(gr, omb1), m.float().numpy() * b1)
        vv = v.float().numpy() * b2
        vv = vv + ((omb2 * gr) * gr)
        pp = w.numpy().astype(np.float32) * wdf
        denom = np.sqrt(vv) / sbc2 + eps
        pp = pp + ((-step * mm) / denom)
    pp = np.ascontiguousarray(pp, dtype=np.float32)
    return R.bits_to_bf16(R.bf16_bits_np(pp)), torch.from_numpy(pp.copy()), R._store(mm, mdtype), R._store(vv, mdtype)
