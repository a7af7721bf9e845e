"""Numpy restatement of the fp32 EMA of the weights (csrc/az_optim.hip az_ema_flat, aozora_sdxl_training_amd/ema.py): the
three-operation update in np.float32, the decay schedule, bf16 -> f32 by bit shift (as elem_ref.py reads bf16)."""
import numpy as np


def bf16_bits_to_f32(bits):
    """uint16 bf16 bit patterns -> float32 (exact: the bits move into the upper half)."""
    return (np.ascontiguousarray(bits).view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def torch_bf16_to_f32(t):
    """CPU bf16 torch tensor (any shape) -> float32 numpy array of that shape, by bit shift."""
    import torch
    b = t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
    return bf16_bits_to_f32(b).reshape(tuple(t.shape))


def check_decay(decay):
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not (0.0 < decay < 1.0):
        raise ValueError(f"decay must be a real number with 0 < decay < 1, got {decay!r}")
    return float(decay)


def decay_at(decay, k, warmup=True):
    """d_k of update number k = 1, 2, ... in float64."""
    decay = check_decay(decay)
    return min(decay, (1.0 + k) / (10.0 + k)) if warmup else decay


def omd_at(decay, k, warmup=True):
    """fp32(1 - d_k): float64 on the host, rounded to fp32 once."""
    return np.float32(1.0 - decay_at(decay, k, warmup))


def omd_bits(decay, k, warmup=True):
    return int(np.array([omd_at(decay, k, warmup)], dtype=np.float32).view(np.uint32)[0])


def ema_update(e, p_f32, omd):
    """e - omd * (e - p): three fp32 operations, each rounded.  e, p_f32 float32 arrays; -> new float32 array."""
    e = np.asarray(e, dtype=np.float32)
    p = np.asarray(p_f32, dtype=np.float32)
    omd = np.float32(omd)
    with np.errstate(all="ignore"):
        t = e - p
        t = omd * t
        return (e - t).astype(np.float32)


def ema_update_f64(e, p, omd):
    """The same recurrence in float64 with the same fp32 omd (the yardstick of the error bound)."""
    e = np.asarray(e, dtype=np.float64)
    return e - np.float64(np.float32(omd)) * (e - np.asarray(p, dtype=np.float64))


def replay(snapshots, decay, warmup=True, start=None, k0=0):
    """EMA over parameter snapshots {name: bf16 torch tensor}: start (default: float32 of the first snapshot = the value at
    construction), then one update per later snapshot.  -> list of {name: float32 array}, one per update."""
    e = start if start is not None else {n: torch_bf16_to_f32(t) for n, t in snapshots[0].items()}
    out = []
    for k, snap in enumerate(snapshots[1:], start=k0 + 1):
        omd = omd_at(decay, k, warmup)
        e = {n: ema_update(e[n], torch_bf16_to_f32(snap[n]), omd) for n in e}
        out.append(e)
    return out
