"""NOISE_MODE -- noise offset, multi-resolution ("pyramid") noise and input perturbation (options outside the reference, whose
trainer carries NOISE_MODE = "normal" and never reads it).  parse_noise_mode reads `kind[:key=value[,key=value...]]` -- kinds normal,
offset, pyramid; keys offset, levels, discount, perturb -- into a NoiseSpec, the one parser of the trainer and TrainStep.  With eps
the base draw (schedule.generate_noise, unchanged) the shaped noise of sample b is

    u[b,c,y,x] = eps[b,c,y,x] + offset * o[b,c] + sum_{l=1..levels} discount^l * up_l(z_l)[b,c,y,x]
    eps'[b]    = u[b] / std(u[b])    for pyramid (unbiased std over the sample's C*H*W elements, about their mean), u[b] otherwise
    mix noise  = eps' + perturb * xi      (enters the noisy latents only; the target is built from eps')

o = randn(B,C), z_l = randn(B,C,ceil(H/2^l),ceil(W/2^l)), xi = randn(B,C,H,W); up_l is bilinear resampling to (H,W) with half-pixel
centres.  The std is per sample, never over the batch: data-parallel ranks take rows of the global draw, and a sample's noise must not
depend on which other samples share its rank.  draw_aux makes the draws on the CPU from (seed, micro_step) alone -- one seeding
domain per draw -- so a resumed run needs no new checkpoint state.  The element math is az_noise_shape's and az_noise_target_ex's
(csrc/az_elem.hip; INTEGRATION.md "Noise modes")."""
from __future__ import annotations

import math
import struct
from typing import List, NamedTuple, Optional

import torch

from .schedule import seeded_torch_generator

KINDS = ("normal", "offset", "pyramid")
KEYS = ("offset", "levels", "discount", "perturb")
MAX_LEVELS = 8
# seeding domains of schedule.seeded_torch_generator(device, seed, micro_step, DOMAIN); the rectified-flow jitter holds 0x5D1
DOMAIN_OFFSET = 0x0FF5
DOMAIN_PERTURB = 0x9E7B
DOMAIN_LEVEL = 0x1E00                      # level l (1-based) draws under DOMAIN_LEVEL + l


class NoiseSpec(NamedTuple):
    kind: str            # one of KINDS
    offset: float        # weight of the per-(sample, channel) draw o; 0: none
    levels: int          # number of pyramid levels; 0 unless kind == "pyramid"
    discount: float      # level l weighs discount^l
    perturb: float       # weight of xi in the noise that enters the noisy latents; 0: none

    @property
    def normalises(self):
        return self.kind == "pyramid"

    @property
    def needs_shape(self):
        """az_noise_shape has something to add (or sums to form)."""
        return self.offset > 0.0 or self.levels > 0

    @property
    def needs_aux(self):
        return self.needs_shape or self.perturb > 0.0

    def describe(self):
        if self.kind == "pyramid":
            s = f"pyramid ({self.levels} levels, discount {self.discount:g}" + (f", offset {self.offset:g}" if self.offset > 0 else "") + ", per-sample unit std)"
        elif self.kind == "offset":
            s = f"offset ({self.offset:g})"
        else:
            s = "normal"
        return s + (f", input perturbation {self.perturb:g}" if self.perturb > 0 else "")


def _number(key, text, integer=False):
    try:
        v = int(text) if integer else float(text)
    except ValueError:
        raise ValueError(f"NOISE_MODE: {key}={text!r} is not {'an integer' if integer else 'a number'}") from None
    if not math.isfinite(v):
        raise ValueError(f"NOISE_MODE: {key} must be finite, got {text!r}")
    return v


def parse_noise_mode(s) -> NoiseSpec:
    """`kind[:key=value[,key=value...]]`, kind and keys in any letter case; None, "" and "normal" are today's noise.  ValueError for an
    unknown kind or key, a repeated key, a key on the wrong kind, a value that is no number or not finite, and a value out of range
    (offset >= 0, levels 1..8, 0 < discount <= 1, perturb >= 0)."""
    if isinstance(s, NoiseSpec):
        return s
    text = "normal" if s is None or not str(s).strip() else str(s).strip()
    kind, _, rest = text.partition(":")
    kind = kind.strip().lower()
    if kind not in KINDS:
        raise ValueError(f"NOISE_MODE: unknown noise {kind!r} (known: {', '.join(KINDS)})")
    opts = {}
    for item in (rest.split(",") if rest.strip() else []):
        key, eq, val = item.partition("=")
        key, val = key.strip().lower(), val.strip()
        if not eq or key not in KEYS or key in opts:
            raise ValueError(f"NOISE_MODE: cannot read {item.strip()!r} (keys: {', '.join(KEYS)}, each once, as key=value)")
        opts[key] = val
    if "offset" in opts and kind == "normal":
        raise ValueError("NOISE_MODE: offset belongs to offset and pyramid, not to normal")
    for key in ("levels", "discount"):
        if key in opts and kind != "pyramid":
            raise ValueError(f"NOISE_MODE: {key} belongs to pyramid, not to {kind}")
    offset = _number("offset", opts["offset"]) if "offset" in opts else (0.05 if kind == "offset" else 0.0)
    levels = _number("levels", opts["levels"], integer=True) if "levels" in opts else (6 if kind == "pyramid" else 0)
    discount = _number("discount", opts["discount"]) if "discount" in opts else 0.3
    perturb = _number("perturb", opts["perturb"]) if "perturb" in opts else 0.0
    if offset < 0.0:
        raise ValueError(f"NOISE_MODE: offset must be at least 0, got {opts['offset']!r}")
    if kind == "pyramid" and not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"NOISE_MODE: levels must lie in 1..{MAX_LEVELS}, got {opts['levels']!r}")
    if not 0.0 < discount <= 1.0:
        raise ValueError(f"NOISE_MODE: discount must lie in (0, 1], got {opts['discount']!r}")
    if perturb < 0.0:
        raise ValueError(f"NOISE_MODE: perturb must be at least 0, got {opts['perturb']!r}")
    return NoiseSpec(kind, float(offset), int(levels), float(discount), float(perturb))


def level_shapes(H, W, levels):
    """(h_l, w_l) = (ceil(H / 2^l), ceil(W / 2^l)) for l = 1..levels."""
    return [(-(-H // (1 << l)), -(-W // (1 << l))) for l in range(1, levels + 1)]


def partial_blocks(HW):
    """Blocks per sample of az_noise_shape, i.e. pairs per sample of its partial sums."""
    return min((HW + 255) // 256, 64)


class LevelRow(NamedTuple):
    offset: int          # first float of the level in the packed buffer
    h: int
    w: int
    weight: float        # discount^l rounded to fp32


def level_table(B, C, H, W, spec: NoiseSpec):
    """-> ([LevelRow per level], floats of the packed level fields): level l lies at its offset as [B][C][h_l][w_l]."""
    rows, total = [], 0
    for l, (h, w) in enumerate(level_shapes(H, W, spec.levels), start=1):
        wt = struct.unpack("<f", struct.pack("<f", spec.discount ** l))[0]
        rows.append(LevelRow(total, h, w, wt))
        total += B * C * h * w
    return rows, total


def table_tensor(rows: List[LevelRow]):
    """The int32 [levels][4] table az_noise_shape reads on the device: offset, h, w, bits of the fp32 weight (CPU tensor)."""
    flat = []
    for r in rows:
        flat += [r.offset, r.h, r.w, struct.unpack("<i", struct.pack("<f", r.weight))[0]]
    return torch.tensor(flat, dtype=torch.int32).view(-1, 4)


class NoiseAux(NamedTuple):
    """The draws of one micro-step beside the base noise, fp32 on the CPU; None for what the spec does not use."""
    o: Optional[torch.Tensor]                 # (B, C)
    z: Optional[List[torch.Tensor]]           # [(B, C, h_l, w_l) for l = 1..levels]
    xi: Optional[torch.Tensor]                # (B, C, H, W)

    def rows(self, sl):
        """The data-parallel share: these rows of every draw."""
        return NoiseAux(None if self.o is None else self.o[sl], None if self.z is None else [z[sl] for z in self.z],
                        None if self.xi is None else self.xi[sl])

    def packed(self):
        """The level fields as the one buffer az_noise_shape reads (level_table's layout)."""
        return torch.cat([z.reshape(-1) for z in self.z])


def draw_aux(spec: NoiseSpec, shape, seed, micro_step) -> Optional[NoiseAux]:
    """The draws of the GLOBAL micro-batch `shape` = (B, C, H, W), each from its own generator seeded by (seed, micro_step, domain);
    None (and nothing drawn) where the spec needs none."""
    if not spec.needs_aux:
        return None
    B, C, H, W = (int(v) for v in shape)

    def randn(size, domain):
        return torch.randn(size, dtype=torch.float32, generator=seeded_torch_generator("cpu", seed, micro_step, domain))
    o = randn((B, C), DOMAIN_OFFSET) if spec.offset > 0.0 else None
    z = [randn((B, C, h, w), DOMAIN_LEVEL + l) for l, (h, w) in enumerate(level_shapes(H, W, spec.levels), start=1)] if spec.levels else None
    xi = randn((B, C, H, W), DOMAIN_PERTURB) if spec.perturb > 0.0 else None
    return NoiseAux(o, z, xi)
