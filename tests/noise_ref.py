"""Restatements of the NOISE_MODE kernels (csrc/az_elem.hip: noise_shape_kernel, noise_target_ex_kernel) with per-element error
bounds, in the manner of tests/elem_ref.py (whose `bound`, bf16 helpers and K table this file uses and does not edit).  The product
never imports this file; tests/test_noise_gpu.py compares the HIP kernels against it and tests/test_noise_ref_cpu.py checks it
without a GPU.

Two kinds of reference:
  * float64 (numpy): what aozora_sdxl_training_amd/noise.py specifies -- u = eps + offset o + sum_l discount^l up_l(z_l), the
    per-sample unbiased standard deviation, the mix and the three targets.  Each comes with S, the sum of the magnitudes of the
    terms the kernel combined in fp32 for that element;
  * bit-level (numpy float32, one operator per kernel operation, in the kernel's order): the library is built without fast-math
    and the kernels forbid contraction, so numpy's float32 +, *, / and sqrt restate them exactly -- the wave butterfly of block_sum
    included (v[i] + v[i ^ o] for o = 32 .. 1 is the same sum in every lane, since fp32 addition commutes).

K, the count of fp32 roundings that reach one output (the kernels' comments derive the same numbers):
  shaping          8 + levels   a tap weight (1), tap * weight (1), the row sum (1), times the row weight (its rounding and the
                                product: 2), the column sum (1), times weight_l (its rounding to fp32 on the host and the product: 2),
                                the sum into u (1), the sums of the levels behind it (levels - l);  3 without levels (offset rounded
                                to fp32, its product, its sum).  Never above 4 + 12 levels.
  partial sums     A + 1        A = shape_chain: a thread's additions, 6 butterfly steps, 4 waves (block_sum); + the square
  r_b              relative error (A' + 4) 2^-24 with A' = A + blocks per sample: the chain behind S2
  mix and target   A' + 9       r_b (A' + 4), u r_b, perturb xi, their sum, the coefficient product, the last sum;  5 without
                                normalisation (perturb rounded to fp32 and the four after it)
The fp32 rounding of the stored value itself is `rounding` of elem_ref.bound (half a bf16 ulp for the noisy rows)."""
import numpy as np
import torch

import elem_ref as R
from elem_ref import bf16_bits_np, bf16_round_np, bf16_to_np, bits_to_bf16, bound, f32_rounding     # noqa: F401

F = np.float32


# ---------------- geometry -------------------------------------------------------------------------------------------------------
def level_shapes(H, W, levels):
    return [(-(-H // (1 << l)), -(-W // (1 << l))) for l in range(1, levels + 1)]


def nblk_of(HW):
    return min((HW + 255) // 256, 64)


def shape_chain(C, HW):
    """Longest chain of additions behind one partial sum: pixels per thread x C channels, the butterfly, the block's waves."""
    sweep = nblk_of(HW) * 256
    return (HW + sweep - 1) // sweep * C + 6 + 4


def rb_chain(C, HW):
    """... and behind a sample's S1 / S2: its blocks one after the other on top."""
    return shape_chain(C, HW) + nblk_of(HW)


def _k(name, value):
    R.K.setdefault(name, float(value))
    assert R.K[name] == float(value)
    return name


def k_shape(levels):
    return _k(f"noise_shape_{levels}", 8 + levels if levels else 3)


def k_partial(C, HW):
    return _k(f"noise_partial_{C}_{HW}", shape_chain(C, HW) + 1)


def k_target(C, HW, normalised):
    return _k(f"noise_target_{C}_{HW}_{int(normalised)}", rb_chain(C, HW) + 9 if normalised else 5)


def taps(out, src):
    """Bilinear taps of `out` positions over `src` samples, half-pixel centres, from the integer numerator: source coordinate
    max(((2i+1) src - out) / (2 out), 0) -> (i0, i1, remainder r): fraction r / (2 out), both taps clamped to the field."""
    i = np.arange(out, dtype=np.int64)
    num = np.maximum((2 * i + 1) * src - out, 0)
    i0 = num // (2 * out)
    r = num - i0 * 2 * out
    i0 = np.minimum(i0, src - 1)
    return i0, np.minimum(i0 + 1, src - 1), r


# ---------------- float64 --------------------------------------------------------------------------------------------------------
def upsample64(z, H, W):
    """z [..., h, w] -> float64 [..., H, W]."""
    z = np.asarray(z, dtype=np.float64)
    h, w = z.shape[-2:]
    y0, y1, ry = taps(H, h)
    x0, x1, rx = taps(W, w)
    fy, fx = (ry / (2.0 * H))[:, None], (rx / (2.0 * W))[None, :]
    top = z[..., y0, :][..., :, x0] * (1.0 - fx) + z[..., y0, :][..., :, x1] * fx
    bot = z[..., y1, :][..., :, x0] * (1.0 - fx) + z[..., y1, :][..., :, x1] * fx
    return top * (1.0 - fy) + bot * fy


def shape64(eps, o, offset, zs, discount):
    """eps [B][C][H][W], o [B][C] or None, zs the level fields (l = 1 first) -> u float64, S."""
    e = np.asarray(eps, dtype=np.float64)
    H, W = e.shape[-2:]
    u, S = e.copy(), np.abs(e)
    if o is not None:
        t = float(offset) * np.asarray(o, dtype=np.float64)[:, :, None, None]
        u, S = u + t, S + np.abs(t)
    for l, z in enumerate(zs or [], start=1):
        wt = float(discount) ** l
        u = u + wt * upsample64(z, H, W)
        S = S + wt * upsample64(np.abs(np.asarray(z, dtype=np.float64)), H, W)
    return u, S


def std64(u):
    """Unbiased standard deviation of every sample about its mean -> [B]."""
    u = np.asarray(u, dtype=np.float64)
    return u.reshape(u.shape[0], -1).std(axis=1, ddof=1)


def shaped64(spec, eps, aux):
    """noise.py's formula for a NoiseSpec and a NoiseAux -> (eps', mix noise) float64."""
    u, _ = shape64(eps.numpy(), None if aux is None or aux.o is None else aux.o.numpy(), spec.offset,
                   [] if aux is None or aux.z is None else [z.numpy() for z in aux.z], spec.discount)
    if spec.normalises:
        u = u / std64(u)[:, None, None, None]
    mix = u if aux is None or aux.xi is None else u + spec.perturb * aux.xi.numpy().astype(np.float64)
    return u, mix


def partials64(u):
    """The sums of each block's elements in float64 -> (partial [B][nblk][2], S [B][nblk][2])."""
    return _partials(np.asarray(u, dtype=np.float64), np.float64), _partials(np.abs(np.asarray(u, dtype=np.float64)), np.float64)


def target_ex64(mode, lat, u, ca, cb, normalise, xi=None, perturb=0.0):
    """lat [B][C][HW] bf16 (torch), u [B][C][HW] fp32 (torch; the kernel's input), ca / cb [B] fp32 -> dict(noisy [B][HW][C], S_noisy,
    target [B][C][HW], S_target) in float64.  The bf16 coefficient x latent products of the DDPM modes are part of the dataflow (as in
    elem_ref.noise_target_bits), not an approximation."""
    x, x32 = bf16_to_np(lat).astype(np.float64), bf16_to_np(lat)
    uu = u.numpy().astype(np.float64)
    a32, s32 = ca.numpy()[:, None, None], cb.numpy()[:, None, None]
    a, s = a32.astype(np.float64), s32.astype(np.float64)
    with np.errstate(all="ignore"):
        nt = uu / std64(uu)[:, None, None] if normalise else uu
        pz = np.zeros_like(nt) if xi is None else float(perturb) * xi.numpy().astype(np.float64)
        nm = nt + pz
        S_nm = np.abs(nt) + np.abs(pz)
        if mode == 2:
            p1 = a * x
            tg, S_tg = nt - x, np.abs(nt) + np.abs(x)
        else:
            p1 = bf16_round_np(a32 * x32).astype(np.float64)
            if mode == 1:
                q2 = bf16_round_np(s32 * x32).astype(np.float64)
                tg, S_tg = a * nt - q2, np.abs(a * nt) + np.abs(q2)
            else:
                tg, S_tg = nt.copy(), np.abs(nt)
        xt, S_xt = p1 + s * nm, np.abs(p1) + np.abs(s) * S_nm
    t = torch.from_numpy
    return dict(noisy=t(np.ascontiguousarray(xt.transpose(0, 2, 1))), S_noisy=t(np.ascontiguousarray(S_xt.transpose(0, 2, 1))),
                target=t(tg), S_target=t(S_tg))


# ---------------- fp32, the kernels' own order -------------------------------------------------------------------------------------
def shape_bits(eps, o, offset, zs, weights):
    """noise_shape_kernel's u: eps [B][C][H][W] fp32 numpy, o [B][C] or None, zs the level fields, weights their fp32 weights."""
    u = np.ascontiguousarray(eps, dtype=F).copy()
    H, W = u.shape[-2:]
    with np.errstate(all="ignore"):
        if o is not None:
            u = u + F(offset) * np.asarray(o, dtype=F)[:, :, None, None]
        for z, wt in zip(zs or [], weights or []):
            z = np.asarray(z, dtype=F)
            h, w = z.shape[-2:]
            y0, y1, ry = taps(H, h)
            x0, x1, rx = taps(W, w)
            dh, dw = F(2 * H), F(2 * W)
            fy, gy = (ry.astype(F) / dh)[:, None], ((2 * H - ry).astype(F) / dh)[:, None]
            fx, gx = (rx.astype(F) / dw)[None, :], ((2 * W - rx).astype(F) / dw)[None, :]
            t0, t1 = z[..., y0, :][..., :, x0] * gx, z[..., y0, :][..., :, x1] * fx
            b0, b1 = z[..., y1, :][..., :, x0] * gx, z[..., y1, :][..., :, x1] * fx
            top, bot = t0 + t1, b0 + b1
            vt, vb = top * gy, bot * fy
            v = vt + vb
            u = u + F(wt) * v
    assert u.dtype == F
    return u


def _partials(u, dtype):
    """partial[b][block] = (sum u, sum u^2) in noise_shape_kernel's order and geometry, in `dtype`."""
    B, C, H, W = u.shape
    HW = H * W
    gx = nblk_of(HW)
    sweep = gx * 256
    nsw = (HW + sweep - 1) // sweep
    p = np.zeros((B, C, nsw * sweep), dtype=dtype)
    p[:, :, :HW] = u.reshape(B, C, HW)
    out = np.zeros((B, gx, 2), dtype=dtype)
    lane = np.arange(64)
    with np.errstate(all="ignore"):
        for j, q in enumerate((p, p * p)):
            acc = np.zeros((B, sweep), dtype=dtype)
            for s in range(nsw):                       # a thread's pixels, and the channels of each, one after the other
                for c in range(C):
                    acc = acc + q[:, c, s * sweep:(s + 1) * sweep]
            v = acc.reshape(B, gx, 4, 64)
            for o in (32, 16, 8, 4, 2, 1):             # wave_sum: every lane ends with the same sum
                v = v + v[..., lane ^ o]
            r = np.zeros((B, gx), dtype=dtype)
            for w in range(4):                         # block_sum: 0 + wave 0 + wave 1 + ...
                r = r + v[:, :, w, 0]
            out[:, :, j] = r
    return out


def partials_bits(u):
    return _partials(np.ascontiguousarray(u, dtype=F), F)


def rb_bits(partials, C, HW):
    """noise_target_ex_kernel's r_b from the partial sums [B][nblk][2] -> fp32 [B]."""
    part = np.ascontiguousarray(partials, dtype=F)
    with np.errstate(all="ignore"):
        s1 = np.zeros(part.shape[0], dtype=F)
        s2 = np.zeros(part.shape[0], dtype=F)
        for k in range(part.shape[1]):
            s1, s2 = s1 + part[:, k, 0], s2 + part[:, k, 1]
        cnt = F(C) * F(HW)
        m2 = s1 * (s1 / cnt)
        var = (s2 - m2) / (cnt - F(1.0))
        return F(1.0) / np.sqrt(var)


def target_ex_bits(mode, lat, u, ca, cb, cpad, partials=None, xi=None, perturb=0.0):
    """noise_target_ex_kernel: lat [B][C][HW] bf16, u [B][C][HW] fp32, ca / cb [B] fp32 (torch), partials [B][nblk][2] fp32 numpy or
    None, xi [B][C][HW] fp32 torch or None -> noisy [B][HW][cpad] bf16 (padding 0), target [B][C][HW] fp32."""
    x, nt = bf16_to_np(lat), u.numpy()
    B, C, HW = x.shape
    a, s = ca.numpy()[:, None, None], cb.numpy()[:, None, None]
    with np.errstate(all="ignore"):
        if partials is not None:
            nt = nt * rb_bits(partials, C, HW)[:, None, None]
        nm = nt if xi is None else nt + F(perturb) * xi.numpy()
        if mode == 2:
            xt, tg = a * x + s * nm, nt - x
        else:
            xt = bf16_round_np(a * x) + s * nm
            tg = (a * nt - bf16_round_np(s * x)) if mode == 1 else nt.copy()
    noisy = np.zeros((B, HW, cpad), dtype=np.uint16)
    noisy[..., :C] = bf16_bits_np(xt).transpose(0, 2, 1)
    return bits_to_bf16(noisy), torch.from_numpy(np.ascontiguousarray(tg, dtype=F))


# ---------------- inputs -----------------------------------------------------------------------------------------------------------
SHAPES = [(1, 4, 4, 4), (2, 4, 5, 7), (3, 4, 9, 6), (2, 4, 16, 12), (1, 4, 90, 180)]
# (shape, levels): levels 1 and 3 everywhere, 8 where the fields collapse to 1 x 1
CASES = [(s, l) for s in SHAPES for l in (1, 3)] + [(SHAPES[0], 8), (SHAPES[1], 8)]


def draws(shape, levels, seed):
    """eps, o, [z_l], xi (fp32 torch) and lat (bf16) for one case."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn(B, C, H, W, generator=g)
    o = torch.randn(B, C, generator=g)
    zs = [torch.randn(B, C, h, w, generator=g) for h, w in level_shapes(H, W, levels)]
    xi = torch.randn(B, C, H, W, generator=g)
    lat = torch.randn(B, C, H, W, generator=g).bfloat16()
    return eps, o, zs, xi, lat


def coefs(B, mode, seed):
    """ca, cb [B] fp32: bf16-valued for the DDPM modes (schedule.ddpm_coef_tables' dtype), (1 - t, t) for rectified flow."""
    g = torch.Generator().manual_seed(seed + 99)
    t = torch.rand(B, generator=g) * 0.98 + 0.01
    if mode == 2:
        return 1.0 - t, t.clone()
    return torch.sqrt(t).bfloat16().float(), torch.sqrt(1.0 - t).bfloat16().float()


def weights_of(discount, levels):
    return [float(F(float(discount) ** l)) for l in range(1, levels + 1)]
