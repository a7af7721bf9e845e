"""CPU restatement of the Prodigy optimizer of this project (csrc/az_prodigy.hip, optimizers/prodigy.py; INTEGRATION.md "The Prodigy
optimizer"): per element float32 with one rounding per operation in the stated order (numpy float32 operators, elem_ref.fma32 for the
two fused multiply-adds), both sums by math.fsum over terms that are exact in float64, scalars in Python floats.  begin() / finish()
can take the derived float32 constants from outside (the device's), so that a kernel test compares the element-wise results bit for
bit whatever the last bit of a device pow() is."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import elem_ref as R        # noqa: E402

F = np.float32
SCALARS = ("d", "d_max", "d_numerator", "d_denom", "d_hat", "k", "d0")
BEGIN_F32 = ("c_m", "c_v", "c_s", "beta1", "beta2", "beta3")
FINISH_F32 = ("dlr", "wd_dlr", "eps_d")


def f32(x):
    """A Python float rounded once to float32 (returned as numpy float32)."""
    with np.errstate(all="ignore"):
        return F(x)


def options(lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0, use_bias_correction=False, safeguard_warmup=False,
            d0=1e-6, d_coef=1.0, growth_rate=float("inf")):
    b1, b2 = float(betas[0]), float(betas[1])
    return dict(lr=float(lr), beta1=b1, beta2=b2, beta3=math.sqrt(b2) if beta3 is None else float(beta3), eps=float(eps),
                weight_decay=float(weight_decay), use_bias_correction=bool(use_bias_correction), safeguard_warmup=bool(safeguard_warmup),
                d0=float(d0), d_coef=float(d_coef), growth_rate=float(growth_rate))


class ProdigyRef:
    """tensors: a list of bf16 (or float) torch CPU tensors, one per range.  State: w, p0, m, v, s float32 numpy arrays per range, the
    seven scalars as Python floats, p the bf16 image of w."""

    def __init__(self, tensors, **opts):
        self.o = options(**opts)
        self.w = [t.detach().float().numpy().reshape(-1).astype(np.float32).copy() for t in tensors]
        self.p0 = [w.copy() for w in self.w]
        self.m = [np.zeros_like(w) for w in self.w]
        self.v = [np.zeros_like(w) for w in self.w]
        self.s = [np.zeros_like(w) for w in self.w]
        self.p = [R.bits_to_bf16(R.bf16_bits_np(w)) for w in self.w]
        d0 = self.o["d0"]
        self.sc = dict(d=d0, d_max=d0, d_numerator=0.0, d_denom=0.0, d_hat=0.0, k=0.0, d0=d0)
        self.sums = (0.0, 0.0)          # fsum of the last step's numerator / denominator terms
        self.abs_sums = (0.0, 0.0)      # ... and of their magnitudes (the error bound of a device sum scales with these)
        self.nterms = 0

    # ---- the scalar state machine, in the kernels' split -------------------------------------------------------------------------
    def begin(self, lr=None):
        """-> (fp64 values carried to finish, the six float32 constants of the moments pass as the contract derives them)."""
        o, sc = self.o, self.sc
        lr = o["lr"] if lr is None else float(lr)
        d, k, d0 = sc["d"], sc["k"], sc["d0"]
        bc = math.sqrt(1.0 - o["beta2"] ** (k + 1.0)) / (1.0 - o["beta1"] ** (k + 1.0)) if o["use_bias_correction"] else 1.0
        dlr = d * lr * bc
        r = d / d0
        exact = dict(c_m=d * (1.0 - o["beta1"]), c_v=d * d * (1.0 - o["beta2"]), c_s=r * (d if o["safeguard_warmup"] else dlr),
                     beta1=o["beta1"], beta2=o["beta2"], beta3=o["beta3"])
        return dict(dlr=dlr, factor=r * dlr), exact

    def moments(self, grads, cf, coef=None):
        """The moments pass over every range with the float32 constants cf (name -> value); -> (fsum numerator, fsum denominator)."""
        c = {k: F(cf[k]) for k in BEGIN_F32}
        num_terms, den_terms = [], []
        with np.errstate(all="ignore"):
            for r, g in enumerate(grads):
                gr = g.detach().float().numpy().reshape(-1) * (F(coef) if coef is not None else F(1.0))
                if g.dtype == torch.bfloat16:
                    gr = R.bf16_round_np(gr)
                gr = gr.astype(np.float32)
                self.m[r] = R.fma32(gr, np.full_like(gr, c["c_m"]), self.m[r] * c["beta1"])
                self.v[r] = self.v[r] * c["beta2"] + ((c["c_v"] * gr) * gr)
                self.s[r] = R.fma32(gr, np.full_like(gr, c["c_s"]), self.s[r] * c["beta3"])
                diff = self.p0[r] - self.w[r]
                num_terms.append(gr.astype(np.float64) * diff.astype(np.float64))
                den_terms.append(np.abs(self.s[r]).astype(np.float64))
        num = np.concatenate(num_terms) if num_terms else np.zeros(0)
        den = np.concatenate(den_terms) if den_terms else np.zeros(0)
        self.sums = (math.fsum(num.tolist()), math.fsum(den.tolist()))
        self.abs_sums = (math.fsum(np.abs(num).tolist()), self.sums[1])
        self.nterms = int(num.size)
        return self.sums

    def finish(self, carried, sums=None):
        """The step-size update from the two sums (default: this restatement's own); -> None when d_denom == 0 (the step ends), else the
        three float32 constants of the apply pass as the contract derives them (Python floats, unrounded)."""
        o, sc = self.o, self.sc
        snum, sden = self.sums if sums is None else sums
        sc["d_numerator"] = o["beta3"] * sc["d_numerator"] + carried["factor"] * snum
        sc["d_denom"] = sden
        if sden == 0.0:
            return None
        d = sc["d"]
        d_hat = o["d_coef"] * sc["d_numerator"] / sden
        if d == sc["d0"]:
            d = d_hat if d_hat > d else d
        sc["d_max"] = d_hat if d_hat > sc["d_max"] else sc["d_max"]
        grown = d * o["growth_rate"]
        d = grown if grown < sc["d_max"] else sc["d_max"]
        sc["d"], sc["d_hat"], sc["k"] = d, d_hat, sc["k"] + 1.0
        return dict(dlr=carried["dlr"], wd_dlr=o["weight_decay"] * carried["dlr"], eps_d=d * o["eps"])

    def apply(self, cf):
        c = {k: F(cf[k]) for k in FINISH_F32}
        with np.errstate(all="ignore"):
            for r in range(len(self.w)):
                w = self.w[r]
                if self.o["weight_decay"] != 0.0:
                    w = R.fma32(w, np.full_like(w, -c["wd_dlr"]), w)
                denom = np.sqrt(self.v[r]) + c["eps_d"]
                w = w + ((-c["dlr"] * self.m[r]) / denom)
                self.w[r] = np.ascontiguousarray(w, dtype=np.float32)
                self.p[r] = R.bits_to_bf16(R.bf16_bits_np(self.w[r]))

    # ---- one whole step ---------------------------------------------------------------------------------------------------------
    def step(self, grads, coef=None, lr=None, begin_f32=None, finish_f32=None, sums=None):
        """grads: one bf16 / float32 torch CPU tensor per range.  begin_f32 / finish_f32: the float32 constants from outside (dicts by
        name), sums: the two sums from outside; default: this restatement's own.  -> False when nothing was applied."""
        lr = self.o["lr"] if lr is None else float(lr)
        if lr == 0.0:
            return False
        carried, exact = self.begin(lr)
        self.exact_begin = exact
        self.moments(grads, begin_f32 if begin_f32 is not None else {k: f32(v) for k, v in exact.items()}, coef)
        fin = self.finish(carried, sums)
        self.exact_finish = fin
        if fin is None:
            return False
        self.apply(finish_f32 if finish_f32 is not None else {k: f32(v) for k, v in fin.items()})
        return True

    # ---- state ------------------------------------------------------------------------------------------------------------------
    def save(self):
        cat = lambda xs: torch.from_numpy(np.concatenate(xs).copy())
        return dict(options=dict(self.o), scalars=dict(self.sc), ranges=[int(w.size) for w in self.w],
                    **{k: cat(getattr(self, k)) for k in ("w", "p0", "m", "v", "s")})

    def load(self, st):
        if st["ranges"] != [int(w.size) for w in self.w]:
            raise ValueError("the saved ranges differ from this optimizer's")
        self.sc = {k: float(st["scalars"][k]) for k in SCALARS}
        off = 0
        for r, n in enumerate(st["ranges"]):
            for k in ("w", "p0", "m", "v", "s"):
                getattr(self, k)[r] = st[k][off:off + n].numpy().astype(np.float32).copy()
            self.p[r] = R.bits_to_bf16(R.bf16_bits_np(self.w[r]))
            off += n
