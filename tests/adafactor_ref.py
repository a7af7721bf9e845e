"""Float64 restatement of the Adafactor contract (INTEGRATION.md "The Adafactor optimizer": the arithmetic of
transformers.optimization.Adafactor.step on logical tensor shapes), one function per step, on torch float64 tensors.  Imports no
package code: the tests compare the package, the pinned fixture and the HIP kernels against THIS."""
import math

import torch

U = 2.0 ** -24
DEFAULTS = dict(lr=None, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, weight_decay=0.0, scale_parameter=False,
                relative_step=False, warmup_init=False)


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def new_state(shape, opt):
    """Zero state of a tensor of logical `shape` under the package's names."""
    shape = tuple(shape)
    z = lambda s: torch.zeros(s, dtype=torch.float64)
    st = {"exp_avg_sq_row": z(shape[:-1]), "exp_avg_sq_col": z(shape[:-2] + shape[-1:])} if len(shape) >= 2 else {"exp_avg_sq": z(shape)}
    if opt["beta1"] is not None:
        st["exp_avg"] = z(shape)
    return st


def rms(t):
    return math.sqrt(float((t * t).sum()) / t.numel())


def step_lr(opt, step):
    if opt["relative_step"]:
        return min(1e-6 * step if opt["warmup_init"] else 1e-2, 1.0 / math.sqrt(step))
    return float(opt["lr"])


def step(p, g, st, step_no, opt):
    """One step of one tensor.  p, g: float64 tensors of the logical shape (p the bf16 parameter's value, g the bf16 gradient's);
    st: the state (updated in place); step_no counts from 1.  -> (x, u): the UNROUNDED new parameter and the update subtracted from
    the (decayed) parameter, both float64.  The caller rounds x to bf16 once."""
    p, g = p.double(), g.double()
    beta2t = 1.0 - math.pow(step_no, opt["decay_rate"])
    eps1, eps2 = opt["eps"]
    upd = g * g + eps1
    if p.dim() >= 2:
        row, col = st["exp_avg_sq_row"], st["exp_avg_sq_col"]
        row.mul_(beta2t).add_(upd.mean(dim=-1), alpha=1.0 - beta2t)
        col.mul_(beta2t).add_(upd.mean(dim=-2), alpha=1.0 - beta2t)
        rf = (row / row.mean(dim=-1, keepdim=True)).rsqrt().unsqueeze(-1)
        cf = col.unsqueeze(-2).rsqrt()
        u = rf * cf * g
    else:
        v = st["exp_avg_sq"]
        v.mul_(beta2t).add_(upd, alpha=1.0 - beta2t)
        u = v.rsqrt() * g
    u = u / max(1.0, rms(u) / opt["clip_threshold"])
    lr_t = (max(eps2, rms(p)) if opt["scale_parameter"] else 1.0) * step_lr(opt, step_no)
    u = lr_t * u
    if opt["beta1"] is not None:
        m = st["exp_avg"]
        a = st.setdefault("_abs_exp_avg", torch.zeros_like(m))       # the same average of |u|: the scale of exp_avg's error bound
        a.mul_(opt["beta1"]).add_(u.abs(), alpha=1.0 - opt["beta1"])
        m.mul_(opt["beta1"]).add_(u, alpha=1.0 - opt["beta1"])
        u = m.clone()
    x = p
    if opt["weight_decay"] != 0.0:
        x = x - opt["weight_decay"] * lr_t * x
    return x - u, u


def bf16_spacing(a):
    """Spacing of bf16 numbers at magnitude |a| (float64 tensor), the smallest normal's spacing below that."""
    a = a.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def state_terms(name, shape):
    """N of the state bound: the number of terms of the mean behind state `name` of a tensor of logical `shape`."""
    return {"exp_avg_sq_row": shape[-1], "exp_avg_sq_col": shape[-2] if len(shape) >= 2 else 1, "exp_avg_sq": 1}[name]


def _excess(err, bound):
    """max of err / bound over all elements; an exact element (err == 0) counts 0 whatever its bound, NaN counts inf."""
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    return float(q.max())


def state_excess(got, want, n_terms, step_no):
    """max over elements of |got - want| / ((N + 8) U step |want|): <= 1 passes."""
    return _excess((got.double() - want).abs(), (n_terms + 8) * U * step_no * want.abs())


def exp_avg_excess(got, st, shape, step_no):
    """max over elements of |got - exp_avg| / (2 (R + C + 32) U step avg|u|): the slack the parameter bound grants the update,
    averaged as exp_avg averages the updates."""
    R, C = (shape[-2], shape[-1]) if len(shape) >= 2 else (1, 1)
    bound = 2 * (R + C + 32) * U * step_no * st["_abs_exp_avg"]
    return _excess((got.double() - st["exp_avg"]).abs(), bound)


def param_excess(got, x, u, p_before, shape, step_no):
    """max over elements of |got - x| / (half the bf16 spacing at max(|x|, |got|) + 2 (R + C + 32) U step |u| + 4 U |p_before|)."""
    R, C = (shape[-2], shape[-1]) if len(shape) >= 2 else (1, 1)
    got = got.double()
    bound = 0.5 * bf16_spacing(torch.maximum(x.abs(), got.abs())) + 2 * (R + C + 32) * U * step_no * u.abs() + 4 * U * p_before.double().abs()
    return _excess((got - x).abs(), bound)


def check_run(shapes, opt, p0, grads, p_after, state_after):
    """p0: bf16 tensors; grads[step][tensor] bf16; p_after[step][tensor] bf16 and state_after[step][tensor] {name: fp32} of the
    implementation under test.  -> the largest excess of each kind over all tensors, steps and elements."""
    worst = {"state": 0.0, "param": 0.0, "exp_avg": 0.0}
    for ti, shape in enumerate(shapes):
        st, before = new_state(shape, opt), p0[ti]
        for k in range(len(grads)):
            x, u = step(before.double(), grads[k][ti].double(), st, k + 1, opt)
            got = state_after[k][ti]
            assert sorted(got) == sorted(state_names(shape, opt))
            for name, t in got.items():
                assert tuple(t.shape) == state_shape(name, shape), (shape, name, t.shape)
                if name == "exp_avg":
                    worst["exp_avg"] = max(worst["exp_avg"], exp_avg_excess(t, st, shape, k + 1))
                else:
                    worst["state"] = max(worst["state"], state_excess(t, st[name], state_terms(name, shape), k + 1))
            worst["param"] = max(worst["param"], param_excess(p_after[k][ti], x, u, before, shape, k + 1))
            before = p_after[k][ti]
    return worst



# ---- the pinned fixture (tests/golden/make_golden_adafactor.py writes it, tests/test_adafactor_ref_cpu.py reads it) --------------------
# The shapes of the GPU tests with the largest ones made smaller, so that the file stays under 200 KB.
FIXTURE_SHAPES = [(1,), (7,), (320,), (16, 1), (1, 16), (3, 5), (20, 20), (10, 33), (4, 136), (136, 4), (36, 20), (4, 5, 3, 3), (8, 4, 1, 1),
                  (6, 8, 3, 3)]
GRAD_SCALES = (1e-1, 1e-2, 1e-3)
OPTION_SETS = [options(lr=1e-2),
               options(lr=1e-2, weight_decay=0.01, beta1=0.9, scale_parameter=True, clip_threshold=0.5),
               options(lr=None, weight_decay=0.01, scale_parameter=True, relative_step=True, warmup_init=True, clip_threshold=2.0)]


def state_names(shape, opt):
    names = ["exp_avg_sq_row", "exp_avg_sq_col"] if len(shape) >= 2 else ["exp_avg_sq"]
    return names + (["exp_avg"] if opt["beta1"] is not None else [])


def state_shape(name, shape):
    shape = tuple(shape)
    return {"exp_avg_sq_row": shape[:-1], "exp_avg_sq_col": shape[:-2] + shape[-1:], "exp_avg_sq": shape, "exp_avg": shape}[name]


def pack(tensors):
    """Tensors -> one flat tensor (the fixture keeps few large tensors: a saved tensor costs more in bookkeeping than these hold)."""
    return torch.cat([t.reshape(-1) for t in tensors])


def unpack(flat, shapes):
    out, o = [], 0
    for s in shapes:
        n = math.prod(s)
        out.append(flat[o:o + n].reshape(s))
        o += n
    assert o == flat.numel()
    return out
