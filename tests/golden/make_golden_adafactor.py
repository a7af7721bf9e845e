"""The Adafactor pin: inputs and outputs of transformers.optimization.Adafactor (transformers 5.15.0, the implementation kohya-ss
sd-scripts calls), recorded once:

    python tests/golden/make_golden_adafactor.py

Writes tests/golden/adafactor_golden.pt: for the shapes, gradient scales and three option sets of tests/adafactor_ref.py, the bf16
parameters, three bf16 gradients, and the package's parameters and state after each of the three steps.  Everything is packed into a
few flat tensors in the order of FIXTURE_SHAPES (state: per tensor in the order of adafactor_ref.state_names); bf16 values travel as
int16 bit patterns."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import adafactor_ref as R  # noqa: E402


def main():
    import transformers
    from transformers.optimization import Adafactor
    gen = torch.Generator().manual_seed(20241)
    p0 = [(torch.randn(s, generator=gen) * 0.05).bfloat16() for s in R.FIXTURE_SHAPES]
    grads = [[(torch.randn(s, generator=gen) * sc).bfloat16() for s in R.FIXTURE_SHAPES] for sc in R.GRAD_SCALES]
    bits = lambda ts: R.pack(ts).view(torch.int16).clone()
    out = {"transformers": transformers.__version__, "torch": str(torch.__version__), "shapes": [list(s) for s in R.FIXTURE_SHAPES],
           "grad_scales": list(R.GRAD_SCALES), "p0": bits(p0), "grads": [bits(g) for g in grads], "sets": []}
    for opt in R.OPTION_SETS:
        params = [torch.nn.Parameter(p.clone()) for p in p0]
        o = Adafactor(params, **opt)
        rec = {"options": {k: (list(v) if isinstance(v, tuple) else v) for k, v in opt.items()}, "p": [], "state": []}
        for g in grads:
            for p, gi in zip(params, g):
                p.grad = gi.clone()
            o.step()
            rec["p"].append(bits([p.detach() for p in params]))
            rec["state"].append(R.pack([o.state[p][k].float() for p, s in zip(params, R.FIXTURE_SHAPES) for k in R.state_names(s, opt)]).clone())
        out["sets"].append(rec)
    path = os.path.join(HERE, "adafactor_golden.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
