"""Times the loss launch of the micro-step at B = 4, C = 4, 128 x 128 latents (the 1024^2 bucket; prediction [B][HW][4] bf16, target
fp32 NCHW, dpred padded to 8 channels, as TrainStep issues it), HIP events: az_mse_loss_fwd_bwd and az_robust_loss_fwd_bwd (l1, huber,
smooth_l1), ALTERNATING in one process -- the yardstick is the MSE kernel.  Each entry is two launches (the sweep and the one-thread
finish); a timed window is --calls back-to-back calls between two events, so the figure is the issue-limited time per call on a warm
cache (10 bytes per element, 2.6 MB in all: nothing here reaches HBM twice), not an isolated kernel time.
    python tools/loss_time.py [--reps 7] [--warmup 2] [--calls 200]      -> one JSON line"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_time needs a GPU")
    from aozora_sdxl_training_amd import ops
    dev = "cuda:0"
    B, C, H, W = 4, 4, 128, 128
    g = torch.Generator().manual_seed(0)
    pred = torch.randn(B, H, W, C, generator=g).bfloat16().to(dev)
    target = torch.randn(B, C, H, W, generator=g).to(dev)
    w = torch.ones(B, device=dev)
    c = torch.full((B,), 0.1, device=dev)
    loss, per = torch.zeros(1, device=dev), torch.zeros(B, device=dev)
    dpred = torch.zeros(B, H, W, 8, dtype=torch.bfloat16, device=dev)
    fns = {"mse": lambda: ops.mse_loss_fwd_bwd(pred, target, w, 0.25, loss, per, dpred)}
    for kind in ("l1", "huber", "smooth_l1"):
        fns[kind] = (lambda k: lambda: ops.robust_loss_fwd_bwd(k, pred, target, w, None if k == "l1" else c, 0.25, loss, per, dpred))(kind)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls          # microseconds per call

    for _ in range(a.warmup):
        for fn in fns.values():
            once(fn)
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(a.reps):              # alternating: all four see the same box at the same time
        for k, fn in fns.items():
            t[k].append(once(fn))
    out = dict(tool="loss_time", shape=[B, C, H, W], calls_per_window=a.calls, gpu=torch.cuda.get_device_name(0),
               bytes_per_call=B * C * H * W * (2 + 4) + B * H * W * 8 * 2)
    for k, v in t.items():
        out[k + "_us"] = [round(x, 3) for x in v]
        out[k + "_us_min"] = round(min(v), 3)
        out[k + "_us_spread"] = round(max(v) - min(v), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
