"""Times one Prodigy step (csrc/az_prodigy.hip) pass by pass over SDXL-base's trainable element count (one contiguous range, random
bf16 gradients, all state resident in HBM) against az_adamw_flat_master over the same n, HIP events, INTERLEAVED rounds in one process:
  moments:  az_prodigy_begin + az_prodigy_moments   reads w, p0, m, v, s (fp32) and g (bf16), writes m, v, s: 34 bytes per element
  finish:   az_prodigy_finish                        one workgroup over the partial sums
  apply:    az_prodigy_apply                         reads w, m, v, writes w (fp32) and p (bf16): 18 bytes per element
  master:   az_adamw_flat_master                     reads w (fp32), g, m, v (bf16), writes w, m, v, p: 20 bytes per element (the yardstick)
The byte counts are read off the kernels' loads and stores.  Neither side includes the gradient-norm pass; both read the gradients
unclipped (coef = null).
    python tools/prodigy_time.py [--reps 7] [--warmup 2] [--out FILE]      -> one JSON line (also written to FILE)"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

HBM_PEAK_TBPS = 8.0          # MI355X, specification


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prodigy_time needs a GPU")
    from aozora_sdxl_training_amd._lib import lib
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import UNetConfig
    dev = "cuda:0"
    unet = AozoraUNet(UNetConfig(), dev)
    n = sum(b1 - a1 for a1, b1 in unet.trainable_ranges())       # everything trainable: one contiguous range, the whole flat buffer
    del unet
    torch.cuda.empty_cache()
    g = torch.Generator(device=dev).manual_seed(0)
    f32 = lambda: torch.zeros(n, dtype=torch.float32, device=dev)
    p = torch.empty(n, dtype=torch.bfloat16, device=dev)
    grad = torch.empty(n, dtype=torch.bfloat16, device=dev)
    w, p0, m, v, s, wa = f32(), f32(), f32(), f32(), f32(), f32()
    for a0 in range(0, n, 1 << 28):
        b0 = min(n, a0 + (1 << 28))
        p[a0:b0].copy_((torch.randn(b0 - a0, generator=g, device=dev) * 0.02).bfloat16())
        grad[a0:b0].copy_((torch.randn(b0 - a0, generator=g, device=dev) * 1e-3).bfloat16())
        w[a0:b0].copy_(p[a0:b0]); p0[a0:b0].copy_(p[a0:b0]); wa[a0:b0].copy_(p[a0:b0])
    ma = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    va = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    hyper_a = torch.tensor([1e-5, 0.9, 0.999, 1e-8, 1.0 - 1e-7, 1e-4, 0.03, 0.0], dtype=torch.float32, device=dev)
    L = lib()
    vp = ctypes.c_void_p
    npairs = int(L._fn["az_prodigy_partials"](n))
    dstate = torch.tensor([1e-6, 1e-6, 0.0, 0.0, 0.0, 0.0, 1e-6, 0.0], dtype=torch.float64, device=dev)
    consts = torch.zeros(16, dtype=torch.float64, device=dev)
    partials = torch.zeros(2 * npairs, dtype=torch.float64, device=dev)
    hyper = (ctypes.c_double * 16)(1.0, 0.9, 0.999, 0.999 ** 0.5, 1e-8, 0.01, 1.0, 1.1, 0.0, 0.0)      # growth 1.1: d stays finite over the rounds
    st = lambda: vp(torch.cuda.current_stream().cuda_stream)
    P = lambda t: vp(t.data_ptr())

    def moments():
        L.call("az_prodigy_begin", P(dstate), ctypes.cast(hyper, vp), P(consts), st())
        L.call("az_prodigy_moments", n, P(w), P(p0), P(grad), 0, P(m), P(v), P(s), P(consts), vp(0), P(partials), st())

    def finish():
        L.call("az_prodigy_finish", npairs, P(partials), P(dstate), P(consts), st())

    def apply():
        L.call("az_prodigy_apply", n, P(p), P(w), P(m), P(v), P(consts), st())

    def master():
        L.call("az_adamw_flat_master", n, P(p), P(wa), P(grad), 0, P(ma), P(va), 0, P(hyper_a), vp(0), st())

    passes = [("moments", moments, 34.0), ("finish", finish, 0.0), ("apply", apply, 18.0), ("master", master, 20.0)]

    def round_():
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(passes) + 1)]
        evs[0].record()
        for i, (_, fn, _) in enumerate(passes):
            fn()
            evs[i + 1].record()
        evs[-1].synchronize()
        return [evs[i].elapsed_time(evs[i + 1]) for i in range(len(passes))]

    for _ in range(a.warmup):
        round_()
    times = [round_() for _ in range(a.reps)]
    skip = float(consts.cpu().numpy().view("float32")[10])
    out = dict(tool="prodigy_time", elements=n, reps=a.reps, warmup=a.warmup, partial_pairs=npairs, hbm_peak_TBps=HBM_PEAK_TBPS,
               d_after=float(dstate[0].item()), apply_skipped=bool(skip), gpu=torch.cuda.get_device_name(0), passes={})
    for i, (name, _, nbytes) in enumerate(passes):
        t = [r[i] for r in times]
        rec = dict(ms=t, ms_median=statistics.median(t), ms_min=min(t), spread_ms=max(t) - min(t), bytes_per_element=nbytes)
        if nbytes:
            rec["GBps_median"] = nbytes * n / (rec["ms_median"] * 1e-3) / 1e9
            rec["GBps_best"] = nbytes * n / (rec["ms_min"] * 1e-3) / 1e9
            rec["share_of_hbm_peak_best"] = rec["GBps_best"] / (HBM_PEAK_TBPS * 1e3)
        out["passes"][name] = rec
    step = [r[0] + r[1] + r[2] for r in times]
    out["prodigy_step_ms_median"], out["prodigy_step_ms_min"] = statistics.median(step), min(step)
    out["step_over_master_median"] = out["prodigy_step_ms_median"] / out["passes"]["master"]["ms_median"]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
