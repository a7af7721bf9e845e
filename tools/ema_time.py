"""Times the fp32 EMA of the weights ("ema_decay", aozora_sdxl_training_amd/ema.py) at SDXL-base size on one device, HIP events:
  (i)  kernel:   az_ema_flat (10 bytes per element: 2 read of p, 4 read + 4 written of the EMA) and az_adamw_flat (14 bytes per element,
                 bf16 m / v) over the full trainable flat range, ALTERNATING in one process -- the yardstick is the other kernel;
  (ii) boundary: the optimizer_boundary_on_main_stream span of dist.ShardedRaven.timing_summary() at one rank (default overlapped
                 update: regions 1 and 2, and their EMA launches, run on the parameter-gradient stream), two optimizers on the same
                 UNet, one with an EMA attached and one without, stepping ALTERNATELY with the device drained in between.
    python tools/ema_time.py [--reps 5] [--warmup 2]      -> one JSON line"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_time needs a GPU")
    from aozora_sdxl_training_amd._lib import lib
    from aozora_sdxl_training_amd.dist import ShardedRaven
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import UNetConfig
    dev = "cuda:0"
    unet = AozoraUNet(UNetConfig(), dev)
    n = unet.flat_numel
    g = torch.Generator(device=dev).manual_seed(0)
    for a0 in range(0, n, 1 << 28):
        b0 = min(n, a0 + (1 << 28))
        unet.pflat[a0:b0].copy_((torch.randn(b0 - a0, generator=g, device=dev) * 0.02).bfloat16())
        unet.gflat[a0:b0].copy_((torch.randn(b0 - a0, generator=g, device=dev) * 1e-3).bfloat16())
    ranges = unet.trainable_ranges()
    elements = sum(b1 - a1 for a1, b1 in ranges)
    L = lib()
    vp = ctypes.c_void_p

    # ---- (i) the two kernels ---------------------------------------------------------------------------------------------------
    m = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    v = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    e = torch.zeros(n, dtype=torch.float32, device=dev)
    hyper = torch.tensor([1e-5, 0.9, 0.999, 1e-8, 1.0 - 1e-7, 1e-4, 0.03, 0.0], dtype=torch.float32, device=dev)

    def adamw():
        st = vp(torch.cuda.current_stream().cuda_stream)
        for a1, b1 in ranges:
            L.call("az_adamw_flat", b1 - a1, vp(unet.pflat.data_ptr() + a1 * 2), vp(unet.gflat.data_ptr() + a1 * 2),
                   vp(m.data_ptr() + a1 * 2), vp(v.data_ptr() + a1 * 2), 0, vp(hyper.data_ptr()), vp(0), st)

    def ema():
        st = vp(torch.cuda.current_stream().cuda_stream)
        for a1, b1 in ranges:
            L.call("az_ema_flat", b1 - a1, vp(unet.pflat.data_ptr() + a1 * 2), vp(e.data_ptr() + a1 * 4), 1e-3, st)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        adamw(); ema()
    torch.cuda.synchronize()
    t_adamw, t_ema = [], []
    for _ in range(a.reps):              # alternating: both see the same box at the same time
        t_adamw.append(once(adamw))
        t_ema.append(once(ema))
    tbs = lambda nbytes, ms: nbytes * elements / (ms * 1e-3) / 1e12
    del m, v, e

    # ---- (ii) the optimizer boundary on the main stream, one rank ---------------------------------------------------------------------
    kw = dict(lr=8e-7, clip_grad_norm=1.0, force_local=True)
    opts = {"off": ShardedRaven(unet, **kw), "on": ShardedRaven(unet, ema=dict(decay=0.999), **kw)}
    assert all(o.update_overlap for o in opts.values())
    region_elements = [sum(b1 - a1 for a1, b1 in rs) for rs in opts["on"].ranges]

    def boundary(o):
        o.enable_timing(True)
        o.step()
        o.synchronize_params()
        ms = o.timing_summary()["optimizer_boundary_on_main_stream"]["ms"]      # (synchronises the device: the next step starts on an idle one)
        o.enable_timing(False)
        return ms

    for _ in range(a.warmup):
        boundary(opts["off"]); boundary(opts["on"])
    t_off, t_on = [], []
    for _ in range(a.reps):
        t_off.append(boundary(opts["off"]))
        t_on.append(boundary(opts["on"]))
    print(json.dumps(dict(
        tool="ema_time", elements=elements, launches=len(ranges), gpu=torch.cuda.get_device_name(0),
        adamw_ms=t_adamw, ema_ms=t_ema, adamw_ms_min=min(t_adamw), ema_ms_min=min(t_ema), adamw_spread_ms=max(t_adamw) - min(t_adamw),
        ema_spread_ms=max(t_ema) - min(t_ema), adamw_TBps_best=tbs(14.0, min(t_adamw)), ema_TBps_best=tbs(10.0, min(t_ema)),
        region_elements=region_elements, region0_share=region_elements[0] / max(1, sum(region_elements)), ema_bytes=opts["on"].ema.nbytes,
        boundary_off_ms=t_off, boundary_on_ms=t_on, boundary_off_ms_min=min(t_off), boundary_on_ms_min=min(t_on),
        boundary_off_spread_ms=max(t_off) - min(t_off), boundary_on_spread_ms=max(t_on) - min(t_on))))


if __name__ == "__main__":
    main()
