"""Times the flat update of dist.ShardedRaven at one rank over the full SDXL-base flat range (2.567 G elements, random bf16 gradients,
bf16 m / v resident in HBM) on one device, HIP events, the two updates ALTERNATING in one process:
  rn:      az_adamw_flat          (bf16 parameters read and written: 14 bytes per element)
  master:  az_adamw_flat_master   (fp32 master read and written, bf16 parameters written only: 20 bytes per element)
Neither includes the gradient-norm pass; both read the gradients unclipped (coef = null).
    python tools/master_time.py [--reps 5] [--warmup 2] [--out FILE]      -> one JSON line (also written to FILE)"""
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("master_time needs a GPU")
    from aozora_sdxl_training_amd._lib import lib
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import UNetConfig
    dev = "cuda:0"
    unet = AozoraUNet(UNetConfig(), dev)
    n = unet.flat_numel
    g = torch.Generator(device=dev).manual_seed(0)
    w = torch.empty(n, dtype=torch.float32, device=dev)
    for a0 in range(0, n, 1 << 28):
        b0 = min(n, a0 + (1 << 28))
        unet.pflat[a0:b0].copy_((torch.randn(b0 - a0, generator=g, device=dev) * 0.02).bfloat16())
        unet.gflat[a0:b0].copy_((torch.randn(b0 - a0, generator=g, device=dev) * 1e-3).bfloat16())
        w[a0:b0].copy_(unet.pflat[a0:b0])
    m = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    v = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    hyper = torch.tensor([1e-5, 0.9, 0.999, 1e-8, 1.0 - 1e-7, 1e-4, 0.03, 0.0], dtype=torch.float32, device=dev)
    ranges = unet.trainable_ranges()
    elements = sum(b1 - a1 for a1, b1 in ranges)
    L = lib()
    vp = ctypes.c_void_p

    def rn():
        st = vp(torch.cuda.current_stream().cuda_stream)
        for a1, b1 in ranges:
            L.call("az_adamw_flat", b1 - a1, vp(unet.pflat.data_ptr() + a1 * 2), vp(unet.gflat.data_ptr() + a1 * 2),
                   vp(m.data_ptr() + a1 * 2), vp(v.data_ptr() + a1 * 2), 0, vp(hyper.data_ptr()), vp(0), st)

    def master():
        st = vp(torch.cuda.current_stream().cuda_stream)
        for a1, b1 in ranges:
            L.call("az_adamw_flat_master", b1 - a1, vp(unet.pflat.data_ptr() + a1 * 2), vp(w.data_ptr() + a1 * 4), vp(unet.gflat.data_ptr() + a1 * 2), 0,
                   vp(m.data_ptr() + a1 * 2), vp(v.data_ptr() + a1 * 2), 0, vp(hyper.data_ptr()), vp(0), st)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        rn(); master()
    torch.cuda.synchronize()
    t_rn, t_ma = [], []
    for _ in range(a.reps):              # alternating: both see the same box at the same time
        t_rn.append(once(rn))
        t_ma.append(once(master))
    tbs = lambda ms, nbytes: nbytes * elements / (ms * 1e-3) / 1e12
    line = json.dumps(dict(tool="master_time", elements=elements, launches=len(ranges), rn_ms=t_rn, master_ms=t_ma, rn_ms_min=min(t_rn),
                           master_ms_min=min(t_ma), rn_spread_ms=max(t_rn) - min(t_rn), master_spread_ms=max(t_ma) - min(t_ma),
                           rn_bytes_per_element=14, master_bytes_per_element=20, rn_TBps_best=tbs(min(t_rn), 14.0),
                           master_TBps_best=tbs(min(t_ma), 20.0), ratio_best=min(t_ma) / min(t_rn), gpu=torch.cuda.get_device_name(0)))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
