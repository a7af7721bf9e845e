"""Times one full-size SDXL-base optimizer update (2.567 G elements, random bf16 gradients) on one device, HIP events:
  8-bit:  optimizers.PagedAdamW8bit.step()   (az_adamw8bit_step: one launch, uint8 codes + per-block absmax resident in HBM)
  raven:  the flat update of dist.ShardedRaven at one rank (az_adamw_flat over the trainable ranges, bf16 m / v resident in HBM)
Neither includes the gradient-norm pass; both read the gradients unclipped (coef = null).
    python tools/adamw8bit_time.py [--reps 5] [--warmup 2]      -> one JSON line"""
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
        raise SystemExit("adamw8bit_time needs a GPU")
    from aozora_sdxl_training_amd._lib import lib
    from aozora_sdxl_training_amd.optimizers import PagedAdamW8bit
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
    unet.expose_grads()
    params = list(unet.parameters())
    numel = sum(p.numel() for p in params)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    opt = PagedAdamW8bit(params, lr=1e-5, weight_decay=0.01)
    t8 = timed(opt.step)
    state8 = sum(t.numel() * t.element_size() for st in opt.state.values() for k, t in st.items()
                 if torch.is_tensor(t) and not k.startswith("qmap"))
    del opt
    torch.cuda.empty_cache()

    m = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    v = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    hyper = torch.tensor([1e-5, 0.9, 0.999, 1e-8, 1.0 - 1e-7, 1e-4, 0.03, 0.0], dtype=torch.float32, device=dev)
    ranges = unet.trainable_ranges()
    L = lib()

    def raven():
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for a1, b1 in ranges:
            L.call("az_adamw_flat", b1 - a1, ctypes.c_void_p(unet.pflat.data_ptr() + a1 * 2), ctypes.c_void_p(unet.gflat.data_ptr() + a1 * 2),
                   ctypes.c_void_p(m.data_ptr() + a1 * 2), ctypes.c_void_p(v.data_ptr() + a1 * 2), 0,
                   ctypes.c_void_p(hyper.data_ptr()), ctypes.c_void_p(0), st)
    tr = timed(raven)
    print(json.dumps(dict(tool="adamw8bit_time", elements=numel, adamw8bit_ms=t8, raven_flat_ms=tr,
                          adamw8bit_ms_min=min(t8), raven_flat_ms_min=min(tr), adamw8bit_state_bytes=state8,
                          raven_state_bytes=2 * n * 2, gpu=torch.cuda.get_device_name(0))))


if __name__ == "__main__":
    main()
