"""Times one optimizers.Adafactor.step() over all trainable elements of the SDXL-base UNet (everything trainable: 2.57 G elements, 1680
tensors, one descriptor table, five launches) against the flat Raven step of the same tree (dist.ShardedRaven at one rank: global norm,
clip, the fused AdamW update of every region), ALTERNATED in one process on one device.  Each step starts on a drained device with
the gradients put back (the Raven step clears them) and ends when the device is drained again: wall clock between two
synchronisations, so that the streams a step uses do not matter.  The number is recorded, not gated.

    python tools/adafactor_time.py [--reps 5] [--warmup 2] [--out profiles/adafactor_time.json]      -> one JSON line (also written to FILE)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adafactor_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adafactor_time needs a GPU")
    from aozora_sdxl_training_amd.dist import ShardedRaven
    from aozora_sdxl_training_amd.optimizers import Adafactor
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import UNetConfig
    dev = "cuda:0"
    unet = AozoraUNet(UNetConfig(), dev)
    n = unet.flat_numel
    g = torch.Generator(device=dev).manual_seed(0)
    grads = torch.empty(n, dtype=torch.bfloat16, device=dev)
    for a0 in range(0, n, 1 << 28):
        b0 = min(n, a0 + (1 << 28))
        unet.pflat[a0:b0].copy_((torch.randn(b0 - a0, generator=g, device=dev) * 0.02).bfloat16())
        grads[a0:b0].copy_((torch.randn(b0 - a0, generator=g, device=dev) * 1e-3).bfloat16())
    params = [p for p in unet.parameters() if p.requires_grad]
    elements = sum(p.numel() for p in params)
    raven = ShardedRaven(unet, lr=8e-7, clip_grad_norm=1.0, force_local=True)
    ada = Adafactor(params, lr=8e-7, scale_parameter=False, relative_step=False, warmup_init=False, stochastic_rounding=True, sr_seed=1)

    def once(which):
        unet.gflat.copy_(grads)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if which == "raven":
            raven.step()
            raven.synchronize_params()
        else:
            ada.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        once("raven"); once("adafactor")
    t = {"raven": [], "adafactor": []}
    for _ in range(a.reps):              # alternating: both see the same box at the same time
        for k in t:
            t[k].append(once(k))
    side = lambda v: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), spread_ms=round(max(v) - min(v), 3))
    classes = {c: sum(e["cls"] == i for e in ada.entries) for i, c in enumerate(("vector", "matrix", "batch"))}
    res = dict(tool="adafactor_time", device=torch.cuda.get_device_name(0), trainable_elements=elements, tensors=len(ada.entries), classes=classes,
               reps=a.reps, warmup=a.warmup, launches_per_adafactor_step=5, workgroups_per_pass=ada._nwg,
               adafactor=dict(side(t["adafactor"]), state_bytes=ada.state_bytes, scratch_bytes=4 * (ada._scratch_numel + ada._fac_numel),
                              options="scale_parameter=False relative_step=False warmup_init=False stochastic_rounding=True"),
               raven=dict(side(t["raven"]), state_bytes=4 * elements, what="dist.ShardedRaven, one rank: norm, clip, fused AdamW, bf16 m and v"),
               ratio_adafactor_over_raven=round(statistics.median(t["adafactor"]) / statistics.median(t["raven"]), 3),
               how="wall clock between two device synchronisations, gradients restored before every step, the two optimizers alternated")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
