"""Times the adapter kernels for 3x3 convolutions (csrc/az_lora.hip az_lora_conv_*) against az_conv2d_bf16 on the same product, and the
LoRA micro-step of scope "unet", by the procedure of tools/lora_time.py: both sides alternate in one process, each as a native launch
tape of `inner` back-to-back launches; `spread` is max - min over the repetitions of the SAME side.

  kernels:  the SDXL resnet shapes at B = 4, 1024^2 -- (H W, Cin) = (128^2, 320), (64^2, 640), (32^2, 1280) and the widest up-path
            input (32^2, 2560: up_blocks.0.resnets.0.conv1 reads the concatenation) -- at rank 16 and 64, s = 1 (the factor rides on
            the up product and on du in the executor, and the general kernel has none).
              down   u = A (*) x           [B H W][r]        vs  az_conv2d_bf16 forward, Cout = r
              dgrad  dx += A^T (*) du      [B H W][Cin]      vs  az_conv2d_bf16 data gradient over the transposed copy, accumulate
              wgrad  dA += du^T (*) x      [r][3][3][Cin]    vs  az_conv2d_bf16 weight gradient, accumulate, split_k auto
            lora_exec.LoraRoutes.CONV_*_GEMM name the (rows, rank) from which the general kernel is issued: where it wins here beyond the
            spread, the adapter kernel everywhere else.
  step:     one micro-step at 1024^2, B = 4, rank 16, conv_rank 16, the base frozen: scope "unet" against scope "transformer" and
            against the full fine-tune micro-step (everything trainable, LoRA off), alternated in one process, and the launches each
            records on its tape.

    python tools/lora_conv_time.py [--reps 9] [--inner 100] [--no-kernels] [--no-step] [--out profiles/lora_conv_time.json]
                                                                                     -> one JSON line (also written to FILE)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from lora_time import ab  # noqa: E402

DEV = "cuda:0"
BATCH = 4
SHAPES = [("128x128 Cin=320", 128, 320), ("64x64 Cin=640", 64, 640), ("32x32 Cin=1280", 32, 1280), ("32x32 Cin=2560 (widest up-path input)", 32, 2560)]
RANKS = (16, 64)


def kernels(reps, inner):
    from aozora_sdxl_training_amd import ops
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s: (torch.randn(*s, generator=g, device=DEV) * 0.05).bfloat16()
    out = {}
    for label, side, Cin in SHAPES:
        geom, M = (BATCH, side, side), BATCH * side * side
        as4 = lambda t: t.view(BATCH, side, side, t.shape[1])
        for r in RANKS:
            x, A, At, u, du = rnd(M, Cin), rnd(r, 3, 3, Cin), rnd(Cin, 3, 3, r), rnd(M, r), rnd(M, r)
            dx, dA = rnd(M, Cin), rnd(r, 3, 3, Cin)
            u2, dx2, dA2 = u.clone(), dx.clone(), dA.clone()
            res = {
                "down": ab(lambda: ops.lora_conv_down(x, geom, A, u), lambda: ops.conv_fwd(as4(x), A, as4(u2)), reps, inner),
                "dgrad": ab(lambda: ops.lora_conv_dgrad(du, geom, At, dx), lambda: ops.conv_dgrad_wt(as4(du), At, as4(dx2), accumulate=True), reps, inner),
                "wgrad": ab(lambda: ops.lora_conv_wgrad(du, x, geom, dA, accumulate=True),
                            lambda: ops.conv_wgrad(as4(du), as4(x), dA2, accumulate=True, split_k=0), reps, inner),
            }
            for k, v in res.items():        # the sides by their names here: the adapter kernel and the general convolution
                v["adapter"], v["general"] = v.pop("lora"), v.pop("gemm")
                if "lora_wins_beyond_spread" in v:
                    v["adapter_wins_beyond_spread"] = v.pop("lora_wins_beyond_spread")
                    v["general_wins_beyond_spread"] = bool(v["adapter"]["median_us"] - v["general"]["median_us"] >
                                                           max(v["adapter"]["spread_us"], v["general"]["spread_us"]))
                if "gemm_refused" in v:
                    v["general_refused"] = v.pop("gemm_refused")
            out[f"{label} r={r}"] = res
    return out


def step_ab(rounds, per_round):
    from bench import init_weights_on_device, synthetic_batch
    from aozora_sdxl_training_amd._lib import Call
    from aozora_sdxl_training_amd.train_step import TrainStep
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import SDXL_BASE, LoraSpec
    batch = synthetic_batch(0, 0, 0, BATCH, DEV)
    sides = {}
    for name, spec in (("full", None), ("lora_transformer", LoraSpec(16, 16.0, "", "transformer")), ("lora_unet", LoraSpec(16, 16.0, "", "unet", 16, 16.0))):
        unet = AozoraUNet(SDXL_BASE, DEV, lora=spec)
        init_weights_on_device(unet)
        if spec is not None:
            for n, p in unet.named_parameters():
                p.requires_grad = ".lora_" in n
        step = TrainStep(unet, mode="epsilon", grad_accum=1, world_size=1, use_graph=False)
        for _ in range(3):          # pool allocation, tape recording, first replay
            step.micro_step(*batch)
        step.synchronize()
        unet.zero_grad()
        sides[name] = (unet, step)
    times = {k: [] for k in sides}
    for _ in range(rounds):
        for name, (unet, step) in sides.items():
            step.micro_step(*batch); step.synchronize()
            t0 = time.perf_counter()
            for _ in range(per_round):
                step.micro_step(*batch)
            step.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / per_round)
            unet.zero_grad()
    launches = {}
    for name, (unet, step) in sides.items():
        tapes = [bk.tape for bk in step._buckets.values() if getattr(bk, "tape", None) is not None]
        launches[name] = sum(1 for op in tapes[0] if isinstance(op, Call) and op.name != "az_set_launch_stop_event") if tapes else None
    res = {k: dict(median_ms=round(statistics.median(v), 3), spread_ms=round(max(v) - min(v), 3)) for k, v in times.items()}
    res["launches_per_micro_step"] = launches
    res["lora_unet_over_full"] = round(res["lora_unet"]["median_ms"] / res["full"]["median_ms"], 4)
    res["lora_unet_over_lora_transformer"] = round(res["lora_unet"]["median_ms"] / res["lora_transformer"]["median_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--per-round", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_conv_time needs a GPU")
    rep = dict(tool="tools/lora_conv_time.py", device=torch.cuda.get_device_name(0))
    if not a.no_kernels:
        rep["kernels"] = kernels(a.reps, a.inner)
    if not a.no_step:
        rep["micro_step_1024_B4_rank16_conv_rank16"] = step_ab(a.rounds, a.per_round)
    line = json.dumps(rep, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rep, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
