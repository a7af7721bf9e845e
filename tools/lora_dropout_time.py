"""Times LoRA dropout (az_lora_dropout_bf16, csrc/az_lora.hip), HIP events / wall clock, INTERLEAVED rounds in one process.

  kernel:   the in-place mask alone at [16384][48] (the fused q|k|v group of a self-attention at 1024^2, B = 4, rank 16: three parts)
            and [308][32] (the k|v group of a cross-attention: 4 x 77 context rows, two parts), every kind alone and all three
            together, as a native launch tape of `inner` back-to-back launches; `spread` is max - min over the repetitions.
  step:     one micro-step at 1024^2, B = 4, rank 16, alpha 16, scope "attention", the base frozen: dropout off against on (all three
            at 0.1), alternated in one process; launches on the recorded tape and milliseconds per side, with the repeat spread.

    python tools/lora_dropout_time.py [--reps 9] [--inner 200] [--rounds 4] [--per-round 4] [--no-kernel] [--no-step] [--out FILE]
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

from lora_time import taped, timed  # noqa: E402

DEV = "cuda:0"
SHAPES = [("self q|k|v [16384][48]", 16384, 4096, 16, 3), ("context k|v [308][32]", 308, 77, 16, 2)]
KINDS = {"element 0.1": (0.1, 0.0, 0.0), "rank 0.1": (0.0, 0.1, 0.0), "module 0.1": (0.0, 0.0, 0.1), "all three 0.1": (0.1, 0.1, 0.1)}


def kernel(reps, inner):
    from aozora_sdxl_training_amd import ops
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    g = torch.Generator(device=DEV).manual_seed(0)
    word = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    out = {}
    for label, rows, rps, r, parts in SHAPES:
        u = (torch.randn(rows, parts * r, generator=g, device=DEV) * 0.05).bfloat16()
        res = {}
        for kind, (pn, pr, pm) in KINDS.items():
            spec = LoraSpec(r, float(r), dropout=pn, rank_dropout=pr, module_dropout=pm)
            tape = taped(lambda: ops.lora_dropout(u, r, parts, rps, [401, 402, 403][:parts], spec.dropout_thresholds, spec.dropout_inv, 42, word), inner)[0]
            timed(tape, inner)
            t = [timed(tape, inner) for _ in range(reps)]
            res[kind] = dict(median_us=round(statistics.median(t), 2), spread_us=round(max(t) - min(t), 2))
        out[label] = res
    return out


def step_ab(rounds, per_round):
    from bench import init_weights_on_device, synthetic_batch
    from aozora_sdxl_training_amd._lib import Call
    from aozora_sdxl_training_amd.train_step import TrainStep
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import SDXL_BASE, LoraSpec
    batch = synthetic_batch(0, 0, 0, 4, DEV)
    sides = {}
    for name, spec in (("off", LoraSpec(16, 16.0)), ("on", LoraSpec(16, 16.0, dropout=0.1, rank_dropout=0.1, module_dropout=0.1))):
        unet = AozoraUNet(SDXL_BASE, DEV, lora=spec)
        init_weights_on_device(unet)
        unet.set_lora_dropout_seed(42)
        for n, p in unet.named_parameters():
            p.requires_grad = ".lora_" in n
        step = TrainStep(unet, mode="epsilon", grad_accum=1, world_size=1, use_graph=False)
        sides[name] = (unet, step, dict(lora_step=1) if spec.has_dropout else {})
        for _ in range(3):          # pool allocation, tape recording, first replay
            step.micro_step(*batch, **sides[name][2])
        step.synchronize()
        unet.zero_grad()
    times = {k: [] for k in sides}
    n = 1
    for _ in range(rounds):
        for name, (unet, step, kw) in sides.items():
            step.micro_step(*batch, **kw); step.synchronize()
            t0 = time.perf_counter()
            for _ in range(per_round):
                n += 1
                step.micro_step(*batch, **(dict(lora_step=n) if kw else {}))
            step.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / per_round)
            unet.zero_grad()
    res = {k: dict(median_ms=round(statistics.median(v), 3), spread_ms=round(max(v) - min(v), 3)) for k, v in times.items()}
    for name, (unet, step, _) in sides.items():
        tapes = [bk.tape for bk in step._buckets.values() if getattr(bk, "tape", None) is not None]
        res[name]["launches"] = sum(1 for op in tapes[0] if isinstance(op, Call) and op.name != "az_set_launch_stop_event") if tapes else None
        res[name]["dropout_launches"] = sum(1 for op in tapes[0] if isinstance(op, Call) and op.name == "az_lora_dropout_bf16") if tapes else None
    res["on_minus_off_ms"] = round(res["on"]["median_ms"] - res["off"]["median_ms"], 3)
    res["on_over_off"] = round(res["on"]["median_ms"] / res["off"]["median_ms"], 4)
    res["beyond_spread"] = bool(abs(res["on_minus_off_ms"]) > max(res["on"]["spread_ms"], res["off"]["spread_ms"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--per-round", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_dropout_time needs a GPU")
    rep = dict(tool="tools/lora_dropout_time.py", device=torch.cuda.get_device_name(0))
    if not a.no_kernel:
        rep["kernel"] = kernel(a.reps, a.inner)
    if not a.no_step:
        rep["micro_step_1024_B4_rank16_attention"] = step_ab(a.rounds, a.per_round)
    line = json.dumps(rep, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rep, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
