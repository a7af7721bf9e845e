"""Times LoRA max-norm regularisation (az_lora_max_norm_bf16, csrc/az_lora.hip; lora_norm.LoraMaxNorm) at SDXL size, scope "unet",
rank = conv_rank 16 and 64, with and without fp32 master weights, HIP events / wall clock, INTERLEAVED in one process.

  pass:     the one launch over all 767 modules alone, by HIP events: with a limit nothing exceeds (the two Gram products and the
            decision: what every optimizer step pays) and with a limit everything exceeds (plus the scaling of every A, B and master;
            the adapters are restored from a copy outside the timed region before every repetition).
  update:   the AdamW update of the adapters' range alone (dist.ShardedRaven._update_region of the last region), by HIP events: the
            launch the pass follows.
  step:     dist.ShardedRaven.step() + zero_grad() on fixed random gradients, host-synchronised wall clock, WITHOUT the option (the
            parent's behaviour: no launch, no buffer) against WITH it (the limit at the median module norm), alternated.

    python tools/lora_maxnorm_time.py [--reps 9] [--rounds 5] [--per-round 4] [--ranks 16,64] [--out FILE]
                                                                                     -> one JSON line (also written to FILE)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

DEV = "cuda:0"


def _side(t, unit):
    return {f"median_{unit}": round(statistics.median(t), 3), f"spread_{unit}": round(max(t) - min(t), 3)}


def _events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3          # us


def one(rank, master, reps, rounds, per_round):
    from bench import init_weights_on_device
    from aozora_sdxl_training_amd.dist import ShardedRaven
    from aozora_sdxl_training_amd.lora_norm import LoraMaxNorm
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import SDXL_BASE, LoraSpec
    spec = LoraSpec(rank, float(rank), "", "unet", rank)
    unet = AozoraUNet(SDXL_BASE, DEV, lora=spec)
    init_weights_on_device(unet)              # the adapters too: A and B both U(-1/sqrt(fan_in), 1/sqrt(fan_in)), every module norm > 0
    for n, p in unet.named_parameters():
        p.requires_grad = ".lora_" in n
    (a, b), = unet.trainable_ranges()
    g = torch.Generator(device=DEV).manual_seed(1)
    grads = (torch.randn(b - a, generator=g, device=DEV) * 1e-3).bfloat16()
    opt = ShardedRaven(unet, lr=1e-4, clip_grad_norm=1.0, force_local=True, master_weights=master)
    mn = LoraMaxNorm(unet, 1.0, master=opt.master_address if master else None)
    keep_p = unet.pflat[a:b].clone()
    keep_w = opt.w_dev.clone() if master else None

    def restore():
        unet.pflat[a:b].copy_(keep_p)
        if master:
            opt.w_dev.copy_(keep_w)

    # the pass alone
    mn.max_norm = 3.0e38
    mn.apply(); torch.cuda.synchronize()
    norms = mn.landed()[:, 0].double()
    res = dict(modules=mn.n, adapter_elements=b - a, median_module_norm=float(norms.median()),
               streamed_mbytes=round(sum(2 * r[2] * (r[3] + r[4]) for r in mn.table.cpu().tolist()) / 1e6, 1))
    t = [_events(mn.apply) for _ in range(reps)]
    res["pass_nothing_scaled"] = _side(t, "us")
    mn.max_norm = float(norms.min()) * 0.5
    t = []
    for _ in range(reps):
        restore(); torch.cuda.synchronize()
        t.append(_events(mn.apply))
    assert int((mn.landed()[:, 1] != 1.0).sum()) == mn.n
    res["pass_everything_scaled"] = _side(t, "us")
    restore()
    # the update the pass follows
    last = len(opt.ranges) - 1
    opt._hyper()
    opt.scal[1:2].fill_(1.0)
    cur = torch.cuda.current_stream()
    unet.gflat[a:b].copy_(grads)
    opt._update_region(last, cur); torch.cuda.synchronize()
    t = [_events(lambda: opt._update_region(last, cur)) for _ in range(reps)]
    res["adapter_update"] = _side(t, "us")
    for k in ("pass_nothing_scaled", "pass_everything_scaled"):
        res[k + "_longer_than_the_update"] = bool(res[k]["median_us"] > res["adapter_update"]["median_us"])
    restore()
    # the optimizer step without and with the option
    mn.max_norm = float(norms.median())
    times = {"off": [], "on": []}

    def steps(n):
        for _ in range(n):
            unet.params._wait_wt_ready()      # the previous step cleared the gradients on its background stream (a backward waits here too)
            unet.gflat[a:b].copy_(grads)
            opt.step()
            opt.zero_grad(set_to_none=True)

    for side in ("off", "on"):
        opt.lora_norm = mn if side == "on" else None
        steps(2); torch.cuda.synchronize()
    for _ in range(rounds):
        for side in ("off", "on"):
            opt.lora_norm = mn if side == "on" else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(per_round)
            torch.cuda.synchronize()
            times[side].append((time.perf_counter() - t0) * 1e3 / per_round)
    res["optimizer_step_without_the_option"] = _side(times["off"], "ms")
    res["optimizer_step_with_the_option"] = _side(times["on"], "ms")
    res["keys_scaled_last_step"] = mn.summary()[0]
    d = res["optimizer_step_with_the_option"]["median_ms"] - res["optimizer_step_without_the_option"]["median_ms"]
    res["on_minus_off_ms"] = round(d, 3)
    res["beyond_spread"] = bool(abs(d) > max(res["optimizer_step_with_the_option"]["spread_ms"], res["optimizer_step_without_the_option"]["spread_ms"]))
    del opt, mn, unet
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=4)
    ap.add_argument("--ranks", default="16,64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_maxnorm_time needs a GPU")
    rep = dict(tool="tools/lora_maxnorm_time.py", device=torch.cuda.get_device_name(0), model="SDXL-base, scope unet, rank = conv_rank")
    for rank in (int(r) for r in a.ranks.split(",")):
        for master in (False, True):
            rep[f"rank{rank}_{'master' if master else 'bf16'}"] = one(rank, master, a.reps, a.rounds, a.per_round)
    line = json.dumps(rep, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rep, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
