"""Times the LoRA adapter kernels (csrc/az_lora.hip) and the LoRA micro-step, HIP events / wall clock, INTERLEAVED rounds in one process.

  kernels:  each az_lora_* entry at the model's shapes -- M = 16384, C = 640; M = 4096, C = 1280; the context projection M = 308,
            K = 2048, N = 1280 -- at rank 16 and 64, against az_gemm_bf16 on the same product (the general product cannot apply the
            scale s; it is timed at s = 1).  The two sides alternate, each as a native launch tape of `inner` back-to-back
            launches (the interpreter's ctypes call costs more than these kernels run); `spread` is max - min over the repetitions of the
            SAME side.
              down   u = x A^T             [M][r]   = [M][K] . [r][K]^T          vs  gemm nt
              up     y += s u B^T          [M][N]  += [M][r] . [N][r]^T          vs  gemm nt, accumulate
              wgrad  dA += du^T x          [r][K]  += [M][r]^T . [M][K]          vs  gemm tn, accumulate, split_k auto
            lora_exec.LoraRoutes.up / tall route a product to the side that wins here (the general product where s = 1 and the rank is a
            multiple of 8 allow it).
  geglu:    az_lora_up_geglu_bf16 (the up product of ff.net.0.proj with the GEGLU in its epilogue) against the two-launch form -- the up
            product as lora_exec.LoraRoutes.up issues it today (az_lora_up_bf16 or accumulate-az_gemm_bf16), then az_geglu_fwd -- at
            M = 4096, H = 5120 and M = 16384, H = 2560, rank 16 and 64, s = 1 and s = 1/2.  Same procedure as `kernels`.
            lora_exec.LoraRoutes.up_geglu issues the side that wins here (profiles/lora_ff_time.json).
  step:     one micro-step at 1024^2, B = 4: rank 16, alpha 16 with the base frozen -- scope "attention" (all eight projections) and
            scope "transformer" (every Linear of every Transformer2DModel) -- against the full fine-tune micro-step (everything
            trainable) of the SAME tree with LoRA off, alternated in one process; and the number of launches each records on its tape.
            (With LoRA off this tree issues the parent commit's launches: profiles/lora_bench_ab.json and lora_ff_bench_ab.json hold
            the alternated bench.py runs of the builds.)

  dora:     (--dora: this leg alone; profiles/dora_time.json) the three az_dora_* kernels at the shapes above and at the two GEGLU
            projections [M][2 H] -- az_dora_norm_bf16 on a one-module table, az_dora_scale_bf16 with bias and residual,
            az_dora_bwd_bf16 with the magnitude's gradient -- each as a native launch tape, `reps` repetitions dealt round-robin over
            the kernels; the norm pass over all modules of scope "attention" and "transformer" at SDXL size, rank 16; and one micro-step
            at 1024^2, B = 4, rank 16 with DoRA against plain LoRA of this tree for both scopes, alternated in one process, with the
            launches each records.

    python tools/lora_time.py [--reps 9] [--inner 200] [--no-kernels] [--no-geglu] [--no-step] [--dora] [--out FILE]
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
SHAPES = [("self M=16384 C=640", 16384, 640, 640), ("self M=4096 C=1280", 4096, 1280, 1280), ("context M=308 K=2048 N=1280", 308, 2048, 1280)]
RANKS = (16, 64)
GEGLU_SHAPES = [("ff M=4096 H=5120", 4096, 5120), ("ff M=16384 H=2560", 16384, 2560)]


def taped(fn, inner):
    """`inner` launches of fn as a native launch tape (tape.NativeTape): issued from C back to back, so that a kernel of a few
    microseconds is timed by the GPU and not by the interpreter's 14 us per ctypes call."""
    from aozora_sdxl_training_amd._lib import lib
    from aozora_sdxl_training_amd.tape import NativeTape
    L = lib()
    L.recorder = []
    try:
        fn()
    finally:
        rec, L.recorder = L.recorder, None
    return NativeTape(rec * inner), inner * len(rec)


def timed(tape, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    tape.play()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner          # us per call of the wrapper (a tall reduction is two launches)


def ab(fa, fb, reps, inner):
    side = lambda t: dict(median_us=round(statistics.median(t), 2), spread_us=round(max(t) - min(t), 2))
    tape_a = taped(fa, inner)[0]
    try:
        tape_b = taped(fb, inner)[0]
    except Exception as e:          # the general product refuses the shape: the adapter kernel has no rival there
        timed(tape_a, inner)
        return dict(lora=side([timed(tape_a, inner) for _ in range(reps)]), gemm=None, gemm_refused=str(e)[:120])
    for t in (tape_a, tape_b):
        timed(t, inner)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(tape_a, inner)); tb.append(timed(tape_b, inner))
    a, b = side(ta), side(tb)
    return dict(lora=a, gemm=b, lora_wins_beyond_spread=bool(b["median_us"] - a["median_us"] > max(a["spread_us"], b["spread_us"])))


def kernels(reps, inner):
    from aozora_sdxl_training_amd import ops
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s: (torch.randn(*s, generator=g, device=DEV) * 0.05).bfloat16()
    out = {}
    for label, M, K, N in SHAPES:
        for r in RANKS:
            x, A, u = rnd(M, K), rnd(r, K), rnd(M, r)
            B, y, dA = rnd(N, r), rnd(M, N), rnd(r, K)
            u2, y2, dA2 = u.clone(), y.clone(), dA.clone()
            res = {
                "down": ab(lambda: ops.lora_down(x, A, u), lambda: ops.gemm(x, A, u2, trans_b=True), reps, inner),
                "up": ab(lambda: ops.lora_up(u, B, y, scale=1.0), lambda: ops.gemm(u, B, y2, trans_b=True, accumulate=True), reps, inner),
                "wgrad": ab(lambda: ops.lora_wgrad(u, x, dA, accumulate=True), lambda: ops.gemm(u, x, dA2, trans_a=True, trans_b=False, accumulate=True, split_k=0),
                            reps, inner),
            }
            if K == N:      # the fused q|k|v group in one adapter launch against one general product per part
                u3, B3, y3 = rnd(M, 3 * r), rnd(3 * N, r), rnd(M, 3 * N)
                y3b = y3.clone()

                def three(u3=u3, B3=B3, y3b=y3b, r=r, N=N):
                    for p in range(3):
                        ops.gemm(u3[:, p * r:(p + 1) * r], B3[p * N:(p + 1) * N], y3b[:, p * N:(p + 1) * N], trans_b=True, accumulate=True)
                res["up, 3 fused parts"] = ab(lambda: ops.lora_up(u3, B3, y3, parts=3, scale=1.0), three, reps, inner)
            out[f"{label} r={r}"] = res
    return out


def geglu_kernels(reps, inner):
    from aozora_sdxl_training_amd import ops
    from aozora_sdxl_training_amd.lora_exec import LoraRoutes
    g = torch.Generator(device=DEV).manual_seed(1)
    rnd = lambda *s: (torch.randn(*s, generator=g, device=DEV) * 0.05).bfloat16()
    rule = LoraRoutes()
    out = {}
    for label, M, H in GEGLU_SHAPES:
        for r in RANKS:
            u, B, proj, o = rnd(M, r), rnd(2 * H, r), rnd(M, 2 * H), rnd(M, H)
            proj2, o2 = proj.clone(), o.clone()
            for s in (1.0, 0.5):
                def two(s=s):
                    rule.up(u, B, proj2, s)
                    ops.geglu_fwd(proj2, o2)
                res = ab(lambda s=s: ops.lora_up_geglu(u, B, proj, o, scale=s), two, reps, inner)
                res = dict(fused=res["lora"], two_launch=res["gemm"], fused_wins_beyond_spread=res["lora_wins_beyond_spread"],
                           two_launch_wins_beyond_spread=bool(res["lora"]["median_us"] - res["gemm"]["median_us"] >
                                                              max(res["lora"]["spread_us"], res["gemm"]["spread_us"])))
                out[f"{label} r={r} s={s:g}"] = res
    return out


def step_ab(rounds, per_round):
    from bench import init_weights_on_device, synthetic_batch
    from aozora_sdxl_training_amd._lib import Call
    from aozora_sdxl_training_amd.train_step import TrainStep
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import SDXL_BASE, LoraSpec
    batch = synthetic_batch(0, 0, 0, 4, DEV)
    sides = {}
    for name, spec in (("full", None), ("lora", LoraSpec(16, 16.0)), ("lora_transformer", LoraSpec(16, 16.0, "", "transformer"))):
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
    if launches["full"] and launches["lora"]:
        res["lora_launches_minus_full"] = launches["lora"] - launches["full"]
    res["lora_over_full"] = round(res["lora"]["median_ms"] / res["full"]["median_ms"], 4)
    res["lora_transformer_over_full"] = round(res["lora_transformer"]["median_ms"] / res["full"]["median_ms"], 4)
    return res


def _sdxl_unet(spec):
    from bench import init_weights_on_device
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import SDXL_BASE
    unet = AozoraUNet(SDXL_BASE, DEV, lora=spec)
    init_weights_on_device(unet)
    adapters = set(unet.lora_state_dict())
    g = torch.Generator(device=DEV).manual_seed(3)
    with torch.no_grad():
        for n, p in unet.named_parameters():
            p.requires_grad = n in adapters
            if n.endswith(".lora_A.weight"):
                p.copy_((torch.randn(p.shape, generator=g, device=DEV) * 0.02).bfloat16())
    if spec.dora:
        unet.dora.refresh(init=True)        # B = 0: the magnitudes are the base weight's row norms
    return unet


def dora_kernels(reps, inner):
    """us per call of the three az_dora_* entry points (median and spread over `reps`, the kernels taking turns)."""
    from aozora_sdxl_training_amd import dora, ops
    from aozora_sdxl_training_amd.lora_norm import s_bits
    g = torch.Generator(device=DEV).manual_seed(2)
    rnd = lambda *s: (torch.randn(*s, generator=g, device=DEV) * 0.05).bfloat16()
    side = lambda t: dict(median_us=round(statistics.median(t), 2), spread_us=round(max(t) - min(t), 2))
    shapes = SHAPES + [(f"{label} (N = 2 H)", M, 1280 if H == 5120 else 640, 2 * H) for label, M, H in GEGLU_SHAPES]
    out = {}
    for label, M, K, N in shapes:
        for r in RANKS:
            W, A, B, m = rnd(N, K), rnd(r, K), rnd(N, r), rnd(N)
            gg, inv = torch.ones(N, device=DEV), torch.ones(N, device=DEV)
            row = [W.data_ptr(), A.data_ptr(), B.data_ptr(), m.data_ptr(), gg.data_ptr(), inv.data_ptr(), r, K, N, s_bits(1.0), 0, 0]
            dora.check_row(row)
            table, tiles = torch.tensor([row], dtype=torch.int64, device=DEV), (N + dora.TILE_ROWS - 1) // dora.TILE_ROWS
            v, y, res, bias, dy, dv, dm = rnd(M, N), rnd(M, N), rnd(M, N), rnd(N), rnd(M, N), rnd(M, N), rnd(N)
            tapes = {"norm (one module)": taped(lambda: ops.dora_norm(table, tiles, False), inner)[0],
                     "scale": taped(lambda: ops.dora_scale(v, gg, y, bias=bias, residual=res), inner)[0],
                     "bwd": taped(lambda: ops.dora_bwd(dy, gg, dv, v=v, inv=inv, dm=dm), inner)[0]}
            times = {k: [] for k in tapes}
            for t in tapes.values():
                timed(t, inner)
            for _ in range(reps):
                for k, t in tapes.items():
                    times[k].append(timed(t, inner))
            out[f"{label} r={r}"] = {k: side(v_) for k, v_ in times.items()}
            if r == RANKS[0]:       # scale and bwd do not see the rank
                out[f"{label} r={r}"]["bytes_scale"] = 2 * M * N * 3
    return out


def dora_norm_pass(reps, inner):
    """az_dora_norm_bf16 over every module of a scope at SDXL size, rank 16: us per pass, modules, rows, bytes of W read."""
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    out = {}
    for scope in ("attention", "transformer"):
        unet = _sdxl_unet(LoraSpec(16, 16.0, "", scope, dora=True))
        tape = taped(lambda: unet.dora.refresh(), inner)[0]
        timed(tape, inner)
        t = [timed(tape, inner) for _ in range(reps)]
        w_bytes = sum(2 * int(row[7]) * int(row[8]) for row in unet.dora.table.cpu().tolist())
        out[scope] = dict(median_us=round(statistics.median(t), 1), spread_us=round(max(t) - min(t), 1), modules=unet.dora.n,
                          rows=int(unet.dora.g.numel()), tiles=unet.dora.tiles, base_weight_bytes_read=w_bytes,
                          GB_per_s=round(w_bytes / statistics.median(t) / 1e3, 1))
        del unet, tape
        torch.cuda.empty_cache()
    return out


def dora_step_ab(rounds, per_round):
    """One micro-step at 1024^2, B = 4, rank 16: DoRA against plain LoRA of this tree, both scopes, alternated in one process."""
    from bench import synthetic_batch
    from aozora_sdxl_training_amd._lib import Call
    from aozora_sdxl_training_amd.train_step import TrainStep
    from aozora_sdxl_training_amd.unet_spec import LoraSpec
    batch = synthetic_batch(0, 0, 0, 4, DEV)
    sides = {}
    for name, spec in (("lora", LoraSpec(16, 16.0)), ("dora", LoraSpec(16, 16.0, dora=True)),
                       ("lora_transformer", LoraSpec(16, 16.0, "", "transformer")), ("dora_transformer", LoraSpec(16, 16.0, "", "transformer", dora=True))):
        unet = _sdxl_unet(spec)
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
    res = {k: dict(median_ms=round(statistics.median(v), 3), spread_ms=round(max(v) - min(v), 3)) for k, v in times.items()}
    launches, act = {}, {}
    for name, (unet, step) in sides.items():
        tapes = [bk.tape for bk in step._buckets.values() if getattr(bk, "tape", None) is not None]
        launches[name] = sum(1 for op in tapes[0] if isinstance(op, Call) and op.name != "az_set_launch_stop_event") if tapes else None
        act[name] = max(unet.activation_bytes()["need"].values())
    res["launches_per_micro_step"] = launches
    res["activation_bytes"] = act
    for scope in ("", "_transformer"):
        a, b = res["lora" + scope], res["dora" + scope]
        res["dora_over_lora" + scope] = round(b["median_ms"] / a["median_ms"], 4)
        res["dora_slower_beyond_spread" + scope] = bool(b["median_ms"] - a["median_ms"] > max(a["spread_ms"], b["spread_ms"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--per-round", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-geglu", action="store_true")
    ap.add_argument("--dora", action="store_true", help="the DoRA leg alone (profiles/dora_time.json)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_time needs a GPU")
    rep = dict(tool="tools/lora_time.py", device=torch.cuda.get_device_name(0))
    if a.dora:
        rep["procedure"] = f"native launch tapes of {a.inner} launches, {a.reps} repetitions, sides taking turns in one process; spread = max - min of one side"
        if not a.no_kernels:
            rep["dora_kernels_us"] = dora_kernels(a.reps, a.inner)
            rep["dora_norm_pass_sdxl_rank16"] = dora_norm_pass(a.reps, max(1, a.inner // 10))
        if not a.no_step:
            rep["micro_step_1024_B4_rank16"] = dora_step_ab(a.rounds, a.per_round)
        a.no_kernels = a.no_geglu = a.no_step = True
    if not a.no_kernels:
        rep["kernels"] = kernels(a.reps, a.inner)
    if not a.no_geglu:
        rep["up_geglu"] = geglu_kernels(a.reps, a.inner)
    if not a.no_step:
        rep["micro_step_1024_B4_rank16"] = step_ab(a.rounds, a.per_round)
    line = json.dumps(rep, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rep, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
