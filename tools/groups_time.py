"""Times the flat AdamW update of dist.ShardedRaven at one rank over SDXL-base's real trainable ranges (2.567 G elements, random bf16
gradients, bf16 m / v resident in HBM) with the real "bias, norm -> no weight decay" segment table (param_groups.resolve_unet), HIP
events, the four variants ALTERNATING in one process:
  A  uniform:      az_adamw_flat_ex, one launch per contiguous trainable range, one hyper vector       (today's update: the floor)
  B  per_segment:  az_adamw_flat_ex, one launch per SEGMENT with its group's hyper vector              (groups without the new kernel)
  C  seg:          az_adamw_flat_seg, one launch per contiguous trainable range, the real table
  D  seg_single:   az_adamw_flat_seg, one launch per contiguous trainable range, a table of ONE segment
None includes the gradient-norm pass; all read the gradients unclipped (coef = null).  14 bytes per element in all four.
    python tools/groups_time.py [--reps 5] [--warmup 2] [--out FILE]      -> one JSON line (also written to FILE)"""
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
        raise SystemExit("groups_time needs a GPU")
    from aozora_sdxl_training_amd import ops
    from aozora_sdxl_training_amd import param_groups as PG
    from aozora_sdxl_training_amd._lib import lib
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
    m = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    v = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    ranges = unet.trainable_ranges()
    elements = sum(b1 - a1 for a1, b1 in ranges)
    res = PG.resolve_unet(unet, PG.parse_rules([{"match": "bias, norm", "weight_decay": 0.0}], 0.01), 0.01)
    lr, step = 1e-5, 1e-4
    rows = [[lr, 0.9, 0.999, 1e-8, (1.0 - lr * wd if wd != 0 else 1.0), step * s, 0.03, 0.0] for s, wd in res.groups]
    hyper = torch.tensor(rows, dtype=torch.float32, device=dev)                       # [group][8]; row 0 = the base = the uniform vector
    ghyper = hyper[:, 4:6].contiguous()
    seg_end, seg_gid = ops.upload_group_tables(res.seg_end, res.seg_gid, len(res.groups), ranges, dev)
    one_end, one_gid = ops.upload_group_tables([n], [0], len(res.groups), ranges, dev)
    # the pieces of the trainable ranges that lie in one segment each: what B launches
    pieces, s = [], 0
    for a1, b1 in ranges:
        x = a1
        while x < b1:
            while res.seg_end[s] <= x:
                s += 1
            e = min(b1, res.seg_end[s])
            pieces.append((x, e, res.seg_gid[s]))
            x = e
    L = lib()
    vp = ctypes.c_void_p
    P, G, M, V = unet.pflat.data_ptr(), unet.gflat.data_ptr(), m.data_ptr(), v.data_ptr()

    def uniform():
        st = vp(torch.cuda.current_stream().cuda_stream)
        for a1, b1 in ranges:
            L.call("az_adamw_flat_ex", b1 - a1, vp(P + a1 * 2), vp(G + a1 * 2), 0, vp(M + a1 * 2), vp(V + a1 * 2), 0, vp(hyper[0].data_ptr()), vp(0), st)

    hptr = [hyper[k].data_ptr() for k in range(len(res.groups))]

    def per_segment():
        st = vp(torch.cuda.current_stream().cuda_stream)
        for a1, b1, k in pieces:
            L.call("az_adamw_flat_ex", b1 - a1, vp(P + a1 * 2), vp(G + a1 * 2), 0, vp(M + a1 * 2), vp(V + a1 * 2), 0, vp(hptr[k]), vp(0), st)

    def seg_with(ends, gids):
        def run():
            st = vp(torch.cuda.current_stream().cuda_stream)
            for a1, b1 in ranges:
                L.call("az_adamw_flat_seg", b1 - a1, vp(P + a1 * 2), vp(0), vp(G + a1 * 2), 0, vp(M + a1 * 2), vp(V + a1 * 2), 0, vp(hyper[0].data_ptr()),
                       vp(0), vp(ends.data_ptr()), vp(gids.data_ptr()), ends.numel(), vp(ghyper.data_ptr()), len(res.groups), a1, 0, 0, 0, 0, st)
        return run

    variants = [("A_uniform", uniform), ("B_per_segment", per_segment), ("C_seg", seg_with(seg_end, seg_gid)), ("D_seg_single", seg_with(one_end, one_gid))]

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(a.reps):              # alternating: all four see the same box at the same time
        for name, fn in variants:
            times[name].append(once(fn))
    best = {k: min(t) for k, t in times.items()}
    line = json.dumps(dict(tool="groups_time", elements=elements, launches=len(ranges), segments=len(res.seg_end), segment_launches=len(pieces),
                           groups=[list(x) for x in res.groups], group_counts=[list(c) for c in res.counts], ms=times, ms_min=best,
                           spread_ms={k: max(t) - min(t) for k, t in times.items()}, bytes_per_element=14,
                           TBps_best={k: 14.0 * elements / (t * 1e-3) / 1e12 for k, t in best.items()},
                           C_over_A=best["C_seg"] / best["A_uniform"], D_over_A=best["D_seg_single"] / best["A_uniform"],
                           C_over_B=best["C_seg"] / best["B_per_segment"], gpu=torch.cuda.get_device_name(0)))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
