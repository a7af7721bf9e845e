"""The launch sequence and the result bits of one eager micro-step, for an executor refactor to compare before and after: equal
hashes on two trees mean the same entry points with the same scalars over the same aliasing of buffers, streams and events, and the
same loss, prediction and gradients.

One micro-step through TrainStep(..., use_graph=False), recorded with lib().recorder, for every pair of adapter setup (none and five
LoraSpecs over the three scopes) and freeze mask (base frozen / everything trainable) at the mini configuration, B = 2, latents 8x8 and
5x7 (weights, adapters and inputs seeded as tests/test_lora_model_gpu.py seeds them).  Per step: the number of operations, the count per
entry point, and the SHA-256 of the canonical sequence --
    Call    its name and arguments: one the header declares as a pointer (streams included) becomes the index of that value's first
            appearance in the recording, a scalar is kept exactly
    Record / Wait   the same indices over their event and stream handles
    Live    fn.__name__ and its arguments
so the hash does not depend on where the allocator put things and still sees every aliasing relation -- and the SHA-256 of the bytes of
the loss, of last_pred_nhwc and of gflat after the step.

    python tools/launch_signature.py OUT.json"""
import collections
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

DEV = "cuda:0"
B = 2
LATENTS = ((8, 8), (5, 7))
SETUPS = (None, (4, 8.0), (16, 16.0, "", "transformer"), (4, 8.0, "", "unet", 8, 4.0), (16, 16.0, "", "unet", 16, None), (8, 8.0, "", "unet", 64, 16.0))
MASKS = ("base_frozen", "all_trainable")


def canonical(rec, protos):
    """The recording as a list of JSON-able rows (see the module docstring)."""
    from aozora_sdxl_training_amd._lib import Call, Record, Wait, Live
    seen = {}

    def handle(v):
        v = getattr(v, "value", v)
        if v is None or v == 0:
            return "null"
        if not isinstance(v, int):
            return "host:" + type(v).__name__          # a by-reference host argument
        return seen.setdefault(v, len(seen))

    def scalar(v):
        if isinstance(v, float):
            return v.hex()
        if isinstance(v, (bool, int, str, bytes, type(None))):
            return repr(v)
        return ["obj", seen.setdefault(("obj", id(v)), len(seen))]
    rows = []
    for op in rec:
        if isinstance(op, Call):
            types = [t for t, _ in protos[op.name][1]]
            rows.append([op.name] + [handle(a) if "*" in t else scalar(a) for t, a in zip(types, op.args)])
        elif isinstance(op, Record):
            rows.append(["record", handle(op.event.cuda_event), handle(op.stream.cuda_stream)])
        elif isinstance(op, Wait):
            rows.append(["wait", handle(op.stream.cuda_stream), handle(op.event.cuda_event)])
        elif isinstance(op, Live):
            rows.append(["live", op.fn.__name__] + [scalar(a) for a in op.args])
        else:
            raise TypeError(f"unknown tape operation {type(op).__name__}")
    return rows


def sha(data) -> str:
    return hashlib.sha256(data).hexdigest()


def tensor_sha(t) -> str:
    return sha(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes())


def inputs(h, w, pc, seed=7):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(B, 4, h, w, generator=g).bfloat16()
    noise = torch.randn(B, 4, h, w, generator=g)
    ctx = torch.randn(B, 77, pc.cross_attention_dim, generator=g).bfloat16()
    pooled = torch.randn(B, pc.pooled_dim, generator=g).bfloat16()
    tid = torch.tensor([[h * 8, w * 8, 0, 0, h * 8, w * 8]] * B, dtype=torch.bfloat16)
    ts = torch.tensor([37, 911])
    jit = torch.rand(B, generator=g)
    return lat.to(DEV), noise.to(DEV), ts, ctx.to(DEV), pooled.to(DEV), tid.to(DEV), jit


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    if not torch.cuda.is_available():
        raise SystemExit("launch_signature needs a GPU")
    from aozora_sdxl_training_amd._lib import lib
    from aozora_sdxl_training_amd.train_step import TrainStep
    from aozora_sdxl_training_amd.unet import AozoraUNet
    from aozora_sdxl_training_amd.unet_spec import LoraSpec, mini_config
    from oracle.unet_ref import UNetConfig as OC, init_params
    pc = mini_config()
    oc = OC(block_out_channels=pc.block_out_channels, transformer_layers=pc.transformer_layers, head_dim=64,
            cross_attention_dim=pc.cross_attention_dim, addition_time_embed_dim=pc.addition_time_embed_dim,
            pooled_dim=pc.pooled_dim, norm_groups=pc.norm_groups)
    params = {k: v.bfloat16().float() for k, v in init_params(oc, seed=1234).items()}
    L = lib()
    steps = {}
    for setup in SETUPS:
        for mask in MASKS:
            unet = AozoraUNet(pc, DEV, lora=LoraSpec(*setup) if setup is not None else None).load_state_dict(params)
            if setup is not None:
                unet.init_lora(42)
                g = torch.Generator().manual_seed(5)         # Gaussian up matrices: with B = 0 every dA would be zero
                sd = {n: t.float().cpu() for n, t in unet.lora_state_dict().items()}
                for n in sd:
                    if n.endswith(".lora_B.weight"):
                        sd[n] = (0.02 * torch.randn(sd[n].shape, generator=g)).bfloat16().float()
                unet.load_lora_state_dict(sd)
            if mask == "base_frozen":
                for n, p in unet.named_parameters():
                    p.requires_grad = ".lora_" in n
            step = TrainStep(unet, mode="epsilon", grad_accum=1, use_graph=False)
            for h, w in LATENTS:
                args = inputs(h, w, pc)
                unet.zero_grad()
                L.recorder = []
                try:
                    loss = step.micro_step(*args)
                    step.synchronize()
                finally:
                    rec, L.recorder = L.recorder, None
                rows = canonical(rec, L.protos)
                counts = collections.Counter(r[0] for r in rows)
                key = f"{'none' if setup is None else ','.join(str(v) for v in setup)}|{mask}|{h}x{w}"
                steps[key] = dict(operations=len(rows), counts=dict(sorted(counts.items())), sequence_sha256=sha(json.dumps(rows).encode()),
                                  loss_sha256=tensor_sha(loss), pred_sha256=tensor_sha(step.last_pred_nhwc), gflat_sha256=tensor_sha(unet.gflat))
                print(key, steps[key]["operations"], steps[key]["sequence_sha256"][:16], steps[key]["gflat_sha256"][:16], flush=True)
    rep = dict(tool="tools/launch_signature.py", device=torch.cuda.get_device_name(0), steps=steps)
    with open(sys.argv[1], "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
