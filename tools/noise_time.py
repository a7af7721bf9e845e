"""Two-stream micro-step time (B = 4, 1024^2, all trainable; the setup of tools/policy_time.py) under one NOISE_MODE: the host draws
(noise.draw_aux) and the staging of their buffers are inside the timed window, as in trainer.train.  One process per variant; run the
variants to compare one after the other on the same box and repeat the yardstick to see that box's run-to-run spread.
    python tools/noise_time.py [--noise SPEC] [--root DIR] [--reps 6] [--steps 4]      -> one JSON line
--root: a checkout to import the package (and bench.py) from instead of this one -- a tree without NOISE_MODE is timed with
--noise normal, where TrainStep is built without the argument."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--noise", default="normal")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=6)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--label", default=None)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))

import torch  # noqa: E402
import bench  # noqa: E402
from aozora_sdxl_training_amd.unet import AozoraUNet, ExecPolicy  # noqa: E402
from aozora_sdxl_training_amd.unet_spec import SDXL_BASE  # noqa: E402
from aozora_sdxl_training_amd.train_step import TrainStep  # noqa: E402

normal = a.noise.strip().lower() in ("", "normal")
dev = torch.device("cuda", 0)
unet = AozoraUNet(SDXL_BASE, dev, policy=ExecPolicy())
bench.init_weights_on_device(unet)
batch = bench.synthetic_batch(0, 0, 0, 4, dev)
shape = tuple(batch[0].shape)
if normal:
    step = TrainStep(unet, mode="epsilon", grad_accum=8, use_graph=False)
    draw = lambda i: {}
else:
    from aozora_sdxl_training_amd.noise import draw_aux, parse_noise_mode
    spec = parse_noise_mode(a.noise)
    step = TrainStep(unet, mode="epsilon", grad_accum=8, use_graph=False, noise=spec)
    draw = lambda i: {"noise_aux": draw_aux(spec, shape, 42, i)}
n = 0
for _ in range(3):
    n += 1
    step.micro_step(*batch, **draw(n)); step.synchronize()
ts = []
for r in range(a.reps):
    t0 = time.perf_counter()
    for _ in range(a.steps):
        n += 1
        step.micro_step(*batch, **draw(n))
    step.synchronize()
    ts.append((time.perf_counter() - t0) / a.steps * 1e3)
names = [op.name for op in getattr(step.last_bucket, "tape", None) or [] if hasattr(op, "name")]
print(json.dumps(dict(tool="noise_time", label=a.label or a.noise, noise=a.noise, shape=list(shape), gpu=torch.cuda.get_device_name(0),
                      micro_step_ms=[round(x, 3) for x in ts], median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3),
                      noise_launches=[x for x in names if "noise" in x])), flush=True)
