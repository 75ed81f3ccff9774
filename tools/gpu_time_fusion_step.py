#!/usr/bin/env python3
"""ms per captured window step of MCAT medium (bf16 window, training mode, Adam in the graph) for each `fusion` value, in
ONE GPU process:
    python tools/gpu_time_fusion_step.py [--fusions concat,bilinear,gated_concat] [--window 32] [--patches 15000]
                                         [--repeats 7] [--steps 10] [--only FUSION]
The three models share one resident window.  Each repeat is `steps` replays between two HIP events; the fusions alternate
repeat by repeat so that a drift of the machine lands on all of them; two untimed repeats come first.  Prints every repeat,
then one JSON line with the medians and each fusion's own spread (max - min over its repeats).
--only FUSION: build and replay that one step alone (`repeats * steps` replays, one timing) -- the workload for a
`rocprofv3 --kernel-trace --stats -- python tools/gpu_time_fusion_step.py --only bilinear` run.
--grad-guard: instead of the fusions, the first fusion's step with dp.FlatOptimizer('adam') in the graph, its gradient guard
off and on (max_grad_norm=1.0, skip_nonfinite=True: the norm pass's two launches in front of the optimiser pass), timed the
same alternating way: what the guard costs per step.
The script uses nothing but the package's public training API, so the same file times an older checkout."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_path_omic_amd import harness                                                    # noqa: E402
from multimodal_path_omic_amd.dp import FlatAdam, FlatGradBucket, FlatOptimizer                 # noqa: E402
from multimodal_path_omic_amd.models import MultimodalCoAttentionTransformer                    # noqa: E402
from multimodal_path_omic_amd.ops import BagBatch, make_cu                                      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--fusions", default="concat,bilinear,gated_concat")
ap.add_argument("--only", default=None)
ap.add_argument("--window", type=int, default=32)
ap.add_argument("--patches", type=int, default=15000)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--grad-guard", action="store_true")
a = ap.parse_args()
fusions = [a.only] if a.only else a.fusions.split(",")
dev = torch.device("cuda:0")

g = torch.Generator(device=dev)
g.manual_seed(1234)
lengths = [a.patches] * a.window
data = torch.randn(sum(lengths), 1024, device=dev, dtype=torch.float32, generator=g).to(torch.bfloat16)
bags = BagBatch(data, make_cu(lengths, dev), lengths)
omics = [torch.randn(a.window, 256, device=dev, generator=g) for _ in range(6)]
idx = torch.arange(a.window, device=dev)
window = (bags, omics, idx % 4, (idx % 2).float())

guards = {"guard off": {}, "guard on": dict(max_grad_norm=1.0, skip_nonfinite=True)}
steps = {}
for label in (guards if a.grad_guard else fusions):         # (the labels below are fusions, or the two guard settings)
    torch.manual_seed(0)
    model = MultimodalCoAttentionTransformer(omic_sizes=[256] * 6, model_size="medium",
                                             fusion=fusions[0] if a.grad_guard else label,
                                             bag_dtype=torch.bfloat16).to(dev).train()
    bucket = FlatGradBucket(list(model.parameters()))
    if a.grad_guard:
        opt = FlatOptimizer(bucket, "adam", lr=2e-4, weight_decay=1e-5, **guards[label])
    else:
        opt = FlatAdam(bucket, lr=2e-4, weight_decay=1e-5)
    steps[label] = harness.GraphedWindowStep(model, bucket, window, a.window, opt=opt)
if a.grad_guard:
    what_opt, fusions = f" fusion={fusions[0]} FlatOptimizer(adam)", list(guards)


def timed(step, n):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        step()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / n


what = f"mcat medium bf16 {a.window} x {a.patches}" + (what_opt if a.grad_guard else "")
if a.only:
    ms = timed(steps[a.only], a.repeats * a.steps)
    print(json.dumps({"workload": what, "fusion": a.only, "replays": a.repeats * a.steps, "ms_per_step": round(ms, 4)}))
    sys.exit(0)
for _ in range(2):
    for fusion in fusions:
        timed(steps[fusion], a.steps)
times = {fusion: [] for fusion in fusions}
for _ in range(a.repeats):
    for fusion in fusions:
        times[fusion].append(timed(steps[fusion], a.steps))
for fusion in fusions:
    print(f"{what} {'' if a.grad_guard else 'fusion='}{fusion}: " + " ".join(f"{t:.3f}" for t in times[fusion]) + " ms/step", flush=True)
print(json.dumps({"workload": what, "steps_per_repeat": a.steps,
                  "ms_per_step": {f: round(statistics.median(t), 4) for f, t in times.items()},
                  "spread_ms": {f: round(max(t) - min(t), 4) for f, t in times.items()}}))
