#!/usr/bin/env python3
"""Per-bag time of the gene-expression model's training step at M rows (bf16 bag, training mode, every dropout on), three
ways in ONE process:
  (a) forward() + torch.nn.functional.cross_entropy + backward, as bench.py's ge_extra spells it (the M x M map written);
  (b) harness.train_ge_window on a FlatGradBucket, eager (head + `ce` loss in one launch each way, no map);
  (c) the same step captured in harness.GraphedWindowStep.
    python tools/gpu_time_ge_train.py [M] [repeats] [steps_per_repeat]
Each repeat is `steps` back-to-back steps between two HIP events (warm-up discarded); the three ways alternate repeat by
repeat so that a drift of the machine lands on all of them.  Prints every repeat, the medians and (a)'s own spread."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_path_omic_amd import harness, synthetic as syn                       # noqa: E402
from multimodal_path_omic_amd.dp import FlatGradBucket                               # noqa: E402
from multimodal_path_omic_amd.models import GeneExprNarrowContextualAttentionGateTransformer  # noqa: E402

m = int(sys.argv[1]) if len(sys.argv) > 1 else 15000
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device("cuda:0")
torch.manual_seed(0)


def make_model():
    torch.manual_seed(0)
    return GeneExprNarrowContextualAttentionGateTransformer(bag_dtype=torch.bfloat16).to(dev).train()


wsi = syn.make_bag(m, 77).to(dev).to(torch.bfloat16)
target = torch.tensor([1], device=dev)

model_a = make_model()


def step_a():
    model_a.zero_grad(set_to_none=True)
    y, _ = model_a(wsi=wsi)
    torch.nn.functional.cross_entropy(y.unsqueeze(0), target).backward()


model_b = make_model()
bucket_b = FlatGradBucket(list(model_b.parameters()))
bags, labels = harness.make_ge_window([{"wsi": wsi, "gene_expr_class": 1}], dev, torch.bfloat16)


def step_b():
    bucket_b.begin()
    harness.train_ge_window(model_b, bags, labels, 1)
    bucket_b.finish()


model_c = make_model()
bucket_c = FlatGradBucket(list(model_c.parameters()))
step_c = harness.GraphedWindowStep(model_c, bucket_c, (bags, labels), 1, opt=None, warmup=2)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


ways = (("a forward() + F.cross_entropy", step_a), ("b train_ge_window eager", step_b), ("c train_ge_window graphed", step_c))
for _, fn in ways:
    for _ in range(2):
        fn()
torch.cuda.synchronize()
times = {name: [] for name, _ in ways}
for r in range(repeats):
    for name, fn in ways:
        times[name].append(timed(fn))
for name, _ in ways:
    t = times[name]
    print(f"ge_nacagat medium, M={m}, bf16, train [{name}]: " + " ".join(f"{x:.2f}" for x in t) +
          f" ms/bag; median {statistics.median(t):.2f}, spread {max(t) - min(t):.2f}", flush=True)
