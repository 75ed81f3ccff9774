#!/usr/bin/env python3
"""Times of the fixed-budget row sampler (csrc/bag_sample.hip, ops.RowSampler, GraphedWindowStep(sample_rows=k)) in ONE process:
  1. the gather at n_slides x M -> k rows x 1024 bf16, beside torch.index_select with the same indices (the yardstick) and
     a plain torch copy of as many bytes (what tools/gpu_probe_copybw.py measures);
  2. the graphed MCAT and NaCAGaT training step at k rows per slide against the unsampled M-row step;
  3. the graphed ge_nacagat step of one M-row bag at k against the unsampled bag;
  4. bind(window) + replay against a replay alone.
    python tools/gpu_time_row_sampling.py [n_slides] [M] [k] [repeats] [steps_per_repeat]
Each repeat is `steps` back-to-back calls between two HIP events after warm-up; the ways of one comparison alternate repeat
by repeat so that a drift of the machine lands on all of them.  Prints every repeat and the medians."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import row_sampling_replay as R                                                       # noqa: E402
from multimodal_path_omic_amd import harness, ops                                     # noqa: E402
from multimodal_path_omic_amd.dp import FlatGradBucket                                # noqa: E402
from multimodal_path_omic_amd.models import (GeneExprNarrowContextualAttentionGateTransformer,  # noqa: E402
                                             MultimodalCoAttentionTransformer, NarrowContextualAttentionGateTransformer)
from multimodal_path_omic_amd.ops import BagBatch                                     # noqa: E402

n_slides = int(sys.argv[1]) if len(sys.argv) > 1 else 32
m = int(sys.argv[2]) if len(sys.argv) > 2 else 15000
k = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 7
steps = int(sys.argv[5]) if len(sys.argv) > 5 else 10
dev = torch.device("cuda:0")
torch.manual_seed(0)
SIZES = [64] * 6


def timed(fn, n=steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def compare(title, ways, unit="ms"):
    for _, fn in ways:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in ways}
    for _ in range(repeats):
        for name, fn in ways:
            times[name].append(timed(fn))
    scale = 1e3 if unit == "us" else 1.0
    med = {}
    for name, _ in ways:
        t = [x * scale for x in times[name]]
        med[name] = statistics.median(t)
        print(f"{title} [{name}]: " + " ".join(f"{x:.1f}" if unit == "us" else f"{x:.3f}" for x in t) +
              f" {unit}; median {med[name]:.3f}, spread {max(t) - min(t):.3f}", flush=True)
    return med


def make_window(seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    data = torch.randn(n_slides * m, 1024, device=dev, generator=g, dtype=torch.float32).to(torch.bfloat16)
    omics = [torch.randn(n_slides, s, device=dev, generator=g) for s in SIZES]
    labels = torch.randint(0, 4, (n_slides,), device=dev, generator=g)
    cens = (torch.rand(n_slides, device=dev, generator=g) < 0.3).float()
    return BagBatch.from_lengths(data, [m] * n_slides), omics, labels, cens


window = make_window(1)
window2 = make_window(2)           # two sources alternate: 2 x 983 MB at the default size, far beyond the Infinity Cache

# ---- 1. the gather
samplers = [ops.RowSampler(n_slides, k, 1024, torch.bfloat16, dev).bind(w[0]) for w in (window, window2)]
idx = [torch.from_numpy(R.window_indices(1, 2, 0, [m] * n_slides, k)[1]).to(dev) for _ in range(2)]
outs = [torch.empty(n_slides * k, 1024, dtype=torch.bfloat16, device=dev) for _ in range(2)]
flip = [0]


def gather():
    flip[0] ^= 1
    samplers[flip[0]]()


def index_select():
    flip[0] ^= 1
    torch.index_select((window, window2)[flip[0]][0].data, 0, idx[flip[0]], out=outs[flip[0]])


def plain_copy():
    flip[0] ^= 1
    outs[flip[0]].copy_((window, window2)[flip[0]][0].data[:n_slides * k])


moved = 2 * n_slides * k * 1024 * 2
med = compare(f"gather {n_slides} x {m} -> {k} rows x 1024 bf16", (("bag_sample_rows", gather), ("torch.index_select", index_select),
                                                                  ("torch copy, same bytes", plain_copy)), unit="us")
for name, us in med.items():
    print(f"    {name}: {moved / us / 1e6:.2f} TB/s (read + written bytes, {moved / 1e6:.0f} MB)")
del idx, outs, samplers


# ---- 2. the graphed fusion-model steps, 4. bind + replay
def fusion_step(cls, win, sample_rows):
    torch.manual_seed(0)
    model = cls(omic_sizes=SIZES, bag_dtype=torch.bfloat16).to(dev).train()
    bucket = FlatGradBucket(list(model.parameters()))
    return harness.GraphedWindowStep(model, bucket, win, n_slides, opt=None, warmup=2, sample_rows=sample_rows)


for name, cls in (("mcat", MultimodalCoAttentionTransformer), ("nacagat", NarrowContextualAttentionGateTransformer)):
    full, sampled = fusion_step(cls, window, None), fusion_step(cls, window, k)
    compare(f"{name} graphed window step, {n_slides} slides, bf16, train", ((f"all {m} rows", full), (f"sample_rows={k}", sampled)))
    if name == "mcat":
        wins = [window, window2]

        def bind_and_replay():
            flip[0] ^= 1
            sampled.bind(wins[flip[0]])
            sampled()

        compare(f"{name} sample_rows={k}", (("replay alone", sampled), ("bind(window) + replay", bind_and_replay)))
    del full, sampled
    torch.cuda.empty_cache()

# ---- 3. the gene-expression model, one bag
bag = BagBatch.from_lengths(window[0].data[:m], [m])
labels = torch.tensor([1], device=dev)


def ge_step(sample_rows):
    torch.manual_seed(0)
    model = GeneExprNarrowContextualAttentionGateTransformer(bag_dtype=torch.bfloat16).to(dev).train()
    bucket = FlatGradBucket(list(model.parameters()))
    return harness.GraphedWindowStep(model, bucket, (bag, labels), 1, opt=None, warmup=2, sample_rows=sample_rows)


compare("ge_nacagat graphed step, one bag, bf16, train", ((f"all {m} rows", ge_step(None)), (f"sample_rows={k}", ge_step(k))))
print(f"protocol: {repeats} repeats of {steps} back-to-back calls between two HIP events, 3 warm-up calls per way, ways alternated; "
      f"{torch.cuda.get_device_name(0)}, numpy {np.__version__}, torch {torch.__version__}")
