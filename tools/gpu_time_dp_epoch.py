#!/usr/bin/env python3
"""What taking the optimiser out of the graph costs: milliseconds per window of harness.train_epoch_dp at WORLD SIZE 1
-- no process group, so no collective: replay, then an eager FlatAdam step -- beside harness.train_epoch with Adam inside
the graph, both over the same resident cohort (MCAT, bf16) in ONE process.  Nothing here measures N > 1.
    python tools/gpu_time_dp_epoch.py [cohort_slides] [M] [k] [n_per_window] [repeats] [epochs_per_repeat]
Each repeat is `epochs` back-to-back epochs between two HIP events after 3 warm-up epochs; the two ways alternate repeat by
repeat so that a drift of the machine lands on both.  Prints every repeat, the medians and the spread (max - min)."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimodal_path_omic_amd import dp, harness                                      # noqa: E402
from multimodal_path_omic_amd.dp import FlatAdam, FlatGradBucket                      # noqa: E402
from multimodal_path_omic_amd.models import MultimodalCoAttentionTransformer          # noqa: E402

arg = [int(a) for a in sys.argv[1:]]
n_cohort, m, k, n, repeats, epochs = arg + [64, 15000, 4096, 32, 7, 5][len(arg):]
dev = torch.device("cuda:0")
torch.manual_seed(0)
SIZES = [64] * 6


def cohort_dicts():
    """Slide dicts whose rows are generated on the device (tools/gpu_time_cohort_epoch.py)."""
    g = torch.Generator().manual_seed(3)
    return [dict(wsi=(torch.randn(m, 1024, device=dev, dtype=torch.float32) * 0.5).to(torch.bfloat16),
                 omics=[torch.randn(s, generator=g) for s in SIZES], survival_class=int(torch.randint(0, 4, (1,), generator=g)),
                 censorship=int(torch.rand(1, generator=g) < 0.3), survival_months=float(torch.rand(1, generator=g) * 100))
            for _ in range(n_cohort)]


cohort = harness.ResidentCohort(cohort_dicts(), dev)
torch.cuda.empty_cache()
ids = list(range(n))
first = cohort.window(torch.tensor(ids, dtype=torch.int32).to(dev), ids)


def build(in_graph: bool):
    torch.manual_seed(0)
    model = MultimodalCoAttentionTransformer(omic_sizes=SIZES, bag_dtype=torch.bfloat16).to(dev).train()
    bucket = FlatGradBucket(list(model.parameters()))
    opt = FlatAdam(bucket, lr=1e-4)
    return harness.GraphedWindowStep(model, bucket, first, n, opt=opt if in_graph else None, warmup=2, sample_rows=k), opt


graphed, _ = build(True)
outside, opt = build(False)
epoch_no = [0]


def plan():
    epoch_no[0] += 1
    orders, n_windows = dp.epoch_orders([cohort.n_slides], n, seed=1, epoch=epoch_no[0])
    return orders[0], n_windows


def epoch_in_graph():
    order, _ = plan()
    harness.train_epoch(graphed, cohort, order)


def epoch_dp():
    order, n_windows = plan()
    harness.train_epoch_dp(outside, cohort, order, opt, n_windows)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(epochs):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / epochs


windows = cohort.n_slides // n
ways = ((f"train_epoch, Adam in the graph, {windows} windows", epoch_in_graph),
        (f"train_epoch_dp at world 1, eager Adam step, {windows} windows", epoch_dp))
for _, fn in ways:
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {name: [] for name, _ in ways}
for _ in range(repeats):
    for name, fn in ways:
        times[name].append(timed(fn) / windows)
print(f"MCAT bf16, {n_cohort} slides x {m} x 1024, sample_rows={k}, {n}-slide windows: ms per window")
for name, t in times.items():
    print(f"  [{name}]: " + " ".join(f"{x:.3f}" for x in t) + f"; median {statistics.median(t):.3f}, spread {max(t) - min(t):.3f}",
          flush=True)
print(f"protocol: {repeats} repeats of {epochs} back-to-back epochs between two HIP events, 3 warm-up epochs per way, ways "
      f"alternated; nothing measured at N > 1; {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
