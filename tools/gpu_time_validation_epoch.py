#!/usr/bin/env python3
"""Times of a validation epoch over a resident cohort (harness.CohortEvaluator, csrc/concordance.hip) in ONE process:
  1. one epoch over `n_slides` slides of M x 1024 bf16 in windows of `window` slides, three ways: what a caller did before
     the evaluator existed (per window harness.make_window + forward_window under no_grad, the risks copied to the host,
     harness.concordance_index_censored there -- the loop of tests/test_gpu_cohort.py; the slides' rows already lie on the
     device, so its make_window pays one device-side torch.cat per window and NO upload: the kindest reading of that loop),
     CohortEvaluator eager, CohortEvaluator captured;
  2. harness.concordance_index_device beside harness.concordance_index_censored at n = 1 000 and n = 16 384, with the host
     form's peak memory (tracemalloc, which numpy reports its buffers to).
    python tools/gpu_time_validation_epoch.py [n_slides] [M] [window] [repeats]
An epoch is timed on the host clock from the call to the end of a device synchronise (the old way's C-index is host work
behind a copy, so device events would not see it); "enqueue" is the host time until the call returns.  The ways alternate
repeat by repeat; every repeat is printed, with the median and the spread."""
import os
import statistics
import sys
import time
import tracemalloc

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimodal_path_omic_amd import harness                                          # noqa: E402
from multimodal_path_omic_amd.models import MultimodalCoAttentionTransformer          # noqa: E402

arg = [int(a) for a in sys.argv[1:]]
n_slides, m, window, repeats = arg + [256, 15000, 32, 7][len(arg):]
dev = torch.device("cuda:0")
torch.manual_seed(0)
SIZES = [64] * 6
WIDTH = 1024


def cohort_dicts(n):
    """Slide dicts whose rows are generated on the device (tools/gpu_time_cohort_epoch.py does the same)."""
    g = torch.Generator().manual_seed(3)
    return [dict(wsi=(torch.randn(m, WIDTH, device=dev) * 0.5).to(torch.bfloat16), omics=[torch.randn(s, generator=g) for s in SIZES],
                 survival_class=int(torch.randint(0, 4, (1,), generator=g)), censorship=int(torch.rand(1, generator=g) < 0.3),
                 survival_months=float(torch.randint(1, 120, (1,), generator=g))) for _ in range(n)]


def epoch_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3, out


def compare(title, ways):
    for _, fn in ways:
        for _ in range(2):
            fn()
    total, enqueue = {name: [] for name, _ in ways}, {name: [] for name, _ in ways}
    for _ in range(repeats):
        for name, fn in ways:
            t, e, _ = epoch_time(fn)
            total[name].append(t)
            enqueue[name].append(e)
    for name, _ in ways:
        t = total[name]
        print(f"{title} [{name}]: " + " ".join(f"{x:.2f}" for x in t) + f" ms; median {statistics.median(t):.2f}, spread "
              f"{max(t) - min(t):.2f}; enqueue median {statistics.median(enqueue[name]):.2f} ms", flush=True)


# ---- 1. the validation epoch
slides = cohort_dicts(n_slides)
cohort = harness.ResidentCohort(slides, dev, slab_bytes=window * m * WIDTH * 2)       # a slab holds exactly one window
model = MultimodalCoAttentionTransformer(omic_sizes=SIZES, bag_dtype=torch.bfloat16).to(dev).eval()
ids = list(range(n_slides))
event = np.array([1 - s["censorship"] for s in slides]).astype(bool)
months = np.array([s["survival_months"] for s in slides])


def old_way():
    risks = []
    with torch.no_grad():
        for w0 in range(0, n_slides, window):
            bags, omics, _, _ = harness.make_window(slides[w0:w0 + window], dev, torch.bfloat16)
            _, sv, _, _ = model.forward_window(bags, omics)
            risks.append(harness.risk_score(sv).cpu())
    return harness.concordance_index_censored(event, months, torch.cat(risks).numpy())


eager = harness.CohortEvaluator(model, cohort, ids, max_window_slides=window)
captured = harness.CohortEvaluator(model, cohort, ids, max_window_slides=window, capture=True)
print(f"{n_slides} slides x {m} x {WIDTH} bf16, MCAT medium, {len(eager.windows)} windows of {window}: C-index old way "
      f"{old_way()!r}, eager {eager().c_index_value()!r}, captured {captured().c_index_value()!r}")
compare("validation epoch", (("make_window + forward_window + host C-index", old_way), ("CohortEvaluator eager", eager),
                             ("CohortEvaluator captured", captured)))
del slides, cohort, eager, captured
torch.cuda.empty_cache()

# ---- 2. the C-index alone
for n in (1000, 16384):
    g = np.random.default_rng(n)
    cens = (g.random(n) < 0.3).astype(np.float32)
    tm = g.integers(1, 120, n).astype(np.float64)
    risk = g.standard_normal(n).astype(np.float32)
    d = [torch.from_numpy(x).to(dev) for x in (cens, tm, risk)]
    for _ in range(3):
        c_index, counts = harness.concordance_index_device(*d)
    reps = 20
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        harness.concordance_index_device(*d)
    b.record()
    b.synchronize()
    tracemalloc.start()
    t0 = time.perf_counter()
    host = harness.concordance_index_censored(1 - cens, tm, risk)
    host_s = time.perf_counter() - t0
    peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    print(f"C-index n = {n}: device {a.elapsed_time(b) / reps * 1e3:.1f} us per call (events around {reps} calls), host form "
          f"{host_s * 1e3:.1f} ms with {peak / 2 ** 20:.0f} MiB peak; |device - host| {abs(float(c_index) - host):.1e}, "
          f"counts {counts.tolist()}", flush=True)
print(f"protocol: {repeats} repeats, 2 warm-up calls per way, ways alternated; {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
