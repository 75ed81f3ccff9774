#!/usr/bin/env python3
"""Times of the gene-expression model's epochs over a resident cohort (harness.GeResidentCohort, train_ge_epoch,
GeCohortEvaluator, csrc/class_metrics.hip) in ONE process:
  1. one training epoch over `n_slides` slides of M x 1024 bf16 in windows of `window` slides with k sampled rows per slide,
     two ways: the eager loop (per window harness.make_ge_window + train_ge_window(sample_rows=k) + the optimiser step; the
     slides' rows already lie on the device, so its make_ge_window pays one device-side torch.cat per window and NO upload:
     the kindest reading of that loop) against harness.train_ge_epoch on a captured step with the optimiser in the graph;
  2. one validation epoch three ways: a per-slide loop with .item() (forward_window on one slide with no map -- kinder than
     the reference's forward(), which returns the M x M map --, the loss and the prediction read by the host per slide),
     GeCohortEvaluator eager, GeCohortEvaluator captured;
  3. harness.classification_metrics_device beside harness.classification_metrics at n = 1 000 and n = 2^20 (3 classes).
    python tools/gpu_time_ge_epoch.py [n_slides] [M] [k] [window] [repeats]
An epoch is timed on the host clock from the call to the end of a device synchronise; "enqueue" is the host time until the
call returns.  The ways alternate repeat by repeat after 2 warm-up calls each; every repeat is printed, with the median and
the spread."""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimodal_path_omic_amd import harness, ops                                                     # noqa: E402
from multimodal_path_omic_amd.dp import FlatAdam, FlatGradBucket                                      # noqa: E402
from multimodal_path_omic_amd.models import GeneExprNarrowContextualAttentionGateTransformer         # noqa: E402

arg = [int(a) for a in sys.argv[1:]]
n_slides, m, k, window, repeats = arg + [64, 15000, 4096, 8, 7][len(arg):]
dev = torch.device("cuda:0")
torch.manual_seed(0)
WIDTH, CLASSES = 1024, 3


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


g = torch.Generator().manual_seed(3)
slides = [dict(wsi=(torch.randn(m, WIDTH, device=dev) * 0.5).to(torch.bfloat16),
               gene_expr_class=int(torch.randint(0, CLASSES, (1,), generator=g))) for _ in range(n_slides)]
cohort = harness.GeResidentCohort(slides, dev, cycle=True, slab_bytes=window * m * WIDTH * 2)   # a slab holds exactly one window
ids = list(range(n_slides))


def new_model():
    return GeneExprNarrowContextualAttentionGateTransformer(bag_dtype=torch.bfloat16, n_classes=CLASSES).to(dev)


# ---- 1. the training epoch
model_e, model_g = new_model().train(), new_model().train()
bucket_e, bucket_g = FlatGradBucket(list(model_e.parameters())), FlatGradBucket(list(model_g.parameters()))
opt_e, opt_g = FlatAdam(bucket_e, lr=1e-4), FlatAdam(bucket_g, lr=1e-4)


def eager_epoch():
    losses = []
    for w0 in range(0, n_slides - window + 1, window):
        bags, labels = harness.make_ge_window(slides[w0:w0 + window], dev, torch.bfloat16)
        bucket_e.begin()
        losses.append(harness.train_ge_window(model_e, bags, labels, window, sample_rows=k))
        bucket_e.finish()
        opt_e.step()
    return torch.cat(losses)


first = ids[:window]
step = harness.GraphedWindowStep(model_g, bucket_g, cohort.window(torch.tensor(first, dtype=torch.int32, device=dev), first),
                                 window, opt=opt_g, sample_rows=k)
print(f"{n_slides} slides x {m} x {WIDTH} bf16, gene-expression model medium, k = {k}, {n_slides // window} windows of {window}")
compare("training epoch", (("make_ge_window + train_ge_window", eager_epoch),
                           ("train_ge_epoch", lambda: harness.train_ge_epoch(step, cohort, ids))))
del step, model_g, bucket_g, opt_g, bucket_e, opt_e
ops.set_rng_epoch(None)
torch.cuda.empty_cache()

# ---- 2. the validation epoch
model = model_e.eval()
labels_host = [s["gene_expr_class"] for s in slides]
one = torch.ones(1, device=dev)


def per_slide():
    total, right = 0.0, 0
    with torch.no_grad():
        for i in ids:
            y, att = model.forward_window(ops.BagBatch.from_lengths(cohort.rows[i], [m]), ce_targets=(cohort.labels[i:i + 1], one))
            total += att["loss"].item()
            right += int(y.argmax(1).item() == labels_host[i])
    return total / n_slides, right / n_slides


eager = harness.GeCohortEvaluator(model, cohort, ids, max_window_slides=window)
captured = harness.GeCohortEvaluator(model, cohort, ids, max_window_slides=window, capture=True)
print(f"{len(eager.windows)} validation windows: accuracy per slide {per_slide()[1]!r}, eager {eager().accuracy_value()!r}, "
      f"captured {captured().accuracy_value()!r}")
compare("validation epoch", (("per-slide loop with .item()", per_slide), ("GeCohortEvaluator eager", eager),
                             ("GeCohortEvaluator captured", captured)))
del slides, cohort, eager, captured
torch.cuda.empty_cache()

# ---- 3. the metrics alone
for n in (1000, 1 << 20):
    g = torch.Generator().manual_seed(n)
    y = torch.softmax(torch.randn(n, CLASSES, generator=g), 1)
    label = torch.randint(0, CLASSES, (n,), generator=g)
    loss = -torch.log(y[torch.arange(n), label])
    d = [t.to(dev) for t in (y, label, loss)]
    for _ in range(3):
        out = harness.classification_metrics_device(*d)
    reps = 20
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        harness.classification_metrics_device(*d)
    b.record()
    b.synchronize()
    harness.classification_metrics(y, label, loss)
    t0 = time.perf_counter()
    host = harness.classification_metrics(y, label, loss)
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_from_device = harness.classification_metrics(*d)
    copy_ms = (time.perf_counter() - t0) * 1e3
    same = all(torch.equal(p.cpu(), q) for p, q in zip(out[:3], host[:3]))
    print(f"classification metrics n = {n}: device {a.elapsed_time(b) / reps * 1e3:.1f} us per call (events around {reps} calls), "
          f"host form {host_ms:.2f} ms from host tensors, {copy_ms:.2f} ms from device tensors (with the copy); integer outputs "
          f"equal: {same}; accuracy device {float(out[3][0])!r} host {float(host[3][0])!r}", flush=True)
print(f"protocol: {repeats} repeats, 2 warm-up calls per way, ways alternated; {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
