#!/usr/bin/env python3
"""Times of the resident-cohort sampler (csrc/bag_sample.hip, ops.SlideSet, harness.ResidentCohort / train_epoch) in
ONE process:
  1. the gather at n_slides x M -> k rows x 1024 bf16: from n_slides separate allocations scattered through a cohort of
     `cohort_slides`, beside the contiguous gather on the same slides concatenated (the yardstick) and beside what a user
     without the slide gather must do for a shuffled window, torch.cat of the slides followed by the contiguous gather;
  2. the same with every second slide cut to `short` rows and lapped (for the record);
  3. milliseconds per window of harness.train_epoch (MCAT and NaCAGaT, Adam in the graph) beside replays of one resident
     window, a replay + bind of a contiguous window, and a replay alone.
    python tools/gpu_time_cohort_epoch.py [n_slides] [M] [k] [repeats] [steps_per_repeat] [cohort_slides] [short]
Each repeat is `steps` back-to-back calls between two HIP events after warm-up; the ways of one comparison alternate repeat
by repeat so that a drift of the machine lands on all of them.  Prints every repeat, the medians and the spread (max - min)."""
import os
import random
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimodal_path_omic_amd import harness, ops                                     # noqa: E402
from multimodal_path_omic_amd.dp import FlatAdam, FlatGradBucket                      # noqa: E402
from multimodal_path_omic_amd.models import MultimodalCoAttentionTransformer, NarrowContextualAttentionGateTransformer  # noqa: E402
from multimodal_path_omic_amd.ops import BagBatch, SlideSet                           # noqa: E402

arg = [int(a) for a in sys.argv[1:]]
n_slides, m, k, repeats, steps, n_cohort, short = arg + [32, 15000, 4096, 7, 10, 200, 1000][len(arg):]
dev = torch.device("cuda:0")
torch.manual_seed(0)
SIZES = [64] * 6
WIDTH = 1024


def timed(fn, n=steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def compare(title, ways, unit="ms", n=steps):
    for _, fn in ways:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in ways}
    for _ in range(repeats):
        for name, fn in ways:
            times[name].append(timed(fn, n))
    scale = 1e3 if unit == "us" else 1.0
    med = {}
    for name, _ in ways:
        t = [x * scale for x in times[name]]
        med[name] = statistics.median(t)
        print(f"{title} [{name}]: " + " ".join(f"{x:.1f}" if unit == "us" else f"{x:.3f}" for x in t) +
              f" {unit}; median {med[name]:.3f}, spread {max(t) - min(t):.3f}", flush=True)
    return med


# ---- the cohort: one allocation per slide, so that a window's slides are scattered through the card's memory
def slide_rows(rows):
    return (torch.randn(rows, WIDTH, device=dev, dtype=torch.float32) * 0.5).to(torch.bfloat16)


def gather_ways(title, lengths_of):
    """Two windows of n_slides ids drawn from the cohort alternate (2 x 983 MB of source rows at the default size)."""
    slides = [slide_rows(lengths_of(i)) for i in range(n_cohort)]
    table = SlideSet.slide_table(slides)
    rng = random.Random(1)
    wins, flip = [], [0]
    for _ in range(2):
        ids = rng.sample(range(n_cohort), n_slides)
        ss = SlideSet([slides[i] for i in ids], [int(slides[i].shape[0]) for i in ids], table[0], table[1],
                      torch.tensor(ids, dtype=torch.int32).to(dev), cycle=True)
        wins.append((ss, ss.materialize()))
    lapped = any(mm < k for ss, _ in wins for mm in ss.lengths)
    by_slide = [ops.RowSampler(n_slides, k, WIDTH, torch.bfloat16, dev, source="slides").bind(ss) for ss, _ in wins]
    ways = [("bag_sample_slides, separate allocations", lambda: by_slide[flip[0]]())]
    if not lapped:                      # (the contiguous gather refuses a slide shorter than k in static mode)
        by_rows = [ops.RowSampler(n_slides, k, WIDTH, torch.bfloat16, dev).bind(bags) for _, bags in wins]
        cat_sampler = ops.RowSampler(n_slides, k, WIDTH, torch.bfloat16, dev)

        def cat_then_gather():
            ss = wins[flip[0]][0]
            cat_sampler.bind(BagBatch(torch.cat(ss.slides), wins[flip[0]][1].cu, ss.lengths))()

        ways = [("bag_sample_rows, the slides concatenated", lambda: by_rows[flip[0]]())] + ways + \
               [("torch.cat + bag_sample_rows", cat_then_gather)]

    def alternating(fn):
        def call():
            flip[0] ^= 1
            fn()
        return call
    med = compare(title, [(name, alternating(fn)) for name, fn in ways], unit="us")
    moved = 2 * n_slides * k * WIDTH * 2
    for name, us in med.items():
        print(f"    {name}: {moved / us / 1e6:.2f} TB/s of gathered bytes read + written ({moved / 1e6:.0f} MB)")
    if not lapped:
        a, b = by_rows[0].out, by_slide[0].out
        flip[0] = 0
        ops.set_rng_epoch(None)
        state = ops.rng_state()
        by_rows[0]()
        ops.set_rng_state(state)
        by_slide[0]()
        print(f"    same bits as the contiguous gather at the same stream: {bool(torch.equal(a.view(torch.int16), b.view(torch.int16)))}")


gather_ways(f"gather {n_slides} of {n_cohort} slides x {m} -> {k} rows x {WIDTH} bf16", lambda i: m)
torch.cuda.empty_cache()
gather_ways(f"lapped gather, every second slide {short} rows", lambda i: short if i % 2 else m)
torch.cuda.empty_cache()


# ---- 3. the epoch loop
def cohort_dicts(n):
    """Slide dicts whose rows are generated on the device (uploading 8 windows of M rows from the host would only measure the
    host); harness.ResidentCohort packs them into its slabs."""
    g = torch.Generator().manual_seed(3)
    return [dict(wsi=slide_rows(m), omics=[torch.randn(s, generator=g) for s in SIZES],
                 survival_class=int(torch.randint(0, 4, (1,), generator=g)), censorship=int(torch.rand(1, generator=g) < 0.3),
                 survival_months=float(torch.rand(1, generator=g) * 100)) for _ in range(n)]


cohort = harness.ResidentCohort(cohort_dicts(8 * n_slides), dev)
torch.cuda.empty_cache()
for name, cls in (("mcat", MultimodalCoAttentionTransformer), ("nacagat", NarrowContextualAttentionGateTransformer)):
    def build(window):
        torch.manual_seed(0)
        model = cls(omic_sizes=SIZES, bag_dtype=torch.bfloat16).to(dev).train()
        bucket = FlatGradBucket(list(model.parameters()))
        return harness.GraphedWindowStep(model, bucket, window, n_slides, opt=FlatAdam(bucket, lr=1e-4), warmup=2, sample_rows=k)
    ids = list(range(n_slides))
    first = cohort.window(torch.tensor(ids, dtype=torch.int32).to(dev), ids)
    on_slides = build(first)
    contiguous = [(first[0].materialize(), *first[1:])]
    ids2 = list(range(n_slides, 2 * n_slides))
    second = cohort.window(torch.tensor(ids2, dtype=torch.int32).to(dev), ids2)
    contiguous.append((second[0].materialize(), *second[1:]))
    on_rows = build(contiguous[0])
    rng = random.Random(2)
    flip = [0]

    def epoch():
        order = list(range(cohort.n_slides))
        rng.shuffle(order)
        harness.train_epoch(on_slides, cohort, order)

    def bind_and_replay():
        flip[0] ^= 1
        on_rows.bind(contiguous[flip[0]])
        on_rows()

    windows = cohort.n_slides // n_slides
    med = compare(f"{name} sample_rows={k}, {n_slides}-slide windows, Adam in the graph, per call",
                  ((f"train_epoch of {windows} windows", epoch), ("replay alone, contiguous window", on_rows),
                   ("bind(contiguous window) + replay", bind_and_replay), ("replay alone, slide window", on_slides)), n=max(1, steps // 2))
    print(f"    {name}: train_epoch {med[f'train_epoch of {windows} windows'] / windows:.3f} ms per window")
    del on_slides, on_rows, contiguous, first, second
    torch.cuda.empty_cache()
print(f"protocol: {repeats} repeats of back-to-back calls between two HIP events, 3 warm-up calls per way, ways alternated; "
      f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}")
