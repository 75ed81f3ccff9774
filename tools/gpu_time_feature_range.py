#!/usr/bin/env python3
"""Times of the device feature scale (csrc/feature_range.hip, ops.feature_scale_device, GraphedWindowStep(device_feature_scale=
True)) in ONE process:
  1. the range pass alone over n_slides x k and over big_slides x big_rows rows x 1024 fp32, beside the host path it replaces
     (ops.feature_scale on a tensor with no cached scale: |x| temporary, library reduction, blocking read) and the bytes it
     reads over the 8 TB/s HBM peak;
  2. the fp32 gather alone and the gather with the range pass behind it (ops.RowSampler(device_feature_scale=True)): what the
     pass costs right after the launch that wrote its input;
  3. the captured, sampled fp32 MCAT step against the eager sampled fp32 step (train_window(sample_rows=k): a sampler per
     call, the scale through the host) on the same windows, and the range pass as a share of the captured step;
  4. the captured unsampled fp32 step over the big window with the range pass inside the graph against the same step with
     the scale baked in.
    python tools/gpu_time_feature_range.py [n_slides] [M] [k] [big_slides] [big_rows] [repeats] [steps_per_repeat]
Each repeat is `steps` back-to-back calls between two HIP events after warm-up; the ways of one comparison alternate repeat
by repeat so that a drift of the machine lands on all of them.  Prints every repeat and the medians."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimodal_path_omic_amd import harness, ops                                     # noqa: E402
from multimodal_path_omic_amd.dp import FlatGradBucket                                # noqa: E402
from multimodal_path_omic_amd.models import MultimodalCoAttentionTransformer          # noqa: E402
from multimodal_path_omic_amd.ops import BagBatch                                     # noqa: E402

arg = [int(a) for a in sys.argv[1:]]
n_slides, m, k, big_slides, big_rows, repeats, steps = arg + [32, 15000, 4096, 8, 100000, 7, 10][len(arg):]
dev = torch.device("cuda:0")
torch.manual_seed(0)
SIZES = [64] * 6
HBM_PEAK = 8e12


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def compare(title, ways, unit="ms", n=None):
    n = n or steps
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


def make_window(slides, rows, seed, gain=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    data = torch.randn(slides * rows, 1024, device=dev, generator=g, dtype=torch.float32) * gain
    omics = [torch.randn(slides, s, device=dev, generator=g) for s in SIZES]
    labels = torch.randint(0, 4, (slides,), device=dev, generator=g)
    cens = (torch.rand(slides, device=dev, generator=g) < 0.3).float()
    return BagBatch.from_lengths(data, [rows] * slides), omics, labels, cens


flip = [0]
range_us = {}

# ---- 1. the range pass alone
for title, rows in ((f"{n_slides} x {k}", n_slides * k), (f"{big_slides} x {big_rows}", big_slides * big_rows)):
    xs = [torch.randn(rows, 1024, device=dev) for _ in range(2)]            # two sources alternate: far beyond the Infinity Cache
    out = torch.empty(1, device=dev)

    def on_device():
        flip[0] ^= 1
        ops.feature_scale_device(xs[flip[0]], out=out)

    def on_host():
        flip[0] ^= 1
        xs[flip[0]].__dict__.pop("_mpo_feature_scale", None)
        ops.feature_scale(xs[flip[0]])

    assert float(ops.feature_scale_device(xs[0])) == ops.feature_scale(xs[0])
    nbytes = rows * 1024 * 4
    med = compare(f"range of {title} rows x 1024 fp32 ({nbytes / 1e9:.2f} GB)", (("feature_scale_device", on_device),
                                                                                ("ops.feature_scale, uncached", on_host)), unit="us")
    range_us[title] = med["feature_scale_device"]
    print(f"    feature_scale_device: {nbytes / med['feature_scale_device'] / 1e6:.2f} TB/s read; the bytes over the 8 TB/s peak: "
          f"{nbytes / HBM_PEAK * 1e6:.1f} us ({nbytes / HBM_PEAK * 1e6 / med['feature_scale_device'] * 100:.0f} % of peak)")
    del xs
    torch.cuda.empty_cache()

# ---- 2. the gather, alone and with the range pass behind it
windows = [make_window(n_slides, m, 1, 1e-3), make_window(n_slides, m, 2, 1e2)]
plain = [ops.RowSampler(n_slides, k, 1024, torch.float32, dev).bind(w[0]) for w in windows]
scaled = [ops.RowSampler(n_slides, k, 1024, torch.float32, dev, device_feature_scale=True).bind(w[0]) for w in windows]


def gather():
    flip[0] ^= 1
    plain[flip[0]]()


def gather_and_range():
    flip[0] ^= 1
    scaled[flip[0]]()


med = compare(f"gather {n_slides} x {m} -> {k} rows x 1024 fp32", (("gather", gather), ("gather + range pass", gather_and_range)), unit="us")
behind = med["gather + range pass"] - med["gather"]
print(f"    the range pass behind the gather: {behind:.1f} us ({behind / med['gather'] * 100:.0f} % of the gather; alone it took "
      f"{range_us[f'{n_slides} x {k}']:.1f} us)")
del plain, scaled


# ---- 3. the sampled fp32 step: captured against eager
def model_and_bucket():
    torch.manual_seed(0)
    model = MultimodalCoAttentionTransformer(omic_sizes=SIZES, bag_dtype=torch.float32).to(dev).train()
    return model, FlatGradBucket(list(model.parameters()))


model_g, bucket_g = model_and_bucket()
step = harness.GraphedWindowStep(model_g, bucket_g, windows[0], n_slides, opt=None, warmup=2, sample_rows=k, device_feature_scale=True)
model_e, _ = model_and_bucket()


def captured():
    flip[0] ^= 1
    step.bind(windows[flip[0]])
    step()


def eager():
    flip[0] ^= 1
    model_e.zero_grad(set_to_none=True)
    harness.train_window(model_e, *windows[flip[0]], n_slides, sample_rows=k)


med = compare(f"mcat fp32 sampled step, {n_slides} slides x {m} -> {k} rows, train", (("captured, bind + replay", captured),
                                                                                    ("eager train_window(sample_rows)", eager)))
print(f"    range pass behind the gather = {behind / 1e3 / med['captured, bind + replay'] * 100:.1f} % of the captured step; "
      f"captured / eager = {med['captured, bind + replay'] / med['eager train_window(sample_rows)']:.2f}")
del step, model_g, bucket_g, model_e, windows
torch.cuda.empty_cache()

# ---- 4. the unsampled fp32 step over the big window: the range pass inside the graph against a baked scale
window = make_window(big_slides, big_rows, 3)
model_a, bucket_a = model_and_bucket()
model_b, bucket_b = model_and_bucket()
with_pass = harness.GraphedWindowStep(model_a, bucket_a, window, big_slides, opt=None, warmup=2, device_feature_scale=True)
baked = harness.GraphedWindowStep(model_b, bucket_b, window, big_slides, opt=None, warmup=2)
med = compare(f"mcat fp32 unsampled step, {big_slides} x {big_rows} rows, train", (("scale baked in", baked), ("range pass in the graph", with_pass)))
extra = med["range pass in the graph"] - med["scale baked in"]
print(f"    the range pass in the graph: {extra * 1e3:.1f} us = {extra / med['range pass in the graph'] * 100:.1f} % of the step (alone it took "
      f"{range_us[f'{big_slides} x {big_rows}']:.1f} us)")
print(f"protocol: {repeats} repeats of {steps} back-to-back calls between two HIP events, 3 warm-up calls per way, ways alternated; "
      f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}")
