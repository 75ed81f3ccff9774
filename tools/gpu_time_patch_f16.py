"""Timing: the patch layer of an fp16-stored window beside the fp32 window's (both csrc/patch_fc_split.hip) and
the bf16 window's (csrc/patch_fc_fwd.hip, csrc/patch_wgrad.hip), forward and weight gradient, at 8 x 100 000 and 32 x 15 000
rows; then the eager MCAT window step (harness.train_window, dropout on) on an fp32 against an fp16 window of 8 x 15 000 rows.
HIP events around 10 calls, 3 warm-up calls, 7 repeats with the ways alternated inside each repeat; median and spread
(max - min) per way.  One process, one machine: the fp32 line is the yardstick of the fp16 line.

The bar NOTES.md holds the fp16 kernels to: median <= the fp32 kernel's median + its spread, both directions, both sizes.
Algorithmic bytes (forward: X read once, H_bag written once; weight gradient: dH, H_bag and X read once) over the time are
printed as a fraction of 8 TB/s.

    python tools/gpu_time_patch_f16.py [--json PATH]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from multimodal_path_omic_amd import _lib as L  # noqa: E402
from multimodal_path_omic_amd import harness, ops  # noqa: E402
from multimodal_path_omic_amd import synthetic as syn  # noqa: E402
from multimodal_path_omic_amd.models import MultimodalCoAttentionTransformer  # noqa: E402
from multimodal_path_omic_amd.ops import BagBatch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("gpu_time_patch_f16: no GPU (a timing taken anywhere else says nothing)")
dev = torch.device("cuda:0")
torch.manual_seed(0)
EMBED, K, REPEATS, CALLS, WARM, PEAK, P = 256, 1024, 7, 10, 3, 8e12, 0.25
SIZES = ((8, 100000), (32, 15000))
WAYS = ("fp32", "fp16", "bf16")


def events(fn, n=CALLS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3                          # us per call


def alternate(work):
    """{way: fn} -> {way: (median, spread, [samples])}"""
    for fn in work.values():
        events(fn, WARM)
    samples = {w: [] for w in work}
    for _ in range(REPEATS):
        for w, fn in work.items():
            samples[w].append(events(fn))
    return {w: (statistics.median(v), max(v) - min(v), v) for w, v in samples.items()}


def patch_layer(slides, rows):
    t = slides * rows
    lib = L.lib()
    x32 = torch.randn(t, K, device=dev)
    x = {"fp32": x32, "fp16": x32.half(), "bf16": x32.bfloat16()}
    del x32
    w = torch.randn(EMBED, K, device=dev) / K ** 0.5
    b = torch.randn(EMBED, device=dev) * 0.1
    batch = BagBatch(x["bf16"], ops.make_cu([rows] * slides, dev), [rows] * slides)
    h = {"fp32": ops.patch_fc_f32(x["fp32"], w, b, P), "fp16": ops.patch_fc_f16(x["fp16"], w, b, P)}
    dh = torch.randn(t, EMBED, device=dev) * 0.01
    g16 = dh.bfloat16()
    dw, db = torch.empty(EMBED, K, device=dev), torch.empty(EMBED, device=dev)
    ws = ops._workspace(lib.mpo_patch_fc_f32_workspace_bytes(1), dev)
    gate, s = 256.0 / (256.0 - 64.0), L.stream_of(dh)
    fwd = {"fp32": lambda: ops.patch_fc_f32(x["fp32"], w, b, P), "fp16": lambda: ops.patch_fc_f16(x["fp16"], w, b, P),
           "bf16": lambda: ops.patch_fc(x["bf16"], w, b, P, batch=batch)}
    # (the bf16 window's weight gradient takes a pre-gated bf16 g: its gate runs in the co-attention backward)
    bwd = {"fp32": lambda: L.call("mpo_patch_fc_f32_backward", L.ptr(dh), L.ptr(h["fp32"]), L.ptr(x["fp32"]), t, EMBED, K, gate, L.ptr(dw),
                                  L.ptr(db), L.ptr(ws), ws.numel(), s),
           "fp16": lambda: L.call("mpo_patch_fc_f16_backward", L.ptr(dh), L.ptr(h["fp16"]), L.ptr(x["fp16"]), t, EMBED, K, 64, L.ptr(dw),
                                  L.ptr(db), L.ptr(ws), ws.numel(), s),
           "bf16": lambda: ops.patch_weight_grad(g16, x["bf16"], dw)}
    elem = {"fp32": 4, "fp16": 2, "bf16": 2}
    out = {}
    with torch.no_grad():
        for name, work in (("forward", fwd), ("weight gradient", bwd)):
            res = alternate(work)
            for way in WAYS:
                hb = 2 if way == "bf16" else 4                    # H_bag / dH bytes per element
                nbytes = t * (K * elem[way] + EMBED * hb * (1 if name == "forward" else (1 if way == "bf16" else 2)))
                med, spread, v = res[way]
                out[f"{name}/{way}"] = dict(median_us=med, spread_us=spread, samples_us=v, hbm_fraction=nbytes / (med * 1e-6) / PEAK)
                print(f"{slides:2d} x {rows:6d} {name:15s} {way}: median {med:8.1f} us, spread {spread:6.1f} ({min(v):.1f} - {max(v):.1f}), "
                      f"{nbytes / (med * 1e-6) / PEAK * 100:5.1f} % of HBM", flush=True)
            f32, f16 = res["fp32"], res["fp16"]
            ok = f16[0] <= f32[0] + f32[1]
            out[f"{name}/bar"] = dict(fp16_over_fp32=f16[0] / f32[0], holds=bool(ok))
            print(f"{slides:2d} x {rows:6d} {name:15s} fp16 / fp32 = {f16[0] / f32[0]:.3f}; bar (fp16 median <= fp32 median + fp32 spread = "
                  f"{f32[0] + f32[1]:.1f} us): {'holds' if ok else 'MISSED'}", flush=True)
    return out


def window_step(slides=8, rows=15000):
    omic_sizes = [256] * 6
    cohort = syn.make_cohort(slides, rows, rows, omic_sizes, 77)
    work = {}
    for way, dt in (("fp32", torch.float32), ("fp16", torch.float16)):
        model = MultimodalCoAttentionTransformer(omic_sizes=omic_sizes, bag_dtype=dt).to(dev).train()
        window = harness.make_window(cohort, dev, dt)

        def step(model=model, window=window):
            model.zero_grad(set_to_none=True)
            harness.train_window(model, *window, slides)
        work[way] = step
    res = alternate(work)
    for way, (med, spread, v) in res.items():
        print(f"eager MCAT window step, {slides} x {rows} rows, {way} window: median {med:8.1f} us, spread {spread:6.1f} "
              f"({min(v):.1f} - {max(v):.1f})", flush=True)
    return {way: dict(median_us=m, spread_us=sp, samples_us=v) for way, (m, sp, v) in res.items()}


results = {}
for slides, rows in SIZES:
    results[f"{slides}x{rows}"] = patch_layer(slides, rows)
    torch.cuda.empty_cache()
results["mcat_window_step"] = window_step()
if "--json" in sys.argv:
    path = sys.argv[sys.argv.index("--json") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(results, f, indent=1)
