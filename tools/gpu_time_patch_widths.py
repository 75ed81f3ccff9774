"""Diagnostic timing: the bf16 patch layer at patch feature widths 512, 1024 and 2048 (embed 256) on a 32 x 15 000-row
window -- the forward (mpo_patch_fc_forward: weight packing + csrc/patch_fc_fwd.hip) and the weight gradient
(csrc/patch_wgrad.hip).  HIP events around 10 calls, five repeats with the widths alternated inside each repeat, the
median per width; algorithmic bytes (X read once, H_bag written once / g and X read once) over the time, as a fraction of
8 TB/s.  The 1024 line is the yardstick of the other two: same run, same machine."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from multimodal_path_omic_amd import ops  # noqa: E402
from multimodal_path_omic_amd.ops import BagBatch  # noqa: E402

dev = torch.device("cuda:0")
torch.manual_seed(0)
WIDTHS, EMBED, SLIDES, ROWS, REPEATS, CALLS, PEAK = (512, 1024, 2048), 256, 32, 15000, 5, 10, 8e12
T = SLIDES * ROWS


def events(fn, n=CALLS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3                          # us per call


work = {}
for k in WIDTHS:
    x = torch.randn(T, k, device=dev).to(torch.bfloat16)
    batch = BagBatch(x, ops.make_cu([ROWS] * SLIDES, dev), [ROWS] * SLIDES)
    w = torch.randn(EMBED, k, device=dev) / k ** 0.5
    b = torch.randn(EMBED, device=dev) * 0.1
    g = (torch.randn(T, EMBED, device=dev) * 0.01).to(torch.bfloat16)
    dw = torch.empty(EMBED, k, device=dev)
    work[k] = (lambda x=x, w=w, b=b, batch=batch: ops.patch_fc(x, w, b, 0.25, batch=batch),
               lambda g=g, x=x, dw=dw: ops.patch_weight_grad(g, x, dw))
with torch.no_grad():
    for k in WIDTHS:                                              # warm-up: workspaces, the plan, code objects
        for fn in work[k]:
            events(fn, 3)
    fwd, bwd = {k: [] for k in WIDTHS}, {k: [] for k in WIDTHS}
    for _ in range(REPEATS):
        for k in WIDTHS:
            fwd[k].append(events(work[k][0]))
            bwd[k].append(events(work[k][1]))
print(f"{SLIDES} x {ROWS} rows bf16, embed {EMBED}, dropout 0.25; median of {REPEATS} (min - max), us; HBM = algorithmic bytes / time / 8 TB/s")
for k in WIDTHS:
    bytes_f, bytes_b = T * (k + EMBED) * 2, T * (k + EMBED) * 2
    f, d = statistics.median(fwd[k]), statistics.median(bwd[k])
    print(f"patch_dim {k:4d}: forward {f:7.1f} ({min(fwd[k]):.1f} - {max(fwd[k]):.1f}) {bytes_f / (f * 1e-6) / PEAK * 100:5.1f} % HBM | "
          f"weight gradient {d:7.1f} ({min(bwd[k]):.1f} - {max(bwd[k]):.1f}) {bytes_b / (d * 1e-6) / PEAK * 100:5.1f} % HBM")
