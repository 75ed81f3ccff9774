#!/usr/bin/env python3
"""What the host side of fit costs: milliseconds per epoch of fit.Fit.epoch() beside the hand-written epoch of INTEGRATION.md
(harness.train_epoch, the training C-index, the scheduler, a captured CohortEvaluator) over the same resident cohort (MCAT,
bf16) in ONE process on ONE card.  Both enqueue the same window steps and the same validation; Fit adds the device copies
into its history.  Nothing here measures N > 1.
    python tools/gpu_time_fit_epoch.py [train_slides] [val_slides] [M] [k] [n_per_window] [repeats] [epochs_per_repeat]
Each repeat is `epochs` back-to-back epochs between two HIP events after 3 warm-up epochs; the two ways alternate repeat by
repeat so that a drift of the machine lands on both.  Prints every repeat, the medians and the spread (max - min)."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multimodal_path_omic_amd import dp, fit, harness                                 # noqa: E402
from multimodal_path_omic_amd.dp import FlatGradBucket                                # noqa: E402
from multimodal_path_omic_amd.models import MultimodalCoAttentionTransformer          # noqa: E402

arg = [int(a) for a in sys.argv[1:]]
n_train, n_val, m, k, n, repeats, epochs = arg + [64, 16, 15000, 4096, 32, 7, 5][len(arg):]
dev = torch.device("cuda:0")
torch.manual_seed(0)
SIZES = [64] * 6
TOTAL = 3 + repeats * epochs
CONFIG = {"dataset": {"name": "timing"},
          "model": {"name": "MCAT", "load_from_checkpoint": None, "checkpoint_epoch": 0, "checkpoint_dir": None},
          "training": {"leave_one_out": None, "output_attn_epoch": 0, "test_output_dir": None, "train_size": 0.8, "loss": "ces",
                       "epochs": TOTAL, "optimizer": "adam", "lr": 1e-4, "weight_decay": 1e-5, "grad_acc_step": n,
                       "scheduler": "exp", "alpha": 0.75, "lambda": 0.0, "gamma": 0.99}}


def cohort_dicts():
    """Slide dicts whose rows are generated on the device (tools/gpu_time_dp_epoch.py)."""
    g = torch.Generator().manual_seed(3)
    return [dict(wsi=(torch.randn(m, 1024, device=dev, dtype=torch.float32) * 0.5).to(torch.bfloat16),
                 omics=[torch.randn(s, generator=g) for s in SIZES], survival_class=int(torch.randint(0, 4, (1,), generator=g)),
                 censorship=int(torch.rand(1, generator=g) < 0.3), survival_months=float(torch.rand(1, generator=g) * 100))
            for _ in range(n_train + n_val)]


cohort = harness.ResidentCohort(cohort_dicts(), dev)
torch.cuda.empty_cache()
train_ids, val_ids = list(range(n_train)), list(range(n_train, n_train + n_val))
options = fit.fit_options(CONFIG, "mcat")


def model():
    torch.manual_seed(0)
    return MultimodalCoAttentionTransformer(omic_sizes=SIZES, bag_dtype=torch.bfloat16).to(dev).train()


run = fit.Fit(model(), cohort, train_ids, val_ids, options, sample_rows=k, seed=1, stamp="timing")


class ByHand:
    """The loop a user writes from INTEGRATION.md, one epoch per call."""

    def __init__(self):
        o = options.train
        self.model = model()
        bucket = FlatGradBucket(list(self.model.parameters()))
        self.opt = o.make_optimizer(bucket)
        self.sched = o.make_scheduler(self.opt)
        first = train_ids[:n]
        window = cohort.window(torch.tensor(first, dtype=torch.int32).to(dev), first)
        self.step = harness.GraphedWindowStep(self.model, bucket, window, n, opt=self.opt, sample_rows=k, **o.train_kwargs())
        self.evaluator = harness.CohortEvaluator(self.model, cohort, val_ids, loss=o.loss, alpha=o.alpha, l1=o.l1, capture=True)
        self.history, self.epoch_no = [], 0

    def epoch(self):
        orders, _ = dp.epoch_orders([n_train], n, 1, self.epoch_no)
        loss, risk, ids_run, _ = harness.train_epoch(self.step, cohort, [train_ids[i] for i in orders[0]])
        c_index, _ = harness.concordance_index_device(cohort.censorship[ids_run.long()], cohort.survival_months[ids_run.long()], risk)
        self.sched.step()
        r = self.evaluator()
        self.history.append((loss.mean(), c_index, r.mean_loss, r.c_index))
        self.epoch_no += 1


hand = ByHand()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(epochs):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / epochs


windows = n_train // n
ways = ((f"the hand-written epoch, {windows} windows + validation of {n_val}", hand.epoch),
        (f"Fit.epoch(), {windows} windows + validation of {n_val}", run.epoch))
for _, fn in ways:
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {name: [] for name, _ in ways}
for _ in range(repeats):
    for name, fn in ways:
        times[name].append(timed(fn))
print(f"MCAT bf16, {n_train} + {n_val} slides x {m} x 1024, sample_rows={k}, {n}-slide windows: ms per epoch")
for name, t in times.items():
    print(f"  [{name}]: " + " ".join(f"{x:.3f}" for x in t) + f"; median {statistics.median(t):.3f}, spread {max(t) - min(t):.3f}",
          flush=True)
print(f"protocol: {repeats} repeats of {epochs} back-to-back epochs between two HIP events, 3 warm-up epochs per way, ways "
      f"alternated; nothing measured at N > 1; {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
