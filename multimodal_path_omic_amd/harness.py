"""Caller-side semantics of the reference's train()/validate() loops (row H9 of SURVEY.md section
8(a); models/mcat/main.py:19-155), restated for window-batched execution: `ces` loss, risk score,
gradient accumulation over `grad_acc_step` slides, Harrell's C-index.  No per-slide host sync
(the reference's loss.item() at main.py:49 is exactly what this harness must not do)."""
from __future__ import annotations

import math
from contextlib import contextmanager
from dataclasses import dataclass
from typing import List, Sequence

import numpy as np
import torch

from .ops import BagBatch, SlideSet


def ces_loss(hazards, survs, label, censorship, alpha: float = 0.75, eps: float = 1e-7, reduction: str = "mean"):
    """CrossEntropySurvivalLoss (models/loss.py:5-28) for B slides at once: hazards/survs (B,C),
    label (B,) int64, censorship (B,) float.  reduction 'mean' | 'sum' | 'none' over slides."""
    y = label.view(-1, 1).long()
    c = censorship.view(-1, 1).float()
    s_pad = torch.cat([torch.ones_like(c), survs], 1)
    reg = -(1 - c) * (torch.log(torch.gather(s_pad, 1, y).clamp(min=eps))
                      + torch.log(torch.gather(hazards, 1, y).clamp(min=eps)))
    s_y = torch.gather(survs, 1, y).clamp(min=eps)
    ce = -(c * torch.log(s_y) + (1 - c) * torch.log(1 - s_y))
    loss = ((1 - alpha) * ce + alpha * reg).view(-1)
    if reduction == "mean":
        return loss.mean()
    if reduction == "sum":
        return loss.sum()
    return loss


def risk_score(survs):
    """risk = -sum_j survs_j (models/mcat/main.py:56)."""
    return -survs.sum(dim=1)


def concordance_index_censored(event, time, risk, tied_tol: float = 1e-8) -> float:
    """Harrell's C with scikit-survival's conventions (the reference calls
    sksurv.metrics.concordance_index_censored, models/mcat/main.py:81): comparable pairs need an
    event at the earlier time, or equal times with the other subject censored; risk ties within
    tied_tol count one half.  Vectorised O(n^2) numpy."""
    event = np.asarray(event, dtype=bool)
    time = np.asarray(time, dtype=np.float64)
    risk = np.asarray(risk, dtype=np.float64)
    later = (time[None, :] > time[:, None]) | ((time[None, :] == time[:, None]) & ~event[None, :])
    comparable = later & event[:, None]
    np.fill_diagonal(comparable, False)
    den = comparable.sum()
    if den == 0:
        raise ValueError("no comparable pairs")
    diff = risk[:, None] - risk[None, :]
    ties = np.abs(diff) <= tied_tol
    num = ((diff > 0) & ~ties & comparable).sum() + 0.5 * (ties & comparable).sum()
    return float(num) / float(den)


def make_window(slides: Sequence[dict], device, bag_dtype=torch.float32):
    """List of slide dicts (synthetic.make_cohort layout) -> (BagBatch, omics per group (B,d_i), labels, censorship).
    bag_dtype: the window's storage -- torch.float32 (the reference's), torch.bfloat16 (the benchmarked mode) or torch.float16
    (the patch matrix alone in fp16, H_bag fp32: ops.patch_fc_f16)."""
    bags = BagBatch.from_list([s["wsi"].to(device=device, dtype=bag_dtype, non_blocking=True) for s in slides])
    n_groups = len(slides[0]["omics"])
    omics = [torch.stack([s["omics"][i] for s in slides]).to(device, non_blocking=True) for i in range(n_groups)]
    labels = torch.tensor([s["survival_class"] for s in slides], dtype=torch.int64).to(device, non_blocking=True)
    cens = torch.tensor([float(s["censorship"]) for s in slides]).to(device, non_blocking=True)
    return bags, omics, labels, cens


CE_REFUSAL = ("loss 'ce' cannot train these models: the reference computes nn.CrossEntropyLoss()(Y, label.unsqueeze(0)) "
              "with Y (1, C) and a (1, 1) target (models/mcat/main.py:46-47), which torch rejects on the first slide "
              "('0D or 1D target tensor expected') -- there is no behaviour to reproduce; use 'ces' or 'sct'")


def make_ge_window(slides: Sequence[dict], device, bag_dtype=torch.float32):
    """List of gene-expression slide dicts ({'wsi': (M, 1024), 'gene_expr_class': int}, the pairs
    dataset/ge_dataset.py yields) -> (BagBatch, labels (B,) int64).  bag_dtype: as make_window's (fp32, bf16 or fp16)."""
    bags = BagBatch.from_list([s["wsi"].to(device=device, dtype=bag_dtype, non_blocking=True) for s in slides])
    labels = torch.tensor([int(s["gene_expr_class"]) for s in slides], dtype=torch.int64).to(device, non_blocking=True)
    return bags, labels


def sample_window_rows(model, bags, sample_rows) -> BagBatch:
    """The window a training step runs on under `sample_rows` (None / 0: off): in training mode min(sample_rows, M_b) rows
    of every slide, drawn anew on every call without replacement (ops.RowSampler, eager form); in eval mode the whole
    window, so validation sees every patch.
    A SlideSet (separately stored slides) is gathered from where its slides lie (with `cycle`: sample_rows rows of every
    slide, short ones lapped); wherever the whole window is needed -- eval mode, no sample_rows -- it is materialized by one
    torch.cat, since every bag kernel reads a contiguous window."""
    if not sample_rows or not model.training:
        return bags.materialize() if isinstance(bags, SlideSet) else bags
    from . import ops
    return ops.RowSampler.for_window(bags, sample_rows, static=False).bind(bags)()


def train_ge_window(model, bags: BagBatch, labels, grad_acc_step: int, l1: float = 0.0, sample_rows: "int | None" = None):
    """Forward + backward of one window of the gene-expression model (models/ge_nacagat/main.py:24-52): the `ce` loss on Y
    in the head's launch, gradients ACCUMULATE into .grad with the reference's 1 / grad_acc_step per bag (main.py:51), no
    M x M map is allocated.  Returns the per-bag loss (B,) on the device -- no host sync.  l1: as in train_window (the
    REPORTED loss gains l1 * sum|W|, main.py:41-43; the penalty's gradient is folded by dp.FlatOptimizer).
    sample_rows: as in train_window; at least the model's row floor (17)."""
    if sample_rows and sample_rows < model.MIN_WINDOW_ROWS:
        raise ValueError(f"sample_rows {sample_rows}: the gene-expression model's window step needs at least "
                         f"{model.MIN_WINDOW_ROWS} rows per bag")
    bags = sample_window_rows(model, bags, sample_rows)
    w = _slide_weights(bags.n_slides, grad_acc_step, labels.device)
    _, att = model.forward_window(bags, need_maps=False, ce_targets=(labels, w))
    per_bag = att["loss"]
    per_bag.backward(w)
    return _with_penalty(model, per_bag.detach(), l1)


def train_window(model, bags: BagBatch, omics, labels, cens, grad_acc_step: int, loss: str = "ces", lambda_reg: float = 0.01,
                 alpha: float = 0.75, l1: float = 0.0, sample_rows: "int | None" = None):
    """Forward + backward of one window; gradients ACCUMULATE into .grad with the reference's
    1/grad_acc_step scaling per slide (models/mcat/main.py:69-70).  Returns (per-slide loss, risk) tensors
    on the device -- no host sync.  loss: 'ces' (models/loss.py:5-28, weight `alpha`), 'sct' (:62-85 on Y) or 'cesar'
    (:88-101: ces + lambda_reg * ||A_b||_2 of the slide's co-attention map, models/nacagat/main.py:49-50).
    l1 > 0 (training.lambda): every slide's REPORTED loss gains l1 * sum|W| over the weights the window runs with
    (models/mcat/main.py:51-54,61); the penalty's gradient is not taken here -- the flat optimiser folds it into its
    pass (dp.FlatOptimizer(l1_lambda=l1), step(l1_slides=...)).
    sample_rows = k (default off; beyond the reference): in training mode the step runs on k rows of every slide drawn
    anew per call without replacement (a slide shorter than k whole); in eval mode on the whole window."""
    from . import ops
    bags = sample_window_rows(model, bags, sample_rows)
    if loss == "cesar":
        hazards, survs, _, att = model.forward_window(bags, omics, inference=True)    # the map is an output here
        per_slide, risk = ops.ces_loss(hazards, survs, labels, cens, alpha)
        per_slide = per_slide + lambda_reg * ops.map_block_norm(att["coattn"])
    elif loss in ("ces", "sct"):
        # head, loss and the backward of both in one launch: the loss gradient is known before the forward
        w = _slide_weights(bags.n_slides, grad_acc_step, labels.device)
        _, _, _, att = model.forward_window(bags, omics, ces_targets=(labels, cens, w), fused_loss=loss, alpha=alpha)
        per_slide, risk = att["loss"], att["risk"]
        per_slide.backward(w)
        return _with_penalty(model, per_slide.detach(), l1), risk
    elif loss == "ce":
        raise ValueError(CE_REFUSAL)
    else:
        raise ValueError(f"loss '{loss}' is not built (ces | sct | cesar)")
    # d(sum(loss) / grad_acc_step) / d(loss_b) = 1 / grad_acc_step: hand it over as a cached constant instead of
    # building the sum / div graph (five tiny launches per window)
    per_slide.backward(_slide_weights(per_slide.numel(), grad_acc_step, per_slide.device))
    return _with_penalty(model, per_slide.detach(), l1), risk


def _with_penalty(model, per_slide, l1: float):
    return per_slide if not l1 else per_slide + l1 * weights_abs_sum(model)


def weights_abs_sum(model) -> torch.Tensor:
    """l1_reg(model) = sum over every parameter of sum |W| (models/utils.py:33-40) as a device scalar (1,), no host sync.
    Parameters re-pointed into a flat optimiser's buffer (dp.FlatOptimizer, whose padding stays zero) cost one
    deterministic reduction over that buffer; any other parameter one reduction of its own."""
    from . import ops
    bases, rest = {}, []
    for p in model.parameters():
        base = getattr(p, "_mpo_flat_param_base", None)
        if base is not None and p.untyped_storage().data_ptr() == base.untyped_storage().data_ptr():
            bases[id(base)] = base
        else:
            rest.append(p)
    parts = [ops.flat_abs_sum(b) for b in bases.values()] + [ops.flat_abs_sum(p.detach().float()) for p in rest]
    return parts[0] if len(parts) == 1 else torch.cat(parts).sum(0, keepdim=True)


# ------------------------------------------------------------------------------------ the reference's training: config
LOSSES = {"mcat": ("ces", "sct"), "nacagat": ("ces", "sct", "cesar"), "ge_nacagat": ("ce",)}
OPTIMISERS = ("adam", "adamax", "adadelta", "sgd")


@dataclass
class TrainOptions:
    """The reference's `training:` choices as this package runs them (models/mcat/main.py:272-318,
    models/nacagat/main.py:283-296, models/ge_nacagat/main.py:223-263).  train_kwargs() feeds train_window /
    GraphedWindowStep (for the gene-expression model, whose only loss is `ce`: train_ge_window(..., l1=o.l1));
    make_optimizer() and make_scheduler() build the flat optimiser (with the L1 fold) and the per-epoch schedule."""
    loss: str
    alpha: float
    lambda_reg: float             # cesar's attention-map weight (fixed 0.01 in the reference)
    grad_acc_step: int
    optimizer: str
    lr: float
    weight_decay: float
    l1: float                     # training.lambda; 0.0 = no penalty
    gamma: "float | None"         # ExponentialLR gamma, None = no schedule
    max_grad_norm: "float | None" = None      # not the reference's: clip the global gradient norm (FlatOptimizer)
    skip_nonfinite: bool = False              # not the reference's: drop a step whose gradient holds an inf or a NaN

    def train_kwargs(self) -> dict:
        return dict(loss=self.loss, alpha=self.alpha, lambda_reg=self.lambda_reg, l1=self.l1)

    def make_optimizer(self, bucket):
        from .dp import FlatOptimizer
        wd = 0.0 if self.optimizer == "sgd" else self.weight_decay          # main.py:288-289 passes lr only
        return FlatOptimizer(bucket, self.optimizer, lr=self.lr, weight_decay=wd, l1_lambda=self.l1,
                             max_grad_norm=self.max_grad_norm, skip_nonfinite=self.skip_nonfinite)

    def make_scheduler(self, opt):
        from .dp import FlatExponentialLR
        return None if self.gamma is None else FlatExponentialLR(opt, self.gamma)


def training_options(training: dict, model: str = "mcat") -> TrainOptions:
    """The reference's `training:` config dict -> TrainOptions, by the reference's own mapping: an unknown loss raises;
    'cesar' exists for NaCAGaT only and always runs with alpha 0.75, lambda_reg 0.01 (CrossEntropySurvivalAttnRegLoss());
    'ce' raises for the fusion models (CE_REFUSAL) and is the one loss of 'ge_nacagat' (models/ge_nacagat/main.py:223-227, where
    the call is well-formed); unknown optimiser names (e.g. 'rms') become 'adam'; 'sgd' gets no weight decay;
    lambda 0 / None means no penalty; any scheduler other than 'exp' means none.  Two keys the reference's YAML does not
    have are read when present: max_grad_norm and skip_nonfinite (FlatOptimizer's guard; both off when absent)."""
    if model not in LOSSES:
        raise ValueError(f"model '{model}' has no training loop here ({' | '.join(LOSSES)})")
    loss = training["loss"]
    if loss == "ce" and "ce" not in LOSSES[model]:
        raise ValueError(CE_REFUSAL)
    if loss not in LOSSES[model]:
        raise ValueError(f'Loss "{loss}" not implemented for {model} ({" | ".join(LOSSES[model])})')
    alpha, lambda_reg = (0.75, 0.01) if loss == "cesar" else (float(training.get("alpha", 0.75)), 0.01)
    name = training.get("optimizer")
    name = name if name in OPTIMISERS else "adam"
    lam = training.get("lambda")
    gamma = float(training["gamma"]) if training.get("scheduler") == "exp" else None
    max_norm = training.get("max_grad_norm")
    return TrainOptions(loss=loss, alpha=alpha, lambda_reg=lambda_reg, grad_acc_step=int(training["grad_acc_step"]),
                        optimizer=name, lr=float(training["lr"]), weight_decay=float(training.get("weight_decay") or 0.0),
                        l1=float(lam) if lam else 0.0, gamma=gamma, max_grad_norm=float(max_norm) if max_norm else None,
                        skip_nonfinite=bool(training.get("skip_nonfinite", False)))


_slide_weight_cache = {}


def _slide_weights(n: int, grad_acc_step: int, device) -> torch.Tensor:
    key = (n, grad_acc_step, str(device))
    w = _slide_weight_cache.get(key)
    if w is None:
        w = _slide_weight_cache[key] = torch.full((n,), 1.0 / grad_acc_step, device=device, dtype=torch.float32)
    return w


@contextmanager
def _device_feature_scale(bags, scale):
    """For the length of one forward (and backward) over `bags`, the window carries the feature scale of what it holds now,
    found on the device into `scale` (1,) (ops.feature_scale_device: three tiny launches, enqueued on entry) and read by the
    fp32 patch layer through a pointer (bags.data._mpo_feature_scale_dev).  scale None -- a window that never reaches the
    scaled kernel -- carries nothing."""
    if scale is None:
        yield
        return
    from . import ops
    bags.data._mpo_feature_scale_dev = ops.feature_scale_device(bags.data, out=scale)
    try:
        yield
    finally:
        del bags.data._mpo_feature_scale_dev


class GraphedWindowStep:
    """One window step (forward, `ces` loss, backward, gradients into the flat bucket, optionally the Adam
    update) captured ONCE into a HIP graph and replayed: ~500 launches per window cost one graph launch on
    the host instead of ~4 ms of Python / launch overhead.

    Static inputs: the window's tensors are resident and fixed (one captured graph per resident window).  An fp32 window's
    feature scale (ops.feature_scale) is baked into the graph as a kernel argument: a replay after an in-place write to
    that window raises instead of computing with the stale scale.  With device_feature_scale=True the body starts, behind
    the counter bump, with the range pass over the whole window (ops.feature_scale_device: three tiny launches) and the
    patch layer reads the scale through a pointer: a replay follows whatever the window holds -- rows that
    ingest.WindowFeeder or copy_ refilled in place -- and never raises.
    Frozen-at-capture values that must change per step live on the device: the dropout epoch (ops.set_rng_epoch,
    bumped inside the graph) and Adam's step count (dp.FlatAdam.t_dev).  With world_size > 1 leave the optimiser
    out (`opt=None`): replay, then all-reduce the bucket and step eagerly.

    The gene-expression model takes the window (bags, labels) of make_ge_window: the body is train_ge_window (its one
    loss, `ce`), the call returns the per-bag loss alone, and split_patch_grad is refused: that model's data-parallel
    step (opt=None, train_epoch_dp) reduces its whole bucket in one all-reduce.

    sample_rows = k lifts the one-window restriction: the captured body starts (right behind the counter bump, so that a
    replay's sample and masks share its epoch) with the gather of ops.RowSampler -- k rows of every slide into a buffer of
    static shape -- and everything behind it sees the same lengths, plan and grids whatever window the sampler reads.
    bind(window) then re-points the captured step at another window of the same slide count, width and dtype with at least
    k rows per slide; every replay draws a fresh sample (the device epoch).  Model in training mode.  bf16 windows, and
    with device_feature_scale=True fp32 windows: the captured body is counter bump, gather, range pass over the sample
    (the sampler's, `step.sampler.scale`), then the step -- the scale is that of the rows the step runs on, as the eager
    sampled path finds it on the host.  A window with a non-finite value runs unscaled (scale 1; its rows of H_bag come
    out non-finite, as ever).  An fp32 window that never reaches the scaled kernel (small / big models, patch_dim 512 /
    2048: the exact-fp32 GEMM) has no scale: the flag only lifts the refusal, `step.sampler.scale` is None.  A step binds
    windows of the dtype it was captured on.

    A window whose first element is an ops.SlideSet (ResidentCohort.window) captures the gather from separately stored
    slides instead: bind() then takes further SlideSet windows -- slide ids into a cohort that lives on the device, no copy
    and no H2D transfer per window -- and a SlideSet with `cycle` may hold slides shorter than k (lapped).  A step captured
    on one kind of window refuses the other: the two gathers read different descriptors.  train_epoch drives an epoch
    (the gene-expression model's (SlideSet, labels) windows of a GeResidentCohort: train_ge_epoch; one rank's share of a
    data-parallel epoch over a sharded cohort, either model: train_epoch_dp).
    """

    def __init__(self, model, bucket, window, grad_acc_step: int, opt=None, warmup: int = 2, pool=None,
                 split_patch_grad: bool = False, prime: bool = True, loss: str = "ces", alpha: float = 0.75,
                 lambda_reg: float = 0.01, l1: "float | None" = None, rng_base: "int | None" = None,
                 device_feature_scale: bool = False, sample_rows: "int | None" = None):
        """split_patch_grad (data-parallel steps, opt=None): the patch layer's weight gradient -- a 0.3 ms GEMM nobody
        downstream waits for -- is captured into a SECOND graph, `replay_tail()`.  The caller replays the main graph,
        starts the all-reduce of every other gradient (bucket.all_reduce_mean_async(lo=head)), replays the tail while
        that collective runs, then reduces the head slice: the exchange step hides behind compute.
        loss / alpha / lambda_reg / l1: train_window's (TrainOptions.train_kwargs()); l1 defaults to the optimiser's
        l1_lambda, whose gradient fold the captured opt.step() applies for this window's slides.
        rng_base: the value of the dropout generator's host counter the capture starts from (default: wherever the
        counter stands after the warm-up).  The capture bakes stream offsets taken from that counter into the graph, so
        a step re-captured in another process at the `rng_base` the original reports (self.rng_base, stored by
        checkpoint.save) draws the masks the original would have drawn, whatever ran before; on return the counter
        stands at the larger of its value on entry and the end of the captured streams.
        device_feature_scale (fp32 windows; nothing changes for bf16): the feature scale of the rows the step runs on is
        found inside the graph (ops.feature_scale_device) and read by the patch layer through a pointer, instead of being
        baked in as a number -- the class docstring says what that lifts."""
        from . import ops
        calls_on_entry = ops._rng_calls
        self.model, self.bucket, self.opt = model, bucket, opt
        self.device_feature_scale = bool(device_feature_scale)
        self.scale = None                                   # an unsampled fp32 step's own (1,) scale tensor
        self.l1 = float(getattr(opt, "l1_lambda", 0.0) if l1 is None else l1)
        self.train_kwargs = dict(loss=loss, alpha=alpha, lambda_reg=lambda_reg, l1=self.l1)
        self.window, self.acc = window, grad_acc_step
        self.split = bool(split_patch_grad)
        self.ge = len(window) == 2                          # (bags, labels): the gene-expression model's window
        if self.ge and self.split:
            raise ValueError("split_patch_grad is built for the fusion models' data-parallel steps, not for the "
                             "gene-expression model")
        if self.ge and loss not in ("ces", "ce"):           # ('ces' is this constructor's default)
            raise ValueError(f"loss '{loss}' is not built for the gene-expression model (ce)")
        if self.split and opt is not None:
            raise ValueError("split_patch_grad is for steps whose optimiser runs after an all-reduce (opt=None)")
        self.tail_graph = None
        self.sampler = None
        if sample_rows:
            # built (output batch, its cu and work plan: H2D copies) and bound before the warm-up
            reason = self._sampling_refusal(window[0], int(sample_rows))
            if reason:
                raise ValueError(f"GraphedWindowStep(sample_rows={sample_rows}): {reason}")
            bags = window[0]
            self.sampler = ops.RowSampler.for_window(bags, sample_rows, device_feature_scale=self._scaled(bags)).bind(bags)
        else:
            if isinstance(window[0], SlideSet):
                raise ValueError("GraphedWindowStep: a SlideSet window is read by the row sampler alone (sample_rows=k); every "
                                 "bag kernel reads a contiguous window -- materialize() it for an unsampled step")
            window[0].plan()                  # the work plan's H2D copy must not happen inside the capture
            if self._scaled(window[0]):
                self.scale = torch.ones(1, dtype=torch.float32, device=window[0].device)
        dev = bucket.flat.device
        if ops._rng_epoch_tensor is None:
            ops.set_rng_epoch(torch.zeros(1, dtype=torch.int64, device=dev))
        self.epoch = ops._rng_epoch_tensor
        # warm-up runs execute real steps (allocator, lazy initialisation): construction must not train the model, so the
        # optimiser state they touch is put back afterwards (the capture itself executes nothing)
        keep = None if opt is None else [t.clone() for t in opt.state_tensors()]
        keep_epoch = self.epoch.clone()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._body()
            if keep is not None:
                for t, k in zip(opt.state_tensors(), keep):
                    t.copy_(k)
            self.epoch.copy_(keep_epoch)
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        if rng_base is not None:
            ops._rng_calls = int(rng_base)
        self.rng_base = ops._rng_calls
        # (without device_feature_scale a sampled step refuses fp32 windows: only an unsampled step's BagBatch gets here with
        #  one, and the scale its graph bakes in is that of the window's contents now)
        baked = window[0].dtype == torch.float32 and not self.device_feature_scale
        self._fp32_window_version = window[0].data._version if baked else None
        # thread_local: other threads (RCCL's watchdog under torch.distributed) may issue HIP calls meanwhile
        with torch.cuda.graph(self.graph, pool=pool, capture_error_mode="thread_local"):
            out = self._body(flush=not self.split)
        self.loss, self.risk = (out, None) if self.ge else out
        if self.split:
            self._held = list(ops._deferred_patch)          # keep the queued operands alive between the two graphs
            self.tail_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.tail_graph, pool=self.graph.pool(), capture_error_mode="thread_local"):
                ops.flush_patch_weight_grads()
        if rng_base is not None:
            ops._rng_calls = max(calls_on_entry, ops._rng_calls)
        # The FIRST replay of a captured graph pays for its upload (2-4 ms against a 1.2 ms step, measured): pay it here,
        # with the state it touches put back, so that a caller's first step is a step like any other.
        if prime:
            grads = bucket.flat.clone()
            for _ in range(2):
                self.graph.replay()
                if self.tail_graph is not None:
                    self.tail_graph.replay()
            if keep is not None:
                for t, k in zip(opt.state_tensors(), keep):
                    t.copy_(k)
            self.epoch.copy_(keep_epoch)
            bucket.flat.copy_(grads)
            torch.cuda.current_stream(dev).synchronize()

    def _body(self, flush: bool = True):
        from . import ops
        ops.bump_step_counters(self.epoch, self.opt.t_dev if self.opt is not None else None)   # one launch for both
        bags = self.window[0] if self.sampler is None else self.sampler()
        # the range pass over the whole window as it is at this replay; the window carries the result for the length of the
        # forward and backward only (an eager step on the same tensor afterwards finds its scale on the host, as ever)
        with _device_feature_scale(bags, self.scale):
            self.bucket.begin()
            try:
                if self.ge:
                    out = train_ge_window(self.model, bags, self.window[1], self.acc, l1=self.l1)
                else:
                    _, omics, labels, cens = self.window
                    ops.defer_patch_weight_grad = self.split
                    out = train_window(self.model, bags, omics, labels, cens, self.acc, **self.train_kwargs)
            finally:
                ops.defer_patch_weight_grad = False
        self.bucket.finish()
        if self.split and flush:
            ops.flush_patch_weight_grads()
        if self.opt is not None:
            if getattr(self.opt, "l1_lambda", 0.0):
                self.opt.step(bump=False, l1_slides=bags.n_slides)
            else:
                self.opt.step(bump=False)
        return out

    def _scaled(self, bags) -> bool:
        """Whether the step finds a feature scale on the device: device_feature_scale, and an fp32 window that reaches
        mpo_patch_fc_f32 (Linear(1024, 256); the small / big models and patch_dim 512 / 2048 run the exact-fp32 GEMM, which
        has no scale -- for them the flag only lifts the refusals)."""
        from . import ops
        probe = torch.empty(0, bags.width, dtype=bags.dtype, device=bags.device)
        return self.device_feature_scale and ops.patch_fc_f32_supported(probe, self.model.H[0].weight)

    def _sampling_refusal(self, bags, k: int) -> "str | None":
        """Why a sampled step cannot run on `bags` (None: it can)."""
        if bags.dtype == torch.float32 and not self.device_feature_scale:
            return ("an fp32 window's feature scale is baked into the graph as a kernel argument; the sampled step is built "
                    "for bf16 windows (device_feature_scale=True finds the scale inside the graph instead)")
        if not self.model.training:
            return ("the model is in eval mode, where the whole window is passed through (validation sees every patch): "
                    "nothing a re-pointable graph could capture")
        if self.ge and k < self.model.MIN_WINDOW_ROWS:
            return f"the gene-expression model's window step needs at least {self.model.MIN_WINDOW_ROWS} rows per bag"
        return None

    def bind(self, window):
        """Re-point the captured step at `window` (same layout as the constructor's): before the next replay, ordered on
        the current stream (the one that replays), the sampler's descriptor is rewritten (one tiny launch) and omics,
        labels and censorship are copied into the tensors the graph reads.  No host synchronisation.  The window's rows
        must stay valid until the replays that read them have finished.  Raises ValueError with the reason when the
        window does not fit the capture: another slide count, a slide shorter than k (unless a SlideSet laps it), another
        width or dtype, fp32 for a step captured without device_feature_scale, a BagBatch for a step captured on a SlideSet
        or the reverse.  A refused bind changes nothing."""
        if self.sampler is None:
            raise ValueError("GraphedWindowStep.bind: the step was captured without sample_rows -- its graph reads one "
                             "resident window's rows directly")
        if len(window) != len(self.window):
            raise ValueError(f"GraphedWindowStep.bind: a window of {len(window)} parts for a step captured on {len(self.window)}")
        bags = window[0]
        if not isinstance(bags, (BagBatch, SlideSet)):
            raise ValueError(f"GraphedWindowStep.bind: a window starts with a BagBatch or a SlideSet, not a {type(bags).__name__}")
        reason = self._sampling_refusal(bags, self.sampler.k)
        if reason:
            raise ValueError(f"GraphedWindowStep.bind: {reason}")
        try:
            self.sampler.check(bags)
        except ValueError as e:
            raise ValueError(f"GraphedWindowStep.bind: {e}") from None
        static = self.window[1:]
        flat_new = list(window[1]) + list(window[2:]) if not self.ge else list(window[1:])
        flat_old = list(static[0]) + list(static[1:]) if not self.ge else list(static)
        if len(flat_new) != len(flat_old) or any(a.shape != b.shape or a.dtype != b.dtype for a, b in zip(flat_new, flat_old)):
            raise ValueError("GraphedWindowStep.bind: omics / labels / censorship differ in shape or dtype from the captured window's")
        self.sampler.bind(bags)
        for dst, src in zip(flat_old, flat_new):
            if dst is not src:
                dst.copy_(src, non_blocking=True)
        self.window = (bags, *static)

    def head_numel(self) -> int:
        """Number of leading bucket elements that only replay_tail() writes (the patch layer's weight)."""
        return self.bucket.head_numel(self.model.H[0].weight)

    def replay_tail(self):
        if self.tail_graph is not None:
            self.tail_graph.replay()

    def pool(self):
        return self.graph.pool()

    def __call__(self):
        if self._fp32_window_version is not None and self.window[0].data._version != self._fp32_window_version:
            raise RuntimeError("GraphedWindowStep: the fp32 window was written in place after capture; its feature scale "
                               "is baked into the graph -- capture a new step for the new contents (or capture with "
                               "device_feature_scale=True)")
        self.graph.replay()
        return self.loss if self.ge else (self.loss, self.risk)


# ------------------------------------------------------------------------------------ a cohort resident on the device
class _ResidentRows:
    """The row storage of a resident cohort (ResidentCohort, GeResidentCohort; the subclass's name heads the refusals), on
    `device`: `lengths`, `slabs` (at most slab_bytes each, a slide never split), `rows` (per slide a view of its slab), where
    a slide lies (`slab_index` / `row_offset`), the pointer / length table csrc/bag_sample.hip's slide gather is addressed
    through (`table_ptrs`, `table_lens`), and `cycle`.  A subclass adds its per-slide targets and window()'s selects."""

    def __init__(self, slides: Sequence[dict], device, bag_dtype, cycle: bool, slab_bytes: int):
        who = type(self).__name__
        self.device, self.cycle = torch.device(device), bool(cycle)
        if len(slides) == 0:
            raise ValueError(f"{who}: no slides")
        self.lengths = [int(s["wsi"].shape[0]) for s in slides]
        width = int(slides[0]["wsi"].shape[1])
        row_bytes = width * torch.empty(0, dtype=bag_dtype).element_size()
        if row_bytes % 16:
            raise ValueError(f"{who}: a row of {row_bytes} bytes is not a multiple of 16 bytes")
        if any(m < 1 for m in self.lengths) or any(int(s["wsi"].shape[1]) != width for s in slides):
            raise ValueError(f"{who}: every slide needs at least one patch row, and all the same width")
        self.slabs, self.rows, group = [], [], []
        # where a slide lies: its slab and its first row there (slides of one slab lie back to back in id order, so a run of
        # consecutive ids inside one slab is a contiguous row range: the evaluators' windows are views of it)
        self.slab_index, self.row_offset = [], []

        def flush():
            if group:
                slab = torch.cat([slides[i]["wsi"] for i in group]).to(device=self.device, dtype=bag_dtype, non_blocking=True)
                self.slabs.append(slab)
                self.rows.extend(slab.split([self.lengths[i] for i in group]))
                first = 0
                for i in group:
                    self.slab_index.append(len(self.slabs) - 1)
                    self.row_offset.append(first)
                    first += self.lengths[i]
                group.clear()
        filled = 0
        for i, m in enumerate(self.lengths):
            if group and filled + m * row_bytes > slab_bytes:
                flush()
                filled = 0
            group.append(i)
            filled += m * row_bytes
        flush()
        self.table_ptrs, self.table_lens = SlideSet.slide_table(self.rows)

    @property
    def n_slides(self):
        return len(self.lengths)

    def _slide_set(self, ids_dev, ids_host) -> SlideSet:
        """The SlideSet a window() starts with: the slides `ids_host` (checked against the cohort) = `ids_dev`."""
        ids_host = [int(i) for i in ids_host]
        for i in ids_host:
            if not 0 <= i < self.n_slides:
                raise ValueError(f"{type(self).__name__}.window: slide id {i} outside the cohort's {self.n_slides} slides")
        return SlideSet([self.rows[i] for i in ids_host], [self.lengths[i] for i in ids_host], self.table_ptrs, self.table_lens,
                        ids_dev, self.cycle)


class ResidentCohort(_ResidentRows):
    """A cohort that lives on the device once, for shuffled epochs of the sampled, captured step (bag_dtype bf16, fp16 -- bf16's
    bytes, fp32 H_bag behind the patch layer, no feature scale: captured like a bf16 cohort -- or fp32
    for a step captured with device_feature_scale=True): every slide's rows (in
    slabs of at most `slab_bytes`, a slide never split), the pointer / length table csrc/bag_sample.hip's slide gather is addressed
    through, omics per group (N, d_i), labels, censorship and survival_months (all (N,)).  A window is a list of slide ids:
    nothing is copied to form it and nothing crosses PCIe (1 000 slides of 15 000 x 1024 bf16 are 30 GB).

    slides: the dict layout make_window takes (synthetic.make_cohort).  cycle: the windows lap a slide shorter than the
    step's k in its permuted order instead of refusing it (ops.SlideSet).  Only the survival layout is built; a
    gene-expression cohort ((SlideSet, labels) windows) is not -- GeResidentCohort is that one, over the same storage."""

    def __init__(self, slides: Sequence[dict], device, bag_dtype=torch.bfloat16, cycle: bool = False, slab_bytes: int = 1 << 30):
        super().__init__(slides, device, bag_dtype, cycle, slab_bytes)
        n_groups = len(slides[0]["omics"])
        self.omics = [torch.stack([s["omics"][i] for s in slides]).to(self.device, non_blocking=True) for i in range(n_groups)]
        self.labels = torch.tensor([s["survival_class"] for s in slides], dtype=torch.int64).to(self.device, non_blocking=True)
        self.censorship = torch.tensor([float(s["censorship"]) for s in slides]).to(self.device, non_blocking=True)
        self.survival_months = torch.tensor([float(s["survival_months"]) for s in slides],
                                            dtype=torch.float64).to(self.device, non_blocking=True)

    def window(self, ids_dev, ids_host, out=None):
        """(SlideSet, omics, labels, cens) for the slides `ids_host` (host ints) = `ids_dev` (DEVICE int32, the same values; in
        an epoch a slice of the uploaded order): the tuple a step takes.  omics, labels and censorship are selected on the
        device, into `out` = (omics list, labels, cens) where given (a captured step's static tensors, step.window[1:]).
        No H2D copy and no host synchronisation.  ids_dev and ids_host are the caller's two copies of one list; nothing
        compares them (ops.SlideSet says what a mismatch does).  With `out`, the selects overwrite those tensors here, BEFORE
        any step.bind() has looked at the window: if that bind then refuses, the step is left with the new omics, labels and
        censorship beside the old rows -- validate first, as train_epoch does for the whole order, or leave `out` away and let
        bind() copy."""
        bags = self._slide_set(ids_dev, ids_host)
        o_omics, o_labels, o_cens = out if out is not None else ([None] * len(self.omics), None, None)
        omics = [torch.index_select(x, 0, ids_dev, out=o) for x, o in zip(self.omics, o_omics)]
        labels = torch.index_select(self.labels, 0, ids_dev, out=o_labels)
        cens = torch.index_select(self.censorship, 0, ids_dev, out=o_cens)
        return bags, omics, labels, cens


def _check_epoch_order(who: str, step, cohort, order) -> "List[int]":
    """An epoch's validation of a whole order (train_epoch, train_ge_epoch, train_epoch_dp: `who`) -- the cohort's layout
    against the step's capture, every id in range, every slide at least k rows unless the cohort laps -- before anything
    runs.  -> the order as host ints."""
    if (int(cohort.rows[0].shape[1]), cohort.rows[0].dtype) != (step.sampler.width, step.sampler.dtype):
        raise ValueError(f"{who}: the cohort's rows are {int(cohort.rows[0].shape[1])} x {cohort.rows[0].dtype}, the step was "
                         f"captured for {step.sampler.width} x {step.sampler.dtype}")
    order, k = [int(i) for i in order], step.sampler.k
    for i in order:
        if not 0 <= i < cohort.n_slides:
            raise ValueError(f"{who}: slide id {i} outside the cohort's {cohort.n_slides} slides")
        if not cohort.cycle and cohort.lengths[i] < k:
            raise ValueError(f"{who}: slide {i} has {cohort.lengths[i]} rows, fewer than k = {k}, and the cohort does not lap "
                             "short slides (cycle=False)")
    return order


def _run_epoch(step, cohort, order: "List[int]", n_windows: int, between=None):
    """The loop of every resident epoch, over a validated `order`: the first n_windows * n ids are uploaded once; per window
    of the step's n slides it enqueues the bind (one tiny launch), the selects into the step's static tensors, one replay,
    `between()` where given (a data-parallel epoch's exchange and optimiser step) and the device-to-device copies of loss and
    risk into epoch-long buffers.  No host synchronisation and no H2D copy of its own inside the loop.
    -> (loss, risk, ids_run, leftover); risk is None for a gene-expression step, leftover the host ids that did not run."""
    n = step.sampler.n_slides
    leftover = order[n_windows * n:]
    dev = cohort.device
    order_dev = torch.tensor(order[:n_windows * n], dtype=torch.int32).to(dev, non_blocking=True)
    loss = torch.empty(n_windows * n, dtype=torch.float32, device=dev)
    risk = None if step.ge else torch.empty(n_windows * n, dtype=torch.float32, device=dev)
    static = step.window[1:]
    for w in range(n_windows):
        lo, hi = w * n, (w + 1) * n
        step.bind(cohort.window(order_dev[lo:hi], order[lo:hi], out=static))
        out = step()
        if between is not None:
            between()
        if risk is None:
            loss[lo:hi].copy_(out.view(-1), non_blocking=True)
        else:
            loss[lo:hi].copy_(out[0].view(-1), non_blocking=True)
            risk[lo:hi].copy_(out[1].view(-1), non_blocking=True)
    return loss, risk, order_dev, leftover


def train_epoch(step: "GraphedWindowStep", cohort: ResidentCohort, order):
    """One shuffled epoch of the captured, sampled step over a resident cohort, bf16 or fp32 (an fp32 step is captured with
    device_feature_scale=True: every window's sample gets its own scale inside the graph).  `order`: host sequence of slide ids (the
    epoch's permutation), validated once -- range, and every slide at least k rows unless the cohort laps -- and uploaded
    once.  Per window of the step's slide count the loop enqueues: the bind (one tiny launch), the selects of omics, labels
    and censorship into the step's static tensors, one replay, two device-to-device copies of loss and risk into
    epoch-long buffers.  No host synchronisation and no H2D copy inside the loop.

    Returns (loss, risk, ids_run, leftover): loss and risk (n_run,) fp32 and ids_run (n_run,) int32 on the device, in the
    order the slides ran; `leftover` the host ids of the final partial window, which are NOT run (the graph has one
    shape).  Run them eagerly where they matter:
        bags, omics, labels, cens = cohort.window(torch.tensor(leftover, dtype=torch.int32, device=dev), leftover)
        train_window(model, bags.materialize(), omics, labels, cens, grad_acc_step, sample_rows=k)
    -- that eager path passes a slide shorter than k whole instead of lapping it.  The epoch's training C-index stays on the
    device as well:
        c_index, counts = concordance_index_device(cohort.censorship[ids_run], cohort.survival_months[ids_run], risk)
    (two more launches, no synchronisation; CohortEvaluator does the same for the validation set).  The host form,
    concordance_index_censored(1 - cens[ids_run], months[ids_run], risk) after one synchronise, gives the same number."""
    if step.sampler is None or step.sampler.source != "slides" or step.ge:
        raise ValueError("train_epoch: the step must be a fusion-model step captured with sample_rows on a ResidentCohort window")
    order = _check_epoch_order("train_epoch", step, cohort, order)
    return _run_epoch(step, cohort, order, len(order) // step.sampler.n_slides)


# ------------------------------------------------------------------------------------ validation and test on the device
def concordance_index_device(censorship, time, risk):
    """concordance_index_censored(1 - censorship, time, risk) computed on the device (csrc/concordance.hip): the same
    pair-by-pair definition with scikit-survival's default tied_tol 1e-8, counted in integers.  censorship, time, risk: (n,)
    tensors on one GPU (censorship and risk are read as fp32, time as fp64 -- ResidentCohort.survival_months' dtype;
    converted where they are not).  Returns (c_index (1,) fp64, counts (3,) int64 = concordant, tied, comparable) on the
    device; c_index is NaN where the host form raises "no comparable pairs".  Two launches, no n x n temporary, no host
    synchronisation; capturable.  Raises ValueError for what the host knows: a tensor that is not on the GPU, lengths that
    differ, n == 0."""
    from . import ops
    for name, t in (("censorship", censorship), ("time", time), ("risk", risk)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"concordance_index_device: {name} must be a tensor on the GPU "
                             "(concordance_index_censored is the host form)")
    if len({t.device for t in (censorship, time, risk)}) != 1:
        raise ValueError("concordance_index_device: censorship, time and risk lie on different devices")
    n = int(risk.numel())
    if n == 0 or int(censorship.numel()) != n or int(time.numel()) != n:
        raise ValueError(f"concordance_index_device: {int(censorship.numel())} censorship values, {int(time.numel())} times "
                         f"and {n} risks (equal and at least one)")
    return ops.concordance_index(censorship.detach().reshape(-1).to(torch.float32).contiguous(),
                                 time.detach().reshape(-1).to(torch.float64).contiguous(),
                                 risk.detach().reshape(-1).to(torch.float32).contiguous())


@dataclass
class StratResult:
    """A cohort cut into a low-risk (0) and a high-risk (1) group at a risk cut-off, as risk_stratification defines it, in
    numpy arrays: cutoff (1,) fp64; group (n,) int32 (-1: excluded, a NaN risk or time); at_risk, deaths (2, n) int32 and
    surv (2, n) fp64, both groups' counts and Kaplan-Meier estimates at every subject's time, in subject order; sizes (4,)
    int64 = low, high, excluded, distinct event times; logrank (5,) fp64 = O1, E1, V, chi2, p; time (n,) fp64, the times as
    they were read (an input, kept for curves())."""
    cutoff: np.ndarray
    group: np.ndarray
    at_risk: np.ndarray
    deaths: np.ndarray
    surv: np.ndarray
    sizes: np.ndarray
    logrank: np.ndarray
    time: np.ndarray

    def _statistic(self, k: int) -> float:
        if int(self.sizes[0]) == 0 or int(self.sizes[1]) == 0:
            raise ValueError("one risk group is empty")
        return float(self.logrank[k])

    def chi2_value(self) -> float:
        """The log-rank chi-square (one degree of freedom) as a Python float.  Raises ValueError("one risk group is empty")
        where that is why there is none; NaN where V == 0 (nobody has an event)."""
        return self._statistic(3)

    def logrank_p_value(self) -> float:
        """The log-rank p-value, erfc(sqrt(chi2 / 2)), as a Python float: raises and is NaN as chi2_value."""
        return self._statistic(4)

    def curves(self):
        """For plotting: per group g (0 low, 1 high) a dict of arrays over the sorted distinct times of the group's subjects:
        'time', 'surv' (S_g), 'at_risk' and 'deaths' (of the group at that time)."""
        out = []
        for g in (0, 1):
            members = np.flatnonzero(self.group == g)
            t, first = np.unique(self.time[members], return_index=True)
            pick = members[first]
            out.append({"time": t, "surv": self.surv[g][pick], "at_risk": self.at_risk[g][pick], "deaths": self.deaths[g][pick]})
        return out


def risk_stratification(censorship, time, risk, cutoff=None) -> StratResult:
    """The other half of a survival report beside Harrell's C: the cohort cut into a high- and a low-risk group at a risk
    cut-off, both groups' Kaplan-Meier curves and the log-rank test of their separation, on the host in numpy.
    censorship, time, risk: (n,) array-likes (censorship and risk are read as fp32, time as fp64 -- what ResidentCohort and
    EvalResult hold, after a copy to the host); cutoff: None or a number.  Returns a StratResult.  THE DEFINITION:
      event_i   = (1 - censorship_i) != 0, as in concordance_index_censored.
      excluded  a subject whose risk or time is NaN: group -1.  It is counted in no set below; its own at_risk and deaths
                are 0 and its surv is NaN.
      r_i       = (double)risk_i + 0.0: -0 and +0 are one value.
      cutoff    given, or the median of the m non-excluded r: (r_(lo) + r_(hi)) / 2.0 at the order statistics (m - 1) // 2
                and m // 2 -- numpy.median's arithmetic, the same bits; NaN when m = 0.  E.g. the training cohort's median
                for the validation cohort, which is the sound protocol.
      group_i   = 1 (high) if r_i > cutoff, else 0 (low): a risk equal to the cut-off is low.
      at_risk[g][i] = #{j in g : t_j >= t_i},  deaths[g][i] = #{j in g : t_j == t_i and event_j}, for every i not excluded.
      surv[g][i] = S_g(t_i): the product of (n_g(u) - d_g(u)) / n_g(u) over the group's distinct event times u <= t_i, each
                factor one fp64 division of two exact integers, multiplied in ascending time; 1 before the first event,
                exactly 0 from a factor of 0 on.
      log-rank  over the m_u distinct event times u of both groups together, n = n_0 + n_1 and d = d_0 + d_1 at u:
                O1 = sum d_1;  E1 = sum (d * n_1) / n;  V = sum (((d * q) * (1 - q)) * (n - d)) / (n - 1) with q = n_1 / n (a
                term of 0 where n == 1), both added in ascending time;  x = O1 - E1;  chi2 = (x * x) / V;  p = erfc(sqrt(chi2
                / 2)) (one degree of freedom).  chi2 and p are NaN where a group is empty or V == 0.
    By sorting, O(n log n).  The integers and the cut-off are exact; surv is within (2k + 1) 2^-53 of the exact product of its k
    factors and E1, V within (m_u + 8) 2^-53 of the exact sums (tests/stratify_cases.py counts the roundings)."""
    c = np.asarray(censorship, dtype=np.float32).reshape(-1)
    t = np.asarray(time, dtype=np.float64).reshape(-1)
    r = np.asarray(risk, dtype=np.float32).reshape(-1).astype(np.float64) + 0.0          # (-0 and +0: one value)
    n = r.size
    if n == 0 or c.size != n or t.size != n:
        raise ValueError(f"risk_stratification: {c.size} censorship values, {t.size} times and {n} risks (equal and at least one)")
    event = (np.float32(1.0) - c) != 0
    valid = ~(np.isnan(r) | np.isnan(t))
    if cutoff is None:
        cut = float(np.median(r[valid])) if valid.any() else float("nan")
    else:
        cut = float(np.asarray(cutoff, dtype=np.float64).reshape(-1)[0])
    with np.errstate(invalid="ignore"):
        group = np.where(valid, (r > cut).astype(np.int32), np.int32(-1)).astype(np.int32)
    at_risk, deaths = np.zeros((2, n), dtype=np.int32), np.zeros((2, n), dtype=np.int32)
    surv = np.full((2, n), np.nan, dtype=np.float64)
    pooled = np.unique(t[valid & event])                                  # the distinct event times of both groups
    n_at, d_at = [], []
    for g in (0, 1):
        times = np.sort(t[group == g])
        deaths_at = np.sort(t[(group == g) & event])
        count_at = lambda u: (times.size - np.searchsorted(times, u, "left"),
                              np.searchsorted(deaths_at, u, "right") - np.searchsorted(deaths_at, u, "left"))
        a, d = count_at(t[valid])
        at_risk[g, valid], deaths[g, valid] = a, d
        u = np.unique(deaths_at)
        a, d = count_at(u)
        s = np.concatenate([[1.0], np.cumprod((a - d).astype(np.float64) / a.astype(np.float64))])
        surv[g, valid] = s[np.searchsorted(u, t[valid], "right")]          # as many factors as event times <= t_i
        a, d = count_at(pooled)
        n_at.append(a.astype(np.float64))
        d_at.append(d.astype(np.float64))
    nn, dd, n1 = n_at[0] + n_at[1], d_at[0] + d_at[1], n_at[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        q = n1 / nn
        e_terms = (dd * n1) / nn
        v_terms = np.where(nn == 1.0, 0.0, (((dd * q) * (1.0 - q)) * (nn - dd)) / (nn - 1.0))
    o1, e1, v = float(d_at[1].sum()), 0.0, 0.0
    for e_term, v_term in zip(e_terms.tolist(), v_terms.tolist()):
        e1 += e_term
        v += v_term
    sizes = np.array([int((group == 0).sum()), int((group == 1).sum()), int((~valid).sum()), pooled.size], dtype=np.int64)
    chi2 = p = float("nan")
    if sizes[0] and sizes[1] and v != 0.0:
        x = o1 - e1
        chi2 = (x * x) / v
        p = math.erfc(math.sqrt(chi2 / 2.0))
    return StratResult(np.array([cut], dtype=np.float64), group, at_risk, deaths, surv, sizes,
                       np.array([o1, e1, v, chi2, p], dtype=np.float64), t)


def cut_eval_windows(ids, lengths, slab_index, max_window_rows: int = 1 << 19, max_window_slides: int = 32):
    """The windows CohortEvaluator runs for the slides `ids` of a cohort whose slides have `lengths` rows and lie in slabs
    `slab_index` (one entry per slide; slides of one slab back to back in id order -- ResidentCohort's storage).  A pure
    function of host lists.  The ids are sorted into storage order and cut into maximal runs of consecutive ids inside one
    slab -- each a contiguous row range, so a window over it is a view -- that hold at most max_window_slides slides and at
    most max_window_rows rows (a single longer slide is a window of its own).
    -> (windows, perm): windows, a list of id lists in the order they run; perm[k], the position of ids[k] in the
    concatenation of the windows (results in run order, indexed by perm, are in the caller's order).
    A duplicate or out-of-range id raises ValueError."""
    ids = [int(i) for i in ids]
    if not ids:
        raise ValueError("cut_eval_windows: no slide ids")
    if max_window_rows < 1 or max_window_slides < 1:
        raise ValueError(f"cut_eval_windows: max_window_rows {max_window_rows} / max_window_slides {max_window_slides} below 1")
    for i in ids:
        if not 0 <= i < len(lengths):
            raise ValueError(f"cut_eval_windows: slide id {i} outside the cohort's {len(lengths)} slides")
    if len(set(ids)) != len(ids):
        seen = set()
        dup = next(i for i in ids if i in seen or seen.add(i))
        raise ValueError(f"cut_eval_windows: slide id {dup} is listed twice (every slide is evaluated once)")
    windows, rows = [], 0
    for i in sorted(ids):
        run = windows[-1] if windows else None
        if (run is not None and run[-1] + 1 == i and slab_index[run[-1]] == slab_index[i] and len(run) < max_window_slides
                and rows + lengths[i] <= max_window_rows):
            run.append(i)
            rows += lengths[i]
        else:
            windows.append([i])
            rows = lengths[i]
    position = {i: k for k, i in enumerate(i for run in windows for i in run)}
    return windows, [position[i] for i in ids]


@dataclass
class EvalResult:
    """What one evaluation of a cohort leaves on the device, per slide in the caller's `ids` order: loss, risk (n,);
    hazards, survs, Y (n, C); and over all of them mean_loss (1,), c_index (1,) fp64 and counts (3,) int64 (concordant,
    tied, comparable pairs).  maps / map_stats: only where the evaluator ran with the co-attention maps (test()): per
    slide the (N, M_b) map and (n, 3) [min, max, mean] of it.  Nothing here has been read by the host."""
    loss: torch.Tensor
    risk: torch.Tensor
    hazards: torch.Tensor
    survs: torch.Tensor
    Y: torch.Tensor
    mean_loss: torch.Tensor
    c_index: torch.Tensor
    counts: torch.Tensor
    maps: "List[torch.Tensor] | None" = None
    map_stats: "torch.Tensor | None" = None

    def c_index_value(self) -> float:
        """The C-index as a Python float: the one method that reads the host (it waits for the evaluation).  Raises
        ValueError("no comparable pairs") where concordance_index_censored would."""
        if int(self.counts[2]) == 0:
            raise ValueError("no comparable pairs")
        return float(self.c_index)


def _model_kind(model) -> str:
    from .models import MultimodalCoAttentionTransformer, NarrowContextualAttentionGateTransformer
    if isinstance(model, MultimodalCoAttentionTransformer):
        return "mcat"
    if isinstance(model, NarrowContextualAttentionGateTransformer):
        return "nacagat"
    raise ValueError(f"CohortEvaluator: {type(model).__name__} is not a survival model (MCAT | NaCAGaT); the gene-expression "
                     "model's validation is a mean ce loss and ResidentCohort holds the survival layout only")


def check_eval_loss(kind: str, loss: str, capture: bool = False, need_maps: bool = False):
    """The evaluator's refusals that depend on names alone: `ce` (CE_REFUSAL), a loss LOSSES does not list for the model,
    and under capture whatever makes the co-attention map an output."""
    if loss == "ce" and "ce" not in LOSSES[kind]:
        raise ValueError(CE_REFUSAL)
    if loss not in LOSSES[kind]:
        raise ValueError(f'Loss "{loss}" not implemented for {kind} ({" | ".join(LOSSES[kind])})')
    if capture and (loss == "cesar" or need_maps):
        raise ValueError("CohortEvaluator(capture=True): " + ("loss 'cesar' reads" if loss == "cesar" else "need_maps returns") +
                         " the co-attention map, an output of the forward whose size follows the window: the captured "
                         "evaluator keeps no map -- run it eagerly (capture=False)")


class _EvalWindow:
    """One window of an evaluator: a BagBatch over a row range of a slab (a view) and the selects that go with it."""
    __slots__ = ("ids", "lo", "hi", "bags", "omics", "labels", "cens", "scale", "graph")


class _WindowEvaluator:
    """What CohortEvaluator and GeCohortEvaluator share: the slides `ids` of a resident cohort cut into windows that are views
    of its slabs (cut_eval_windows), run once per call -- eagerly, or one captured graph per window -- into run-order buffers,
    and one device permutation (`perm`; `perm_host` on the host) that puts results into the caller's order.
    A subclass refuses what it cannot evaluate, then calls this constructor, and supplies
      _set_up(ids_dev)     (ids_dev: `ids` as int64 on the device) its refusals that need valid ids; `_targets`, the cohort's
                           tensors the result is computed against, in `ids` order; `_buffers`, the run-order result tensors;
      _select(w, run_dev)  one window's selects (w.labels, ...);
      _body(w)             forward + loss of one window, _write()-n into the buffers -> the window's maps, or None;
      PER_SLIDE and _result(per_slide, targets): the result type's per-slide fields, in the buffers' order, and the result over
                           them and the targets -- of this evaluator's slides (__call__) or of all ranks' (validate_dp)."""

    def __init__(self, model, cohort, ids, max_window_rows: int, max_window_slides: int, capture: bool, pool):
        from . import ops
        self.model, self.cohort, self.capture = model, cohort, bool(capture)
        self.ids = [int(i) for i in ids]
        runs, self.perm_host = cut_eval_windows(self.ids, cohort.lengths, cohort.slab_index, max_window_rows, max_window_slides)
        dev = cohort.device
        self.perm = torch.tensor(self.perm_host, dtype=torch.int64).to(dev, non_blocking=True)
        self._set_up(torch.tensor(self.ids, dtype=torch.int64).to(dev, non_blocking=True))
        weight = model.H[0].weight
        if weight.device != cohort.labels.device:
            raise ValueError(f"{type(self).__name__}: the model lies on {weight.device}, the cohort on {dev}")
        self.windows, lo = [], 0
        for run in runs:
            w = _EvalWindow()
            w.ids, w.lo, w.hi = run, lo, lo + len(run)
            lo = w.hi
            first, lengths = cohort.row_offset[run[0]], [cohort.lengths[i] for i in run]
            # the run's rows as a view of their slab (BagBatch.from_lengths builds its cu)
            w.bags = BagBatch.from_lengths(cohort.slabs[cohort.slab_index[run[0]]][first:first + sum(lengths)], lengths)
            w.omics = w.cens = w.scale = w.graph = None
            self._select(w, torch.tensor(run, dtype=torch.int64).to(dev, non_blocking=True))
            if dev.type == "cuda":
                w.bags.plan()                   # (its H2D copy happens here, never inside a call or a capture)
                if ops.patch_fc_f32_supported(w.bags.data, weight):
                    w.scale = torch.ones(1, dtype=torch.float32, device=dev)
            self.windows.append(w)
        self.pool = pool
        if self.capture:
            self._capture(pool)

    def _capture(self, pool):
        dev = self.cohort.device
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    for w in self.windows:          # allocator, lazy initialisation, every window's own shapes
                        self._body(w)
                torch.cuda.current_stream(dev).wait_stream(side)
                for w in self.windows:
                    w.graph = torch.cuda.CUDAGraph()
                    # thread_local: other threads (RCCL's watchdog under torch.distributed) may issue HIP calls meanwhile
                    with torch.cuda.graph(w.graph, pool=pool, capture_error_mode="thread_local"):
                        self._body(w)
                    pool = w.graph.pool() if pool is None else pool
            self.pool = pool
        finally:
            self.model.train(was_training)

    def _run_windows(self):
        """Every window once, in run order: one replay each when captured (-> None), otherwise _body in eval mode under
        torch.no_grad(), the mode it found put back (-> what every window's _body returned)."""
        if self.capture:
            for w in self.windows:
                w.graph.replay()
            return None
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                return [self._body(w) for w in self.windows]
        finally:
            self.model.train(was_training)

    def _write(self, w, *rows):
        """One window's results into its rows of the run-order buffers (`rows` in the order of PER_SLIDE)."""
        for dst, src in zip(self._buffers, rows):
            dst[w.lo:w.hi].copy_(src, non_blocking=True)

    def _in_ids_order(self, per_window):
        """Per-slide maps as the windows returned them (a list per window) -> one list in the caller's `ids` order."""
        per_run = [m for window_maps in per_window for m in window_maps]
        return [per_run[k] for k in self.perm_host]


class CohortEvaluator(_WindowEvaluator):
    """A validation epoch over slides of a ResidentCohort with nothing copied and nothing read by the host: the reference's
    validate() (models/mcat/main.py:106-155) -- eval mode, no gradients, per-slide loss and risk, Harrell's C over the set
    -- without its per-slide .item().

    ids: host sequence of slide ids, validated and uploaded once, here; a duplicate is an error.  They are sorted into
    storage order and cut into runs of slides that lie back to back in one slab (cut_eval_windows, capped by
    max_window_rows / max_window_slides): each run's window is a BagBatch over a row slice of the slab -- a view; no
    materialize(), no torch.cat, no H2D copy of rows.  Its cu, work plan and omics / labels / censorship selects are
    built once.  Ids that are not adjacent form windows of one slide.  Results come back in the caller's `ids` order, by
    one device permutation.

    A call runs, per window, the model's forward_window in eval mode under torch.no_grad() (the mode it found is put
    back) and the forward-only loss launch: loss 'ces' (ops.ces_loss, weight alpha), 'sct' (ops.sct_loss on Y, risk =
    -survs.sum(1)), 'cesar' (NaCAGaT: ces + lambda_reg * ||A_b||_2, which needs the map: forward_window(inference=True));
    l1 > 0 adds l1 * sum|W| to every reported loss, as train_window and the reference's validate() do.  'ce' raises
    CE_REFUSAL; a loss LOSSES does not list for the model raises.  An fp32 cohort's windows that reach the scaled patch
    kernel find their feature scale on the device (ops.feature_scale_device), carried for the length of the forward as
    GraphedWindowStep does.  Then one permutation per result, the mean loss, and concordance_index_device over
    cohort.censorship[ids], cohort.survival_months[ids] and the risks.  Everything is enqueued on the current stream;
    the call returns an EvalResult without synchronising.

    capture=True: each window's forward + loss is captured once into a HIP graph, here (eager warm-up on a side stream,
    plans built before, capture_error_mode thread_local -- GraphedWindowStep's recipe); the graphs share one memory pool
    (`pool`, or the first graph's) and replay in order on the calling stream.  Every later call is one replay per window,
    the permutations and the C-index launches: no Python forward, ~no host launch work.  The set is the same every epoch
    and eval mode draws no masks, so nothing is frozen that must change; parameters are read where they live, so an
    evaluator captured once follows a model that FlatOptimizer / FlatAdam update in place.  A parameter REPLACED by another
    tensor is not followed: build the flat optimiser, which re-points the parameters into its buffer, before this.  The
    slides' rows are read in place too: whatever the cohort holds at the replay.  'cesar' and need_maps are refused under
    capture: the map is an output.  Measured (NOTES.md, "Validation epoch on the device": 256 slides x 15 000 x 1024
    bf16, MCAT, 8 windows): 3.80 ms per epoch against the eager evaluator's 4.01 -- the device runs the same forward --
    with 0.69 ms instead of 3.87 ms of host launch work, which is what the capture is for.

    need_maps (eager only; test() sets it): forward_window(inference=True); the result carries every slide's map and
    ops.map_block_stats of it."""

    PER_SLIDE = ("loss", "risk", "hazards", "survs", "Y")

    def __init__(self, model, cohort: ResidentCohort, ids, loss: str = "ces", alpha: float = 0.75, lambda_reg: float = 0.01,
                 l1: float = 0.0, max_window_rows: int = 1 << 19, max_window_slides: int = 32, capture: bool = False,
                 pool=None, need_maps: bool = False):
        self.kind = _model_kind(model)
        check_eval_loss(self.kind, loss, bool(capture), bool(need_maps))
        self.loss_name, self.alpha, self.lambda_reg, self.l1 = loss, float(alpha), float(lambda_reg), float(l1)
        self.need_maps = bool(need_maps) or loss == "cesar"
        self.return_maps = bool(need_maps)
        super().__init__(model, cohort, ids, max_window_rows, max_window_slides, capture, pool)

    def _set_up(self, ids_dev):
        cohort, dev, n = self.cohort, self.cohort.device, len(self.ids)
        self.censorship = cohort.censorship.index_select(0, ids_dev)
        self.survival_months = cohort.survival_months.index_select(0, ids_dev)
        self._targets = (self.censorship, self.survival_months)
        n_classes = int(self.model.classifier.out_features)
        self._buffers = ([torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2)] +
                         [torch.empty(n, n_classes, dtype=torch.float32, device=dev) for _ in range(3)])

    def _select(self, w, run_dev):
        w.omics = [x.index_select(0, run_dev) for x in self.cohort.omics]
        w.labels = self.cohort.labels.index_select(0, run_dev)
        w.cens = self.cohort.censorship.index_select(0, run_dev)

    def _body(self, w):
        """forward + loss of one window into the run-order buffers -> the window's maps (need_maps) or None."""
        from . import ops
        with _device_feature_scale(w.bags, w.scale):
            hazards, survs, y, att = self.model.forward_window(w.bags, w.omics, inference=self.need_maps)
        if self.loss_name == "sct":
            per_slide, risk = ops.sct_loss(y, w.labels, w.cens), -survs.sum(1)
        else:
            per_slide, risk = ops.ces_loss(hazards, survs, w.labels, w.cens, self.alpha)
            if self.loss_name == "cesar":
                per_slide = per_slide + self.lambda_reg * ops.map_block_norm(att["coattn"])
        per_slide = _with_penalty(self.model, per_slide, self.l1)
        self._write(w, per_slide.view(-1), risk.view(-1), hazards, survs, y)
        return att["coattn"] if self.need_maps else None

    def _result(self, per_slide, targets) -> EvalResult:
        loss, risk, hazards, survs, y = per_slide
        c_index, counts = concordance_index_device(*targets, risk)
        return EvalResult(loss, risk, hazards, survs, y, loss.mean(0, keepdim=True), c_index, counts)

    def __call__(self) -> EvalResult:
        from . import ops
        maps = self._run_windows()
        out = self._result([t.index_select(0, self.perm) for t in self._buffers], self._targets)
        if self.return_maps:
            out.maps = self._in_ids_order(maps)
            out.map_stats = torch.cat([ops.map_block_stats(m) for m in maps]).index_select(0, self.perm)
        return out


def _one_shot(evaluator, who: str, model, cohort, ids, options):
    """validate() / validate_ge(): an eager evaluator of class `evaluator`, built and called once."""
    if options.get("capture"):
        raise ValueError(f"{who}: a one-shot evaluation has nothing to replay; build a {evaluator.__name__}(capture=True) and "
                         "call it every epoch")
    return evaluator(model, cohort, ids, **options)()


def _save_maps(slides, key: str, save_dir, name: str):
    """test() / test_ge() with save_dir: every slide's slides[.][key] to save_dir/{name}_{id}.pt as a CPU tensor (the copy
    synchronises), the path into the slide's 'file'."""
    import os
    os.makedirs(save_dir, exist_ok=True)
    for slide in slides:
        slide["file"] = os.path.join(save_dir, f"{name}_{slide['id']}.pt")
        torch.save(slide[key].cpu(), slide["file"])


def validate(model, cohort: ResidentCohort, ids, **options) -> EvalResult:
    """The reference's validate() (models/mcat/main.py:106-155) over the slides `ids` of a resident cohort: a one-shot eager
    CohortEvaluator(model, cohort, ids, **options) and its call.  No host synchronisation; result.c_index_value() reads
    the C-index.  An epoch loop that validates the same set every epoch keeps one CohortEvaluator instead (its windows,
    and with capture=True its graphs, are built once)."""
    return _one_shot(CohortEvaluator, "validate", model, cohort, ids, options)


def test(model, cohort: ResidentCohort, ids, save_dir=None, name: str = "ATTN"):
    """The reference's test() (models/nacagat/main.py:169-194) over the slides `ids` of a resident cohort, always eager with
    forward_window(inference=True).  Returns one dict per slide, in `ids` order: 'id', 'hazards', 'survs', 'Y' ((C,)),
    'risk' (scalar tensor), 'attn_stats' ((3,) [min, max, mean] of the slide's co-attention map, ops.map_block_stats)
    and 'coattn' (the (N, M_b) map), all on the device.  Without save_dir nothing is read by the host.  With save_dir
    every slide's map is written with torch.save to save_dir/{name}_{id}.pt (a CPU tensor) and the file's path is the
    dict's 'file': THIS IS THE ONE PLACE THAT SYNCHRONISES -- every map is copied to the host."""
    ev = CohortEvaluator(model, cohort, ids, need_maps=True)
    r = ev()
    out = []
    for k, slide_id in enumerate(ev.ids):
        out.append({"id": slide_id, "hazards": r.hazards[k], "survs": r.survs[k], "Y": r.Y[k], "risk": r.risk[k],
                    "attn_stats": r.map_stats[k], "coattn": r.maps[k]})
    if save_dir is not None:
        _save_maps(out, "coattn", save_dir, name)
    return out


test.__test__ = False           # (a public name that starts with "test": not a pytest case where a test module imports it)


# ------------------------------------------------------------------------------------ the gene-expression model's epochs
def classification_metrics(y, label, loss=None):
    """The host form of csrc/class_metrics.hip, and its definition: y (n, C) class scores, label (n,) integers, loss (n,) or
    None, tensors anywhere (copied to the host) -> (pred (n,) int64, confusion (C, C) int64, counts (4,) int64, summary
    (3,) fp64), CPU tensors.
      pred_b = torch.argmax(y[b]): the first index of a NaN if the row holds one, otherwise the first index of the maximum;
      a label is valid when 0 <= label_b < C;  confusion[label_b][pred_b] += 1 over the valid rows;
      counts = [valid, correct, invalid labels, rows with a NaN];
      summary[0] = correct / valid (NaN when valid == 0);  summary[1] = the mean of confusion[c][c] / support_c over the classes
      with support_c > 0, added in class order (NaN when there is none);  summary[2] = sum(loss) / n in fp64 over all n rows
      (NaN when loss is None; a NaN loss propagates)."""
    y = torch.as_tensor(y).detach().to("cpu", torch.float32)
    label = torch.as_tensor(label).detach().to("cpu", torch.int64).reshape(-1)
    if y.dim() != 2 or int(y.shape[0]) != int(label.numel()) or y.shape[0] == 0:
        raise ValueError(f"classification_metrics: y {tuple(y.shape)} for {int(label.numel())} labels ((n, C) and n, n at least 1)")
    n, c = int(y.shape[0]), int(y.shape[1])
    pred = torch.argmax(y, dim=1)
    valid = (label >= 0) & (label < c)
    cells = label[valid] * c + pred[valid]
    confusion = torch.bincount(cells, minlength=c * c).view(c, c).to(torch.int64)
    n_valid, correct = int(valid.sum()), int(confusion.diagonal().sum())
    counts = torch.tensor([n_valid, correct, n - n_valid, int(torch.isnan(y).any(dim=1).sum())], dtype=torch.int64)
    nan = float("nan")
    recalls = [int(confusion[k, k]) / int(confusion[k].sum()) for k in range(c) if int(confusion[k].sum()) > 0]
    recall_sum = 0.0
    for r in recalls:
        recall_sum += r
    mean_loss = nan
    if loss is not None:
        loss = torch.as_tensor(loss).detach().to("cpu", torch.float64).reshape(-1)
        if int(loss.numel()) != n:
            raise ValueError(f"classification_metrics: {int(loss.numel())} losses for {n} rows")
        mean_loss = float(loss.sum()) / n
    summary = torch.tensor([correct / n_valid if n_valid else nan, recall_sum / len(recalls) if recalls else nan, mean_loss],
                           dtype=torch.float64)
    return pred, confusion, counts, summary


def classification_metrics_device(y, label, loss=None, want_pred: bool = True):
    """classification_metrics(y, label, loss) computed on the device (csrc/class_metrics.hip): y (n, C) and loss (n,) are read
    as fp32, label as int64 (converted where they are not).  Returns (pred (n,) int64 -- None with want_pred=False --,
    confusion (C, C) int64, counts (4,) int64 = valid, correct, invalid labels, rows with a NaN, summary (3,) fp64 =
    accuracy, balanced accuracy, mean loss) on the device.  Two launches, no host synchronisation; capturable.  Raises
    ValueError for what the host knows: a tensor that is not on the GPU, different devices, lengths that differ, n == 0, C
    outside 2..8."""
    from . import ops
    given = [("y", y), ("label", label)] + ([("loss", loss)] if loss is not None else [])
    for name, t in given:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"classification_metrics_device: {name} must be a tensor on the GPU "
                             "(classification_metrics is the host form)")
    if len({t.device for _, t in given}) != 1:
        raise ValueError("classification_metrics_device: y, label and loss lie on different devices")
    if y.dim() != 2:
        raise ValueError(f"classification_metrics_device: y is (n, C), got {tuple(y.shape)}")
    n, c = int(y.shape[0]), int(y.shape[1])
    if n == 0 or int(label.numel()) != n or (loss is not None and int(loss.numel()) != n):
        raise ValueError(f"classification_metrics_device: {n} rows of y, {int(label.numel())} labels"
                         + (f" and {int(loss.numel())} losses" if loss is not None else "") + " (equal and at least one)")
    if not 2 <= c <= 8:
        raise ValueError(f"classification_metrics_device: {c} classes outside 2..8 (the head's range)")
    return ops.class_metrics(y.detach().to(torch.float32).contiguous(), label.detach().reshape(-1).to(torch.int64).contiguous(),
                             None if loss is None else loss.detach().reshape(-1).to(torch.float32).contiguous(), want_pred)


class GeResidentCohort(_ResidentRows):
    """ResidentCohort for the gene-expression model: every slide's rows on the device once, in the same storage -- slabs of at
    most `slab_bytes`, a slide never split; `rows`, `lengths`, `slab_index`, `row_offset`, the pointer / length table
    (`table_ptrs`, `table_lens`), `cycle`, `n_slides` -- and `labels` (N,) int64 on the device.
    slides: the dict layout make_ge_window takes ({'wsi', 'gene_expr_class'}: synthetic.make_ge_cohort).  bag_dtype: bf16, fp16
    (captured like bf16: no feature scale) or fp32 (a step captured with device_feature_scale=True)."""

    def __init__(self, slides: Sequence[dict], device, bag_dtype=torch.bfloat16, cycle: bool = False, slab_bytes: int = 1 << 30):
        super().__init__(slides, device, bag_dtype, cycle, slab_bytes)
        self.labels = torch.tensor([int(s["gene_expr_class"]) for s in slides], dtype=torch.int64).to(self.device, non_blocking=True)

    def window(self, ids_dev, ids_host, out=None):
        """(SlideSet, labels) for the slides `ids_host` (host ints) = `ids_dev` (DEVICE int32, the same values): the tuple a
        gene-expression step takes.  The labels are selected on the device, into `out` = (labels,) where given (a captured
        step's static tensor, step.window[1:]).  No H2D copy and no host synchronisation; what ResidentCohort.window says
        about the two copies of the ids and about `out` holds here."""
        bags = self._slide_set(ids_dev, ids_host)
        return bags, torch.index_select(self.labels, 0, ids_dev, out=None if out is None else out[0])


def train_ge_epoch(step: "GraphedWindowStep", cohort: GeResidentCohort, order):
    """train_epoch for the gene-expression model: one shuffled epoch of a step captured on a (SlideSet, labels) window of a
    GeResidentCohort with sample_rows=k, bf16 or fp32 (an fp32 step is captured with device_feature_scale=True).  `order`:
    host sequence of slide ids, validated once -- range, and every slide at least k rows unless the cohort laps -- and
    uploaded once.  Per window of the step's slide count the loop enqueues the bind (one tiny launch), the label select
    into the step's static tensor, one replay and one device-to-device copy of the per-bag loss.  No host synchronisation
    and no H2D copy inside the loop.

    Returns (loss, ids_run, leftover): loss (n_run,) fp32 and ids_run (n_run,) int32 on the device, in the order the slides
    ran; `leftover` the host ids of the final partial window, which are NOT run (the graph has one shape) -- run them
    eagerly where they matter:
        bags, labels = cohort.window(torch.tensor(leftover, dtype=torch.int32, device=dev), leftover)
        train_ge_window(model, bags.materialize(), labels, grad_acc_step, sample_rows=k)"""
    if not step.ge or step.sampler is None or step.sampler.source != "slides":
        raise ValueError("train_ge_epoch: the step must be a gene-expression step captured with sample_rows on a "
                         "GeResidentCohort window")
    if not isinstance(cohort, GeResidentCohort):
        raise ValueError(f"train_ge_epoch: a GeResidentCohort holds the gene-expression layout, not a {type(cohort).__name__}")
    order = _check_epoch_order("train_ge_epoch", step, cohort, order)
    loss, _, ids_run, leftover = _run_epoch(step, cohort, order, len(order) // step.sampler.n_slides)
    return loss, ids_run, leftover


@dataclass
class GeEvalResult:
    """What one evaluation of a gene-expression cohort leaves on the device, per slide in the caller's `ids` order: loss (n,),
    Y (n, C), pred (n,) int64; and over all of them confusion (C, C) and counts (4,) int64 (valid, correct, invalid labels,
    rows with a NaN), mean_loss, accuracy, balanced_accuracy (1,) fp64.  paths / path_stats: only where the evaluator ran
    with need_paths (test_ge()): per slide the (1, M_b) pooling attention and (n, 3) [min, max, mean] of it.  Nothing here has
    been read by the host."""
    loss: torch.Tensor
    Y: torch.Tensor
    pred: torch.Tensor
    confusion: torch.Tensor
    counts: torch.Tensor
    mean_loss: torch.Tensor
    accuracy: torch.Tensor
    balanced_accuracy: torch.Tensor
    paths: "List[torch.Tensor] | None" = None
    path_stats: "torch.Tensor | None" = None

    def accuracy_value(self) -> float:
        """The accuracy as a Python float: the one method that reads the host (it waits for the evaluation).  NaN where no
        label was valid."""
        return float(self.accuracy)


class GeCohortEvaluator(_WindowEvaluator):
    """CohortEvaluator for the gene-expression model: the reference's validate() (models/ge_nacagat/main.py:85-119) -- eval
    mode, no gradients, per-slide `ce` loss and Y, accuracy over the set -- over slides of a GeResidentCohort with nothing
    copied and nothing read by the host.

    ids: host sequence of slide ids, validated and uploaded once, here; a duplicate is an error, and so is a slide shorter
    than the model's window floor (MIN_WINDOW_ROWS).  cut_eval_windows cuts them into runs of slides that lie back to back in
    one slab; each run's window is a BagBatch over a row slice of the slab -- a view -- whose cu, work plan and label select
    are built once.  Results come back in the caller's `ids` order, by one device permutation.

    A call runs, per window, forward_window(bags, need_maps=False) in eval mode under torch.no_grad() (the mode it found is
    put back) with the `ce` loss riding in the head's launch (ops.ge_head_loss, forward only): no M x M map is ever
    allocated.  l1 > 0 adds l1 * sum|W| to every reported loss.  An fp32 cohort's windows that reach the scaled patch kernel
    find their feature scale on the device (ops.feature_scale_device).  Then one classification_metrics_device over the set.
    Everything is enqueued on the current stream; the call returns a GeEvalResult without synchronising.

    capture=True: CohortEvaluator's recipe -- one graph per window, a shared pool, capture_error_mode thread_local; parameters
    and rows are read in place, so the evaluator follows FlatOptimizer updates (build the optimiser first).  need_paths is
    refused under capture: the map is an output.
    need_paths (eager only; test_ge() sets it): the result carries every slide's (1, M_b) pooling attention and
    ops.map_block_stats of it (n_q = 1)."""

    PER_SLIDE = ("loss", "Y")

    def __init__(self, model, cohort: GeResidentCohort, ids, l1: float = 0.0, max_window_rows: int = 1 << 19,
                 max_window_slides: int = 32, capture: bool = False, pool=None, need_paths: bool = False):
        from .models import GeneExprNarrowContextualAttentionGateTransformer
        if not isinstance(model, GeneExprNarrowContextualAttentionGateTransformer):
            raise ValueError(f"GeCohortEvaluator: {type(model).__name__} is not the gene-expression model; a survival model's "
                             "validation is CohortEvaluator's")
        if not isinstance(cohort, GeResidentCohort):
            raise ValueError(f"GeCohortEvaluator: a GeResidentCohort holds the gene-expression layout, not a {type(cohort).__name__}")
        if capture and need_paths:
            raise ValueError("GeCohortEvaluator(capture=True): need_paths returns the pooling attention map, an output of the "
                             "forward whose size follows the window: the captured evaluator keeps no map -- run it eagerly "
                             "(capture=False)")
        self.l1, self.need_paths = float(l1), bool(need_paths)
        super().__init__(model, cohort, ids, max_window_rows, max_window_slides, capture, pool)

    def _set_up(self, ids_dev):
        cohort, model, dev, n = self.cohort, self.model, self.cohort.device, len(self.ids)
        for i in self.ids:
            if cohort.lengths[i] < model.MIN_WINDOW_ROWS:
                raise ValueError(f"GeCohortEvaluator: slide {i} has {cohort.lengths[i]} rows, fewer than the {model.MIN_WINDOW_ROWS} "
                                 "the gene-expression model's window forward needs (shorter bags go through forward())")
        self.labels = cohort.labels.index_select(0, ids_dev)
        self._targets = (self.labels,)
        self._buffers = [torch.empty(n, dtype=torch.float32, device=dev),
                         torch.empty(n, int(model.classifier.out_features), dtype=torch.float32, device=dev)]

    def _select(self, w, run_dev):
        w.labels = self.cohort.labels.index_select(0, run_dev)

    def _body(self, w):
        """forward + loss of one window into the run-order buffers -> the window's pooling attentions (a list of (1, M_b))."""
        with _device_feature_scale(w.bags, w.scale):
            targets = (w.labels, _slide_weights(w.bags.n_slides, 1, w.labels.device))
            y, att = self.model.forward_window(w.bags, need_maps=False, ce_targets=targets)
        self._write(w, _with_penalty(self.model, att["loss"], self.l1).view(-1), y)
        return att["path"]

    def _result(self, per_slide, targets) -> GeEvalResult:
        loss, y = per_slide
        pred, confusion, counts, summary = classification_metrics_device(y, targets[0], loss)
        return GeEvalResult(loss, y, pred, confusion, counts, summary[2:3], summary[0:1], summary[1:2])

    def __call__(self) -> GeEvalResult:
        from . import ops
        paths = self._run_windows()
        out = self._result([t.index_select(0, self.perm) for t in self._buffers], self._targets)
        if self.need_paths:
            out.paths = self._in_ids_order(paths)
            stats = [ops.map_block_stats(w.bags.split_map(torch.cat([p.reshape(-1) for p in window_paths]), 1))
                     for w, window_paths in zip(self.windows, paths)]
            out.path_stats = torch.cat(stats).index_select(0, self.perm)
        return out


def validate_ge(model, cohort: GeResidentCohort, ids, **options) -> GeEvalResult:
    """The reference's validate() (models/ge_nacagat/main.py:85-119) over the slides `ids` of a resident gene-expression
    cohort: a one-shot eager GeCohortEvaluator(model, cohort, ids, **options) and its call.  No host synchronisation;
    result.accuracy_value() reads the accuracy.  An epoch loop that validates the same set every epoch keeps one
    GeCohortEvaluator instead."""
    return _one_shot(GeCohortEvaluator, "validate_ge", model, cohort, ids, options)


def test_ge(model, cohort: GeResidentCohort, ids, save_dir=None, name: str = "ATTN"):
    """The reference's test() (models/ge_nacagat/main.py:122-142) over the slides `ids` of a resident gene-expression cohort,
    always eager.  Returns one dict per slide, in `ids` order: 'id', 'Y' ((C,)), 'pred' and 'label' (scalar tensors),
    'attn_stats' ((3,) [min, max, mean] of the slide's pooling attention, ops.map_block_stats) and 'path' (the (1, M_b)
    pooling attention), all on the device.  Without save_dir nothing is read by the host.  With save_dir every slide's path
    is written with torch.save to save_dir/{name}_{id}.pt (a CPU tensor) and the file's path is the dict's 'file': THIS IS
    THE ONE PLACE THAT SYNCHRONISES."""
    ev = GeCohortEvaluator(model, cohort, ids, need_paths=True)
    r = ev()
    out = []
    for k, slide_id in enumerate(ev.ids):
        out.append({"id": slide_id, "Y": r.Y[k], "pred": r.pred[k], "label": ev.labels[k], "attn_stats": r.path_stats[k],
                    "path": r.paths[k]})
    if save_dir is not None:
        _save_maps(out, "path", save_dir, name)
    return out


test_ge.__test__ = False


# ------------------------------------------------------------------------------------ data-parallel epochs (one process per GPU)
def train_epoch_dp(step: "GraphedWindowStep", cohort, order, opt, n_windows: int, group=None):
    """One rank's share of a data-parallel epoch: train_epoch / train_ge_epoch with the gradient exchange and the optimiser
    between the replays.  The plan is dp's: shards = shard_slides(lengths, world); this rank's `cohort` is a ResidentCohort
    (GeResidentCohort) over [slides[i] for i in shards[rank]]; (orders, n_windows) = epoch_orders(shard sizes, n, seed,
    epoch) and `order` = orders[rank], ids local to this rank's cohort.

    step: a GraphedWindowStep captured with opt=None and sample_rows=k on a window of `cohort`; its grad_acc_step is the
    PER-RANK window size n (the mean over ranks completes 1 / (n * world)) and its `l1` is passed explicitly (the optimiser
    is not inside the step) and must be `opt`'s l1_lambda.  Fusion models may be captured with split_patch_grad=True.
    opt: the flat optimiser over the step's bucket, stepped eagerly here; FlatOptimizer(max_grad_norm=, skip_nonfinite=)
    works unchanged: it measures the REDUCED gradient, the same on every rank, so every rank clips or skips alike.
    n_windows: the loop runs exactly that many windows ON EVERY RANK -- a rank that ran one more would wait in its
    collective for ever.  The whole `order` is validated as train_epoch validates it, and an order of fewer than
    n_windows * n ids is refused, before the first collective; what lies behind n_windows * n comes back as `leftover`
    and is not run.

    Per window the loop enqueues: the bind, the selects into the step's static tensors, the replay; with split_patch_grad
    the all-reduce of flat[head:] while replay_tail() computes the patch layer's weight gradient, then that of flat[:head],
    otherwise (always for the gene-expression model) one all-reduce of the bucket; opt.step(l1_slides = n * world); the
    device copies of loss (and risk) into epoch-long buffers.  Under nccl (RCCL) there is no host synchronisation and no H2D
    copy inside the loop; gloo, which the tests run on one card, stages every collective through the host.  The nccl leg is
    the same calls and is exercised by multi-GPU bench runs (bench.py --gpus N) alone.  With no process group
    initialised the world is 1: no collective, the same loop.

    Ranks must not share dropout masks and row samples: the generator's seed is torch.initial_seed() (ops._reserve), read
    when the step is captured, so call torch.manual_seed(base + rank) BEFORE the capture.

    Returns what train_epoch (loss, risk, ids_run, leftover) or train_ge_epoch (loss, ids_run, leftover) returns, for this
    rank's slides, ids local to this rank's cohort; epoch_c_index_dp gives the epoch's training C-index over all ranks."""
    from . import dp
    who = "train_epoch_dp"
    if step.sampler is None or step.sampler.source != "slides":
        raise ValueError(f"{who}: the step must be captured with sample_rows on a window of a resident cohort")
    if step.opt is not None:
        raise ValueError(f"{who}: the step was captured with its optimiser inside; a data-parallel step leaves it out "
                         "(opt=None): the update comes after the exchange")
    if isinstance(cohort, GeResidentCohort) != step.ge:
        raise ValueError(f"{who}: a {'gene-expression' if step.ge else 'fusion-model'} step over a {type(cohort).__name__}")
    if opt.bucket is not step.bucket:
        raise ValueError(f"{who}: the optimiser steps another gradient bucket than the one the step writes")
    if float(getattr(opt, "l1_lambda", 0.0)) != step.l1:
        raise ValueError(f"{who}: the step reports the L1 penalty with l1 = {step.l1}, the optimiser folds its gradient with "
                         f"l1_lambda = {float(getattr(opt, 'l1_lambda', 0.0))}: pass the optimiser's value to the step")
    order = _check_epoch_order(who, step, cohort, order)
    n, n_win = step.sampler.n_slides, int(n_windows)
    if n_win < 0 or len(order) < n_win * n:
        raise ValueError(f"{who}: {n_win} windows of {n} slides need {n_win * n} ids, the order holds {len(order)}; n_windows is "
                         "dp.epoch_orders' -- the same on every rank")
    world = dp._world(group)
    bucket = step.bucket
    head = step.head_numel() if step.split else None
    folds_l1 = bool(getattr(opt, "l1_lambda", 0.0))

    def exchange_and_step():
        if step.split:
            rest = bucket.all_reduce_mean_async(lo=head, group=group)
            step.replay_tail()
            first = bucket.all_reduce_mean_async(lo=0, hi=head, group=group)
            for handle in (rest, first):
                if handle is not None:
                    handle.wait()
        else:
            bucket.all_reduce_mean(group)
        if folds_l1:
            opt.step(l1_slides=n * world)
        else:
            opt.step()
    loss, risk, ids_run, leftover = _run_epoch(step, cohort, order, n_win, exchange_and_step)
    return (loss, ids_run, leftover) if step.ge else (loss, risk, ids_run, leftover)


def epoch_c_index_dp(cohort: ResidentCohort, ids_run, risk, group=None):
    """The training C-index of a data-parallel epoch over ALL ranks' slides: this rank's risks (train_epoch_dp's `risk`) and
    the censorship and survival months of the slides it ran (`ids_run`) are gathered rank-major -- three all-gathers of
    equal sizes, n_windows * n per rank -- and concordance_index_device runs over the union.  -> (c_index (1,) fp64, counts
    (3,) int64) on the device: integer counts over the same gathered vectors, so every rank holds the same counts and the
    same C-index bits."""
    from . import dp
    sizes = [int(risk.numel())] * dp._world(group)
    ids = ids_run.to(torch.int64)
    cens, months, risks = (dp.gather_ragged(t, sizes, group) for t in
                           (cohort.censorship.index_select(0, ids), cohort.survival_months.index_select(0, ids), risk.detach()))
    return concordance_index_device(cens, months, risks)


def validate_dp(evaluator, sizes, group=None):
    """A validation epoch over a sharded cohort: every rank calls its own CohortEvaluator (GeCohortEvaluator) -- eager or
    captured, over the validation slides it holds; nothing in those classes knows about ranks -- and the per-slide results are
    gathered (dp.gather_ragged; sizes[r] = the number of slides rank r evaluates, from the shard plan; unequal sizes are
    the normal case).  Returns the evaluator's result type over the UNION of the slides in rank-major order, the same bits
    on every rank: loss, risk, hazards, survs, Y with mean_loss and the C-index (counts) recomputed on the device over the
    gathered risks, censorship and survival months; for the gene-expression model loss, Y and, over them and the gathered
    labels, classification_metrics_device.  Maps and pooling attentions (need_maps / need_paths) stay with their rank: the
    union's result carries none.  At world size 1 the evaluator's own result comes back."""
    from . import dp
    world = dp._world(group)
    sizes = [int(s) for s in sizes]
    if len(sizes) != world or sizes[dp._rank(group)] != len(evaluator.ids):
        raise ValueError(f"validate_dp: sizes {sizes} for a world of {world} whose rank here evaluates {len(evaluator.ids)} slides")
    r = evaluator()
    if world == 1:
        return r

    def gather(t):
        return dp.gather_ragged(t, sizes, group)
    per_slide = [gather(getattr(r, name)) for name in evaluator.PER_SLIDE]
    return evaluator._result(per_slide, [gather(t) for t in evaluator._targets])
