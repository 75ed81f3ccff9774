"""A whole training run: the reference's main() (models/mcat/main.py:218-337, models/nacagat/main.py, models/ge_nacagat/
main.py:171-282) over a cohort that lives on the device, joined from the pieces this package already has.

    split_patients   MultimodalDataset.split (dataset/dataset.py:145-185) on slide indices
    fit_options      the reference's whole YAML dict -> FitOptions (harness.training_options for its `training:` block)
    Fit              construction does every capture; epoch() enqueues one epoch in the reference's order; run() the rest
    fit              Fit(...).run()

Pure host code over public functions of harness, dp and checkpoint: no kernel, no C entry.  The hot path of a run is the
captured window step and the captured evaluator; this module adds no launch per window to them and no host
synchronisation per epoch (Fit's docstring names the four options that do read the host).
"""
from __future__ import annotations

import datetime
import os
from dataclasses import dataclass
from typing import Callable, Hashable, List, NamedTuple, Sequence

import torch

from . import checkpoint, dp, harness

SPLIT_EPOCH = -1        # the `epoch` of split_patients' shuffle key: 2^64 - 1 after masking, which no epoch order uses

SURVIVAL_COLUMNS = ("lr", "train_loss", "train_c_index", "val_loss", "val_c_index")
GE_COLUMNS = ("lr", "train_loss", "val_loss", "val_accuracy", "val_balanced_accuracy")
LARGER_IS_BETTER = {"val_c_index": True, "val_accuracy": True, "val_loss": False}


# ------------------------------------------------------------------------------------ the patient-level split
class Split(NamedTuple):
    """Slide indices of the three parts, each ascending; `test` is empty without leave_one_out."""
    train: List[int]
    val: List[int]
    test: List[int]


def split_patients(patients: Sequence[Hashable], train_size: float, leave_one_out=None, seed: int = 0,
                   permutation=None) -> Split:
    """The reference's MultimodalDataset.split (dataset/dataset.py:145-185) on slide indices.  patients[i] is the patient of
    slide i.  The unique patients, in order of first appearance (pandas.unique's order), are shuffled; the first
    int(len(unique) * train_size) of them are train, the rest val, and every slide follows its patient.  With
    leave_one_out = p, p's slides are `test` and are taken out of whichever side p fell on AFTER the cut, as the reference
    does: the counts of the cut are those of all patients, p included.

    The shuffle is dp's splitmix64 Fisher-Yates (integer arithmetic alone: the same split on every host), not numpy's
    unseeded one, under the key (seed, epoch = SPLIT_EPOCH = -1 -> 2^64 - 1, rank = 0): dp.epoch_orders keys its orders
    by (seed, epoch >= 0, rank), so no epoch order of the same seed shares the stream.  permutation: an explicit order of
    the unique patients (every one exactly once) used instead of the shuffle -- `seed` is ignored -- to reproduce a split made
    elsewhere, for example by the reference.

    ValueError: train_size outside (0, 1); leave_one_out naming no patient; a permutation of another length than the unique
    patients, or one that is not a permutation of them; a train or val side without a slide (a side that held the leave-one-out patient alone included)."""
    if not 0 < train_size < 1:
        raise ValueError("train_size should be a float between 0 and 1.")
    patients = list(patients)
    unique = list(dict.fromkeys(patients))
    if leave_one_out is not None and leave_one_out not in unique:
        raise ValueError(f"split_patients: leave_one_out patient {leave_one_out!r} is not among the {len(unique)} patients")
    if permutation is not None:
        shuffled = list(permutation)
        if len(shuffled) != len(unique):
            raise ValueError(f"split_patients: permutation holds {len(shuffled)} patients, the slides name {len(unique)}")
        if set(shuffled) != set(unique):
            raise ValueError(f"split_patients: permutation is not a permutation of the {len(unique)} unique patients")
    else:
        shuffled = [unique[i] for i in dp._permutation(len(unique), seed, SPLIT_EPOCH, 0)]
    cut = int(len(unique) * train_size)
    train_patients = set(shuffled[:cut]) - {leave_one_out}
    val_patients = set(shuffled[cut:]) - {leave_one_out}
    train = [i for i, p in enumerate(patients) if p in train_patients]
    val = [i for i, p in enumerate(patients) if p in val_patients]
    test = [i for i, p in enumerate(patients) if leave_one_out is not None and p == leave_one_out]
    if not train or not val:
        raise ValueError(f"split_patients: {len(unique)} patients at train_size {train_size}"
                         f"{'' if leave_one_out is None else f' without {leave_one_out!r}'} leave "
                         f"{len(train)} train and {len(val)} val slides: both sides need one")
    return Split(train, val, test)


# ------------------------------------------------------------------------------------ the reference's config
@dataclass
class FitOptions:
    """What a run reads from the reference's config.yaml beyond its `training:` choices (`train`: harness.TrainOptions,
    unchanged): training.{epochs, train_size, leave_one_out, output_attn_epoch, test_output_dir},
    model.{name, checkpoint_epoch, checkpoint_dir, load_from_checkpoint} and dataset.name."""
    model_kind: str
    epochs: int
    train_size: float
    leave_one_out: object                 # the test patient, None = no test()
    output_attn_epoch: int
    test_output_dir: "str | None"
    model_name: str
    checkpoint_epoch: int                 # 0 = never
    checkpoint_dir: "str | None"
    load_from_checkpoint: "str | None"
    dataset_name: str
    train: harness.TrainOptions


def fit_options(config: dict, model_kind: str = "mcat") -> FitOptions:
    """The reference's whole YAML dict (models/*/config/config.yaml, as yaml.safe_load returns it) -> FitOptions.  Keys this
    package has no use for (device, wandb, the dataset's files, model.fusion / model_size / gene: the model is built by the
    caller) are not read.  `train` is harness.training_options(config['training'], model_kind): its refusals (CE_REFUSAL
    for a fusion model with loss 'ce') are raised here."""
    training, model, dataset = config["training"], config["model"], config["dataset"]
    train = harness.training_options(training, model_kind)
    return FitOptions(model_kind=model_kind, epochs=int(training["epochs"]), train_size=float(training["train_size"]),
                      leave_one_out=training.get("leave_one_out"), output_attn_epoch=int(training.get("output_attn_epoch") or 0),
                      test_output_dir=training.get("test_output_dir"), model_name=str(model["name"]),
                      checkpoint_epoch=int(model.get("checkpoint_epoch") or 0), checkpoint_dir=model.get("checkpoint_dir"),
                      load_from_checkpoint=model.get("load_from_checkpoint"), dataset_name=str(dataset["name"]), train=train)


# ------------------------------------------------------------------------------------ the run
class EpochResult(NamedTuple):
    """What one Fit.epoch() leaves, all of it on the device but `epoch`, `leftover` and `checkpoint`: the per-slide training
    loss and risk (risk None for the gene-expression model) of the slides `ids_run` (cohort ids, in the order they ran),
    the host ids of the final partial window, which did not run, the validation's result, harness.test's / test_ge's list
    (None without test_ids) and the checkpoint's path (None where none was written)."""
    epoch: int
    loss: torch.Tensor
    risk: "torch.Tensor | None"
    ids_run: torch.Tensor
    leftover: List[int]
    val: object
    test: "list | None"
    checkpoint: "str | None"


@dataclass
class FitResult:
    """history: (epochs, len(columns)) fp64 on the device, NaN in the rows this process did not run (before a resume, behind
    an early stop).  final: the "final validation"'s EvalResult / GeEvalResult.  epochs_run: the epoch indices run here.
    best_epoch: () int64 on the device, -1 while nothing improved (None without keep_best).  leftover: how many slides the
    last epoch's final partial window held (they are not run).  Nothing here has been read by the host; table() is the one
    reader."""
    history: torch.Tensor
    columns: tuple
    final: object
    epochs_run: List[int]
    stopped_early: bool
    leftover: int
    best_epoch: "torch.Tensor | None" = None
    _fit: "Fit | None" = None

    def table(self) -> "List[dict]":
        """The history on the host: one dict per epoch of the table, {'epoch': index, column: float, ...}.  One copy, one
        synchronisation."""
        rows = self.history.cpu().tolist()
        return [{"epoch": e, **dict(zip(self.columns, row))} for e, row in enumerate(rows)]

    def restore_best(self):
        """Copy the parameters of the best epoch back into the optimiser's flat buffer, in place (every captured graph
        keeps reading the same addresses); nothing changes while no epoch improved.  No host synchronisation."""
        f = self._fit
        if f is None or f.best_p is None:
            raise ValueError("FitResult.restore_best: the run kept no best parameters (keep_best=None)")
        torch.where(f.best_epoch >= 0, f.best_p, f.opt.flat_p, out=f.opt.flat_p)


def _is_ge_model(model) -> bool:
    from .models import GeneExprNarrowContextualAttentionGateTransformer
    return isinstance(model, GeneExprNarrowContextualAttentionGateTransformer)


def _ids(name: str, ids, n_slides: int) -> "List[int]":
    out = [int(i) for i in ids]
    for i in out:
        if not 0 <= i < n_slides:
            raise ValueError(f"Fit: {name} names slide {i}, outside the cohort's {n_slides} slides")
    if len(set(out)) != len(out):
        raise ValueError(f"Fit: {name} names a slide twice")
    return out


class Fit:
    """One training run over a resident cohort: the reference's main() with every epoch enqueued on the device.

    model: MCAT or NaCAGaT over a harness.ResidentCohort, or the gene-expression model over a harness.GeResidentCohort.
    train_ids / val_ids / test_ids: slide ids into that ONE cohort (split_patients gives them), pairwise disjoint.
    options: fit_options(config, kind).  sample_rows: the captured step's k rows per slide.

    Construction does all host work, H2D copies and captures, in this order:
      0. every refusal below (ValueError, naming the argument), before anything is built or captured;
      1. dp.FlatGradBucket over the model's parameters;
      2. options.train.make_optimizer / make_scheduler -- the flat optimiser re-points the parameters, so everything
         captured below follows them;
      3. with `resume` (default: options.load_from_checkpoint): checkpoint.load of that file into model, optimiser,
         scheduler and dropout generator; the run continues at res.epoch + 1 (this package's documented choice: the
         reference repeats the stored epoch).  In a world, the rank's own torch seed is put back (the file holds rank
         0's) and opt.flat_p is then broadcast from rank 0;
      4. the harness.GraphedWindowStep on the first grad_acc_step train ids, with sample_rows, rng_base =
         res.graph_rng_base (a resumed run draws the masks the interrupted one would have), device_feature_scale=True for
         an fp32 cohort; the optimiser inside the graph in a single process, opt=None (and split_patch_grad=True for the
         fusion models) in a data-parallel run;
      5. the validation evaluator (CohortEvaluator / GeCohortEvaluator over val_ids with the training loss, alpha,
         lambda_reg and l1), captured with capture_eval unless the loss is 'cesar', which no evaluator captures;
      6. the test evaluation's part: test_ids and the patient's name (test_patient, default options.leave_one_out) are
         fixed; harness.test / test_ge are eager and build their windows per call.

    epoch() enqueues, in the reference's order (train() :19-103, then main() :326-333):
      1. the training epoch: order = dp.epoch_orders(sizes, grad_acc_step, seed, epoch) mapped through train_ids, sizes =
         [len(train_ids)] in a single process and train_shard_sizes in a world (a world of one and a single process run
         the same order), through harness.train_epoch / train_ge_epoch / train_epoch_dp.  The final partial window is
         not run, as in those functions; EpochResult.leftover and FitResult.leftover report it;
      2. the epoch's mean reported loss (over every rank's slides) and, for the survival models, its C-index
         (harness.concordance_index_device; epoch_c_index_dp in a world), and the learning rate the epoch ran at;
      3. scheduler.step();
      4. a checkpoint iff checkpoint_epoch > 0 and (epoch + 1) % checkpoint_epoch == 0 and epoch != 0 (the reference's
         condition, main.py:88-89), to checkpoint_dir/{model name}_{dataset name}_E{epoch + 1}_{stamp}.pt by
         checkpoint.save(..., scheduler=, graphed_step=), on rank 0 alone;
      5. the validation: the evaluator, or harness.validate_dp over val_shard_sizes;
      6. with test_ids: harness.test / test_ge over them, with save_dir = test_output_dir only when (epoch + 1) %
         output_attn_epoch == 0, under the name ATTN_{model name}_{patient}_{stamp}_E{epoch + 1} (gene-expression model:
         ATTN_{patient}_{stamp}_E{epoch + 1}); those functions append _{slide id}.pt where the reference has the loader's
         batch index.
    run() runs the epochs that remain and then the reference's "final validation".

    Host reads.  An epoch without a checkpoint, a saved test file, `log` and `patience` makes no host synchronisation
    that torch.cuda.set_sync_debug_mode("error") can see: harness.train_epoch's guarantee, kept.  Each of those four
    synchronises: the checkpoint and the test files copy tensors to the host, `log` (called with the epoch's row of the
    table as a dict) reads that row, `patience` reads one scalar per epoch.

    History: one (epochs, columns) fp64 tensor on the device, NaN in rows this process did not run, filled by device
    copies -- SURVIVAL_COLUMNS or GE_COLUMNS; `lr` is the rate the epoch's steps ran at (what the reference prints).

    keep_best: 'val_c_index' / 'val_accuracy' (larger is better) or 'val_loss' (smaller).  After each validation one strict
    comparison on the device -- NaN never improves, a tie keeps the earlier epoch -- then one torch.where of opt.flat_p
    into a second flat buffer and one of the epoch index into best_epoch; FitResult.restore_best() copies the buffer
    back in place.  The best-so-far is NOT written into checkpoints: a resumed run tracks the epochs it runs itself.
    patience = p (needs keep_best): stop after p consecutive epochs without improvement; one scalar read per epoch.  In a
    world validate_dp gives every rank the same bits, so every rank reads the same scalar and all stop together.

    Data parallelism (group=, or shard sizes given: one process per GPU): the cohort holds this rank's slides alone (train
    and validation shards side by side), train_ids / val_ids / test_ids are local to it, train_shard_sizes[r] /
    val_shard_sizes[r] are rank r's counts of train and val ids (dp.shard_slides' plan), the same lists on every rank.
    torch.manual_seed(base + rank) BEFORE Fit stays the caller's duty: the captured step reads the seed, and ranks that
    share one draw the same masks and rows.  Shard sizes without a process group are a world of one.

    stamp: the string in the file names; default the reference's timestamps, taken once here ('%Y%m%d%H%M' for
    checkpoints and the gene-expression model's test files, '%Y%m%d%H%M%S' for the fusion models' test files).
    warmup: GraphedWindowStep's.

    ValueError, before anything is captured: train_ids / val_ids / test_ids out of range, repeated or overlapping;
    train_ids fewer than one window (in a world: a rank's shard); cohort of the other model's layout; options built for
    another model kind; a slide shorter than sample_rows in a cohort that does not lap; test_ids without a patient's
    name; patience without keep_best; keep_best naming a metric the model kind does not have; train_shard_sizes /
    val_shard_sizes missing in a world or not matching the world and the local id lists."""

    def __init__(self, model, cohort, train_ids, val_ids, options: FitOptions, *, sample_rows: int, seed: int = 0,
                 test_ids=None, test_patient=None, capture_eval: bool = True, keep_best: "str | None" = None,
                 patience: "int | None" = None, resume=None, group=None, train_shard_sizes=None, val_shard_sizes=None,
                 stamp: "str | None" = None, log: "Callable | None" = None, warmup: int = 2):
        # ---- 0. refusals
        self.ge = _is_ge_model(model)
        kind = "ge_nacagat" if self.ge else harness._model_kind(model)
        if isinstance(cohort, harness.GeResidentCohort) != self.ge or not isinstance(
                cohort, (harness.ResidentCohort, harness.GeResidentCohort)):
            raise ValueError(f"Fit: cohort is a {type(cohort).__name__}; the {'gene-expression' if self.ge else 'survival'} model "
                             f"{type(model).__name__} trains over a {'GeResidentCohort' if self.ge else 'ResidentCohort'}")
        if options.model_kind != kind:
            raise ValueError(f"Fit: options were read for '{options.model_kind}', the model is '{kind}'")
        o = options.train
        n = int(o.grad_acc_step)
        self.train_ids = _ids("train_ids", train_ids, cohort.n_slides)
        self.val_ids = _ids("val_ids", val_ids, cohort.n_slides)
        self.test_ids = _ids("test_ids", test_ids, cohort.n_slides) if test_ids is not None else []
        for a, b, ids_a, ids_b in (("train_ids", "val_ids", self.train_ids, self.val_ids),
                                   ("train_ids", "test_ids", self.train_ids, self.test_ids),
                                   ("val_ids", "test_ids", self.val_ids, self.test_ids)):
            both = sorted(set(ids_a) & set(ids_b))
            if both:
                raise ValueError(f"Fit: {a} and {b} overlap (slides {both[:5]}{' ...' if len(both) > 5 else ''})")
        if not self.val_ids:
            raise ValueError("Fit: val_ids is empty")
        if len(self.train_ids) < n:
            raise ValueError(f"Fit: train_ids holds {len(self.train_ids)} slides, fewer than one window of grad_acc_step = {n}")
        k = int(sample_rows)
        short = [i for i in self.train_ids if cohort.lengths[i] < k]
        if short and not cohort.cycle:
            raise ValueError(f"Fit: sample_rows = {k}, but slide {short[0]} has {cohort.lengths[short[0]]} rows and the cohort "
                             "does not lap short slides (cycle=False)")
        self.test_patient = options.leave_one_out if test_patient is None else test_patient
        if self.test_ids and self.test_patient is None:
            raise ValueError("Fit: test_ids without test_patient (or options.leave_one_out): the test files carry the patient's name")
        columns = GE_COLUMNS if self.ge else SURVIVAL_COLUMNS
        if patience is not None and keep_best is None:
            raise ValueError("Fit: patience counts epochs without improvement of the keep_best metric; keep_best is None")
        if patience is not None and int(patience) < 1:
            raise ValueError(f"Fit: patience = {patience} (at least 1)")
        if keep_best is not None and (keep_best not in LARGER_IS_BETTER or keep_best not in columns):
            have = [c for c in columns if c in LARGER_IS_BETTER]
            raise ValueError(f"Fit: keep_best = {keep_best!r} is not a validation metric of '{kind}' ({' | '.join(have)})")
        self.group = group
        self.world, self.rank = dp._world(group), dp._rank(group)
        self.dp = group is not None or train_shard_sizes is not None or val_shard_sizes is not None or self.world > 1
        self.train_sizes = self.val_sizes = None
        if self.dp:
            for name, sizes, mine in (("train_shard_sizes", train_shard_sizes, self.train_ids),
                                      ("val_shard_sizes", val_shard_sizes, self.val_ids)):
                if sizes is None:
                    raise ValueError(f"Fit: a data-parallel run needs {name} (every rank's count, the same list on every rank)")
                sizes = [int(s) for s in sizes]
                if len(sizes) != self.world or sizes[self.rank] != len(mine):
                    raise ValueError(f"Fit: {name} = {sizes} for a world of {self.world} whose rank {self.rank} holds {len(mine)} "
                                     f"such ids")
            self.train_sizes, self.val_sizes = [int(s) for s in train_shard_sizes], [int(s) for s in val_shard_sizes]
            if min(self.train_sizes) < n:
                raise ValueError(f"Fit: train_shard_sizes = {self.train_sizes}: a rank holds fewer than one window of "
                                 f"grad_acc_step = {n}, and every rank must run the same number of windows")
        self.model, self.cohort, self.options, self.kind = model, cohort, options, kind
        self.n, self.k, self.seed = n, k, int(seed)
        self.columns, self.log = columns, log
        self.keep_best, self.patience = keep_best, None if patience is None else int(patience)
        now = datetime.datetime.now()
        self.checkpoint_stamp = now.strftime("%Y%m%d%H%M") if stamp is None else str(stamp)
        self.test_stamp = now.strftime("%Y%m%d%H%M" if self.ge else "%Y%m%d%H%M%S") if stamp is None else str(stamp)
        dev = cohort.device

        # ---- 1. - 3. bucket, optimiser and schedule, the checkpoint
        self.bucket = dp.FlatGradBucket(list(model.parameters()))
        self.opt = o.make_optimizer(self.bucket)
        self.sched = o.make_scheduler(self.opt)
        self.next_epoch, rng_base = 0, None
        resume = options.load_from_checkpoint if resume is None else resume
        if resume is not None:
            own_seed = torch.initial_seed()
            res = checkpoint.load(resume, model, self.opt, self.sched)
            self.next_epoch, rng_base = int(res.epoch) + 1, res.graph_rng_base
            if self.dp and torch.initial_seed() != own_seed:
                torch.manual_seed(own_seed)         # the file holds rank 0's seed; a rank keeps drawing its own masks and rows
        self.first_epoch = self.next_epoch
        if self.world > 1:
            import torch.distributed as dist
            dist.broadcast(self.opt.flat_p, src=0 if group is None else dist.get_global_rank(group, 0), group=group)

        # ---- 4. the captured step
        model.train()
        first = self.train_ids[:n]
        window = cohort.window(torch.tensor(first, dtype=torch.int32).to(dev, non_blocking=True), first)
        kw = dict(l1=o.l1) if self.ge else o.train_kwargs()
        if self.dp:
            kw.update(opt=None, split_patch_grad=not self.ge)
        else:
            kw.update(opt=self.opt)
        self.step = harness.GraphedWindowStep(model, self.bucket, window, n, warmup=warmup, sample_rows=k, rng_base=rng_base,
                                              device_feature_scale=cohort.rows[0].dtype == torch.float32, **kw)

        # ---- 5. the validation evaluator
        if self.ge:
            self.evaluator = harness.GeCohortEvaluator(model, cohort, self.val_ids, l1=o.l1, capture=bool(capture_eval))
        else:
            self.evaluator = harness.CohortEvaluator(model, cohort, self.val_ids, loss=o.loss, alpha=o.alpha,
                                                     lambda_reg=o.lambda_reg, l1=o.l1,
                                                     capture=bool(capture_eval) and o.loss != "cesar")

        # ---- the history and the best-so-far
        self.history = torch.full((options.epochs, len(columns)), float("nan"), dtype=torch.float64, device=dev)
        self.best_p = self.best_epoch = self.best_value = None
        if keep_best is not None:
            self.best_p = self.opt.flat_p.clone()
            self.best_epoch = torch.full((), -1, dtype=torch.int64, device=dev)
            worst = float("-inf") if LARGER_IS_BETTER[keep_best] else float("inf")
            self.best_value = torch.full((), worst, dtype=torch.float64, device=dev)
        self.epochs_run: List[int] = []
        self.stale = 0                      # consecutive epochs without improvement (patience)
        self.stopped_early = False
        self.last: "EpochResult | None" = None

    # ---- the pieces of an epoch
    def _train(self, epoch: int):
        sizes = self.train_sizes if self.dp else [len(self.train_ids)]
        orders, n_windows = dp.epoch_orders(sizes, self.n, self.seed, epoch)
        order = [self.train_ids[i] for i in orders[self.rank]]
        if self.dp:
            out = harness.train_epoch_dp(self.step, self.cohort, order, self.opt, n_windows, group=self.group)
        elif self.ge:
            out = harness.train_ge_epoch(self.step, self.cohort, order)
        else:
            out = harness.train_epoch(self.step, self.cohort, order)
        return (out[0], None, out[1], out[2]) if self.ge else out

    def _validate(self):
        if self.dp:
            return harness.validate_dp(self.evaluator, self.val_sizes, group=self.group)
        return self.evaluator()

    def _write(self, epoch: int, column: str, value: torch.Tensor):
        self.history[epoch, self.columns.index(column)].copy_(value.reshape(()), non_blocking=True)

    def checkpoint_path(self, epoch: int) -> str:
        o = self.options
        return os.path.join(o.checkpoint_dir or "", f"{o.model_name}_{o.dataset_name}_E{epoch + 1}_{self.checkpoint_stamp}.pt")

    def test_name(self, epoch: int) -> str:
        head = "ATTN" if self.ge else f"ATTN_{self.options.model_name}"
        return f"{head}_{self.test_patient}_{self.test_stamp}_E{epoch + 1}"

    def _track_best(self, epoch: int) -> "torch.Tensor":
        metric = self.history[epoch, self.columns.index(self.keep_best)]
        better = metric > self.best_value if LARGER_IS_BETTER[self.keep_best] else metric < self.best_value
        torch.where(better, self.opt.flat_p, self.best_p, out=self.best_p)
        self.best_epoch = torch.where(better, epoch, self.best_epoch)
        self.best_value = torch.where(better, metric, self.best_value)
        return better

    def epoch(self) -> EpochResult:
        """Enqueue the next epoch (the class docstring's six steps) -> EpochResult."""
        epoch, o = self.next_epoch, self.options
        if epoch >= o.epochs or self.stopped_early:
            raise ValueError(f"Fit.epoch: the run is over ({'stopped early' if self.stopped_early else f'{o.epochs} epochs'})")
        loss, risk, ids_run, leftover = self._train(epoch)
        n_run = int(loss.numel())
        self._write(epoch, "lr", self.opt.lr_dev)
        train_loss = dp.gather_ragged(loss, [n_run] * self.world, self.group).mean(0, keepdim=True) if self.dp \
            else loss.mean(0, keepdim=True)
        self._write(epoch, "train_loss", train_loss)
        if not self.ge:
            if self.dp:
                c_index, _ = harness.epoch_c_index_dp(self.cohort, ids_run, risk, group=self.group)
            else:
                ids = ids_run.to(torch.int64)
                c_index, _ = harness.concordance_index_device(self.cohort.censorship.index_select(0, ids),
                                                              self.cohort.survival_months.index_select(0, ids), risk)
            self._write(epoch, "train_c_index", c_index)
        if self.sched is not None:
            self.sched.step()
        path = None
        if o.checkpoint_epoch > 0 and (epoch + 1) % o.checkpoint_epoch == 0 and epoch != 0 and self.rank == 0:
            path = self.checkpoint_path(epoch)
            if o.checkpoint_dir:
                os.makedirs(o.checkpoint_dir, exist_ok=True)
            checkpoint.save(path, self.model, self.opt, epoch, train_loss, scheduler=self.sched, graphed_step=self.step)
        r = self._validate()
        self._write(epoch, "val_loss", r.mean_loss)
        if self.ge:
            self._write(epoch, "val_accuracy", r.accuracy)
            self._write(epoch, "val_balanced_accuracy", r.balanced_accuracy)
        else:
            self._write(epoch, "val_c_index", r.c_index)
        tested = None
        if self.test_ids:
            save = o.output_attn_epoch > 0 and (epoch + 1) % o.output_attn_epoch == 0
            run_test = harness.test_ge if self.ge else harness.test
            tested = run_test(self.model, self.cohort, self.test_ids, save_dir=o.test_output_dir if save else None,
                              name=self.test_name(epoch))
        if self.keep_best is not None:
            better = self._track_best(epoch)
            if self.patience is not None:
                self.stale = 0 if bool(better) else self.stale + 1          # the one scalar read
                self.stopped_early = self.stale >= self.patience
        if self.log is not None:
            self.log({"epoch": epoch, **dict(zip(self.columns, self.history[epoch].tolist())), "leftover": len(leftover)})
        self.epochs_run.append(epoch)
        self.next_epoch = epoch + 1
        self.last = EpochResult(epoch, loss, risk, ids_run, leftover, r, tested, path)
        return self.last

    def run(self) -> FitResult:
        """The epochs that remain (all of them, or from res.epoch + 1 after a resume; fewer where patience stops the run),
        then the reference's "final validation" (main.py:337)."""
        while self.next_epoch < self.options.epochs and not self.stopped_early:
            self.epoch()
        final = self._validate()
        return FitResult(self.history, self.columns, final, list(self.epochs_run), self.stopped_early,
                         0 if self.last is None else len(self.last.leftover), self.best_epoch, self)


def fit(model, cohort, train_ids, val_ids, options: FitOptions, **kwargs) -> FitResult:
    """Fit(model, cohort, train_ids, val_ids, options, **kwargs).run(): the reference's main() from the split onwards."""
    return Fit(model, cohort, train_ids, val_ids, options, **kwargs).run()
