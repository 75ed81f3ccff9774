"""A whole run (multimodal_path_omic_amd/fit.py) on the device, against the loop INTEGRATION.md spells out, written here by
hand from harness / dp / checkpoint: fit is that loop; no synchronisation in an epoch; resume; leave-one-out files;
keep_best; patience; a world of two on one card; every refusal before any capture.

Measure of equality (tests/test_gpu_checkpoint.py::_hold, restated): the hand-written loop runs twice from identical state
-- the same weight seed, ops.set_rng_state to a fixed counter, ops.set_rng_epoch(None), the same torch.manual_seed -- and
the two runs' largest difference is the run-to-run noise (the atomically summed gradients).  What is compared to the loop
must be bit-equal where that noise is zero and within twice the noise otherwise.  No other tolerance.

Shapes: 14 slides of 40-120 rows, seven patients of two slides, omic sizes [64] * 6, medium models, bf16 rows, a lapping
cohort, sample_rows 32, windows of 4 slides (2 per rank in the world of two), three or four epochs, one warm-up run."""
import os

import pytest
import torch
import torch.distributed as dist

import cases as C
from dp_spawn import run_world
from multimodal_path_omic_amd import checkpoint, dp, fit, harness, ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.dp import FlatGradBucket
from multimodal_path_omic_amd.models import (GeneExprNarrowContextualAttentionGateTransformer,
                                             MultimodalCoAttentionTransformer, NarrowContextualAttentionGateTransformer)

pytestmark = pytest.mark.gpu

SIZES = [64] * 6
ACC, K = 4, 32
PATIENTS = [f"P{i // 2}" for i in range(14)]
SPLIT = fit.split_patients(PATIENTS, 0.8, seed=7)                     # 5 patients train (10 slides), 2 val (4 slides)
PLAN_SEED = 23              # the epoch orders' seed
RNG_START = 1000            # the dropout counter every compared run starts from
WEIGHTS = 61
STAMP = "S0"
KINDS = ("mcat", "nacagat", "ge_nacagat")
NAMES = {"mcat": "MCAT", "nacagat": "NaCAGaT", "ge_nacagat": "GeneExpr-NaCAGaT"}

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def slides_of(kind):
    if kind == "ge_nacagat":
        return cached("ge slides", lambda: syn.make_ge_cohort(14, 40, 120, seed=771))
    return cached("slides", lambda: syn.make_cohort(14, 40, 120, SIZES, 770))


def cohort_of(kind, dev):
    cls = harness.GeResidentCohort if kind == "ge_nacagat" else harness.ResidentCohort
    return cached(("cohort", kind == "ge_nacagat"), lambda: cls(slides_of(kind), dev, cycle=True))


def build(kind, dev, seed=WEIGHTS):
    if kind == "ge_nacagat":
        model = GeneExprNarrowContextualAttentionGateTransformer(model_size="medium", bag_dtype=torch.bfloat16)
        shapes = C.ge_model_shapes(d=256)
    else:
        cls = MultimodalCoAttentionTransformer if kind == "mcat" else NarrowContextualAttentionGateTransformer
        model = cls(omic_sizes=SIZES, bag_dtype=torch.bfloat16)
        shapes = C.model_shapes(SIZES, kind == "nacagat")
    model.load_state_dict(syn.fill_state_dict(shapes, seed), strict=True)
    return model.to(dev).train()


def config(kind, epochs=3, out=None, **over):
    """The reference's config layout; `over` goes to `training:` unless it names a `model:` key."""
    c = {"dataset": {"name": "SYN-OV"},
         "model": {"name": NAMES[kind], "load_from_checkpoint": None, "checkpoint_epoch": 0,
                   "checkpoint_dir": None if out is None else os.path.join(str(out), "checkpoints"), "fusion": "concat",
                   "model_size": "medium"},
         "training": {"leave_one_out": None, "output_attn_epoch": 20,
                      "test_output_dir": None if out is None else os.path.join(str(out), "outputs"), "train_size": 0.8,
                      "loss": "ce" if kind == "ge_nacagat" else "ces", "epochs": epochs, "optimizer": "adam", "lr": 1e-3,
                      "weight_decay": 1e-5, "grad_acc_step": ACC, "scheduler": None, "alpha": 0.75, "lambda": 0.0, "gamma": 1.0}}
    for key, value in over.items():
        c["model" if key in c["model"] else "training"][key] = value
    return c


def fresh(seed=None):
    """The identical state every compared run starts from (seed: a child process's own; this process keeps the one it has, so
    that the tests behind this file find torch's generator as they always did)."""
    if seed is not None:
        torch.manual_seed(seed)
    ops.set_rng_epoch(None)
    ops.set_rng_state({"seed": torch.initial_seed(), "calls": RNG_START, "epoch": None})


def int32(values, dev):
    return torch.tensor(values, dtype=torch.int32).to(dev)


def final_tensors(kind, r):
    names = ("loss", "Y", "mean_loss", "accuracy") if kind == "ge_nacagat" else ("loss", "risk", "mean_loss", "c_index")
    return [getattr(r, n).clone() for n in names]


def state(opt):
    return [t.clone() for t in opt.state_tensors()]


def hold(what, a, a_again, b):
    """`b` against the loop's run `a`: bit-identical where two runs of the loop are (`a_again`), within twice their largest
    difference otherwise."""
    assert len(a) == len(a_again) == len(b)
    for x in list(a) + list(b):
        assert bool(torch.isfinite(x.double()).all()), what
    noise = max(float((x.double() - y.double()).abs().max()) for x, y in zip(a, a_again))
    diff = max(float((x.double() - y.double()).abs().max()) for x, y in zip(a, b))
    print(f"[fit {what}] the loop run to run: max |diff| {noise:.3e}; against the loop: {diff:.3e}")
    if noise == 0.0:
        assert all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b)), what
    else:
        assert diff <= 2 * noise, (what, diff, noise)


# ------------------------------------------------------------------------------------------------ the hand-written loop
def hand_loop(kind, dev, cfg, train_ids, val_ids, seed=PLAN_SEED):
    """INTEGRATION.md's loop (sections 5 and 6) in one process, from this package's functions as they were before fit:
    -> (history rows, the final validation's tensors, the optimiser's state)."""
    ge = kind == "ge_nacagat"
    cohort = cohort_of(kind, dev)
    o = harness.training_options(cfg["training"], kind)
    model = build(kind, dev)
    bucket = FlatGradBucket(list(model.parameters()))
    opt = o.make_optimizer(bucket)
    sched = o.make_scheduler(opt)
    first = train_ids[:ACC]
    kw = {} if ge else o.train_kwargs()
    step = harness.GraphedWindowStep(model, bucket, cohort.window(int32(first, dev), first), ACC, opt=opt, warmup=1, sample_rows=K,
                                     **kw)
    if ge:
        evaluator = harness.GeCohortEvaluator(model, cohort, val_ids, l1=o.l1, capture=True)
    else:
        evaluator = harness.CohortEvaluator(model, cohort, val_ids, loss=o.loss, alpha=o.alpha, lambda_reg=o.lambda_reg, l1=o.l1,
                                            capture=True)
    rows = []
    for epoch in range(cfg["training"]["epochs"]):
        orders, _ = dp.epoch_orders([len(train_ids)], ACC, seed, epoch)
        order = [train_ids[i] for i in orders[0]]
        lr = opt.lr_dev.double()
        if ge:
            loss, ids_run, leftover = harness.train_ge_epoch(step, cohort, order)
            train = [loss.mean(0, keepdim=True).double()]
        else:
            loss, risk, ids_run, leftover = harness.train_epoch(step, cohort, order)
            c_index, _ = harness.concordance_index_device(cohort.censorship[ids_run.long()], cohort.survival_months[ids_run.long()],
                                                          risk)
            train = [loss.mean(0, keepdim=True).double(), c_index]
        assert len(leftover) == len(train_ids) % ACC
        if sched:
            sched.step()
        r = evaluator()
        val = [r.mean_loss.double(), r.accuracy, r.balanced_accuracy] if ge else [r.mean_loss.double(), r.c_index]
        rows.append(torch.cat([lr] + train + val))
    return torch.stack(rows), final_tensors(kind, evaluator()), state(opt)


def fit_run(kind, dev, cfg, train_ids, val_ids, weights=WEIGHTS, **kwargs):
    model = build(kind, dev, weights)
    f = fit.Fit(model, cohort_of(kind, dev), train_ids, val_ids, fit.fit_options(cfg, kind), sample_rows=K, seed=PLAN_SEED,
                stamp=STAMP, warmup=1, **kwargs)
    return f, f.run()


def whole(history, final, opt_state):
    return [history] + list(final) + list(opt_state)


@pytest.fixture
def generator():
    """The dropout generator as the test found it, afterwards."""
    keep = ops.rng_state()
    yield
    ops.set_rng_epoch(None)
    ops.set_rng_state(keep)


# ------------------------------------------------------------------------------------------------ 1. fit is the hand-written loop
CASES = {"mcat": dict(scheduler="exp", gamma=0.9, **{"lambda": 1e-6}), "nacagat": {}, "ge_nacagat": {}}


@pytest.mark.parametrize("kind", KINDS)
def test_fit_is_the_hand_written_loop(dev, kind, generator):
    cfg = config(kind, epochs=3, **CASES[kind])
    runs = []
    for _ in range(2):
        fresh()
        runs.append(whole(*hand_loop(kind, dev, cfg, SPLIT.train, SPLIT.val)))
    fresh()
    f, res = fit_run(kind, dev, cfg, SPLIT.train, SPLIT.val)
    assert res.history.shape == (3, 5) and res.history.dtype == torch.float64 and res.history.is_cuda
    assert res.columns == (fit.GE_COLUMNS if kind == "ge_nacagat" else fit.SURVIVAL_COLUMNS)
    assert res.epochs_run == [0, 1, 2] and not res.stopped_early and res.leftover == len(SPLIT.train) % ACC == 2
    hold(kind, runs[0], runs[1], whole(res.history, final_tensors(kind, res.final), state(f.opt)))
    table = res.table()
    assert [row["epoch"] for row in table] == [0, 1, 2] and set(table[0]) == {"epoch", *res.columns}
    assert [row["lr"] for row in table] == res.history[:, 0].tolist()
    if kind == "mcat":                                                # the schedule: the rate each epoch RAN at
        lr = torch.tensor([1e-3, 1e-3 * 0.9, 1e-3 * 0.9 * 0.9], dtype=torch.float32).double()
        assert torch.equal(res.history[:, 0].cpu(), lr)


# ------------------------------------------------------------------------------------------------ 2. no synchronisation
@pytest.mark.parametrize("kind", ["mcat", "ge_nacagat"])
def test_an_epoch_makes_no_host_sync(dev, kind, generator):
    fresh()
    model = build(kind, dev)
    f = fit.Fit(model, cohort_of(kind, dev), SPLIT.train, SPLIT.val, fit.fit_options(config(kind, epochs=3), kind), sample_rows=K,
                seed=PLAN_SEED, stamp=STAMP, warmup=1, keep_best="val_loss")
    before = f.opt.flat_p.clone()
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            int(probe)                                               # the mode is honoured: a synchronising call raises
        f.epoch()
        f.epoch()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert not torch.equal(f.opt.flat_p, before) and int(f.opt.t_dev) == 2 * (len(SPLIT.train) // ACC)
    assert bool(torch.isfinite(f.history[:2]).all()) and bool(torch.isnan(f.history[2]).all())
    assert f.next_epoch == 2 and f.epochs_run == [0, 1]


# ------------------------------------------------------------------------------------------------ 3. resume
def move_the_counter(kind, dev, model):
    """An unrelated training-mode forward: reserves dropout streams, i.e. advances the host counter."""
    before = ops.rng_state()["calls"]
    cohort, ids = cohort_of(kind, dev), SPLIT.val[:2]
    window = cohort.window(int32(ids, dev), ids)
    with torch.no_grad():
        if kind == "ge_nacagat":
            model.forward_window(window[0].materialize())
        else:
            model.forward_window(window[0].materialize(), window[1])
    assert ops.rng_state()["calls"] > before


@pytest.mark.parametrize("kind", ["mcat", "ge_nacagat"])
def test_a_resumed_run_is_the_uninterrupted_run(dev, kind, tmp_path, generator):
    cfg = config(kind, epochs=4, out=tmp_path, checkpoint_epoch=2, **CASES[kind])
    runs = []
    for _ in range(2):
        fresh()
        runs.append(hand_loop(kind, dev, cfg, SPLIT.train, SPLIT.val))
    fresh()
    model = build(kind, dev)
    f = fit.Fit(model, cohort_of(kind, dev), SPLIT.train, SPLIT.val, fit.fit_options(cfg, kind), sample_rows=K, seed=PLAN_SEED,
                stamp=STAMP, warmup=1)
    saved = [f.epoch().checkpoint for _ in range(2)]
    path = os.path.join(str(tmp_path), "checkpoints", f"{NAMES[kind]}_SYN-OV_E2_{STAMP}.pt")
    assert saved == [None, path] and os.listdir(os.path.dirname(path)) == [os.path.basename(path)]
    assert checkpoint.peek(path)["epoch"] == 1 and checkpoint.peek(path)["mpo"]["graph_rng_base"] == f.step.rng_base
    move_the_counter(kind, dev, model)
    ops.set_rng_epoch(None)                                           # a new process has no epoch tensor yet
    f2, res = fit_run(kind, dev, cfg, SPLIT.train, SPLIT.val, weights=WEIGHTS + 1, resume=path)
    assert f2.first_epoch == 2 and res.epochs_run == [2, 3] and f2.step.rng_base == f.step.rng_base
    assert bool(torch.isnan(res.history[:2]).all())
    want = [runs[0][0][2:]] + list(runs[0][1]) + list(runs[0][2])
    again = [runs[1][0][2:]] + list(runs[1][1]) + list(runs[1][2])
    hold(f"resume {kind}", want, again, [res.history[2:]] + final_tensors(kind, res.final) + state(f2.opt))
    # the reference's `epoch != 0`: at checkpoint_epoch = 1 the first epoch writes no file
    fresh()
    every = config(kind, epochs=2, out=tmp_path / "every", checkpoint_epoch=1)
    fit_run(kind, dev, every, SPLIT.train, SPLIT.val)
    assert os.listdir(tmp_path / "every" / "checkpoints") == [f"{NAMES[kind]}_SYN-OV_E2_{STAMP}.pt"]


# ------------------------------------------------------------------------------------------------ 4. leave-one-out
@pytest.mark.parametrize("kind", ["nacagat", "ge_nacagat"])
def test_leave_one_out_files(dev, kind, tmp_path, generator):
    patient = PATIENTS[SPLIT.train[0]]
    split = fit.split_patients(PATIENTS, 0.8, leave_one_out=patient, seed=7)
    assert len(split.test) == 2 and len(split.train) == 8 and split.val == SPLIT.val
    cfg = config(kind, epochs=3, out=tmp_path, leave_one_out=patient, output_attn_epoch=2, checkpoint_epoch=2)
    fresh()
    model, cohort = build(kind, dev), cohort_of(kind, dev)
    f = fit.Fit(model, cohort, split.train, split.val, fit.fit_options(cfg, kind), sample_rows=K, seed=PLAN_SEED, stamp=STAMP,
                warmup=1, test_ids=split.test)
    assert f.evaluator.ids == split.val
    results = [f.epoch() for _ in range(3)]
    for r in results:
        assert not set(r.ids_run.tolist()) & set(split.test) and set(r.ids_run.tolist()) <= set(split.train)
        assert [s["id"] for s in r.test] == split.test
    head = "ATTN" if kind == "ge_nacagat" else f"ATTN_{NAMES[kind]}"
    names = [f"{head}_{patient}_{STAMP}_E2_{i}.pt" for i in split.test]
    out_dir = tmp_path / "outputs"
    assert sorted(os.listdir(out_dir)) == sorted(names)                               # epoch 2 only, one per test slide
    assert [s.get("file") for s in results[1].test] == [str(out_dir / n) for n in names]
    assert all("file" not in s for r in (results[0], results[2]) for s in r.test)
    # the files hold the maps of the parameters of that epoch's checkpoint
    then = build(kind, dev, WEIGHTS + 2)
    checkpoint.load(results[1].checkpoint, then)
    key = "path" if kind == "ge_nacagat" else "coattn"
    maps = (harness.test_ge if kind == "ge_nacagat" else harness.test)(then, cohort, split.test)
    for name, slide in zip(names, maps):
        stored = torch.load(out_dir / name, weights_only=True)
        assert stored.shape == slide[key].shape and torch.equal(stored, slide[key].cpu()), name


# ------------------------------------------------------------------------------------------------ 5. keep_best
@pytest.mark.parametrize("kind,metric", [("mcat", "val_c_index"), ("mcat", "val_loss"), ("ge_nacagat", "val_accuracy"),
                                         ("ge_nacagat", "val_loss")])
def test_keep_best(dev, kind, metric, generator):
    fresh()
    model = build(kind, dev)
    # (a small rate for the loss: at 1e-3 the ten training slides are overfitted within the first epoch)
    cfg = config(kind, epochs=4, lr=1e-4 if metric == "val_loss" else 1e-3)
    f = fit.Fit(model, cohort_of(kind, dev), SPLIT.train, SPLIT.val, fit.fit_options(cfg, kind), sample_rows=K, seed=PLAN_SEED,
                stamp=STAMP, warmup=1, keep_best=metric)
    then = []
    for _ in range(4):
        f.epoch()
        then.append(f.opt.flat_p.clone())
    res = f.run()                                                     # no epoch is left: the final validation alone
    column = [row[metric] for row in res.table()]
    best = max(column) if fit.LARGER_IS_BETTER[metric] else min(column)
    assert int(res.best_epoch) == column.index(best)                  # the first arg-best: a tie keeps the earlier epoch
    print(f"[fit keep_best {kind} {metric}] {column} -> epoch {int(res.best_epoch)}")
    assert torch.equal(f.opt.flat_p, then[3]) and not torch.equal(then[0], then[3])
    ptr = f.opt.flat_p.data_ptr()
    res.restore_best()
    assert f.opt.flat_p.data_ptr() == ptr and torch.equal(f.opt.flat_p, then[int(res.best_epoch)])


def test_a_nan_metric_never_becomes_the_best(dev, generator):
    """One validation slide with a NaN feature: every epoch's val_loss is NaN, nothing improves, restore_best leaves the
    parameters alone."""
    slides = [dict(s) for s in slides_of("mcat")]
    bad = SPLIT.val[1]
    slides[bad]["wsi"] = slides[bad]["wsi"].clone()
    slides[bad]["wsi"][3, 5] = float("nan")
    cohort = harness.ResidentCohort(slides, dev, cycle=True)
    fresh()
    f = fit.Fit(build("mcat", dev), cohort, SPLIT.train, SPLIT.val, fit.fit_options(config("mcat", epochs=2), "mcat"),
                sample_rows=K, seed=PLAN_SEED, stamp=STAMP, warmup=1, keep_best="val_loss")
    res = f.run()
    table = res.table()
    assert all(row["val_loss"] != row["val_loss"] for row in table) and all(row["train_loss"] == row["train_loss"] for row in table)
    after = f.opt.flat_p.clone()
    res.restore_best()
    assert int(res.best_epoch) == -1 and torch.equal(f.opt.flat_p, after)


# ------------------------------------------------------------------------------------------------ 6. patience
@pytest.mark.parametrize("kind", ["mcat", "ge_nacagat"])
def test_patience_stops_the_run(dev, kind, generator):
    """lr = 0: every epoch validates to the same bits, nothing improves after epoch 0, patience 2 stops after epoch 2."""
    fresh()
    logged = []
    f, res = fit_run(kind, dev, config(kind, epochs=6, lr=0.0), SPLIT.train, SPLIT.val, keep_best="val_loss", patience=2,
                     log=logged.append)
    assert res.stopped_early and res.epochs_run == [0, 1, 2] and int(res.best_epoch) == 0
    assert logged == [{**row, "leftover": 2} for row in res.table()[:3]]          # log: the epoch's row of the table
    assert bool(torch.isfinite(res.history[:3]).all()) and bool(torch.isnan(res.history[3:]).all())
    assert torch.equal(res.history[0, 3:], res.history[1, 3:]) and torch.equal(res.history[0, 3:], res.history[2, 3:])
    with pytest.raises(ValueError, match="the run is over"):
        f.epoch()


# ------------------------------------------------------------------------------------------------ 7. a world of two, and of one
WORLD = 2
N_RANK = 2                  # slides per rank and window
SEED_BASE = 4300            # torch.manual_seed(SEED_BASE + rank) before the capture


def world_plan(kind):
    """Train and validation slides dealt to the ranks by dp.shard_slides: per rank the GLOBAL slide ids of its cohort --
    its train shard, then its validation shard -- and the shard sizes."""
    slides = slides_of(kind)
    train = dp.shard_slides([int(slides[i]["wsi"].shape[0]) for i in SPLIT.train], WORLD)
    val = dp.shard_slides([int(slides[i]["wsi"].shape[0]) for i in SPLIT.val], WORLD)
    per_rank = [[SPLIT.train[i] for i in train[r]] + [SPLIT.val[i] for i in val[r]] for r in range(WORLD)]
    return per_rank, [len(s) for s in train], [len(s) for s in val]


def hand_loop_dp(kind, dev, cfg, cohort, train_ids, val_ids, train_sizes, val_sizes, rank):
    """INTEGRATION.md section 5's data-parallel loop, one rank's program."""
    ge = kind == "ge_nacagat"
    o = harness.training_options(cfg["training"], kind)
    model = build(kind, dev)
    bucket = FlatGradBucket(list(model.parameters()))
    opt = o.make_optimizer(bucket)
    sched = o.make_scheduler(opt)
    dist.broadcast(opt.flat_p, src=0)
    first = train_ids[:N_RANK]
    kw = dict(l1=o.l1) if ge else dict(split_patch_grad=True, **o.train_kwargs())
    step = harness.GraphedWindowStep(model, bucket, cohort.window(int32(first, dev), first), N_RANK, opt=None, warmup=1,
                                     sample_rows=K, **kw)
    if ge:
        evaluator = harness.GeCohortEvaluator(model, cohort, val_ids, l1=o.l1, capture=True)
    else:
        evaluator = harness.CohortEvaluator(model, cohort, val_ids, loss=o.loss, alpha=o.alpha, lambda_reg=o.lambda_reg, l1=o.l1,
                                            capture=True)
    rows = []
    for epoch in range(cfg["training"]["epochs"]):
        orders, n_windows = dp.epoch_orders(train_sizes, N_RANK, PLAN_SEED, epoch)
        order = [train_ids[i] for i in orders[rank]]
        lr = opt.lr_dev.double()
        out = harness.train_epoch_dp(step, cohort, order, opt, n_windows)
        loss = dp.gather_ragged(out[0], [n_windows * N_RANK] * WORLD)
        train = [loss.mean(0, keepdim=True).double()]
        if not ge:
            train.append(harness.epoch_c_index_dp(cohort, out[2], out[1])[0])
        if sched:
            sched.step()
        r = harness.validate_dp(evaluator, val_sizes)
        val = [r.mean_loss.double(), r.accuracy, r.balanced_accuracy] if ge else [r.mean_loss.double(), r.c_index]
        rows.append(torch.cat([lr] + train + val))
    return torch.stack(rows), final_tensors(kind, harness.validate_dp(evaluator, val_sizes)), state(opt)


def _world_worker(rank, world, kind, out):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    per_rank, train_sizes, val_sizes = world_plan(kind)
    slides = slides_of(kind)
    cls = harness.GeResidentCohort if kind == "ge_nacagat" else harness.ResidentCohort
    cohort = cls([slides[i] for i in per_rank[rank]], dev, cycle=True)
    train_ids = list(range(train_sizes[rank]))
    val_ids = list(range(train_sizes[rank], train_sizes[rank] + val_sizes[rank]))
    cfg = config(kind, epochs=3, out=f"{out}.dir", checkpoint_epoch=2, grad_acc_step=N_RANK, **CASES[kind])
    runs = []
    for _ in range(0 if kind == "nacagat" else 2):
        fresh(SEED_BASE + rank)
        runs.append(whole(*hand_loop_dp(kind, dev, cfg, cohort, train_ids, val_ids, train_sizes, val_sizes, rank)))
    fresh(SEED_BASE + rank)
    f = fit.Fit(build(kind, dev), cohort, train_ids, val_ids, fit.fit_options(cfg, kind), sample_rows=K, seed=PLAN_SEED,
                stamp=STAMP, warmup=1, group=dist.group.WORLD, train_shard_sizes=train_sizes, val_shard_sizes=val_sizes)
    written = [f.epoch().checkpoint for _ in range(3)]
    res = f.run()
    got = whole(res.history, final_tensors(kind, res.final), state(f.opt))
    torch.cuda.synchronize(dev)
    torch.save({"loops": [[t.cpu() for t in run] for run in runs], "fit": [t.cpu() for t in got],
                "flat_p": f.opt.flat_p.cpu(), "history": res.history.cpu(), "epochs_run": res.epochs_run,
                "leftover": res.leftover, "written": written}, f"{out}.{rank}")


@pytest.mark.timeout(420)
@pytest.mark.parametrize("kind", KINDS)
def test_a_world_of_two(dev, tmp_path, kind):
    """Two ranks on one card (gloo), shards of 5 train and 2 validation slides each, windows of 2 slides per rank: fit on
    both ranks against section 5's loop in the same children.  NaCAGaT is held to the two exact properties alone (NOTES.md,
    under tests/test_gpu_dp_epoch.py: its trajectory amplifies last-bit differences some 500 times within a step)."""
    per_rank, train_sizes, val_sizes = world_plan(kind)
    assert train_sizes == [5, 5] and val_sizes == [2, 2] and sorted(i for ids in per_rank for i in ids) == sorted(SPLIT.train + SPLIT.val)
    out = str(tmp_path / "world.pt")
    run_world(_world_worker, WORLD, kind, out, limit=360.0)
    got = [torch.load(f"{out}.{r}", weights_only=True) for r in range(WORLD)]
    assert torch.equal(got[0]["flat_p"].view(torch.int32), got[1]["flat_p"].view(torch.int32))      # replicas, bit for bit
    assert torch.equal(got[0]["history"].view(torch.int64), got[1]["history"].view(torch.int64))    # and one history
    for g in got:
        assert g["epochs_run"] == [0, 1, 2] and g["leftover"] == 1 and bool(torch.isfinite(g["history"]).all())
    path = os.path.join(f"{out}.dir", "checkpoints", f"{NAMES[kind]}_SYN-OV_E2_{STAMP}.pt")
    assert got[0]["written"] == [None, path, None] and got[1]["written"] == [None] * 3          # one writer: rank 0
    assert os.listdir(os.path.dirname(path)) == [os.path.basename(path)]
    if kind != "nacagat":
        for rank, g in enumerate(got):
            hold(f"world of two, {kind}, rank {rank}", g["loops"][0], g["loops"][1], g["fit"])


@pytest.mark.parametrize("kind", ["mcat", "ge_nacagat"])
def test_a_world_of_one_is_the_single_process(dev, kind, generator):
    """Shard sizes and no process group: the data-parallel path (the optimiser outside the graph, train_epoch_dp,
    validate_dp) over the same orders, against the single-process fit run twice."""
    cfg = config(kind, epochs=3, **CASES[kind])
    runs = []
    for sizes in ({}, {}, dict(train_shard_sizes=[len(SPLIT.train)], val_shard_sizes=[len(SPLIT.val)])):
        fresh()
        f, res = fit_run(kind, dev, cfg, SPLIT.train, SPLIT.val, **sizes)
        assert f.dp == bool(sizes) and (f.step.opt is None) == bool(sizes)
        runs.append(whole(res.history, final_tensors(kind, res.final), state(f.opt)))
    hold(f"world of one, {kind}", *runs)


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_come_before_any_capture(dev, generator):
    fresh()
    cohort, ge_cohort = cohort_of("mcat", dev), cohort_of("ge_nacagat", dev)
    model, ge_model = build("mcat", dev), build("ge_nacagat", dev)
    o, ge_o = fit.fit_options(config("mcat"), "mcat"), fit.fit_options(config("ge_nacagat"), "ge_nacagat")
    params = [p.data_ptr() for p in model.parameters()]
    before = ops.rng_state()

    def refused(match, *args, **kwargs):
        kwargs = {"sample_rows": K, "warmup": 1, **kwargs}
        with pytest.raises(ValueError, match=match):
            fit.Fit(*args, **kwargs)

    train, val = SPLIT.train, SPLIT.val
    refused("train_ids and val_ids overlap", model, cohort, train, val + train[:1], o)
    refused("train_ids and test_ids overlap", model, cohort, train, val, o, test_ids=train[2:3], test_patient="P")
    refused("val_ids and test_ids overlap", model, cohort, train[:8], val, o, test_ids=val[:1], test_patient="P")
    refused("train_ids names a slide twice", model, cohort, train + train[:1], val, o)
    refused("val_ids names slide 14, outside the cohort's 14 slides", model, cohort, train, [14], o)
    refused("train_ids holds 3 slides, fewer than one window of grad_acc_step = 4", model, cohort, train[:3], val, o)
    refused("cohort is a GeResidentCohort; the survival model", model, ge_cohort, train, val, o)
    refused("cohort is a ResidentCohort; the gene-expression model", ge_model, cohort, train, val, ge_o)
    refused("options were read for 'nacagat', the model is 'mcat'", model, cohort, train, val,
            fit.fit_options(config("nacagat"), "nacagat"))
    refused("patience counts epochs without improvement of the keep_best metric", model, cohort, train, val, o, patience=2)
    refused("keep_best = 'val_accuracy' is not a validation metric of 'mcat'", model, cohort, train, val, o, keep_best="val_accuracy")
    refused("keep_best = 'val_c_index' is not a validation metric of 'ge_nacagat'", ge_model, ge_cohort, train, val, ge_o,
            keep_best="val_c_index")
    refused("keep_best = 'train_loss' is not a validation metric", model, cohort, train, val, o, keep_best="train_loss")
    refused("test_ids without test_patient", model, cohort, train[:8], val, o, test_ids=train[8:])
    refused(r"train_shard_sizes = \[5, 5\] for a world of 1", model, cohort, train, val, o, train_shard_sizes=[5, 5],
            val_shard_sizes=[4])
    refused(r"train_shard_sizes = \[9\] for a world of 1 whose rank 0 holds 10", model, cohort, train, val, o,
            train_shard_sizes=[9], val_shard_sizes=[4])
    refused(r"val_shard_sizes = \[3\] for a world of 1 whose rank 0 holds 4", model, cohort, train, val, o,
            train_shard_sizes=[10], val_shard_sizes=[3])
    refused("a data-parallel run needs val_shard_sizes", model, cohort, train, val, o, train_shard_sizes=[10])
    no_lap = harness.ResidentCohort(slides_of("mcat"), dev)
    short = min(i for i in train if no_lap.lengths[i] < 100)
    refused(f"sample_rows = 100, but slide {short} has", model, no_lap, train, val, o, sample_rows=100)
    assert ops.rng_state() == before and ops._rng_epoch_tensor is None
    assert [p.data_ptr() for p in model.parameters()] == params      # nothing was re-pointed: no optimiser was built
