"""Data-parallel epochs over a sharded resident cohort (dp.shard_slides / epoch_orders / global_order / gather_ragged,
harness.train_epoch_dp, epoch_c_index_dp, validate_dp) at world size 2 on ONE card: two ranks against one process over
the same global windows, replicas bit for bit, a mismatched plan refused instead of hung, a corrupt slide skipping the
step on every rank, ranks drawing different rows, sharded validation against the fp64 oracle, the gene-expression model.

Backend gloo, as tests/test_gpu_dp.py (RCCL refuses two ranks on one device; gloo stages through the host and moves the
same slices) -- the nccl leg is the same calls and is exercised by multi-GPU bench runs alone.  Two children + this
process use the card.  tests/dp_spawn.py says how trouble ends a test.  Bars restated from tests/test_gpu_dp.py (the
same comparison after two optimiser steps) and tests/test_gpu_validate.py (BAR, imported)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.distributed as dist

import test_gpu_cohort_sampling as CS
import test_gpu_ge_cohort as G
import test_gpu_validate as V
from dp_spawn import run_world
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import dp, harness, ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.dp import FlatGradBucket, FlatOptimizer

pytestmark = pytest.mark.gpu

WORLD = 2
LR, WD, L1 = 1e-3, 1e-5, 1e-4
SEED_BASE = 4100            # torch.manual_seed(SEED_BASE + rank) before the capture
PLAN_SEED = 17              # dp.epoch_orders' seed
K, N = 256, 2               # case 1: slides of exactly K rows, N per rank and window
GE_K = 64


def fusion_setup(kind, dev, **guard):
    model = CS.fusion_model(kind, dev)                     # bf16, omic_sizes [64] * 6, every dropout site at 0, training mode
    bucket = FlatGradBucket(list(model.parameters()))
    return model, bucket, FlatOptimizer(bucket, "adam", lr=LR, weight_decay=WD, **guard)


def whole_slide_cohort():
    return syn.make_cohort(8, K, K, CS.SIZES, 310)


def epoch_plan(n_slides, rows, n):
    shards = dp.shard_slides([rows] * n_slides, WORLD)
    orders, n_windows = dp.epoch_orders([len(s) for s in shards], n, PLAN_SEED, 0)
    return shards, orders, n_windows


def start(rank):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ops.set_rng_epoch(None)
    torch.manual_seed(SEED_BASE + rank)
    return dev


def optimiser_state(opt):
    return {"params": opt.flat_p.cpu(), "state1": opt.state1.cpu(), "state2": opt.state2.cpu(), "t": opt.t_dev.cpu()}


def counts_by_numpy(cens, time, risk):
    """concordant, tied, comparable over every ordered pair (tests/test_gpu_concordance.py's host form)."""
    cens, time, risk = cens.numpy().astype(np.float32), time.numpy().astype(np.float64), risk.numpy().astype(np.float64)
    event = (np.float32(1.0) - cens) != 0
    comparable = event[:, None] & ((time[None, :] > time[:, None]) | ((time[None, :] == time[:, None]) & ~event[None, :]))
    np.fill_diagonal(comparable, False)
    diff = risk[:, None] - risk[None, :]
    tie = np.abs(diff) <= 1e-8
    return [int((comparable & (diff > 0) & ~tie).sum()), int((comparable & tie).sum()), int(comparable.sum())]


def assert_replicas_equal(a, b):
    for name in ("params", "state1", "state2", "t"):
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name


def load(out):
    return [torch.load(f"{out}.{r}", weights_only=True) for r in range(WORLD)]


# ------------------------------------------------------------------------------------------------ 1. two ranks against one process
def _epoch_worker(rank, world, kind, split, out):
    dev = start(rank)
    slides = whole_slide_cohort()
    shards, orders, n_windows = epoch_plan(len(slides), K, N)
    model, bucket, opt = fusion_setup(kind, dev, l1_lambda=L1)
    dist.broadcast(opt.flat_p, src=0)
    cohort = harness.ResidentCohort([slides[i] for i in shards[rank]], dev)
    first = orders[rank][:N]
    step = harness.GraphedWindowStep(model, bucket, cohort.window(CS.int32(first, dev), first), N, opt=None, warmup=1,
                                     split_patch_grad=split, sample_rows=K, l1=L1)
    loss, risk, ids_run, leftover = harness.train_epoch_dp(step, cohort, orders[rank], opt, n_windows)
    c_index, counts = harness.epoch_c_index_dp(cohort, ids_run, risk)
    sizes = [n_windows * N] * world
    ids = ids_run.long()
    gathered = {name: dp.gather_ragged(t, sizes).cpu() for name, t in
                (("loss", loss), ("risk", risk), ("cens", cohort.censorship[ids]), ("months", cohort.survival_months[ids]))}
    torch.cuda.synchronize(dev)
    torch.save({"grads": bucket.flat.cpu(), **optimiser_state(opt), **gathered, "c_index": c_index.cpu(), "counts": counts.cpu(),
                "leftover": leftover, "ids_run": ids_run.cpu()}, f"{out}.{rank}")


@pytest.mark.timeout(420)
@pytest.mark.parametrize("kind,split", [("mcat", True), ("mcat", False)], ids=["mcat_split", "mcat_whole_bucket"])
def test_two_rank_epoch_equals_one_process(dev, tmp_path, kind, split):
    """8 slides of exactly K rows (every sample is the whole slide in permuted order; the models are permutation-invariant up
    to rounding), 2 per rank and window, two windows: train_epoch_dp on two ranks against train_epoch in one process -- the
    optimiser inside the graph, 4-slide windows -- over dp.global_order of the same plan.  Adam with an L1 penalty: a wrong
    l1_slides moves every entry's update.  Measured: gradient error 3.8e-6 (split) and 1.4e-5 (whole bucket) of the largest
    entry, no parameter off by lr / 2.
    MCAT, as in tests/test_gpu_dp.py, whose bars these are.  NaCAGaT's trajectory amplifies last-bit differences some 500
    times within one optimiser step (tests/test_gpu_cohort.py says where that comes from): the same comparison measured
    1.84e-3 against the 2e-3 bar, with atomically summed gradients on both sides -- no bar for a test that must pass every
    time.  NaCAGaT runs train_epoch_dp with the split exchange in test_ranks_draw_different_rows, on exact properties."""
    out = str(tmp_path / "epoch.pt")
    run_world(_epoch_worker, WORLD, kind, split, out, limit=360.0)
    got = load(out)
    slides = whole_slide_cohort()
    shards, orders, n_windows = epoch_plan(len(slides), K, N)
    assert n_windows == 2 and [len(s) for s in shards] == [4, 4]
    assert_replicas_equal(got[0], got[1])
    assert int(got[0]["t"]) == n_windows
    n_run = n_windows * N
    for rank, g in enumerate(got):
        assert g["leftover"] == orders[rank][n_run:] and g["ids_run"].tolist() == orders[rank][:n_run]
        for name in ("loss", "risk"):
            assert g[name].shape == (n_run * WORLD,) and bool(torch.isfinite(g[name]).all()), name
        assert g["counts"].tolist() == counts_by_numpy(g["cens"], g["months"], g["risk"])
    for name in ("loss", "risk", "cens", "months", "counts"):
        assert torch.equal(got[0][name], got[1][name]), name
    assert torch.equal(got[0]["c_index"].view(torch.int64), got[1]["c_index"].view(torch.int64))
    if int(got[0]["counts"][2]):
        host = harness.concordance_index_censored(1 - got[0]["cens"].numpy(), got[0]["months"].numpy(), got[0]["risk"].numpy())
        assert abs(float(got[0]["c_index"]) - host) <= 1e-15
    # the gathered values are rank-major: rank 0's slides in the order they ran, then rank 1's
    ran = [shards[r][i] for r in range(WORLD) for i in orders[r][:n_run]]
    assert got[0]["cens"].tolist() == [float(slides[i]["censorship"]) for i in ran]

    ops.set_rng_epoch(None)
    try:
        model, bucket, opt = fusion_setup(kind, dev, l1_lambda=L1)
        cohort = harness.ResidentCohort(slides, dev)
        order = dp.global_order(orders, shards, N, n_windows)
        first = order[:N * WORLD]
        step = harness.GraphedWindowStep(model, bucket, cohort.window(CS.int32(first, dev), first), N * WORLD, opt=opt, warmup=1,
                                         sample_rows=K)
        _, _, ids_run, leftover = harness.train_epoch(step, cohort, order)
        torch.cuda.synchronize(dev)
        assert leftover == [] and ids_run.tolist() == order and int(opt.t_dev) == n_windows
        g_ref, p_ref = bucket.flat.cpu(), opt.flat_p.cpu()
    finally:
        ops.set_rng_epoch(None)
    # the bars of tests/test_gpu_dp.py: gradients of the second step relative to the largest entry; parameters after two
    # Adam steps, whose entries with a ~0 gradient move by rounding noise -- the bulk must agree far below one step's size
    err = float((got[0]["grads"] - g_ref).abs().max() / g_ref.abs().max())
    d = (got[0]["params"] - p_ref).abs()
    off = float((d > 0.5 * LR).float().mean())
    print(f"[dp epoch {kind} split={split}] grad err {err:.2e}, param diff median {float(d.median()):.2e} (lr {LR}), "
          f"off by more than lr / 2: {off:.3%}")
    assert err < 2e-3, err
    assert float(d.median()) < 1e-2 * LR, float(d.median())
    assert off < 0.01, off


# ------------------------------------------------------------------------------------------------ 2. mismatched plans are refused
def test_a_plan_the_order_cannot_fill_is_refused_before_anything_runs(dev):
    """One process, no group: n_windows beyond what the order holds raises before the first replay (and so, in a world,
    before the first collective); the same step then runs one window of a longer order and hands back the rest."""
    ops.set_rng_epoch(None)
    try:
        model, bucket, opt = fusion_setup("mcat", dev)
        cohort = harness.ResidentCohort(whole_slide_cohort()[:4], dev)
        step = harness.GraphedWindowStep(model, bucket, cohort.window(CS.int32([0, 1], dev), [0, 1]), N, opt=None, warmup=1,
                                         sample_rows=K)
        before = opt.flat_p.clone()
        with pytest.raises(ValueError, match="2 windows of 2 slides need 4 ids, the order holds 3"):
            harness.train_epoch_dp(step, cohort, [0, 1, 2], opt, 2)
        with pytest.raises(ValueError, match="slide id 4 outside the cohort's 4 slides"):
            harness.train_epoch_dp(step, cohort, [0, 1, 2, 4], opt, 1)
        opt.l1_lambda = 1e-3                    # (the step was captured with l1 = 0: its reported loss carries no penalty)
        try:
            with pytest.raises(ValueError, match="l1 = 0.0, the optimiser folds its gradient with l1_lambda = 0.001"):
                harness.train_epoch_dp(step, cohort, [0, 1], opt, 1)
        finally:
            opt.l1_lambda = 0.0
        torch.cuda.synchronize(dev)
        assert int(opt.t_dev) == 0 and torch.equal(opt.flat_p, before)
        loss, risk, ids_run, leftover = harness.train_epoch_dp(step, cohort, [3, 1, 0, 2], opt, 1)
        torch.cuda.synchronize(dev)
        assert leftover == [0, 2] and ids_run.tolist() == [3, 1] and ids_run.dtype == torch.int32
        assert loss.shape == risk.shape == (2,) and bool(torch.isfinite(loss).all()) and bool(torch.isfinite(risk).all())
        assert int(opt.t_dev) == 1 and not torch.equal(opt.flat_p, before)
        c_index, counts = harness.epoch_c_index_dp(cohort, ids_run, risk)              # world 1: the rank's own slides
        assert counts.tolist() == counts_by_numpy(cohort.censorship[ids_run.long()].cpu(), cohort.survival_months[ids_run.long()].cpu(),
                                                  risk.cpu())
    finally:
        ops.set_rng_epoch(None)


# ------------------------------------------------------------------------------------------------ 3. a corrupt slide
PLANTED = 2                 # rank 1's local slide with a NaN feature: in the second window of [0, 1 | 2, 3]


def _corrupt_worker(rank, world, out):
    dev = start(rank)
    slides = whole_slide_cohort()
    shards = dp.shard_slides([K] * len(slides), world)
    mine = [dict(slides[i]) for i in shards[rank]]
    if rank == 1:
        mine[PLANTED]["wsi"] = mine[PLANTED]["wsi"].clone()
        mine[PLANTED]["wsi"][5, 7] = float("nan")
    model, bucket, opt = fusion_setup("mcat", dev, skip_nonfinite=True)
    dist.broadcast(opt.flat_p, src=0)
    cohort = harness.ResidentCohort(mine, dev)
    step = harness.GraphedWindowStep(model, bucket, cohort.window(CS.int32([0, 1], dev), [0, 1]), N, opt=None, warmup=1,
                                     split_patch_grad=True, sample_rows=K)
    start_params = opt.flat_p.cpu()
    harness.train_epoch_dp(step, cohort, [0, 1], opt, 1)
    torch.cuda.synchronize(dev)
    before = optimiser_state(opt)
    skipped_before = int(opt.skipped_steps)
    loss, _, _, _ = harness.train_epoch_dp(step, cohort, [PLANTED, 3], opt, 1)
    torch.cuda.synchronize(dev)
    torch.save({"start": start_params, "before": before, "after": optimiser_state(opt), "skipped_before": skipped_before,
                "skipped": int(opt.skipped_steps), "loss": loss.cpu()}, f"{out}.{rank}")


@pytest.mark.timeout(420)
def test_a_corrupt_slide_skips_the_step_on_every_rank(dev, tmp_path):
    out = str(tmp_path / "corrupt.pt")
    run_world(_corrupt_worker, WORLD, out, limit=360.0)
    got = load(out)
    assert not bool(torch.isfinite(got[1]["loss"]).all()) and bool(torch.isfinite(got[0]["loss"]).all())   # rank 0's own slides are clean
    for g in got:
        assert g["skipped_before"] == 0 and g["skipped"] == 1
        assert not torch.equal(g["before"]["params"], g["start"])                      # the clean window did step
        assert_replicas_equal(g["before"], g["after"])                                 # the corrupt one wrote nothing: moments and count too
        assert int(g["after"]["t"]) == 1 and bool(torch.isfinite(g["after"]["params"]).all())
    assert_replicas_equal(got[0]["after"], got[1]["after"])


# ------------------------------------------------------------------------------------------------ 4. ranks draw different rows
DRAW_ROWS, DRAW_K = 300, 64


def _draw_worker(rank, world, out):
    dev = start(rank)
    slides = syn.make_cohort(4, DRAW_ROWS, DRAW_ROWS, CS.SIZES, 320)
    shards = dp.shard_slides([DRAW_ROWS] * 4, world)
    model, bucket, opt = fusion_setup("nacagat", dev)
    dist.broadcast(opt.flat_p, src=0)
    cohort = harness.ResidentCohort([slides[i] for i in shards[rank]], dev)
    step = harness.GraphedWindowStep(model, bucket, cohort.window(CS.int32([0, 1], dev), [0, 1]), N, opt=None, warmup=1,
                                     split_patch_grad=True, sample_rows=DRAW_K)
    start_params = opt.flat_p.cpu()
    harness.train_epoch_dp(step, cohort, [1, 0], opt, 1)
    torch.cuda.synchronize(dev)
    seed, offset = step.sampler.last_stream
    torch.save({"seed": seed, "offset": offset, "epoch": int(step.epoch), "rows": step.sampler.out.cpu(),
                "slides": [cohort.rows[i].cpu() for i in (1, 0)], "start": start_params, **optimiser_state(opt)}, f"{out}.{rank}")


def host_indices(lengths, k, seed, offset, epoch):
    """(n_slides, k) int32 from the library's host entry (tests/test_row_sampling_cpu.py): row b = pi_b(0 .. k-1)."""
    n = len(lengths)
    ln = (ctypes.c_int32 * n)(*lengths)
    idx = (ctypes.c_int32 * (n * k))()
    L.call("mpo_bag_sample_indices_host", ctypes.addressof(ln), n, k, seed, offset, epoch, ctypes.addressof(idx))
    return np.ctypeslib.as_array(idx).reshape(n, k).copy()


@pytest.mark.timeout(420)
def test_ranks_draw_different_rows(dev, tmp_path):
    """torch.manual_seed(SEED_BASE + rank) before the capture: the two ranks' samplers run on different seeds, and for
    slides of one length at one window position the INDICES they draw differ (the library's host form of the draw, which
    each rank's gathered rows are first shown to follow bit for bit -- indices, not values that could collide).  NaCAGaT
    with the split exchange: the replicas, fed different rows, still hold the same bits after the step."""
    out = str(tmp_path / "draw.pt")
    run_world(_draw_worker, WORLD, out, limit=360.0)
    got = load(out)
    assert_replicas_equal(got[0], got[1])
    assert int(got[0]["t"]) == 1 and not torch.equal(got[0]["params"], got[0]["start"])
    assert bool(torch.isfinite(got[0]["params"]).all())
    drawn = []
    for rank, g in enumerate(got):
        assert g["seed"] == SEED_BASE + rank
        idx = host_indices([DRAW_ROWS] * N, DRAW_K, g["seed"], g["offset"], g["epoch"])
        assert idx.min() >= 0 and idx.max() < DRAW_ROWS
        for b in range(N):
            want = g["slides"][b][torch.from_numpy(idx[b]).long()]
            assert CS.same_bits(g["rows"][b * DRAW_K:(b + 1) * DRAW_K], want), (rank, b)
        drawn.append(idx)
    assert got[0]["offset"] == got[1]["offset"] and got[0]["epoch"] == got[1]["epoch"]       # the seed alone separates them
    for b in range(N):
        assert not np.array_equal(drawn[0][b], drawn[1][b]), b
        assert not np.array_equal(np.sort(drawn[0][b]), np.sort(drawn[1][b])), b              # other rows, not another order


# ------------------------------------------------------------------------------------------------ 5. sharded validation
VAL_IDS = list(range(13))   # an odd subset of tests/test_gpu_validate.py's 14 slides: shards of 7 and 6
RESULT = ("loss", "risk", "hazards", "survs", "Y", "mean_loss", "c_index", "counts")


def _validate_worker(rank, world, kind, out):
    dev = start(rank)
    slides = V.slides_once()
    shards = dp.shard_slides([V.LENGTHS[i] for i in VAL_IDS], world)
    sizes = [len(s) for s in shards]
    model = V.build(kind, "bf16", dev)
    cohort = harness.ResidentCohort([slides[VAL_IDS[i]] for i in shards[rank]], dev, slab_bytes=V.SLAB_ROWS * 2048)
    saved = {}
    for capture in (False, True):
        ev = harness.CohortEvaluator(model, cohort, list(range(sizes[rank])), capture=capture)
        r = harness.validate_dp(ev, sizes)
        saved[capture] = {name: getattr(r, name).cpu() for name in RESULT}
        saved[capture]["cens"] = dp.gather_ragged(ev.censorship, sizes).cpu()
        saved[capture]["months"] = dp.gather_ragged(ev.survival_months, sizes).cpu()
    with pytest.raises(ValueError, match="validate_dp: sizes"):                       # refused before any collective: on every rank
        harness.validate_dp(ev, [sizes[0] + 1, sizes[1] + 1])
    torch.cuda.synchronize(dev)
    torch.save({"eager": saved[False], "captured": saved[True]}, f"{out}.{rank}")


@pytest.mark.timeout(420)
@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_sharded_validation_matches_the_oracle_on_every_rank(tmp_path, dev, kind):
    out = str(tmp_path / "validate.pt")
    run_world(_validate_worker, WORLD, kind, out, limit=360.0)
    got = load(out)
    shards = dp.shard_slides([V.LENGTHS[i] for i in VAL_IDS], WORLD)
    assert sorted(len(s) for s in shards) == [6, 7]
    ids = [VAL_IDS[i] for s in shards for i in s]                                     # the union, rank-major
    o, (_, cens) = V.oracle(kind), V.targets()
    bar = V.BAR["bf16"]
    for mode in ("eager", "captured"):
        a, b = got[0][mode], got[1][mode]
        for name in RESULT + ("cens", "months"):
            assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, (mode, name)
            assert torch.equal(G.bits(a[name]), G.bits(b[name])), (mode, name)        # the same bits on both ranks
        assert a["loss"].shape == a["risk"].shape == (13,) and a["hazards"].shape == a["survs"].shape == a["Y"].shape == (13, 4)
        figures = {k: V.worst(a[k], o[k][ids]) for k in ("hazards", "survs", "Y")}
        figures["risk"] = V.worst(a["risk"], -o["survs"][ids].sum(1))
        figures["loss"] = V.worst(a["loss"], V.oracle_ces(kind, ids))
        print(f"[validate_dp {kind} {mode}] " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))
        for k, v in figures.items():
            assert v < bar, (mode, k, v)
        assert a["cens"].tolist() == cens[ids].tolist()
        assert torch.equal(a["mean_loss"], a["loss"].mean(0, keepdim=True)) and a["mean_loss"].shape == (1,)
        assert a["counts"].tolist() == counts_by_numpy(a["cens"], a["months"], a["risk"])
        host = harness.concordance_index_censored(1 - a["cens"].numpy(), a["months"].numpy(), a["risk"].numpy())
        assert a["c_index"].dtype == torch.float64 and abs(float(a["c_index"]) - host) <= 1e-15
    for name in RESULT:                                                               # (no atomics in the forward: capture changes no bit)
        assert torch.equal(G.bits(got[0]["eager"][name]), G.bits(got[0]["captured"][name])), name


# ------------------------------------------------------------------------------------------------ 6. the gene-expression model
GE_VAL_LENGTHS = [40, 17, 33, 64, 20]       # shards of 3 and 2


def ge_bags():
    return syn.make_ge_cohort(4, GE_K, GE_K, seed=330)


def ge_validation_bags():
    bags = syn.make_ge_cohort(len(GE_VAL_LENGTHS), max(GE_VAL_LENGTHS), max(GE_VAL_LENGTHS), seed=331)
    for s, m in zip(bags, GE_VAL_LENGTHS):
        s["wsi"] = s["wsi"][:m].contiguous()
    return bags


def ge_setup(dev):
    model = G.build(dev, "bf16", train=True)
    bucket = FlatGradBucket(list(model.parameters()))
    return model, bucket, FlatOptimizer(bucket, "adam", lr=LR, weight_decay=WD, l1_lambda=L1)


def _ge_worker(rank, world, out):
    dev = start(rank)
    bags = ge_bags()
    shards, orders, n_windows = epoch_plan(len(bags), GE_K, 1)
    model, bucket, opt = ge_setup(dev)
    dist.broadcast(opt.flat_p, src=0)
    cohort = harness.GeResidentCohort([bags[i] for i in shards[rank]], dev)
    first = orders[rank][:1]
    step = harness.GraphedWindowStep(model, bucket, cohort.window(CS.int32(first, dev), first), 1, opt=None, warmup=1,
                                     sample_rows=GE_K, l1=L1)
    loss, ids_run, leftover = harness.train_epoch_dp(step, cohort, orders[rank], opt, n_windows)
    val = ge_validation_bags()
    val_shards = dp.shard_slides(GE_VAL_LENGTHS, world)
    sizes = [len(s) for s in val_shards]
    val_cohort = harness.GeResidentCohort([val[i] for i in val_shards[rank]], dev)
    r = harness.validate_dp(harness.GeCohortEvaluator(model, val_cohort, list(range(sizes[rank]))), sizes)
    torch.cuda.synchronize(dev)
    torch.save({"grads": bucket.flat.cpu(), **optimiser_state(opt), "loss": loss.cpu(), "ids_run": ids_run.cpu(), "leftover": leftover,
                "val": {name: getattr(r, name).cpu() for name in G.RESULT_TENSORS}}, f"{out}.{rank}")


@pytest.mark.timeout(420)
def test_gene_expression_epoch_and_validation(dev, tmp_path):
    """4 bags of exactly GE_K rows, one per rank and window, two steps, the whole bucket in one all-reduce: against eager
    train_ge_window accumulation over the same two global windows in one process; then validate_dp over shards of 3 and 2."""
    out = str(tmp_path / "ge.pt")
    run_world(_ge_worker, WORLD, out, limit=360.0)
    got = load(out)
    bags = ge_bags()
    shards, orders, n_windows = epoch_plan(len(bags), GE_K, 1)
    assert n_windows == 2
    assert_replicas_equal(got[0], got[1])
    assert torch.equal(got[0]["grads"].view(torch.int32), got[1]["grads"].view(torch.int32))
    for rank, g in enumerate(got):
        assert g["ids_run"].tolist() == orders[rank] and g["leftover"] == [] and int(g["t"]) == 2
        assert g["loss"].shape == (2,) and bool(torch.isfinite(g["loss"]).all())
    ops.set_rng_epoch(None)
    try:
        model, bucket, opt = ge_setup(dev)
        order = dp.global_order(orders, shards, 1, n_windows)
        for w in range(n_windows):
            window = harness.make_ge_window([bags[i] for i in order[w * WORLD:(w + 1) * WORLD]], dev, torch.bfloat16)
            bucket.begin()
            harness.train_ge_window(model, *window, WORLD, l1=L1)
            bucket.finish()
            opt.step(l1_slides=WORLD)
        torch.cuda.synchronize(dev)
        g_ref, p_ref = bucket.flat.cpu(), opt.flat_p.cpu()
    finally:
        ops.set_rng_epoch(None)
    err = float((got[0]["grads"] - g_ref).abs().max() / g_ref.abs().max())
    d = (got[0]["params"] - p_ref).abs()
    off = float((d > 0.5 * LR).float().mean())
    print(f"[dp epoch ge] grad err {err:.2e}, param diff median {float(d.median()):.2e} (lr {LR}), off by more than lr / 2: {off:.3%}")
    assert err < 2e-3, err
    assert float(d.median()) < 1e-2 * LR, float(d.median())
    assert off < 0.01, off
    # validation: the same bits on both ranks, and the host form over the gathered Y, labels and losses
    val_shards = dp.shard_slides(GE_VAL_LENGTHS, WORLD)
    assert sorted(len(s) for s in val_shards) == [2, 3]
    val = ge_validation_bags()
    labels = torch.tensor([int(val[i]["gene_expr_class"]) for s in val_shards for i in s])
    a, b = got[0]["val"], got[1]["val"]
    for name in G.RESULT_TENSORS:
        assert G.same_bits(a[name], b[name]), name
    assert a["Y"].shape == (5, 3) and a["loss"].shape == a["pred"].shape == (5,)
    pred, confusion, counts, summary = harness.classification_metrics(a["Y"], labels, a["loss"])
    assert torch.equal(a["pred"], pred) and torch.equal(a["confusion"], confusion) and torch.equal(a["counts"], counts)
    assert int(a["counts"][0]) == 5
    assert abs(float(a["accuracy"]) - float(summary[0])) <= 1e-15 and abs(float(a["balanced_accuracy"]) - float(summary[1])) <= 1e-15
    assert abs(float(a["mean_loss"]) - float(summary[2])) <= 5 * 2.0 ** -53 * float(a["loss"].double().abs().sum())
