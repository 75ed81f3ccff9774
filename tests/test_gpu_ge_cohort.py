"""The gene-expression model's resident epochs (harness.GeResidentCohort, train_ge_epoch, GeCohortEvaluator, validate_ge,
test_ge): 7 slides of 40, 17, 33, 64, 20, 25 and 100 rows x 1024 -- the window forward's 17-row floor, three slides under
k = 32 that the sampler laps, one over 64 -- in three slabs, bf16 and fp32 storage (an fp32 step is captured with
device_feature_scale=True), medium model.  The captured step on a (SlideSet, labels) window against the host's restatement
of the draw and the eager step on the same sample; one epoch without host synchronisation; the evaluator against the model
slide by slide, against the copied window bit for bit, captured against eager, and test_ge's pooling attentions.

Dropout is 0 wherever two paths are compared.  Bars restated (not imported) from tests/test_gpu_ge_train.py and
tests/test_gpu_map_stats.py."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases as C
import row_sampling_replay as R
from multimodal_path_omic_amd import harness, ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.dp import FlatAdam, FlatGradBucket
from multimodal_path_omic_amd.models import GeneExprNarrowContextualAttentionGateTransformer
from multimodal_path_omic_amd.ops import BagBatch

pytestmark = pytest.mark.gpu

# tests/test_gpu_ge_train.py (from tests/test_gpu_graph.py): replayed against eager steps
GRAPH_LOSS_TOL, GRAPH_PARAM_TOL = dict(rtol=2e-3, atol=2e-4), dict(rtol=5e-3, atol=5e-4)
LENGTHS = [40, 17, 33, 64, 20, 25, 100]
SLABS = [[0, 1, 2], [3, 4, 5], [6]]             # slabs of at most 125 rows
SLAB_ROWS = 125
K = 32
DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}
EVAL_IDS = [5, 1, 2, 4, 6, 0]
WEIGHT_SEED = 951

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def slides_once():
    def make():
        slides = syn.make_ge_cohort(len(LENGTHS), max(LENGTHS), max(LENGTHS), seed=950)
        for s, m in zip(slides, LENGTHS):
            s["wsi"] = s["wsi"][:m].contiguous()
        return slides
    return cached("slides", make)


def cohort_on(dev, storage, cycle=True):
    def make():
        row_bytes = 1024 * (4 if storage == "f32" else 2)
        cohort = harness.GeResidentCohort(slides_once(), dev, bag_dtype=DTYPE[storage], cycle=cycle,
                                          slab_bytes=SLAB_ROWS * row_bytes)
        assert [[i for i in range(7) if cohort.slab_index[i] == s] for s in range(len(cohort.slabs))] == SLABS
        return cohort
    return cached(("cohort", storage, cycle), make)


def build(dev, storage, train=False):
    """The medium model with every dropout site at 0 (the pooling head's is hard-wired otherwise)."""
    model = GeneExprNarrowContextualAttentionGateTransformer(bag_dtype=DTYPE[storage], dropout=0.0)
    model.load_state_dict(cached("sd", lambda: syn.fill_state_dict(C.ge_model_shapes(), WEIGHT_SEED)), strict=True)
    model.path_attention_head.drop_p = 0.0
    return model.to(dev).train(train)


def int32(values, dev):
    return torch.tensor(values, dtype=torch.int32).to(dev)


def window_of(cohort, ids):
    return cohort.window(int32(ids, cohort.device), ids)


def bits(t):
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64)
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32) if t.is_floating_point() else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def expected_rows(slides, stream, k, epoch):
    """The rows the lapping gather writes: slide b's x[pi_b(j mod M)], j < k (tests/test_gpu_cohort_sampling.py)."""
    out = []
    for b, x in enumerate(slides):
        idx = np.resize(R.permutation_prefix(stream[0], stream[1], epoch, b, int(x.shape[0]), k), k)
        out.append(x[torch.from_numpy(idx).to(x.device)])
    return torch.cat(out)


RESULT_TENSORS = ("loss", "Y", "pred", "confusion", "counts", "mean_loss", "accuracy", "balanced_accuracy")


def result_tensors(r):
    return [getattr(r, name) for name in RESULT_TENSORS]


def assert_same_result(a, b):
    for name in RESULT_TENSORS:
        assert same_bits(getattr(a, name), getattr(b, name)), name


# ------------------------------------------------------------------------------------------------ the captured step
def check_replay(step, cohort, ids, eager):
    """One replay of `step`, bound to the cohort slides `ids`: the sample against the host indices (bit for bit), the labels
    selected on the device, loss and gradients against the eager step on that sample."""
    stream = step.sampler.last_stream
    loss = step().clone()
    sample = step.sampler.out.clone()
    assert same_bits(sample, expected_rows([cohort.rows[i] for i in ids], stream, K, int(step.epoch))), ids
    assert torch.equal(step.window[1], cohort.labels[ids]) and step.window[1].dtype == torch.int64
    eager.zero_grad(set_to_none=True)
    ref = harness.train_ge_window(eager, BagBatch.from_lengths(sample, [K] * len(ids)), cohort.labels[ids], len(ids))
    print(f"[ge cohort step] ids {ids} loss {loss.tolist()} diff {float((loss - ref).abs().max()):.1e}")
    torch.testing.assert_close(loss, ref, **GRAPH_LOSS_TOL)
    mine = {n: p._mpo_grad_view for n, p in step.model.named_parameters()}
    theirs = {n: p.grad for n, p in eager.named_parameters() if p.grad is not None}
    assert len(theirs) > 20
    for n in theirs:
        torch.testing.assert_close(mine[n].view_as(theirs[n]), theirs[n], **GRAPH_PARAM_TOL, msg=lambda m, n=n: f"{n}: {m}")
    return sample


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_captured_step_on_a_ge_cohort_window(dev, storage):
    ops.set_rng_epoch(None)
    try:
        cohort = cohort_on(dev, storage)
        model, eager = build(dev, storage, train=True), build(dev, storage, train=True)
        bucket = FlatGradBucket(list(model.parameters()))
        scaled = storage == "f32"
        first = [0, 3]
        step = harness.GraphedWindowStep(model, bucket, window_of(cohort, first), 2, opt=None, warmup=1, sample_rows=K,
                                         device_feature_scale=scaled)
        assert step.ge and step.sampler.source == "slides" and step.sampler.batch.lengths == [K] * 2
        assert (step.sampler.scale is not None) == scaled
        check_replay(step, cohort, first, eager)
        for ids in ([1, 6], [3, 4], [5, 2]):                 # a short slide lapped at position 0, at position 1, at 0 again
            step.bind(window_of(cohort, ids))
            last = check_replay(step, cohort, ids, eager)
        assert same_bits(last[:K - 25], last[25:K])           # the 25-row slide: rows 25..31 are the second lap's first 7

        # refusals, each with its reason; a refused bind leaves the step as it was
        ids = [5, 2]
        bags, labels = harness.make_ge_window([slides_once()[i] for i in first], dev, DTYPE[storage])
        with pytest.raises(ValueError, match="built for SlideSet windows"):
            step.bind((bags, labels))
        with pytest.raises(ValueError, match="3 slides"):
            step.bind(window_of(cohort, [0, 1, 2]))
        narrow = harness.GeResidentCohort(syn.make_ge_cohort(2, 40, 60, seed=60, patch_dim=512), dev, bag_dtype=DTYPE[storage],
                                          cycle=True)
        with pytest.raises(ValueError, match="width 1024"):
            step.bind(window_of(narrow, [0, 1]))
        with pytest.raises(ValueError, match="slide 1 has 17 rows"):
            step.bind(window_of(cohort_on(dev, storage, cycle=False), [0, 1]))
        with pytest.raises(ValueError, match="train_epoch: the step must be a fusion-model step"):
            harness.train_epoch(step, cohort, [0, 1])
        check_replay(step, cohort, ids, eager)
        torch.cuda.synchronize()
    finally:
        ops.set_rng_epoch(None)


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_train_ge_epoch(dev, storage):
    """7 slides in 2-slide windows, Adam inside the graph: three windows run, one id is left over; the loop runs under
    torch.cuda.set_sync_debug_mode("error") (honoured here: the guarded int(tensor) raises), so a host synchronisation inside
    train_ge_epoch that torch can see fails the test."""
    ops.set_rng_epoch(None)
    try:
        cohort = cohort_on(dev, storage)
        model = build(dev, storage, train=True)
        bucket = FlatGradBucket(list(model.parameters()))
        opt = FlatAdam(bucket, lr=1e-3, weight_decay=1e-5)
        step = harness.GraphedWindowStep(model, bucket, window_of(cohort, [0, 3]), 2, opt=opt, warmup=1, sample_rows=K,
                                         device_feature_scale=storage == "f32")
        before = opt.flat_p.clone()
        orders = [[3, 1, 0, 6, 5, 4, 2], [6, 2, 4, 0, 1, 3, 5]]
        results = []
        probe = torch.ones(1, device=dev)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                int(probe)                                   # the mode is honoured: a synchronising call raises
            for order in orders:
                results.append(harness.train_ge_epoch(step, cohort, order))
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert int(opt.t_dev) == 6 and not torch.equal(opt.flat_p, before)               # three windows per epoch; the parameters moved
        for order, (loss, ids_run, leftover) in zip(orders, results):
            assert leftover == order[6:] and ids_run.tolist() == order[:6] and ids_run.dtype == torch.int32
            assert loss.shape == (6,) and loss.is_cuda and loss.dtype == torch.float32 and bool(torch.isfinite(loss).all())
        print(f"[train_ge_epoch {storage}] losses {results[0][0].tolist()} then {results[1][0].tolist()}")
        assert not torch.equal(results[0][0], results[1][0])
        assert torch.equal(results[1][0][4:], step.loss.view(-1))           # the last window's values are the step's own outputs
        assert torch.equal(step.window[1], cohort.labels[orders[1][4:6]])
        with pytest.raises(ValueError, match="outside the cohort"):
            harness.train_ge_epoch(step, cohort, [0, 1, 2, 7])
        with pytest.raises(ValueError, match="slide 1 has 17 rows"):
            harness.train_ge_epoch(step, cohort_on(dev, storage, cycle=False), list(range(7)))
        other = "bf16" if storage == "f32" else "f32"
        with pytest.raises(ValueError, match="the step was captured for 1024 x"):
            harness.train_ge_epoch(step, cohort_on(dev, other), list(range(7)))
    finally:
        ops.set_rng_epoch(None)


# ------------------------------------------------------------------------------------------------ the evaluator
def per_slide(dev, storage):
    """model(wsi) slide by slide, once per storage: Y (7, 3), the `ce` loss (7,), the pooling attentions."""
    def make():
        model, cohort = build(dev, storage), cohort_on(dev, storage)
        ys, losses, paths = [], [], []
        with torch.no_grad():
            for i in range(7):
                y, att = model(wsi=cohort.rows[i])
                ys.append(y)
                losses.append(F.cross_entropy(y[None], cohort.labels[i:i + 1]))          # models/ge_nacagat/main.py:33
                paths.append(att["path"])
        return torch.stack(ys), torch.stack(losses), paths
    return cached(("per slide", storage), make)


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_evaluator_matches_the_model_slide_by_slide(dev, storage):
    model, cohort = build(dev, storage), cohort_on(dev, storage)
    ids = EVAL_IDS
    model.train()                                                          # the evaluator switches to eval and puts this back
    r = harness.validate_ge(model, cohort, ids)
    assert model.training and all(p.grad is None for p in model.parameters())
    model.eval()
    r2 = harness.GeCohortEvaluator(model, cohort, ids)()
    assert not model.training
    assert_same_result(r, r2)
    assert r.loss.shape == r.pred.shape == (6,) and r.Y.shape == (6, 3) and r.confusion.shape == (3, 3) and r.counts.shape == (4,)
    assert r.mean_loss.shape == r.accuracy.shape == r.balanced_accuracy.shape == (1,) and r.accuracy.dtype == torch.float64
    assert r.paths is None and r.path_stats is None
    y_ref, loss_ref, _ = per_slide(dev, storage)
    for k, i in enumerate(ids):
        e_y = relerr(r.Y[k], y_ref[i])
        want = float(loss_ref[i])
        print(f"[ge evaluator {storage}] slide {i}: Y rel err {e_y:.1e}, loss {float(r.loss[k])!r} against {want!r}")
        assert e_y < 1e-5, (i, e_y)
        assert abs(float(r.loss[k]) - want) < 2e-5 * max(1.0, abs(want)), (i, float(r.loss[k]), want)
    labels = cohort.labels[ids]
    pred, confusion, counts, summary = harness.classification_metrics_device(r.Y, labels, r.loss)
    assert torch.equal(r.pred, pred) and torch.equal(r.confusion, confusion) and torch.equal(r.counts, counts)
    assert same_bits(torch.cat([r.accuracy, r.balanced_accuracy, r.mean_loss]), summary)
    h_pred, h_confusion, h_counts, h_summary = harness.classification_metrics(r.Y.cpu(), labels.cpu(), r.loss.cpu())
    assert torch.equal(r.pred.cpu(), h_pred) and torch.equal(r.confusion.cpu(), h_confusion) and torch.equal(r.counts.cpu(), h_counts)
    assert abs(r.accuracy_value() - float(h_summary[0])) <= 1e-15 and abs(float(r.balanced_accuracy) - float(h_summary[1])) <= 1e-15
    assert abs(float(r.mean_loss) - float(h_summary[2])) <= 6 * 2.0 ** -53 * float(r.loss.double().abs().sum())
    assert int(r.counts[0]) == 6 and int(r.counts[2]) == 0 and int(r.counts[3]) == 0
    # l1 > 0 adds l1 * sum|W| to every reported loss and changes no forward
    l1 = 1e-6
    penalty = l1 * sum(float(p.detach().double().abs().sum()) for p in model.parameters())
    with_l1 = harness.validate_ge(model, cohort, ids, l1=l1)
    assert torch.equal(with_l1.Y, r.Y)
    torch.testing.assert_close(with_l1.loss.double(), r.loss.double() + penalty, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_zero_copy_views_give_the_bits_of_the_copied_window(dev, storage):
    model, cohort = build(dev, storage), cohort_on(dev, storage)
    slides = slides_once()
    for ids, caps in ((list(range(7)), {}), (list(range(7)), dict(max_window_slides=2)), (EVAL_IDS, {}), ([6, 3, 0], {})):
        ev = harness.GeCohortEvaluator(model, cohort, ids, **caps)
        r = ev()
        groups = [w.ids for w in ev.windows]
        if not caps and ids == list(range(7)):
            assert groups == SLABS
        if ids == EVAL_IDS:
            assert groups == [[0, 1, 2], [4, 5], [6]]
        for w in ev.windows:
            assert w.bags.data.data_ptr() == cohort.rows[w.ids[0]].data_ptr()              # no row was copied
            bags, labels = harness.make_ge_window([slides[i] for i in w.ids], dev, DTYPE[storage])
            with torch.no_grad():
                y, att = model.forward_window(bags, ce_targets=(labels, torch.ones(len(w.ids), device=dev)))
            at = torch.tensor([ids.index(i) for i in w.ids], device=dev)
            assert torch.equal(r.Y[at], y) and torch.equal(r.loss[at], att["loss"]), (w.ids, caps)


def _hold(what, a, a_again, b):
    """`b` against `a`: bit-identical where two runs of `a`'s kind are (`a_again`), within twice their difference otherwise
    (the rule of tests/test_gpu_checkpoint.py)."""
    noise = max(float((x.double() - y.double()).abs().max()) for x, y in zip(a, a_again))
    diff = max(float((x.double() - y.double()).abs().max()) for x, y in zip(a, b))
    print(f"[ge evaluator {what}] eager run to run: max |diff| {noise:.3e}; captured against eager: {diff:.3e}")
    if noise == 0.0:
        assert all(same_bits(x, y) for x, y in zip(a, b))
    else:
        assert diff <= 2 * noise


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_captured_equals_eager_and_follows_in_place_weight_updates(dev, storage):
    model, cohort = build(dev, storage), cohort_on(dev, storage)
    ids = EVAL_IDS
    bucket = FlatGradBucket(list(model.parameters()))
    opt = FlatAdam(bucket, lr=1e-3)                                        # (re-points the parameters: before the capture)
    grads = [p.grad for p in model.parameters()]
    eager = harness.GeCohortEvaluator(model, cohort, ids)
    twin_a, twin_b = eager(), eager()
    model.train()
    captured = harness.GeCohortEvaluator(model, cohort, ids, capture=True)
    assert model.training and all(w.graph is not None for w in captured.windows)
    first = captured()
    first_y = first.Y.clone()
    assert model.training and all(p.grad is g for p, g in zip(model.parameters(), grads))
    model.eval()
    _hold(f"{storage} first call", result_tensors(twin_a), result_tensors(twin_b), result_tensors(first))
    _hold(f"{storage} a replay", result_tensors(twin_a), result_tensors(twin_b), result_tensors(captured()))
    g = torch.Generator(device="cpu").manual_seed(7)
    for _ in range(2):
        bucket.flat.copy_(torch.randn(bucket.flat.shape, generator=g).to(dev))
        opt.step()
    after = captured()
    fresh_a, fresh_b = eager(), eager()
    _hold(f"{storage} after two Adam steps", result_tensors(fresh_a), result_tensors(fresh_b), result_tensors(after))
    assert not torch.equal(after.Y, twin_a.Y)                              # the weights did move
    assert torch.equal(first.Y, first_y)                                   # earlier results are the caller's: not overwritten


@pytest.mark.parametrize("capture", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_a_call_makes_no_host_sync(dev, storage, capture):
    model, cohort = build(dev, storage), cohort_on(dev, storage)
    ev = harness.GeCohortEvaluator(model, cohort, EVAL_IDS, capture=capture, l1=1e-6)
    want, want_again = ev(), ev()                                          # (allocator and lazy initialisation behind us)
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            int(probe)                                                     # the mode is honoured: a synchronising call raises
        got = ev()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    _hold(f"{storage} under sync-debug", result_tensors(want), result_tensors(want_again), result_tensors(got))


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_test_ge_returns_paths_and_their_statistics_and_saves_one_file_per_slide(dev, storage, tmp_path):
    model, cohort = build(dev, storage), cohort_on(dev, storage)
    ids = [6, 3, 2, 5, 4]
    out = harness.test_ge(model, cohort, ids)                              # (and the warm-up of the call below)
    plain = harness.validate_ge(model, cohort, ids)
    assert [s["id"] for s in out] == ids and all("file" not in s for s in out)
    _, _, paths = per_slide(dev, storage)
    for k, (s, i) in enumerate(zip(out, ids)):
        assert s["path"].shape == (1, LENGTHS[i]) and relerr(s["path"], paths[i]) < 1e-4
        assert torch.equal(s["Y"], plain.Y[k]) and torch.equal(s["pred"], plain.pred[k]) and int(s["label"]) == int(cohort.labels[i])
        lo, hi, mean = (float(v) for v in s["attn_stats"])
        ref = float(s["path"].double().mean())
        assert s["attn_stats"].shape == (3,)
        assert lo == float(s["path"].min()) and hi == float(s["path"].max())          # tests/test_gpu_map_stats.py's bars
        assert abs(mean - ref) <= 1e-6 * abs(ref), (i, mean, ref)
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            int(probe)
        again = harness.test_ge(model, cohort, ids)                        # without save_dir nothing synchronises
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(a["path"].shape == b["path"].shape and relerr(a["path"], b["path"]) < 1e-5 for a, b in zip(again, out))
    saved = harness.test_ge(model, cohort, ids, save_dir=str(tmp_path / "paths"), name="ATTN_ge")
    files = sorted(p.name for p in (tmp_path / "paths").iterdir())
    assert files == sorted(f"ATTN_ge_{i}.pt" for i in ids)
    for s, ref in zip(saved, out):
        loaded = torch.load(s["file"])
        assert not loaded.is_cuda and loaded.shape == ref["path"].shape and torch.equal(loaded, ref["path"].cpu())
    with pytest.raises(ValueError, match="capture=True.*need_paths"):
        harness.GeCohortEvaluator(model, cohort, ids, capture=True, need_paths=True)
    assert math.isfinite(plain.accuracy_value())
