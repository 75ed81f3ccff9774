"""harness.CohortEvaluator / validate / test over a ResidentCohort: MCAT and NaCAGaT, fp32 and bf16 storage, 14 slides
(lengths include 1, 17, 127, 128, 129 and 700) in four slabs.  Against the fp32 oracle run slide by slide at the bars
tests/test_gpu_models.py holds the window forward to (1e-4 fp32 bags, 1e-3 bf16 bags); against the copied window
(harness.make_window) bit for bit; captured against eager bit for bit, before and after an in-place optimiser step; the C-index
against concordance_index_device and the host form; no host synchronisation; the model's mode restored, no .grad left."""
import pytest
import torch

import cases as C
from multimodal_path_omic_amd import harness, ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.dp import FlatGradBucket, FlatOptimizer
from multimodal_path_omic_amd.models import (MultimodalCoAttentionTransformer,
                                             NarrowContextualAttentionGateTransformer)
from oracle import mpo_oracle as O

pytestmark = pytest.mark.gpu

OMIC_SIZES = [64] * 6
LENGTHS = [700, 17, 127, 128, 129, 300, 64, 1, 255, 256, 257, 33, 512, 90]
SLAB_ROWS = 1000                # slabs of at most 1000 rows: [0..3] [4..8] [9..11] [12, 13]
SLABS = [[0, 1, 2, 3], [4, 5, 6, 7, 8], [9, 10, 11], [12, 13]]
IDS = {"one_slab_in_order": [4, 5, 6, 7, 8],
       "all": list(range(14)),
       "scattered_reversed": [13, 10, 7, 5, 2, 0],
       "across_a_slab_boundary": [2, 3, 4, 5, 11, 12]}
BAR = {"f32": 1e-4, "bf16": 1e-3}
DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}
WEIGHT_SEED = 902


def cohort_slides():
    slides = syn.make_cohort(len(LENGTHS), max(LENGTHS), max(LENGTHS), OMIC_SIZES, seed=901)
    for s, m in zip(slides, LENGTHS):
        s["wsi"] = s["wsi"][:m].contiguous()
    return slides


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def slides_once():
    return cached("slides", cohort_slides)


def state_dict(kind):
    return cached(("sd", kind), lambda: syn.fill_state_dict(C.model_shapes(OMIC_SIZES, kind == "nacagat"), WEIGHT_SEED))


def build(kind, storage, dev):
    cls = MultimodalCoAttentionTransformer if kind == "mcat" else NarrowContextualAttentionGateTransformer
    model = cls(omic_sizes=OMIC_SIZES, bag_dtype=DTYPE[storage])
    model.load_state_dict(state_dict(kind))
    return model.to(dev).eval()


def cohort_on(dev, storage):
    def make():
        row_bytes = 1024 * (4 if storage == "f32" else 2)
        cohort = harness.ResidentCohort(slides_once(), dev, bag_dtype=DTYPE[storage], slab_bytes=SLAB_ROWS * row_bytes)
        assert [[i for i in range(14) if cohort.slab_index[i] == s] for s in range(len(cohort.slabs))] == SLABS
        return cohort
    return cached(("cohort", storage), make)


def oracle(kind):
    """The fp32 oracle slide by slide, once per model kind: hazards, survs, Y (14, 4), the co-attention map's norm (14,)."""
    def make():
        fwd = O.mcat_forward if kind == "mcat" else O.nacagat_forward
        kw = dict(inference=True) if kind == "mcat" else {}
        rows, norms = [], []
        with torch.no_grad():
            for s in slides_once():
                hz, sv, y, att = fwd(state_dict(kind), s["wsi"], s["omics"], **kw)
                rows.append((hz[0], sv[0], y[0]))
                norms.append(torch.norm(att["coattn"], p=2))
        hz, sv, y = (torch.stack([r[k] for r in rows]) for k in range(3))
        return dict(hazards=hz, survs=sv, Y=y, norm=torch.stack(norms))
    return cached(("oracle", kind), make)


def targets():
    slides = slides_once()
    return (torch.tensor([s["survival_class"] for s in slides]), torch.tensor([float(s["censorship"]) for s in slides]))


def oracle_ces(kind, ids, alpha=0.75):
    o, (labels, cens) = oracle(kind), targets()
    return torch.stack([O.ces_loss(o["hazards"][i:i + 1], o["survs"][i:i + 1], labels[i:i + 1], cens[i:i + 1], alpha) for i in ids])


def sct_fp64(y, label, cens, eps=1e-7):
    """SurvivalClassificationTobitLoss (models/loss.py:62-85) on Y, per slide, as tests/test_gpu_sct_loss.py restates it."""
    idx = torch.arange(y.shape[1])[None, :]
    keep = torch.where(cens.view(-1, 1) != 0, idx >= label.view(-1, 1), idx == label.view(-1, 1))
    return -torch.log((y.double() * keep).sum(1) + eps)


def worst(got, ref):
    return float((got.detach().double().cpu() - ref.double()).abs().max())


def assert_same_result(a, b):
    for name in ("loss", "risk", "hazards", "survs", "Y", "mean_loss", "counts"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.c_index.view(torch.int64), b.c_index.view(torch.int64))          # (bits: NaN == NaN too)


@pytest.mark.parametrize("case", list(IDS))
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_validate_matches_the_oracle_per_slide_in_ids_order(dev, kind, storage, case):
    ids, bar = IDS[case], BAR[storage]
    model, cohort = build(kind, storage, dev), cohort_on(dev, storage)
    model.train()                                                          # the evaluator switches to eval and puts this back
    r = harness.validate(model, cohort, ids)
    assert model.training and all(p.grad is None for p in model.parameters())
    model.eval()
    r2 = harness.CohortEvaluator(model, cohort, ids)()
    assert not model.training
    assert_same_result(r, r2)
    o = oracle(kind)
    figures = {k: worst(getattr(r, k), o[k][ids]) for k in ("hazards", "survs", "Y")}
    figures["risk"] = worst(r.risk, -o["survs"][ids].sum(1))
    figures["loss"] = worst(r.loss, oracle_ces(kind, ids))
    print(f"[validate {kind} {storage} {case}] " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    assert r.loss.shape == r.risk.shape == (len(ids),) and r.hazards.shape == r.survs.shape == r.Y.shape == (len(ids), 4)
    for k, v in figures.items():
        assert v < bar, (k, v)
    assert torch.equal(r.mean_loss, r.loss.mean(0, keepdim=True)) and r.mean_loss.shape == (1,)
    # the C-index: the device function on the gathered tensors, and the host form on the copied risks
    idx = torch.tensor(ids, device=dev)
    c_index, counts = harness.concordance_index_device(cohort.censorship[idx], cohort.survival_months[idx], r.risk)
    assert torch.equal(r.counts, counts) and torch.equal(r.c_index, c_index) and r.c_index.dtype == torch.float64
    host = harness.concordance_index_censored(1 - cohort.censorship[idx].cpu().numpy(), cohort.survival_months[idx].cpu().numpy(),
                                              r.risk.cpu().numpy())
    assert abs(r.c_index_value() - host) <= 1e-15


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_zero_copy_views_give_the_bits_of_the_copied_window(dev, kind, storage):
    """Every window of the evaluator -- a view into a slab -- against model.eval().forward_window on harness.make_window of
    the same slides grouped the same way (rows copied to the device anew): the forward has no atomics, so equal bits."""
    model, cohort = build(kind, storage, dev), cohort_on(dev, storage)
    slides = slides_once()
    for ids, caps in ((IDS["all"], {}), (IDS["all"], dict(max_window_slides=2)), (IDS["all"], dict(max_window_rows=600)),
                      (IDS["scattered_reversed"], {}), (IDS["across_a_slab_boundary"], {})):
        ev = harness.CohortEvaluator(model, cohort, ids, **caps)
        r = ev()
        groups = [w.ids for w in ev.windows]
        if not caps and ids == IDS["all"]:
            assert groups == SLABS
        if ids == IDS["across_a_slab_boundary"]:
            assert groups == [[2, 3], [4, 5], [11], [12]]
        assert sorted(i for g in groups for i in g) == sorted(ids)
        for w in ev.windows:
            assert w.bags.data.data_ptr() == cohort.rows[w.ids[0]].data_ptr()              # no row was copied
            bags, omics, labels, cens = harness.make_window([slides[i] for i in w.ids], dev, DTYPE[storage])
            with torch.no_grad():
                hz, sv, y, _ = model.forward_window(bags, omics)
                loss, risk = ops.ces_loss(hz, sv, labels, cens)
            at = torch.tensor([ids.index(i) for i in w.ids], device=dev)
            for got, ref in ((r.hazards, hz), (r.survs, sv), (r.Y, y), (r.loss, loss), (r.risk, risk)):
                assert torch.equal(got[at], ref), (w.ids, caps)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_captured_equals_eager_and_follows_in_place_weight_updates(dev, kind, storage):
    model, cohort = build(kind, storage, dev), cohort_on(dev, storage)
    ids = IDS["scattered_reversed"] + [3, 4, 8, 9, 11, 12]
    bucket = FlatGradBucket(list(model.parameters()))
    opt = FlatOptimizer(bucket, "sgd", lr=1e-3)                            # (re-points the parameters: before the capture)
    grads = [p.grad for p in model.parameters()]                           # (the bucket's views, or nothing)
    eager = harness.CohortEvaluator(model, cohort, ids)()
    model.train()
    captured = harness.CohortEvaluator(model, cohort, ids, capture=True)
    assert model.training and all(w.graph is not None for w in captured.windows)
    first = captured()
    assert model.training and all(p.grad is g for p, g in zip(model.parameters(), grads))
    model.eval()
    assert_same_result(first, eager)
    assert_same_result(captured(), eager)                                  # a replay changes nothing
    g = torch.Generator(device="cpu").manual_seed(7)
    bucket.flat.copy_(torch.randn(bucket.flat.shape, generator=g).to(dev))
    opt.step()
    after = captured()
    fresh = harness.CohortEvaluator(model, cohort, ids)()
    assert_same_result(after, fresh)
    assert not torch.equal(after.hazards, eager.hazards)                   # the weights did move
    assert torch.equal(first.hazards, eager.hazards)                       # earlier results are the caller's: not overwritten


@pytest.mark.parametrize("capture", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_a_call_makes_no_host_sync(dev, kind, storage, capture):
    model, cohort = build(kind, storage, dev), cohort_on(dev, storage)
    ev = harness.CohortEvaluator(model, cohort, IDS["across_a_slab_boundary"], capture=capture, l1=1e-4)
    want = ev()                                                            # (allocator and lazy initialisation behind us)
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
    assert_same_result(got, want)


@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_sct_l1_and_cesar_losses_match_the_oracle(dev, kind):
    """At the bars of tests/test_gpu_models.py::test_cesar_window_loss_matches_oracle (rel 2e-4, abs 2e-5), fp32 storage."""
    model, cohort = build(kind, "f32", dev), cohort_on(dev, "f32")
    ids = IDS["across_a_slab_boundary"]
    o, (labels, cens) = oracle(kind), targets()
    l1 = 1e-6                                   # (sum |W| is about 1.9e5: a penalty of the losses' own size)
    penalty = l1 * sum(float(v.double().abs().sum()) for k, v in state_dict(kind).items())
    cases = [("sct", dict(loss="sct"), sct_fp64(o["Y"][ids], labels[ids], cens[ids])),
             ("sct + l1", dict(loss="sct", l1=l1), sct_fp64(o["Y"][ids], labels[ids], cens[ids]) + penalty),
             ("ces alpha 0.4 + l1", dict(alpha=0.4, l1=l1), oracle_ces(kind, ids, 0.4) + penalty)]
    if kind == "nacagat":
        lam = 0.05
        ref = oracle_ces(kind, ids) + lam * o["norm"][ids]              # O.cesar_loss: ces + lambda ||A_b||_2 per slide
        cases.append(("cesar", dict(loss="cesar", lambda_reg=lam), ref))
        cases.append(("cesar + l1", dict(loss="cesar", lambda_reg=lam, l1=l1), ref + penalty))
    plain = harness.validate(model, cohort, ids)
    for name, options, ref in cases:
        r = harness.validate(model, cohort, ids, **options)
        print(f"[validate {kind} {name}] |loss - oracle| {worst(r.loss, ref):.2e} of {float(ref.abs().max()):.3f}")
        for b in range(len(ids)):
            assert float(r.loss[b]) == pytest.approx(float(ref[b]), rel=2e-4, abs=2e-5), (name, b)
        assert torch.equal(r.hazards, plain.hazards) and torch.equal(r.survs, plain.survs)   # the loss changes no forward
        if options.get("loss") == "sct":
            assert torch.equal(r.risk, -r.survs.sum(1))
        else:
            assert torch.equal(r.risk, plain.risk) and torch.equal(r.counts, plain.counts)
    if kind == "nacagat":
        with pytest.raises(ValueError, match="capture=True.*cesar.*map"):
            harness.CohortEvaluator(model, cohort, ids, loss="cesar", capture=True)
    else:
        with pytest.raises(ValueError, match='Loss "cesar" not implemented for mcat'):
            harness.validate(model, cohort, ids, loss="cesar")
    with pytest.raises(ValueError) as e:
        harness.validate(model, cohort, ids, loss="ce")
    assert str(e.value) == harness.CE_REFUSAL


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_test_returns_maps_and_their_statistics_and_saves_one_file_per_slide(dev, kind, storage, tmp_path):
    model, cohort = build(kind, storage, dev), cohort_on(dev, storage)
    ids = [12, 3, 2, 7, 4]
    out = harness.test(model, cohort, ids)
    plain = harness.validate(model, cohort, ids)
    assert [s["id"] for s in out] == ids and all("file" not in s for s in out)
    slides = slides_once()
    for group in ([2, 3], [4], [7], [12]):                                 # the windows the evaluator cuts these ids into
        bags, omics, _, _ = harness.make_window([slides[i] for i in group], dev, DTYPE[storage])
        with torch.no_grad():
            hz, sv, y, att = model.forward_window(bags, omics, inference=True)
        stats = ops.map_block_stats(att["coattn"])
        for b, i in enumerate(group):
            s = out[ids.index(i)]
            assert s["coattn"].shape == (len(OMIC_SIZES), LENGTHS[i]) and torch.equal(s["coattn"], att["coattn"][b])
            assert torch.equal(s["attn_stats"], stats[b]) and s["attn_stats"].shape == (3,)
            assert float(s["attn_stats"][0]) == float(att["coattn"][b].min())
            assert float(s["attn_stats"][1]) == float(att["coattn"][b].max())
            assert torch.equal(s["hazards"], hz[b]) and torch.equal(s["survs"], sv[b]) and torch.equal(s["Y"], y[b])
            assert torch.equal(s["risk"], plain.risk[ids.index(i)])
    saved = harness.test(model, cohort, ids, save_dir=str(tmp_path / "maps"), name="ATTN_" + kind)
    files = sorted(p.name for p in (tmp_path / "maps").iterdir())
    assert files == sorted(f"ATTN_{kind}_{i}.pt" for i in ids)
    for s, ref in zip(saved, out):
        loaded = torch.load(s["file"])
        assert not loaded.is_cuda and torch.equal(loaded, ref["coattn"].cpu())
