"""CPU-only checks of the gene-expression model's resident epochs (include/mpo_classify.h, harness.classification_metrics,
GeResidentCohort, GeCohortEvaluator's windows and refusals, train_ge_epoch's refusals, synthetic.make_ge_cohort).  Nothing here
launches a kernel."""
import ctypes
import math
import os
import types

import pytest
import torch

from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import harness
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.models import (GeneExprNarrowContextualAttentionGateTransformer,
                                             MultimodalCoAttentionTransformer)

HEADER = "mpo_classify.h"
NAMES = ["mpo_class_metrics_workspace_bytes", "mpo_class_metrics_tile", "mpo_class_metrics"]


def test_header_parses_and_its_entries_are_exported_and_bound():
    with open(L.HEADER_PATH) as f:
        assert f'#include "{HEADER}"' in f.read()
    path = [p for p in L.MORE_HEADER_PATHS if os.path.basename(p) == HEADER]
    assert len(path) == 1 and os.path.dirname(path[0]) == os.path.dirname(L.HEADER_PATH)
    with open(path[0]) as f:
        signatures, constants, version = L.parse_header(f.read())
    assert list(signatures) == NAMES and not constants and version is None
    assert L.header_symbols(HEADER) == NAMES
    handle = ctypes.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert hasattr(handle, name), f"{name} declared in include/{HEADER} but not exported"
        assert name not in L.exported_symbols() + L.all_companion_symbols() + L.later_symbols()
    p, i, i64, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    lib = L.lib()
    assert lib.mpo_class_metrics_workspace_bytes.argtypes == [i64, i] and lib.mpo_class_metrics_workspace_bytes.restype == z
    assert lib.mpo_class_metrics_tile.argtypes == [] and lib.mpo_class_metrics_tile.restype == i
    # y, label, loss, n, n_classes, pred, confusion, counts, summary, workspace, workspace_bytes, stream
    assert lib.mpo_class_metrics.argtypes == [p, p, p, i64, i, p, p, p, p, p, z, p] and lib.mpo_class_metrics.restype == i
    assert lib.mpo_abi_version() == 14 and L.ABI_VERSION == 14


def test_kernel_geometry():
    lib = L.lib()
    t = lib.mpo_class_metrics_tile()
    assert t >= 64 and t % 64 == 0
    need = lib.mpo_class_metrics_workspace_bytes
    for n, c in ((0, 3), (-5, 3), ((1 << 24) + 1, 3), (100, 1), (100, 9), (100, 0)):
        assert need(n, c) == 0, (n, c)
    # one column of C * C + 2 eight-byte words per workgroup; one workgroup per tile while the tiles are few
    for c in (2, 3, 8):
        assert [need(n, c) // (8 * (c * c + 2)) for n in (1, t, t + 1, 3 * t + 5)] == [1, 1, 2, 4]
        assert 0 < need(1 << 24, c) <= (1 << 20)                      # the grid stops growing: the workspace stays small
        assert need(1 << 24, c) % (8 * (c * c + 2)) == 0


def _rc(*args):
    rc = L.lib().mpo_class_metrics(*args)
    msg = L.lib().mpo_last_error()
    return rc, (msg.decode() if msg else "")


def test_refusals_come_before_any_launch():
    fake = 0x1000                 # never dereferenced: every call below is refused while its arguments are checked
    need = L.lib().mpo_class_metrics_workspace_bytes(1000, 3)
    ok = [fake, fake, fake, 1000, 3, fake, fake, fake, fake, fake, need, None]
    # y, label, loss, n, n_classes, pred, confusion, counts, summary, workspace, workspace_bytes, stream

    def but(**changes):
        names = ["y", "label", "loss", "n", "c", "pred", "confusion", "counts", "summary", "ws", "ws_bytes", "stream"]
        args = list(ok)
        for k, v in changes.items():
            args[names.index(k)] = v
        return args

    for args, text in ((but(n=0), "n = 0"), (but(n=(1 << 24) + 1, ws_bytes=1 << 30), "outside"),
                       (but(c=1), "n_classes = 1"), (but(c=9), "n_classes = 9"),
                       (but(y=None), "null"), (but(label=None), "null"), (but(confusion=None), "null"),
                       (but(counts=None), "null"), (but(summary=None), "null"),
                       (but(y=fake + 2), "4-byte aligned"), (but(loss=fake + 1), "4-byte aligned"),
                       (but(label=fake + 4), "8-byte aligned"), (but(pred=fake + 4), "8-byte aligned"),
                       (but(confusion=fake + 4), "8-byte aligned"), (but(counts=fake + 4), "8-byte aligned"),
                       (but(summary=fake + 4), "8-byte aligned"),
                       (but(ws=None), "workspace"), (but(ws=fake + 4), "workspace"), (but(ws_bytes=need - 1), "workspace")):
        rc, msg = _rc(*args)
        assert rc == 1 and text in msg, (args, rc, msg)


# ------------------------------------------------------------------------------------------------------- the host form
def test_host_form_against_a_hand_computed_case():
    nan = float("nan")
    y = torch.tensor([[0.2, 0.5, 0.3],          # pred 1, label 1: correct
                      [0.4, 0.4, 0.2],          # a tie: the first index, 0; label 1: wrong
                      [0.1, nan, 0.9],          # a NaN beside a larger value: pred 1; label 0: wrong
                      [0.3, 0.3, 0.3],          # all equal: pred 0; label 0: correct
                      [0.1, 0.2, 0.7],          # label -1: invalid
                      [0.6, 0.3, 0.1],          # label 3 = C: invalid
                      [0.5, 0.1, 0.4]])         # pred 0, label 0: correct          (class 2 stays empty)
    label = torch.tensor([1, 1, 0, 0, -1, 3, 0])
    loss = torch.tensor([0.5, 1.0, 2.0, 0.25, 4.0, 8.0, 0.25])
    pred, confusion, counts, summary = harness.classification_metrics(y, label, loss)
    assert pred.tolist() == [1, 0, 1, 0, 2, 0, 0] and pred.dtype == torch.int64
    assert confusion.tolist() == [[2, 1, 0], [1, 1, 0], [0, 0, 0]] and confusion.dtype == torch.int64
    assert counts.tolist() == [5, 3, 2, 1] and counts.dtype == torch.int64
    assert summary.dtype == torch.float64
    assert summary[0].item() == 3 / 5
    assert summary[1].item() == (2 / 3 + 1 / 2) / 2                         # the empty class is left out of the mean
    assert summary[2].item() == 16.0 / 7
    # no loss: NaN mean; a NaN loss propagates; no valid label: NaN accuracy and balanced accuracy
    assert math.isnan(harness.classification_metrics(y, label)[3][2].item())
    assert math.isnan(harness.classification_metrics(y, label, torch.tensor([0.5, nan, 2.0, 0.25, 4.0, 8.0, 0.25]))[3][2].item())
    pred, confusion, counts, summary = harness.classification_metrics(y[4:6], label[4:6], loss[4:6])
    assert counts.tolist() == [0, 0, 2, 0] and int(confusion.sum()) == 0
    assert math.isnan(summary[0].item()) and math.isnan(summary[1].item()) and summary[2].item() == 6.0
    with pytest.raises(ValueError, match="GPU"):
        harness.classification_metrics_device(y, label, loss)


# ------------------------------------------------------------------------------------------------------- the cohort
LENGTHS = [40, 17, 33, 40, 16, 25, 40]


def ge_slides(width=1024):
    slides = syn.make_ge_cohort(7, 40, 40, seed=5, patch_dim=width)
    for s, m in zip(slides, LENGTHS):
        s["wsi"] = s["wsi"][:m].contiguous()
    return slides


def cpu_cohort(**kw):
    return harness.GeResidentCohort(ge_slides(), "cpu", bag_dtype=torch.float32, slab_bytes=100 * 4096, **kw)


def test_ge_resident_cohort_says_where_a_slide_lies():
    slides = ge_slides()
    cohort = cpu_cohort()                                       # 100-row slabs: [40, 17, 33] [40, 16, 25] [40]
    assert cohort.n_slides == 7 and cohort.lengths == LENGTHS and cohort.cycle is False
    assert cohort.slab_index == [0, 0, 0, 1, 1, 1, 2] and cohort.row_offset == [0, 40, 57, 0, 40, 56, 0]
    assert [int(s.shape[0]) for s in cohort.slabs] == [90, 81, 40]
    for i in range(cohort.n_slides):
        lo = cohort.row_offset[i]
        view = cohort.slabs[cohort.slab_index[i]][lo:lo + cohort.lengths[i]]
        assert view.data_ptr() == cohort.rows[i].data_ptr() and torch.equal(view, cohort.rows[i])
        assert torch.equal(cohort.rows[i], slides[i]["wsi"])
    assert cohort.labels.dtype == torch.int64 and cohort.labels.tolist() == [s["gene_expr_class"] for s in slides]
    assert cohort.table_lens.tolist() == LENGTHS and cohort.table_ptrs.tolist() == [r.data_ptr() for r in cohort.rows]


def test_ge_window_selects_labels_with_out_and_without():
    cohort = cpu_cohort(cycle=True)
    ids = [5, 1, 6]
    ids_dev = torch.tensor(ids, dtype=torch.int32)
    bags, labels = cohort.window(ids_dev, ids)
    assert isinstance(bags, harness.SlideSet) and bags.lengths == [25, 17, 40] and bags.cycle and bags.ids is ids_dev
    assert all(a.data_ptr() == cohort.rows[i].data_ptr() for a, i in zip(bags.slides, ids))
    assert torch.equal(labels, cohort.labels[ids])
    out = torch.full((3,), -7, dtype=torch.int64)
    bags, labels = cohort.window(ids_dev, ids, out=(out,))
    assert labels.data_ptr() == out.data_ptr() and torch.equal(out, cohort.labels[ids])


def test_ge_resident_cohort_refusals():
    with pytest.raises(ValueError, match="GeResidentCohort: no slides"):
        harness.GeResidentCohort([], "cpu")
    with pytest.raises(ValueError, match="GeResidentCohort: a row of 20 bytes is not a multiple of 16"):
        harness.GeResidentCohort(ge_slides(width=10), "cpu", bag_dtype=torch.bfloat16)
    slides = ge_slides()
    slides[2]["wsi"] = slides[2]["wsi"][:, :512].contiguous()
    with pytest.raises(ValueError, match="GeResidentCohort: every slide needs at least one patch row, and all the same width"):
        harness.GeResidentCohort(slides, "cpu")
    cohort = cpu_cohort()
    for bad in (7, -1):
        with pytest.raises(ValueError, match=f"GeResidentCohort.window: slide id {bad} outside the cohort's 7 slides"):
            cohort.window(torch.tensor([0, bad], dtype=torch.int32), [0, bad])
    # the survival cohort's words are what they were
    with pytest.raises(ValueError, match="^ResidentCohort: no slides$"):
        harness.ResidentCohort([], "cpu")


# ------------------------------------------------------------------------------------------------------- the evaluator
def test_ge_evaluator_windows_are_views_of_the_slabs():
    cohort = cpu_cohort()
    model = GeneExprNarrowContextualAttentionGateTransformer()
    ids = [5, 1, 2, 3, 6]
    ev = harness.GeCohortEvaluator(model, cohort, ids, max_window_slides=2)
    assert [w.ids for w in ev.windows] == [[1, 2], [3], [5], [6]] and ev.perm.tolist() == [3, 0, 1, 2, 4]
    assert ev.perm_host == [3, 0, 1, 2, 4] and ev.ids == ids
    assert [(w.lo, w.hi) for w in ev.windows] == [(0, 2), (2, 3), (3, 4), (4, 5)]
    for w in ev.windows:
        assert w.bags.lengths == [cohort.lengths[i] for i in w.ids]
        assert w.bags.data.data_ptr() == cohort.rows[w.ids[0]].data_ptr()                 # a view: no row was copied
        assert w.bags.data.untyped_storage().data_ptr() == cohort.slabs[cohort.slab_index[w.ids[0]]].untyped_storage().data_ptr()
        assert w.bags.cu.tolist() == [0] + list(torch.tensor(w.bags.lengths).cumsum(0))
        assert torch.equal(w.labels, cohort.labels[w.ids])
    assert torch.equal(ev.labels, cohort.labels[ids])
    run_order = [i for w in ev.windows for i in w.ids]
    assert [run_order[k] for k in ev.perm_host] == ids


def test_ge_evaluator_refusals():
    cohort = cpu_cohort()
    model = GeneExprNarrowContextualAttentionGateTransformer()
    with pytest.raises(ValueError, match="twice"):
        harness.GeCohortEvaluator(model, cohort, [1, 2, 1])
    with pytest.raises(ValueError, match="outside"):
        harness.GeCohortEvaluator(model, cohort, [7])
    with pytest.raises(ValueError, match="slide 4 has 16 rows, fewer than the 17"):
        harness.GeCohortEvaluator(model, cohort, [3, 4, 5])
    sizes = [8, 12, 16]
    mcat = MultimodalCoAttentionTransformer(omic_sizes=sizes)
    with pytest.raises(ValueError, match="is not the gene-expression model"):
        harness.GeCohortEvaluator(mcat, cohort, [0, 1])
    survival = harness.ResidentCohort(syn.make_cohort(3, 20, 20, sizes, seed=5), "cpu", bag_dtype=torch.float32)
    with pytest.raises(ValueError, match="GeResidentCohort holds the gene-expression layout, not a ResidentCohort"):
        harness.GeCohortEvaluator(model, survival, [0, 1])
    with pytest.raises(ValueError, match="capture=True.*need_paths.*map"):
        harness.GeCohortEvaluator(model, cohort, [0, 1], capture=True, need_paths=True)
    with pytest.raises(ValueError, match="nothing to replay"):
        harness.validate_ge(model, cohort, [0, 1], capture=True)
    # the survival evaluator keeps its words for this model
    with pytest.raises(ValueError, match="not a survival model"):
        harness.CohortEvaluator(model, survival, [0, 1])
    assert harness.test_ge.__test__ is False


def test_ge_eval_result_reads_the_host_in_one_method_only():
    z = torch.zeros(2)
    f = lambda v: torch.tensor([v], dtype=torch.float64)
    r = harness.GeEvalResult(z, z.view(1, 2), z.long(), z.long().view(1, 2), torch.tensor([4, 3, 0, 0]), f(0.5), f(0.75), f(0.7))
    assert r.accuracy_value() == 0.75 and r.paths is None and r.path_stats is None
    assert math.isnan(harness.GeEvalResult(z, z, z, z, z, f(0.0), f(float("nan")), f(0.0)).accuracy_value())


# ------------------------------------------------------------------------------------------------------- the epoch
def fake_step(ge=True, source="slides", n_slides=2, k=32, width=1024, dtype=torch.float32, sampled=True):
    sampler = types.SimpleNamespace(source=source, n_slides=n_slides, k=k, width=width, dtype=dtype) if sampled else None
    return types.SimpleNamespace(ge=ge, sampler=sampler, window=(None, None))


def test_train_ge_epoch_refusals_that_need_no_gpu():
    cohort = cpu_cohort()
    order = [0, 2, 3, 6]
    for step in (fake_step(ge=False), fake_step(sampled=False), fake_step(source="window")):
        with pytest.raises(ValueError, match="train_ge_epoch: the step must be a gene-expression step captured with sample_rows"):
            harness.train_ge_epoch(step, cohort, order)
    survival = harness.ResidentCohort(syn.make_cohort(3, 40, 40, [8, 12], seed=5), "cpu", bag_dtype=torch.float32)
    with pytest.raises(ValueError, match="not a ResidentCohort"):
        harness.train_ge_epoch(fake_step(), survival, [0, 1])
    with pytest.raises(ValueError, match="the cohort's rows are 1024 x torch.float32, the step was captured for 512"):
        harness.train_ge_epoch(fake_step(width=512), cohort, order)
    with pytest.raises(ValueError, match="the cohort's rows are 1024 x torch.float32, the step was captured for 1024 x torch.bfloat16"):
        harness.train_ge_epoch(fake_step(dtype=torch.bfloat16), cohort, order)
    with pytest.raises(ValueError, match="slide id 7 outside the cohort's 7 slides"):
        harness.train_ge_epoch(fake_step(), cohort, [0, 7])
    with pytest.raises(ValueError, match="slide 5 has 25 rows, fewer than k = 32, and the cohort does not lap"):
        harness.train_ge_epoch(fake_step(), cohort, [0, 5])
    # train_epoch keeps refusing a gene-expression step in its present words
    with pytest.raises(ValueError, match="train_epoch: the step must be a fusion-model step captured with sample_rows"):
        harness.train_epoch(fake_step(), cohort, order)


# ------------------------------------------------------------------------------------------------------- synthetic
def test_make_ge_cohort_is_seeded_and_fills_every_class():
    a, b = syn.make_ge_cohort(12, 20, 30, seed=3), syn.make_ge_cohort(12, 20, 30, seed=3)
    assert all(torch.equal(x["wsi"], y["wsi"]) and x["gene_expr_class"] == y["gene_expr_class"] for x, y in zip(a, b))
    assert not torch.equal(a[0]["wsi"][:20], syn.make_ge_cohort(12, 20, 30, seed=4)[0]["wsi"][:20])
    assert all(set(s) == {"wsi", "gene_expr_class"} and s["wsi"].shape[1] == 1024 and 20 <= s["wsi"].shape[0] <= 30 for s in a)
    for c in (2, 3, 8):
        classes = [s["gene_expr_class"] for s in syn.make_ge_cohort(12, 17, 17, seed=7, n_classes=c, patch_dim=64)]
        assert sorted(set(classes)) == list(range(c))
