"""CPU-only checks of the resident epochs' host logic (harness.train_epoch, train_epoch_dp: every refusal, in the words and
under the name the caller reads, before anything of the step but `ge`, `sampler` and `window` is touched; how far an
accepted order gets) and of what test_eval_cpu.py leaves open about the survival evaluator's windows.  Nothing here
launches a kernel."""
import types

import pytest
import torch

from multimodal_path_omic_amd import harness
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.models import MultimodalCoAttentionTransformer

OMIC_SIZES = [8, 12, 16]
LENGTHS = [40, 17, 33, 40, 16, 25, 40]


def survival_cohort(**kw):
    slides = syn.make_cohort(7, 40, 40, OMIC_SIZES, seed=5)
    for s, m in zip(slides, LENGTHS):
        s["wsi"] = s["wsi"][:m].contiguous()
    return harness.ResidentCohort(slides, "cpu", bag_dtype=torch.float32, slab_bytes=100 * 4096, **kw)


def ge_cohort(**kw):
    slides = syn.make_ge_cohort(7, 40, 40, seed=5)
    for s, m in zip(slides, LENGTHS):
        s["wsi"] = s["wsi"][:m].contiguous()
    return harness.GeResidentCohort(slides, "cpu", bag_dtype=torch.float32, slab_bytes=100 * 4096, **kw)


class Reached(Exception):
    """Raised by the fake step's bind: every refusal is behind, the order is uploaded, the first window is formed."""


def fake_step(ge=False, source="slides", n_slides=2, k=32, width=1024, dtype=torch.float32, sampled=True, **more):
    """A step of which the refusals may read `ge`, `sampler` and `window` alone (and whatever `more` names); bind() is where
    the loop's first window arrives."""
    def bind(window):
        raise Reached(window)
    sampler = types.SimpleNamespace(source=source, n_slides=n_slides, k=k, width=width, dtype=dtype) if sampled else None
    window = (None, None) if ge else (None, [None] * len(OMIC_SIZES), None, None)
    return types.SimpleNamespace(ge=ge, sampler=sampler, window=window, bind=bind, **more)


def fake_dp_step(bucket="bucket", l1=0.0, **kw):
    return fake_step(opt=None, bucket=bucket, l1=l1, split=False, **kw)


def fake_opt(bucket="bucket", l1_lambda=0.0):
    return types.SimpleNamespace(bucket=bucket, l1_lambda=l1_lambda)


def test_train_epoch_refusals_that_need_no_gpu():
    cohort = survival_cohort()
    order = [0, 2, 3, 6]
    for step in (fake_step(ge=True), fake_step(sampled=False), fake_step(source="window")):
        with pytest.raises(ValueError, match="^train_epoch: the step must be a fusion-model step captured with sample_rows on a "
                                             "ResidentCohort window$"):
            harness.train_epoch(step, cohort, order)
    with pytest.raises(ValueError, match="^train_epoch: the cohort's rows are 1024 x torch.float32, the step was captured for "
                                         "512 x torch.float32$"):
        harness.train_epoch(fake_step(width=512), cohort, order)
    with pytest.raises(ValueError, match="^train_epoch: the cohort's rows are 1024 x torch.float32, the step was captured for "
                                         "1024 x torch.bfloat16$"):
        harness.train_epoch(fake_step(dtype=torch.bfloat16), cohort, order)
    for bad in (7, -1):
        with pytest.raises(ValueError, match=f"^train_epoch: slide id {bad} outside the cohort's 7 slides$"):
            harness.train_epoch(fake_step(), cohort, [0, bad])
    with pytest.raises(ValueError, match=r"^train_epoch: slide 5 has 25 rows, fewer than k = 32, and the cohort does not lap short "
                                         r"slides \(cycle=False\)$"):
        harness.train_epoch(fake_step(), cohort, [0, 5])
    # the layout is looked at before the order, and the order id by id: the first offender speaks
    with pytest.raises(ValueError, match="the cohort's rows are"):
        harness.train_epoch(fake_step(width=512), cohort, [0, 7])
    with pytest.raises(ValueError, match="slide id 7 outside"):
        harness.train_epoch(fake_step(), cohort, [0, 7, 5])
    with pytest.raises(ValueError, match="slide 5 has 25 rows"):
        harness.train_epoch(fake_step(), cohort, [0, 5, 7])


def test_train_epoch_accepts_a_short_slide_of_a_lapping_cohort_as_far_as_the_first_window():
    cohort = survival_cohort(cycle=True)
    with pytest.raises(Reached) as reached:
        harness.train_epoch(fake_step(), cohort, [0, 5, 3, 6, 2])
    bags, omics, labels, cens = reached.value.args[0]
    assert isinstance(bags, harness.SlideSet) and bags.lengths == [40, 25] and bags.cycle
    assert bags.ids.dtype == torch.int32 and bags.ids.tolist() == [0, 5]            # a slice of the uploaded order
    assert torch.equal(labels, cohort.labels[[0, 5]]) and torch.equal(cens, cohort.censorship[[0, 5]])
    assert all(torch.equal(o, x[[0, 5]]) for o, x in zip(omics, cohort.omics))
    # fewer ids than one window: nothing to bind, everything is left over
    loss, risk, ids_run, leftover = harness.train_epoch(fake_step(), cohort, [5])
    assert loss.shape == risk.shape == ids_run.shape == (0,) and leftover == [5]
    assert loss.dtype == risk.dtype == torch.float32 and ids_run.dtype == torch.int32
    # the gene-expression epoch gets as far, and returns three
    ge = ge_cohort(cycle=True)
    with pytest.raises(Reached) as reached:
        harness.train_ge_epoch(fake_step(ge=True), ge, [0, 5, 3])
    bags, labels = reached.value.args[0]
    assert bags.lengths == [40, 25] and torch.equal(labels, ge.labels[[0, 5]])
    loss, ids_run, leftover = harness.train_ge_epoch(fake_step(ge=True), ge, [5])
    assert loss.shape == ids_run.shape == (0,) and leftover == [5]


def test_train_epoch_dp_refusals_that_need_no_gpu():
    cohort, ge = survival_cohort(), ge_cohort()
    order = [0, 2, 3, 6]
    run = lambda step, cohort=cohort, order=order, opt=None, n_windows=2: harness.train_epoch_dp(
        step, cohort, order, fake_opt() if opt is None else opt, n_windows)
    # its own five, in their order
    for step in (fake_dp_step(sampled=False), fake_dp_step(source="window")):
        with pytest.raises(ValueError, match="^train_epoch_dp: the step must be captured with sample_rows on a window of a resident "
                                             "cohort$"):
            run(step)
    step = fake_dp_step()
    step.opt = object()
    with pytest.raises(ValueError, match=r"^train_epoch_dp: the step was captured with its optimiser inside; a data-parallel step "
                                         r"leaves it out \(opt=None\): the update comes after the exchange$"):
        run(step)
    with pytest.raises(ValueError, match="^train_epoch_dp: a gene-expression step over a ResidentCohort$"):
        run(fake_dp_step(ge=True))
    with pytest.raises(ValueError, match="^train_epoch_dp: a fusion-model step over a GeResidentCohort$"):
        run(fake_dp_step(), cohort=ge)
    with pytest.raises(ValueError, match="^train_epoch_dp: the optimiser steps another gradient bucket than the one the step "
                                         "writes$"):
        run(fake_dp_step(), opt=fake_opt(bucket="another"))
    with pytest.raises(ValueError, match="^train_epoch_dp: the step reports the L1 penalty with l1 = 0.0, the optimiser folds its "
                                         "gradient with l1_lambda = 0.001: pass the optimiser's value to the step$"):
        run(fake_dp_step(), opt=fake_opt(l1_lambda=1e-3))
    # the caller's window count against the order
    for n_windows, text in ((3, "3 windows of 2 slides need 6 ids, the order holds 4"),
                            (-1, "-1 windows of 2 slides need -2 ids, the order holds 4")):
        with pytest.raises(ValueError, match=f"^train_epoch_dp: {text}; n_windows is dp.epoch_orders' -- the same on every rank$"):
            run(fake_dp_step(), n_windows=n_windows)
    # train_epoch's three, under this name, for both cohort kinds, before the window count is looked at
    for step, c in ((fake_dp_step(), cohort), (fake_dp_step(ge=True), ge)):
        step.sampler.width = 512
        with pytest.raises(ValueError, match="^train_epoch_dp: the cohort's rows are 1024 x torch.float32, the step was captured "
                                             "for 512 x torch.float32$"):
            run(step, cohort=c, n_windows=5)
        step.sampler.width = 1024
        with pytest.raises(ValueError, match="^train_epoch_dp: slide id 7 outside the cohort's 7 slides$"):
            run(step, cohort=c, order=[0, 7], n_windows=5)
        with pytest.raises(ValueError, match=r"^train_epoch_dp: slide 5 has 25 rows, fewer than k = 32, and the cohort does not lap "
                                             r"short slides \(cycle=False\)$"):
            run(step, cohort=c, order=[0, 5], n_windows=5)
    # own refusals come first: a step that fails several says the first
    with pytest.raises(ValueError, match="another gradient bucket"):
        run(fake_dp_step(width=512), opt=fake_opt(bucket="another", l1_lambda=1e-3))


def test_train_epoch_dp_runs_the_callers_window_count():
    cohort = survival_cohort(cycle=True)
    with pytest.raises(Reached) as reached:
        harness.train_epoch_dp(fake_dp_step(), cohort, [0, 5, 3, 6, 2], fake_opt(), 1)
    assert reached.value.args[0][0].lengths == [40, 25]
    # no window asked for: the whole order is left over although it holds two windows
    loss, risk, ids_run, leftover = harness.train_epoch_dp(fake_dp_step(), cohort, [0, 5, 3, 6, 2], fake_opt(), 0)
    assert loss.shape == risk.shape == ids_run.shape == (0,) and leftover == [0, 5, 3, 6, 2]
    loss, ids_run, leftover = harness.train_epoch_dp(fake_dp_step(ge=True), ge_cohort(cycle=True), [0, 5, 3], fake_opt(), 0)
    assert loss.shape == ids_run.shape == (0,) and leftover == [0, 5, 3]


def test_survival_evaluator_keeps_the_callers_order_on_both_sides():
    cohort = survival_cohort()
    model = MultimodalCoAttentionTransformer(omic_sizes=OMIC_SIZES)
    ids = [5, 1, 2, 3, 6]
    ev = harness.CohortEvaluator(model, cohort, ids, max_window_slides=2)
    assert ev.ids == ids and [w.ids for w in ev.windows] == [[1, 2], [3], [5], [6]]
    assert [(w.lo, w.hi) for w in ev.windows] == [(0, 2), (2, 3), (3, 4), (4, 5)]
    assert ev.perm_host == [3, 0, 1, 2, 4] and ev.perm.dtype == torch.int64 and ev.perm.tolist() == ev.perm_host
    run_order = [i for w in ev.windows for i in w.ids]
    assert [run_order[k] for k in ev.perm_host] == ids
    for w in ev.windows:
        slab = cohort.slabs[cohort.slab_index[w.ids[0]]]
        assert w.bags.data.data_ptr() == slab[cohort.row_offset[w.ids[0]]:].data_ptr()
        assert w.bags.lengths == [cohort.lengths[i] for i in w.ids]
        assert torch.equal(w.labels, cohort.labels[w.ids]) and torch.equal(w.cens, cohort.censorship[w.ids])
        assert len(w.omics) == len(OMIC_SIZES) and all(torch.equal(o, x[w.ids]) for o, x in zip(w.omics, cohort.omics))
        assert w.scale is None and w.graph is None              # on the host: no plan, no scale, nothing captured
    assert ev.pool is None and ev.capture is False
    with pytest.raises(ValueError, match="^CohortEvaluator: the model lies on meta, the cohort on cpu$"):
        harness.CohortEvaluator(model.to("meta"), cohort, ids)
