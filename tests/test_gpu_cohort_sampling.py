"""Patch sampling from a cohort resident on the device (csrc/bag_sample.hip, ops.SlideSet, ops.RowSampler(source=
"slides"), harness.ResidentCohort / train_epoch): the gather from separately allocated slides against x[idx] with idx restated
on the host (tests/row_sampling_replay.py; lapped slides: the prefix tiled), bit for bit; the same bits as the contiguous
gather; a captured gather and a captured training step following their bindings; one epoch without host synchronisation.

Where two training paths are compared, dropout is off (p = 0) and the bars are those of tests/test_gpu_row_sampling.py
(restated, not imported)."""
import numpy as np
import pytest
import torch

import cases as C
import row_sampling_replay as R
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import harness, ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.dp import FlatAdam, FlatGradBucket
from multimodal_path_omic_amd.models import MultimodalCoAttentionTransformer, NarrowContextualAttentionGateTransformer
from multimodal_path_omic_amd.ops import BagBatch, SlideSet

pytestmark = pytest.mark.gpu

LOSS_TOL, PARAM_TOL = dict(rtol=2e-3, atol=2e-4), dict(rtol=5e-3, atol=5e-4)
SIZES = [64] * 6
# a table of 7 separately allocated slides; the window [5, 0, 6, 2] names lengths [1, 33, 700, 4097]
TABLE_LENGTHS = [33, 7, 4097, 40, 2, 1, 700]
WINDOW_IDS = [5, 0, 6, 2]


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def separate_slides(lengths, width, dtype, dev, seed):
    """One allocation per slide."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randn(m, width, generator=g).to(device=dev, dtype=dtype) for m in lengths]


def slide_rows(x, stream, epoch, b, k, cycle):
    """Rows of slide x (position b of the window) the gather writes: x[pi_b(j)] for j < min(k, M); lapped: pi_b(j mod M), j < k."""
    idx = R.permutation_prefix(stream[0], stream[1], epoch, b, int(x.shape[0]), k)
    if cycle:
        idx = np.resize(idx, k)
    return x[torch.from_numpy(idx).to(x.device)]


def expected_rows(slides, stream, k, epoch, cycle):
    return torch.cat([slide_rows(x, stream, epoch, b, k, cycle) for b, x in enumerate(slides)])


def int32(values, dev):
    return torch.tensor(values, dtype=torch.int32).to(dev)


def new_desc(n, dev):
    return torch.zeros(L.lib().mpo_bag_sample_slides_desc_bytes(n) // 8, dtype=torch.int64, device=dev)


def bind_slides(desc, table, ids, k, cycle):
    L.call("mpo_bag_sample_bind_slides", L.ptr(desc), L.ptr(table[0]), L.ptr(table[1]), int(table[1].numel()), L.ptr(ids),
           int(ids.numel()), k, int(cycle), L.stream_of(desc))


def gather_slides(desc, n, k, out, stream, epoch=None):
    L.call("mpo_bag_sample_slides", L.ptr(desc), n, k, out.shape[1], out.element_size(), stream[0], stream[1], L.ptr(epoch),
           L.ptr(out), L.stream_of(out))


# ------------------------------------------------------------------------------------------------ the gather
@pytest.mark.parametrize("dtype,width,k", [(torch.bfloat16, 512, 32), (torch.bfloat16, 1024, 32), (torch.bfloat16, 2048, 32),
                                           (torch.float32, 512, 32), (torch.float32, 1024, 32), (torch.float32, 2048, 32),
                                           (torch.bfloat16, 8, 32), (torch.bfloat16, 264, 32), (torch.float32, 1028, 32),
                                           (torch.bfloat16, 1024, 31), (torch.bfloat16, 2048, 31)])
def test_gather_equals_indexing_bit_for_bit(dev, dtype, width, k):
    """Rows of 1, 2, 4, 8 KiB and the loop form (one vector, fewer than 64, more than 64 with a remainder); with k = 31 a
    slide boundary falls inside one wave's rows (4 rows per wave at 1 KiB and in the loop form, 2 at 2 KiB)."""
    table_slides = separate_slides(TABLE_LENGTHS, width, dtype, dev, 1)
    before = [x.clone() for x in table_slides]
    table = SlideSet.slide_table(table_slides)
    slides = [table_slides[i] for i in WINDOW_IDS]
    assert [int(x.shape[0]) for x in slides] == [1, 33, 700, 4097]
    desc = new_desc(4, dev)
    stream = (77, 5)
    guard = 4

    def run(ids, cycle):
        big = torch.full((4 * k + guard, width), float("nan"), dtype=dtype, device=dev)
        bind_slides(desc, table, int32(ids, dev), k, cycle)
        gather_slides(desc, 4, k, big, stream)
        return big
    # without cycle: a slide shorter than k whole, the output compact
    big = run(WINDOW_IDS, False)
    n_out = 1 + 3 * k
    assert same_bits(big[:n_out], expected_rows(slides, stream, k, 0, False))
    assert bool(torch.isnan(big[n_out:]).all())                              # rows behind the output are not written
    words = desc.view(torch.int32)
    assert desc[:4].tolist() == [x.data_ptr() for x in slides]
    assert words[8:12].tolist() == [1, 33, 700, 4097] and words[12:17].tolist() == [0, 1, 1 + k, 1 + 2 * k, 1 + 3 * k]
    # with cycle: 4 x k rows, the one-row slide repeated k times, the 33-row slide lapped
    big = run(WINDOW_IDS, True)
    assert same_bits(big[:4 * k], expected_rows(slides, stream, k, 0, True))
    assert same_bits(big[:k], slides[0].expand(k, width)) and bool(torch.isnan(big[4 * k:]).all())
    assert desc.view(torch.int32)[12:17].tolist() == [0, k, 2 * k, 3 * k, 4 * k]
    # an id outside the table: length 0, nothing read, nothing written for it
    for bad in (7, -1, 1 << 30):
        big = run([5, 0, bad, 2], True)                                      # lapped: its k rows stay as they were
        want = expected_rows(slides, stream, k, 0, True)
        assert same_bits(big[:2 * k], want[:2 * k]) and same_bits(big[3 * k:4 * k], want[3 * k:])
        assert bool(torch.isnan(big[2 * k:3 * k]).all()) and bool(torch.isnan(big[4 * k:]).all())
        assert int(desc[2]) == 0 and desc.view(torch.int32)[8:12].tolist() == [1, 33, 0, 4097]
    big = run([5, 0, 7, 2], False)                                           # compact: the slide takes no rows
    want = torch.cat([slide_rows(x, stream, 0, b, k, False) for b, x in ((0, slides[0]), (1, slides[1]), (3, slides[3]))])
    assert same_bits(big[:1 + 2 * k], want) and bool(torch.isnan(big[1 + 2 * k:]).all())
    for x, b in zip(table_slides, before):
        assert same_bits(x, b)                                               # the sources are not written


@pytest.mark.parametrize("dtype,width,k", [(torch.bfloat16, 1024, 32), (torch.bfloat16, 2048, 31), (torch.float32, 1028, 32)])
def test_same_draw_as_the_contiguous_gather(dev, dtype, width, k):
    """The same slides in the same order with the same (seed, offset, epoch): mpo_bag_sample_rows on the concatenation and
    mpo_bag_sample_slides on the separate allocations write identical bits."""
    table_slides = separate_slides(TABLE_LENGTHS, width, dtype, dev, 2)
    slides = [table_slides[i] for i in WINDOW_IDS]
    bags = BagBatch.from_list(slides)
    desc_c = torch.zeros(L.lib().mpo_bag_sample_desc_bytes(4) // 8, dtype=torch.int64, device=dev)
    L.call("mpo_bag_sample_bind", L.ptr(desc_c), L.ptr(bags.data), L.ptr(bags.cu), 4, k, L.stream_of(desc_c))
    desc_s = new_desc(4, dev)
    bind_slides(desc_s, SlideSet.slide_table(table_slides), int32(WINDOW_IDS, dev), k, False)
    epoch = torch.zeros(1, dtype=torch.int64, device=dev)
    outs = []
    for e in (0, 1):
        epoch.fill_(e)
        a = torch.full((4 * k, width), float("nan"), dtype=dtype, device=dev)
        b = a.clone()
        L.call("mpo_bag_sample_rows", L.ptr(desc_c), 4, k, width, a.element_size(), 1234567, 9, L.ptr(epoch), L.ptr(a), L.stream_of(a))
        gather_slides(desc_s, 4, k, b, (1234567, 9), epoch)
        assert same_bits(a[:1 + 3 * k], b[:1 + 3 * k]) and bool(torch.isnan(b[1 + 3 * k:]).all())
        assert same_bits(b[:1 + 3 * k], expected_rows(slides, (1234567, 9), k, e, False))
        outs.append(b)
    assert not same_bits(outs[0], outs[1])


@pytest.mark.parametrize("width,lengths,k,cycle", [(1024, [20000, 17000], 17000, False), (8, [3, 40000], 39999, True)])
def test_gather_of_many_rows(dev, width, lengths, k, cycle):
    """Tens of thousands of output rows (thousands of workgroups): a slide drawn whole, and a 3-row slide lapped 13 333 times."""
    ops.set_rng_epoch(None)
    slides = separate_slides(lengths, width, torch.bfloat16, dev, 7)
    table = SlideSet.slide_table(slides)
    window = SlideSet(slides, lengths, table[0], table[1], int32([0, 1], dev), cycle)
    s = ops.RowSampler(2, k, width, torch.bfloat16, dev, static=False, source="slides").bind(window)
    s.out.fill_(float("nan"))
    out = s()
    assert out.lengths == ([k, k] if cycle else [min(k, m) for m in lengths]) and out.total_rows > 30000
    assert same_bits(out.data, expected_rows(slides, s.last_stream, k, 0, cycle))
    assert bool(torch.isnan(s.out[out.total_rows:]).all())
    if cycle:
        counts = torch.bincount(torch.from_numpy(np.resize(R.permutation_prefix(*s.last_stream, 0, 0, 3, k), k)), minlength=3)
        assert counts.tolist() == [13333] * 3


@pytest.mark.parametrize("bind", ["contiguous", "slides", "slides lapped"])
@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_output_offsets_of_both_binds_across_wave_trips(dev, n, bind):
    """ocu of both bind kernels comes from one single-wave prefix sum, 64 slides per trip with a carry from trip to trip: one
    trip partly filled, exactly full, one slide into the second, and into the third.  Rows of one 16-byte vector, k = 3, slide
    lengths 1 .. 5, so some slides are shorter than k.  The descriptor's ocu words equal the host's prefix sums of the rows
    each slide takes -- min(k, M_b); k where the slides are lapped; for an id outside the table (position 64) 0, or, lapped,
    its k rows like every slide's, none of them written (test_gather_equals_indexing_bit_for_bit pins the same) -- the
    gather over that binding equals indexing, bit for bit, and the rows behind ocu[n] keep their fill."""
    width, k, stream, guard = 8, 3, (21, 4), 4
    lapped = bind == "slides lapped"
    table_lengths = [[1, 2, 3, 4, 5][i % 5] for i in range(n)]
    g = torch.Generator(device="cpu").manual_seed(11)
    slab = torch.randn(sum(table_lengths), width, generator=g).to(device=dev, dtype=torch.bfloat16)
    before = slab.clone()
    table_slides = list(slab.split(table_lengths))                           # (16-byte rows: every view is aligned)
    nan = torch.full((n * k + guard, width), float("nan"), dtype=torch.bfloat16, device=dev)
    big = nan.clone()
    if bind == "contiguous":
        ids, bad = list(range(n)), None
        bags = BagBatch.from_lengths(slab, table_lengths)
        desc = torch.zeros(L.lib().mpo_bag_sample_desc_bytes(n) // 8, dtype=torch.int64, device=dev)
        L.call("mpo_bag_sample_bind", L.ptr(desc), L.ptr(bags.data), L.ptr(bags.cu), n, k, L.stream_of(desc))
        L.call("mpo_bag_sample_rows", L.ptr(desc), n, k, width, 2, stream[0], stream[1], L.ptr(None), L.ptr(big), L.stream_of(big))
        words = desc.view(torch.int32)                                       # base | cu[n + 1] | ocu[n + 1]
        assert int(desc[0]) == slab.data_ptr() and words[2:n + 3].tolist() == bags.cu.tolist()
        ocu = words[n + 3:2 * n + 4].tolist()
    else:
        ids, bad = list(reversed(range(n))), (64 if n > 64 else None)        # (position b reads table slide n - 1 - b)
        if bad is not None:
            ids[bad] = n
        desc = new_desc(n, dev)
        bind_slides(desc, SlideSet.slide_table(table_slides), int32(ids, dev), k, lapped)
        gather_slides(desc, n, k, big, stream)
        words = desc.view(torch.int32)                                       # ptr[n] | len[n] | ocu[n + 1]
        assert desc[:n].tolist() == [0 if b == bad else table_slides[i].data_ptr() for b, i in enumerate(ids)]
        assert words[2 * n:3 * n].tolist() == [0 if b == bad else table_lengths[i] for b, i in enumerate(ids)]
        ocu = words[3 * n:4 * n + 1].tolist()
    take, want = [], []
    for b, i in enumerate(ids):
        if b == bad:                            # lapped: its k rows are counted and stay as they were
            take.append(k if lapped else 0)
            want.append(nan[:take[-1]])
        else:
            take.append(k if lapped else min(k, table_lengths[i]))
            want.append(slide_rows(table_slides[i], stream, 0, b, k, lapped))
    assert ocu == np.concatenate([[0], np.cumsum(take)]).tolist()
    assert same_bits(big[:ocu[-1]], torch.cat(want)) and same_bits(big[ocu[-1]:], nan[ocu[-1]:])
    assert same_bits(slab, before)                                           # the sources are not written


def test_captured_gather_follows_its_binding(dev):
    """The gather alone in a graph: the replay reads whichever slides were bound last, and the device epoch moves the draw."""
    width, k, stream = 1024, 32, (5, 11)
    table_slides = separate_slides(TABLE_LENGTHS, width, torch.bfloat16, dev, 3)
    table = SlideSet.slide_table(table_slides)
    desc = new_desc(4, dev)
    out = torch.full((4 * k, width), float("nan"), dtype=torch.bfloat16, device=dev)
    epoch = torch.zeros(1, dtype=torch.int64, device=dev)
    ids_a, ids_b = [5, 0, 6, 2], [2, 3, 0, 6]
    bind_slides(desc, table, int32(ids_a, dev), k, True)
    gather_slides(desc, 4, k, out, stream, epoch)                            # (warm-up: the module is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gather_slides(desc, 4, k, out, stream, epoch)
    for ids, e in ((ids_a, 0), (ids_b, 0), (ids_b, 1), (ids_a, 1)):
        bind_slides(desc, table, int32(ids, dev), k, True)
        epoch.fill_(e)
        out.fill_(float("nan"))
        graph.replay()
        assert same_bits(out, expected_rows([table_slides[i] for i in ids], stream, k, e, True)), (ids, e)
    assert not same_bits(expected_rows([table_slides[i] for i in ids_b], stream, k, 0, True),
                         expected_rows([table_slides[i] for i in ids_b], stream, k, 1, True))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the captured step
def fusion_model(kind, dev):
    cls = MultimodalCoAttentionTransformer if kind == "mcat" else NarrowContextualAttentionGateTransformer
    model = cls(omic_sizes=SIZES, bag_dtype=torch.bfloat16, dropout=0.0)
    model.load_state_dict(syn.fill_state_dict(C.model_shapes(SIZES, kind == "nacagat"), 55))
    model.path_attention_head.drop_p = model.omic_attention_head.drop_p = 0.0       # (hard-wired otherwise)
    if kind == "nacagat":
        model.co_attention.dropout = 0.0                # (the map's dropout, hard-wired 0.25: blocks.PreGatingContextualAttention)
    return model.to(dev).train()


SHORT = 7           # the cohort's 20-row slide


def cohort_slides(seed=56):
    slides = syn.make_cohort(10, 200, 700, SIZES, seed)
    slides[SHORT]["wsi"] = slides[SHORT]["wsi"][:20]
    return slides


def window_of(cohort, ids):
    return cohort.window(int32(ids, cohort.device), ids)


def check_replay(step, cohort, ids, eager, k=32, grads=True):
    """One replay of `step`, bound to the cohort slides `ids`: the sample against the host indices (bit for bit), loss and
    gradients against the eager step on that sample."""
    stream = step.sampler.last_stream
    loss = step()[0].clone()
    sample = step.sampler.out.clone()
    want = expected_rows([cohort.rows[i] for i in ids], stream, k, int(step.epoch), cohort.cycle)
    assert same_bits(sample, want), ids
    fresh = window_of(cohort, ids)
    for a, b in zip(list(step.window[1]) + list(step.window[2:]), list(fresh[1]) + list(fresh[2:])):
        assert torch.equal(a, b)                                             # omics, labels, censorship selected on the device
    eager.zero_grad(set_to_none=True)
    ref, _ = harness.train_window(eager, BagBatch.from_lengths(sample, [k] * len(ids)), *fresh[1:], len(ids))
    print(f"[cohort step] ids {ids} loss diff {float((loss - ref).abs().max()):.1e}")
    torch.testing.assert_close(loss, ref, **LOSS_TOL)
    if grads:
        mine = {n: p._mpo_grad_view for n, p in step.model.named_parameters()}
        theirs = {n: p.grad for n, p in eager.named_parameters() if p.grad is not None}
        assert len(theirs) > 20
        for n in theirs:
            torch.testing.assert_close(mine[n], theirs[n], **PARAM_TOL, msg=lambda m, n=n: f"{n}: {m}")
    return sample


def test_captured_step_on_a_cohort(dev):
    ops.set_rng_epoch(None)
    try:
        cohort = harness.ResidentCohort(cohort_slides(), dev, cycle=True)
        assert cohort.lengths[SHORT] == 20 and min(m for i, m in enumerate(cohort.lengths) if i != SHORT) >= 200
        model, eager = fusion_model("mcat", dev), fusion_model("mcat", dev)
        bucket = FlatGradBucket(list(model.parameters()))
        first = [0, 1, 2, 3]
        step = harness.GraphedWindowStep(model, bucket, window_of(cohort, first), 4, opt=None, warmup=1, sample_rows=32)
        assert step.sampler.source == "slides" and step.sampler.batch.lengths == [32] * 4
        check_replay(step, cohort, first, eager)
        for ids in ([4, 5, SHORT, 6], [9, 8, 3, 0], [SHORT, 2, 9, 1]):       # the short slide lapped at position 2, absent, at 0
            step.bind(window_of(cohort, ids))
            last = check_replay(step, cohort, ids, eager)
        assert same_bits(last[:12], last[20:32])                             # rows 20..31 are the second lap's first 12

        # the same step on a contiguous window presented as slides == a contiguous step captured at the same rng_base
        window = harness.make_window(cohort_slides(57)[:4], dev, torch.bfloat16)
        # (step and step_c share ONE epoch tensor, ops._rng_epoch_tensor, which every replay bumps: it is set to the same value
        #  before each of the two replays, so both draw at epoch 4 with the same seed and offset)
        step.bind((SlideSet.from_batch(window[0]), *window[1:]))
        step.epoch.fill_(3)
        step()
        from_slides = step.sampler.out.clone()
        model_c = fusion_model("mcat", dev)
        step_c = harness.GraphedWindowStep(model_c, FlatGradBucket(list(model_c.parameters())), window, 4, opt=None, warmup=1,
                                           sample_rows=32, rng_base=step.rng_base)
        assert step_c.sampler.source == "window" and step_c.sampler.last_stream == step.sampler.last_stream
        step.epoch.fill_(3)
        step_c()
        assert same_bits(step_c.sampler.out, from_slides)

        # refusals, each with its reason; a refused bind leaves the step as it was
        ids = [SHORT, 2, 9, 1]
        step.bind(window_of(cohort, ids))
        with pytest.raises(ValueError, match="built for SlideSet windows"):
            step.bind(window)
        with pytest.raises(ValueError, match="built for BagBatch windows"):
            step_c.bind(window_of(cohort, ids))
        with pytest.raises(ValueError, match="3 slides"):
            step.bind(window_of(cohort, [0, 1, 2]))
        narrow = harness.ResidentCohort(syn.make_cohort(4, 40, 60, SIZES, 60, patch_dim=512), dev, cycle=True)
        with pytest.raises(ValueError, match="width 1024"):
            step.bind(window_of(narrow, [0, 1, 2, 3]))
        strict = harness.ResidentCohort(cohort_slides(), dev, cycle=False)
        with pytest.raises(ValueError, match="slide 2 has 20 rows"):
            step.bind(window_of(strict, [4, 5, SHORT, 6]))
        with pytest.raises(ValueError, match="fp32 window's feature scale"):
            step.bind(window_of(harness.ResidentCohort(cohort_slides(), dev, bag_dtype=torch.float32, cycle=True), ids))
        with pytest.raises(ValueError, match="sample_rows"):
            harness.GraphedWindowStep(model, bucket, window_of(cohort, first), 4, opt=None, warmup=0)
        check_replay(step, cohort, ids, eager, grads=False)
        torch.cuda.synchronize()
    finally:
        ops.set_rng_epoch(None)


def test_captured_nacagat_step_on_a_cohort(dev):
    ops.set_rng_epoch(None)
    try:
        cohort = harness.ResidentCohort(cohort_slides(), dev, cycle=True)
        model, eager = fusion_model("nacagat", dev), fusion_model("nacagat", dev)
        bucket = FlatGradBucket(list(model.parameters()))
        step = harness.GraphedWindowStep(model, bucket, window_of(cohort, [0, 1, 2, 3]), 4, opt=None, warmup=1, sample_rows=32)
        ids = [6, SHORT, 9, 4]
        step.bind(window_of(cohort, ids))
        check_replay(step, cohort, ids, eager, grads=False)
        torch.cuda.synchronize()
    finally:
        ops.set_rng_epoch(None)


def test_eager_training_on_a_slide_set(dev):
    """train_window(sample_rows=k) on a SlideSet goes to the slide gather (lapped here); in eval mode it materializes."""
    ops.set_rng_epoch(None)
    cohort = harness.ResidentCohort(cohort_slides(), dev, cycle=True)
    ids = [4, SHORT, 6, 5]
    window = window_of(cohort, ids)
    model_a, model_b = fusion_model("mcat", dev), fusion_model("mcat", dev)
    stream = (torch.initial_seed() & 0xFFFFFFFFFFFFFFFF, ops.rng_state()["calls"])       # the sampler's is the step's first stream
    loss_a, _ = harness.train_window(model_a, *window, 4, sample_rows=32)
    rows = expected_rows([cohort.rows[i] for i in ids], stream, 32, 0, True)
    loss_b, _ = harness.train_window(model_b, BagBatch.from_lengths(rows, [32] * 4), *window[1:], 4)
    torch.testing.assert_close(loss_a, loss_b, **LOSS_TOL)
    whole = window[0].materialize()
    assert whole.lengths == [cohort.lengths[i] for i in ids] and same_bits(whole.data, torch.cat([cohort.rows[i] for i in ids]))
    model_a.eval()
    with_k, _ = harness.train_window(model_a, *window, 4, sample_rows=32)
    without, _ = harness.train_window(model_a, whole, *window[1:], 4)
    torch.testing.assert_close(with_k, without, rtol=1e-5, atol=1e-6)


def test_train_epoch(dev):
    """10 slides in 4-slide windows, Adam inside the graph: two windows run, two ids are left over; the loop itself runs
    under torch.cuda.set_sync_debug_mode("error"), which this torch build honours on ROCm (the guarded `int(tensor)` below
    raises), so a host synchronisation inside train_epoch that torch can see fails the test.  torch calls the mode a prototype
    that does not detect every synchronising operation: it sees torch's own (item, nonzero, blocking copies), not one hidden
    inside a library call."""
    ops.set_rng_epoch(None)
    try:
        cohort = harness.ResidentCohort(cohort_slides(), dev, cycle=True)
        model = fusion_model("mcat", dev)
        bucket = FlatGradBucket(list(model.parameters()))
        opt = FlatAdam(bucket, lr=1e-3, weight_decay=1e-5)
        step = harness.GraphedWindowStep(model, bucket, window_of(cohort, [0, 1, 2, 3]), 4, opt=opt, warmup=1, sample_rows=32)
        before = opt.flat_p.clone()
        orders = [[3, SHORT, 0, 9, 5, 1, 8, 2, 6, 4], [9, 2, 4, 6, 0, 8, SHORT, 3, 1, 5]]
        results = []
        probe = torch.ones(1, device=dev)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):
                int(probe)                                   # the mode is honoured: a synchronising call raises
            for order in orders:
                results.append(harness.train_epoch(step, cohort, order))
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert int(opt.t_dev) == 4 and not torch.equal(opt.flat_p, before)               # two windows per epoch; the parameters moved
        for order, (loss, risk, ids_run, leftover) in zip(orders, results):
            assert leftover == order[8:] and ids_run.tolist() == order[:8] and ids_run.dtype == torch.int32
            assert loss.shape == risk.shape == (8,) and loss.is_cuda and risk.is_cuda
            assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(risk).all())
        assert not torch.equal(results[0][0], results[1][0])
        # in the order of ids_run: the last window's values are what the step's own outputs still hold
        torch.testing.assert_close(results[1][0][4:], step.loss.view(-1))
        torch.testing.assert_close(results[1][1][4:], step.risk.view(-1))
        _, risk, ids_run, _ = results[1]
        event = (1 - cohort.censorship[ids_run.long()]).bool().cpu().numpy()
        c = harness.concordance_index_censored(event, cohort.survival_months[ids_run.long()].cpu().numpy(), risk.cpu().numpy())
        assert 0.0 <= c <= 1.0
        with pytest.raises(ValueError, match="outside the cohort"):
            harness.train_epoch(step, cohort, [0, 1, 2, 10])
        strict = harness.ResidentCohort(cohort_slides(), dev, cycle=False)
        with pytest.raises(ValueError, match="slide 7 has 20 rows"):
            harness.train_epoch(step, strict, list(range(10)))
    finally:
        ops.set_rng_epoch(None)
