"""Fixed-budget patch sampling on the device (csrc/bag_sample.hip, ops.RowSampler, harness sample_rows / bind): the gather
against x[idx] with idx restated on the host (tests/row_sampling_replay.py), bit for bit; the device epoch; the models and
the training steps on the sampler's output against the same step on the pre-gathered window; the captured step re-pointed
at another window.

Where two training paths are compared, dropout is off (p = 0) and the bars are the ones tests/test_gpu_graph.py holds a
replay to against an eager step (restated, not imported)."""
import pytest
import torch

import cases as C
import row_sampling_replay as R
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import harness, ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.dp import FlatGradBucket
from multimodal_path_omic_amd.models import (GeneExprNarrowContextualAttentionGateTransformer,
                                             MultimodalCoAttentionTransformer, NarrowContextualAttentionGateTransformer)
from multimodal_path_omic_amd.ops import BagBatch

pytestmark = pytest.mark.gpu

LOSS_TOL, PARAM_TOL = dict(rtol=2e-3, atol=2e-4), dict(rtol=5e-3, atol=5e-4)
SIZES = [64] * 6


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def window_rows(lengths, width, dtype, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return BagBatch.from_list([torch.randn(m, width, generator=g).to(device=dev, dtype=dtype) for m in lengths])


def expected_rows(bags, stream, k, epoch):
    """x[idx] with idx restated on the host from the sampler's (seed, offset) and the epoch."""
    _, flat = R.window_indices(stream[0], stream[1], epoch, bags.lengths, k)
    return bags.data[torch.from_numpy(flat).to(bags.data.device)]


# ------------------------------------------------------------------------------------------------ the gather
@pytest.mark.parametrize("width", [512, 1024, 2048])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_gather_equals_indexing_bit_for_bit(dev, dtype, width):
    ops.set_rng_epoch(None)
    # eager mode: slides shorter than k are passed whole; output lengths [1, 32, 32, 32]
    bags = window_rows([1, 33, 700, 4097], width, dtype, dev, 1)
    before = bags.data.clone()
    s = ops.RowSampler(4, 32, width, dtype, dev, static=False).bind(bags)
    s.out.fill_(float("nan"))
    out = s()
    assert out.lengths == [1, 32, 32, 32] and out.cu.tolist() == [0, 1, 33, 65, 97] and out.data.shape == (97, width)
    assert same_bits(out.data, expected_rows(bags, s.last_stream, 32, 0))
    assert bool(torch.isnan(s.out[97:]).all())                              # rows behind the output are not written
    assert same_bits(bags.data, before)                                     # the source is not written
    # static mode through the C ABI, into a buffer with guard rows behind n_slides * k
    bags = window_rows([32, 33, 4097], width, dtype, dev, 2)
    big = torch.full((3 * 32 + 4, width), float("nan"), dtype=dtype, device=dev)
    desc = torch.zeros(L.lib().mpo_bag_sample_desc_bytes(3) // 8, dtype=torch.int64, device=dev)
    L.call("mpo_bag_sample_bind", L.ptr(desc), L.ptr(bags.data), L.ptr(bags.cu), 3, 32, L.stream_of(desc))
    L.call("mpo_bag_sample_rows", L.ptr(desc), 3, 32, width, bags.data.element_size(), 77, 5, None, L.ptr(big), L.stream_of(big))
    assert same_bits(big[:96], expected_rows(bags, (77, 5), 32, 0))
    assert bool(torch.isnan(big[96:]).all())
    assert desc.view(torch.int32)[2:10].tolist() == [0, 32, 65, 4162, 0, 32, 64, 96] and int(desc[0]) == bags.data.data_ptr()
    # ... and through the sampler: its static batch is built at construction and is the one every call returns
    s = ops.RowSampler(3, 32, width, dtype, dev)
    batch = s.batch
    assert batch.lengths == [32, 32, 32] and batch._plan is not None
    assert s.bind(bags)() is batch and same_bits(batch.data, expected_rows(bags, s.last_stream, 32, 0))
    first = batch.data.clone()
    s()
    assert not same_bits(batch.data, first)                                 # every eager call draws anew
    with pytest.raises(ValueError, match="slide 1 has 31 rows"):
        s.bind(window_rows([40, 31, 50], width, dtype, dev, 3))


@pytest.mark.parametrize("dtype,width,k", [(torch.bfloat16, 8, 32), (torch.bfloat16, 264, 32), (torch.bfloat16, 1032, 32),
                                           (torch.float32, 1028, 32), (torch.bfloat16, 8, 30), (torch.bfloat16, 512, 30),
                                           (torch.bfloat16, 1024, 31), (torch.bfloat16, 2048, 31), (torch.float32, 2048, 31)])
def test_gather_at_other_widths_and_unaligned_k(dev, dtype, width, k):
    """Rows that are a multiple of 16 bytes but not 1, 2, 4 or 8 KiB take the kernel's loop form: one vector, fewer than a
    wave's 64, and more than 64 with a remainder.  A wave moves 4 rows (the loop form, 1 KiB rows), 2 (2 KiB) or 1 (4 and
    8 KiB): with k = 30 resp. 31 a slide boundary falls inside one wave's rows wherever a wave has more than one."""
    ops.set_rng_epoch(None)
    bags = window_rows([1, 33, 700], width, dtype, dev, 6)
    s = ops.RowSampler(3, k, width, dtype, dev, static=False).bind(bags)
    s.out.fill_(float("nan"))
    assert same_bits(s().data, expected_rows(bags, s.last_stream, k, 0))
    assert bool(torch.isnan(s.out[1 + 2 * k:]).all())


@pytest.mark.parametrize("width,lengths,k", [(1024, [20000, 17000], 17000), (8, [40000, 3], 39999)])
def test_gather_of_many_rows(dev, width, lengths, k):
    """Tens of thousands of output rows (thousands of workgroups), and a slide drawn whole: a 17 000-row permutation."""
    ops.set_rng_epoch(None)
    g = torch.Generator(device=dev).manual_seed(7)
    data = torch.randn(sum(lengths), width, device=dev, generator=g).to(torch.bfloat16)
    bags = BagBatch.from_lengths(data, lengths)
    s = ops.RowSampler(2, k, width, torch.bfloat16, dev, static=False).bind(bags)
    s.out.fill_(float("nan"))
    out = s()
    assert out.total_rows == sum(min(k, m) for m in lengths) > 30000
    assert same_bits(out.data, expected_rows(bags, s.last_stream, k, 0))
    assert bool(torch.isnan(s.out[out.total_rows:]).all())


def test_refused_geometries(dev):
    with pytest.raises(ValueError, match="not a multiple of 16 bytes"):
        ops.RowSampler(2, 4, 1020, torch.bfloat16, dev)
    with pytest.raises(ValueError, match="at least 1"):
        ops.RowSampler(2, 0, 1024, torch.bfloat16, dev)
    s = ops.RowSampler(2, 4, 1024, torch.bfloat16, dev)
    with pytest.raises(RuntimeError, match="bind"):
        s()
    with pytest.raises(ValueError, match="3 slides"):
        s.bind(window_rows([5, 5, 5], 1024, torch.bfloat16, dev, 1))
    with pytest.raises(ValueError, match="width 1024"):
        s.bind(window_rows([5, 5], 512, torch.bfloat16, dev, 1))
    with pytest.raises(ValueError, match="float32"):
        s.bind(window_rows([5, 5], 1024, torch.float32, dev, 1))


def test_epoch_bump_moves_the_draw(dev):
    epoch = torch.zeros(1, dtype=torch.int64, device=dev)
    ops.set_rng_epoch(epoch)
    try:
        bags = window_rows([700, 64, 4097], 512, torch.bfloat16, dev, 4)
        s = ops.RowSampler(3, 64, 512, torch.bfloat16, dev).bind(bags)
        assert same_bits(s().data, expected_rows(bags, s.last_stream, 64, 0))
        ops.bump_step_counters(epoch, None)
        got = s().data
        assert int(epoch) == 1
        assert same_bits(got, expected_rows(bags, s.last_stream, 64, 1))
        assert not same_bits(got, expected_rows(bags, s.last_stream, 64, 0))
    finally:
        ops.set_rng_epoch(None)


def test_rng_state_restores_the_draws(dev):
    ops.set_rng_epoch(None)
    bags = window_rows([300, 90], 1024, torch.bfloat16, dev, 5)
    s = ops.RowSampler(2, 48, 1024, torch.bfloat16, dev).bind(bags)
    saved = ops.rng_state()
    a = s().data.clone()
    b = s().data.clone()
    assert not same_bits(a, b)
    assert ops.rng_state()["calls"] == saved["calls"] + 2 * (ops.RowSampler.RNG_SPAN + 1)     # the documented span
    ops.set_rng_state(saved, device=dev)
    assert same_bits(s().data, a) and same_bits(s().data, b)


# ------------------------------------------------------------------------------------------------ models on the sample
def fusion_model(kind, dev, dropout=0.25, bag_dtype=torch.bfloat16):
    cls = MultimodalCoAttentionTransformer if kind == "mcat" else NarrowContextualAttentionGateTransformer
    model = cls(omic_sizes=SIZES, bag_dtype=bag_dtype, dropout=dropout)
    model.load_state_dict(syn.fill_state_dict(C.model_shapes(SIZES, kind == "nacagat"), 55))
    if dropout == 0.0:                       # the pooling heads' rate is hard-wired (models/blocks.py:34-36): off with the rest
        model.path_attention_head.drop_p = model.omic_attention_head.drop_p = 0.0
    return model.to(dev)


@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_model_on_the_sample_equals_model_on_gathered_rows(dev, kind):
    ops.set_rng_epoch(None)
    model = fusion_model(kind, dev).eval()
    slides = syn.make_cohort(3, 40, 300, SIZES, 61)
    bags, omics, _, _ = harness.make_window(slides, dev, torch.bfloat16)
    s = ops.RowSampler(3, 64, 1024, torch.bfloat16, dev, static=False).bind(bags)
    with torch.no_grad():
        hz, sv, y, _ = model.forward_window(s(), omics)
        per, _ = R.window_indices(*s.last_stream, 0, bags.lengths, 64)
        rows = [x[torch.from_numpy(i).to(dev)] for x, i in zip(bags.data.split(bags.lengths), per)]
        hz_r, sv_r, y_r, _ = model.forward_window(BagBatch.from_list(rows), omics)
    # the same bits through the same kernels on the same grids: what is left is the order of fp32 atomic sums
    for a, b in ((hz, hz_r), (sv, sv_r), (y, y_r)):
        print(f"[{kind}] max |diff| {float((a - b).abs().max()):.1e}")
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


def grads_of(model):
    return {n: p.grad for n, p in model.named_parameters() if p.grad is not None}


def test_eager_training_on_the_sample(dev):
    ops.set_rng_epoch(None)
    slides = syn.make_cohort(4, 20, 400, SIZES, 62)
    slides[1]["wsi"] = slides[1]["wsi"][:20]                     # one slide shorter than k: passed whole
    window = harness.make_window(slides, dev, torch.bfloat16)
    bags = window[0]
    model_a, model_b = fusion_model("mcat", dev, dropout=0.0).train(), fusion_model("mcat", dev, dropout=0.0).train()
    stream = (torch.initial_seed() & 0xFFFFFFFFFFFFFFFF, ops.rng_state()["calls"])       # the sampler's is the step's first stream
    loss_a, risk_a = harness.train_window(model_a, *window, 4, sample_rows=32)
    per, _ = R.window_indices(*stream, 0, bags.lengths, 32)
    assert [len(p) for p in per] == [min(32, m) for m in bags.lengths] and min(bags.lengths) == 20
    rows = [x[torch.from_numpy(i).to(dev)] for x, i in zip(bags.data.split(bags.lengths), per)]
    loss_b, risk_b = harness.train_window(model_b, BagBatch.from_list(rows), *window[1:], 4)
    print(f"[eager] loss diff {float((loss_a - loss_b).abs().max()):.1e}")
    torch.testing.assert_close(loss_a, loss_b, **LOSS_TOL)
    torch.testing.assert_close(risk_a, risk_b, **LOSS_TOL)
    ga, gb = grads_of(model_a), grads_of(model_b)
    assert ga.keys() == gb.keys() and len(ga) > 20
    for n in ga:
        torch.testing.assert_close(ga[n], gb[n], **PARAM_TOL, msg=lambda m, n=n: f"{n}: {m}")
    # eval mode: sample_rows changes nothing and takes no stream
    model_a.eval()
    calls = ops.rng_state()["calls"]
    with_k, _ = harness.train_window(model_a, *window, 4, sample_rows=32)
    assert ops.rng_state()["calls"] == calls
    without, _ = harness.train_window(model_a, *window, 4)
    torch.testing.assert_close(with_k, without, rtol=1e-5, atol=1e-6)


def test_eager_ge_training_on_the_sample(dev):
    ops.set_rng_epoch(None)

    def build():
        model = GeneExprNarrowContextualAttentionGateTransformer(dropout=0.0)
        model.load_state_dict(syn.fill_state_dict(C.ge_model_shapes(), 32), strict=True)
        model.path_attention_head.drop_p = 0.0          # (hard-wired 0.25 otherwise)
        return model.to(dev).train()
    model_a, model_b = build(), build()
    wsi, target = C.ge_model_inputs(300, 33)
    bags, labels = harness.make_ge_window([dict(wsi=wsi, gene_expr_class=int(target))], dev)
    stream = (torch.initial_seed() & 0xFFFFFFFFFFFFFFFF, ops.rng_state()["calls"])
    loss_a = harness.train_ge_window(model_a, bags, labels, 1, sample_rows=64)
    idx = torch.from_numpy(R.permutation_prefix(*stream, 0, 0, 300, 64)).to(dev)
    loss_b = harness.train_ge_window(model_b, BagBatch.from_list([bags.data[idx]]), labels, 1)
    print(f"[ge] loss {float(loss_a)} vs {float(loss_b)}")
    torch.testing.assert_close(loss_a, loss_b, **LOSS_TOL)
    ga, gb = grads_of(model_a), grads_of(model_b)
    assert ga.keys() == gb.keys() and len(ga) > 10
    for n in ga:
        torch.testing.assert_close(ga[n], gb[n], **PARAM_TOL, msg=lambda m, n=n: f"{n}: {m}")
    with pytest.raises(ValueError, match="at least 17 rows"):
        harness.train_ge_window(model_a, bags, labels, 1, sample_rows=16)
    model_a.eval()
    with_k = harness.train_ge_window(model_a, bags, labels, 1, sample_rows=64)
    without = harness.train_ge_window(model_a, bags, labels, 1)
    torch.testing.assert_close(with_k, without, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ the captured step
def test_graphed_step_samples_anew_and_follows_bind(dev):
    ops.set_rng_epoch(None)
    try:
        model = fusion_model("mcat", dev, dropout=0.0).train()
        eager = fusion_model("mcat", dev, dropout=0.0).train()          # same weights, no bucket: the eager yardstick
        bucket = FlatGradBucket(list(model.parameters()))
        window = harness.make_window(syn.make_cohort(4, 200, 700, SIZES, 56), dev, torch.bfloat16)
        step = harness.GraphedWindowStep(model, bucket, window, 4, opt=None, warmup=1, sample_rows=32)
        stream = step.sampler.last_stream                                # the offset baked at capture
        assert step.sampler.batch.lengths == [32] * 4

        def replay_and_check(win):
            loss = step()[0].clone()
            sample = step.sampler.out.clone()
            assert same_bits(sample, expected_rows(win[0], stream, 32, int(step.epoch)))
            eager.zero_grad(set_to_none=True)
            ref, _ = harness.train_window(eager, BagBatch.from_lengths(sample, [32] * 4), *win[1:], 4)
            print(f"[graph] epoch {int(step.epoch)} loss diff {float((loss - ref).abs().max()):.1e}")
            torch.testing.assert_close(loss, ref, **LOSS_TOL)
            return sample
        samples = [replay_and_check(window) for _ in range(3)]
        assert not same_bits(samples[0], samples[1]) and not same_bits(samples[1], samples[2]) \
            and not same_bits(samples[0], samples[2])
        # another window, other ragged lengths, other omics / labels / censorship
        window2 = harness.make_window(syn.make_cohort(4, 200, 700, SIZES, 57), dev, torch.bfloat16)
        assert window2[0].lengths != window[0].lengths
        step.bind(window2)
        replay_and_check(window2)
        assert torch.equal(step.window[2], window2[2]) and step.window[2] is window[2]       # copied into the static tensors
        # refusals, each with its reason
        with pytest.raises(ValueError, match="3 slides"):
            step.bind(harness.make_window(syn.make_cohort(3, 200, 300, SIZES, 58), dev, torch.bfloat16))
        short = syn.make_cohort(4, 200, 300, SIZES, 59)
        short[2]["wsi"] = short[2]["wsi"][:31]
        with pytest.raises(ValueError, match="slide 2 has 31 rows"):
            step.bind(harness.make_window(short, dev, torch.bfloat16))
        narrow = syn.make_cohort(4, 200, 300, SIZES, 60, patch_dim=512)
        with pytest.raises(ValueError, match="width 1024"):
            step.bind(harness.make_window(narrow, dev, torch.bfloat16))
        with pytest.raises(ValueError, match="fp32 window's feature scale"):
            step.bind(harness.make_window(syn.make_cohort(4, 200, 300, SIZES, 56), dev, torch.float32))
        replay_and_check(window2)                                        # a refused bind leaves the step as it was
        with pytest.raises(ValueError, match="fp32 window's feature scale"):
            harness.GraphedWindowStep(model, bucket, harness.make_window(syn.make_cohort(4, 200, 300, SIZES, 56), dev, torch.float32),
                                      4, opt=None, warmup=0, sample_rows=32)
        torch.cuda.synchronize()
    finally:
        ops.set_rng_epoch(None)


def test_unsampled_step_cannot_be_rebound(dev):
    ops.set_rng_epoch(None)
    try:
        model = fusion_model("mcat", dev).eval()
        bucket = FlatGradBucket(list(model.parameters()))
        window = harness.make_window(syn.make_cohort(2, 40, 80, SIZES, 56), dev, torch.bfloat16)
        with pytest.raises(ValueError, match="eval mode"):
            harness.GraphedWindowStep(model, bucket, window, 2, opt=None, warmup=0, sample_rows=32)
        step = harness.GraphedWindowStep(model, bucket, window, 2, opt=None, warmup=1, prime=False)
        with pytest.raises(ValueError, match="captured without sample_rows"):
            step.bind(window)
        torch.cuda.synchronize()
    finally:
        ops.set_rng_epoch(None)
