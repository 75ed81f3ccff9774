"""HIP-graph replay of the window step: equals the eager step with dropout off, and draws fresh dropout masks
on every replay with dropout on (device-resident RNG epoch), with Adam's bias correction following the
device-resident step count."""
import pytest
import torch

import cases as C
from multimodal_path_omic_amd import harness, ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.dp import FlatAdam, FlatGradBucket
from multimodal_path_omic_amd.models import MultimodalCoAttentionTransformer

pytestmark = pytest.mark.gpu


def setup(dev, train_mode, bag_dtype=torch.bfloat16):
    sizes = [64] * 6
    model = MultimodalCoAttentionTransformer(omic_sizes=sizes, bag_dtype=bag_dtype)
    model.load_state_dict(syn.fill_state_dict(C.model_shapes(sizes, False), 55))
    model.to(dev)
    model.train(train_mode)
    slides = syn.make_cohort(6, 200, 700, sizes, 56)
    window = harness.make_window(slides, dev, bag_dtype)
    bucket = FlatGradBucket(list(model.parameters()))
    opt = FlatAdam(bucket, lr=1e-3, weight_decay=1e-5)
    return model, bucket, opt, window


def test_graph_replay_equals_eager_steps(dev):
    ops.set_rng_epoch(None)
    model_e, bucket_e, opt_e, window_e = setup(dev, False)
    losses_e = []
    for _ in range(4):
        bucket_e.begin()
        loss, _ = harness.train_window(model_e, *window_e, 6)
        bucket_e.finish()
        opt_e.step()
        losses_e.append(loss.clone())
    ops.set_rng_epoch(None)
    model_g, bucket_g, opt_g, window_g = setup(dev, False)
    step = harness.GraphedWindowStep(model_g, bucket_g, window_g, 6, opt=opt_g, warmup=0)   # capture = step 1
    losses_g = [step.loss.clone()]
    # the capture pass does not execute kernels; replay 4 times = steps 1..4
    losses_g = []
    for _ in range(4):
        loss, _ = step()
        losses_g.append(loss.clone())
    for a, b in zip(losses_e, losses_g):
        torch.testing.assert_close(a, b, rtol=2e-3, atol=2e-4)
    assert float(losses_g[-1].mean()) < float(losses_g[0].mean())        # it trains
    torch.testing.assert_close(opt_e.flat_p, opt_g.flat_p, rtol=5e-3, atol=5e-4)
    assert int(opt_g.t_dev) == 4
    ops.set_rng_epoch(None)


def test_graph_replays_draw_fresh_dropout_masks(dev):
    ops.set_rng_epoch(None)
    model, bucket, _, window = setup(dev, True)
    step = harness.GraphedWindowStep(model, bucket, window, 6, opt=None, warmup=1)
    try:
        epoch0 = int(step.epoch)

        def replay():
            return step()[0].clone(), bucket.flat.clone()
        (l1, b1), (l2, b2), (l3, b3) = replay(), replay(), replay()
        assert not torch.equal(l1, l2) and not torch.equal(l2, l3)           # same weights, different masks
        assert torch.isfinite(l1).all() and torch.isfinite(bucket.flat).all()
        assert not torch.equal(b1, b2) and not torch.equal(b2, b3)           # ... and other gradients
        # the epoch tensor set back: the first replay again, twice -- bit-identical to it where the two re-runs are to each
        # other, else within twice their difference (the rule of tests/test_gpu_checkpoint.py::_hold)
        again = []
        for _ in range(2):
            step.epoch.fill_(epoch0)
            again.append(replay())
        for first, (x, y) in zip((l1, b1), zip(*again)):
            noise = float((x.double() - y.double()).abs().max())
            diff = float((first.double() - x.double()).abs().max())
            assert torch.equal(first, x) if noise == 0.0 else diff <= 2 * noise, (noise, diff)
    finally:
        ops.set_rng_epoch(None)


@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_split_step_fills_the_same_bucket(dev, kind):
    """Data-parallel steps capture the patch layer's weight gradient into a second graph (run while the all-reduce of
    the other gradients is in flight): main + tail must leave exactly the gradients of the one-graph step, and the main
    graph alone must not touch the head slice."""
    from multimodal_path_omic_amd.models import NarrowContextualAttentionGateTransformer
    ops.set_rng_epoch(None)
    sizes = [64] * 6
    cls = MultimodalCoAttentionTransformer if kind == "mcat" else NarrowContextualAttentionGateTransformer

    def build():
        model = cls(omic_sizes=sizes, bag_dtype=torch.bfloat16)
        model.load_state_dict(syn.fill_state_dict(C.model_shapes(sizes, kind == "nacagat"), 55))
        model.to(dev).eval()
        window = harness.make_window(syn.make_cohort(6, 200, 700, sizes, 56), dev, torch.bfloat16)
        return model, FlatGradBucket(list(model.parameters())), window
    model_a, bucket_a, window_a = build()
    one = harness.GraphedWindowStep(model_a, bucket_a, window_a, 6, opt=None, warmup=1)
    one()
    ref = bucket_a.flat.clone()
    model_b, bucket_b, window_b = build()
    two = harness.GraphedWindowStep(model_b, bucket_b, window_b, 6, opt=None, warmup=1, split_patch_grad=True)
    head = two.head_numel()
    assert head == model_b.H[0].weight.numel()
    bucket_b.flat[:head].fill_(123.0)
    two()                                                           # main graph only
    assert torch.equal(bucket_b.flat[:head], torch.full_like(bucket_b.flat[:head], 123.0))
    torch.testing.assert_close(bucket_b.flat[head:], ref[head:], rtol=0, atol=0)
    two.replay_tail()
    torch.testing.assert_close(bucket_b.flat, ref, rtol=0, atol=0)
    assert not ops._deferred_patch
    ops.set_rng_epoch(None)


def test_graph_refuses_an_fp32_window_written_after_capture(dev):
    """An fp32 window's feature scale (ops.feature_scale, one host read) is a kernel argument baked into the graph: a
    replay after an in-place write to that window would compute with the stale scale, so it must raise instead.  The
    check is a host-side compare of the window's version counter; bf16 windows carry no such scale."""
    ops.set_rng_epoch(None)
    model, bucket, _, window = setup(dev, False, torch.float32)
    step = harness.GraphedWindowStep(model, bucket, window, 6, opt=None, warmup=1, prime=False)
    loss, _ = step()
    assert torch.isfinite(loss).all()
    window[0].data.copy_(window[0].data * 50.0)
    with pytest.raises(RuntimeError, match="written in place after capture"):
        step()
    ops.set_rng_epoch(None)
    model, bucket, _, window = setup(dev, False, torch.bfloat16)
    step = harness.GraphedWindowStep(model, bucket, window, 6, opt=None, warmup=1, prime=False)
    window[0].data.mul_(1.0)
    loss, _ = step()                                       # (bf16: nothing frozen from the window's contents)
    assert torch.isfinite(loss).all()
    torch.cuda.synchronize()
    ops.set_rng_epoch(None)
