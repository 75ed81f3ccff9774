"""Patch feature widths 512 and 2048 (constructor argument `patch_dim`) on the bf16 patch-layer kernels: the forward kernel's
K schedule is built per width (csrc/patch_fc_fwd.hip, Sched<PK>: 16 / 64 k-stages per chunk, period 24 / 72, the second
stream 12 / 36 stages behind, chunk rotation wrapping after 512 / 2048 rows), everything above it takes the width from the
weight.  Bars are those of the width-1024 tests named at each check.

A window of a few thousand rows is cut into one 128-row chunk per workgroup, so the schedule's chunk-to-chunk part (two
streams alternating chunks, requests crossing chunk boundaries, the rotation's wrap) would not run at test sizes:
`ops.plan_workgroups` = 1 / 3 gives a workgroup up to 18 chunks, and every cut must give the same bits."""
import math

import pytest
import torch

import cases as C
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import checkpoint, harness, ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.dp import FlatAdam, FlatGradBucket, FlatOptimizer
from multimodal_path_omic_amd.harness import ces_loss
from multimodal_path_omic_amd.models import (GeneExprNarrowContextualAttentionGateTransformer,
                                             MultimodalCoAttentionTransformer, NarrowContextualAttentionGateTransformer)
from multimodal_path_omic_amd.ops import BagBatch
from oracle import mpo_oracle as O

pytestmark = pytest.mark.gpu
WIDTHS = [512, 2048]
EMBEDS = [128, 256, 512]
RAGGED = [2200, 65, 1, 515]
NAN = float("nan")


def relmax(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def relerr(a, b):
    a, b = a.detach().float().cpu().reshape(-1), b.detach().float().cpu().reshape(-1)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


_layers = {}


def _layer(dev, width, embed):
    """W_H (embed, width) ~ N(0, 1 / width), b ~ N(0, 0.01), 2781 rows of N(0, 1) features in bf16 and the layer's fp64 value
    on the bf16-rounded operands: made once per geometry, shared by the tests below, never written."""
    key = (width, embed)
    if key not in _layers:
        g = syn.rng(7000 + width + embed)
        w = syn.normal(g, (embed, width), 1.0 / math.sqrt(width)).to(dev)
        b = syn.normal(g, (embed,), 0.1).to(dev)
        x = syn.normal(g, (sum(RAGGED), width)).to(dev).to(torch.bfloat16)
        ref = torch.relu(x.double() @ w.bfloat16().double().t() + b.double())
        _layers[key] = (w, b, x, ref)
    return _layers[key]


class _Cut:
    """ops.plan_workgroups for the plans built inside the block."""

    def __init__(self, wgs):
        self.wgs = wgs

    def __enter__(self):
        self.old, ops.plan_workgroups = ops.plan_workgroups, self.wgs

    def __exit__(self, *exc):
        ops.plan_workgroups = self.old


def _raw_forward(x_rows, lengths, w, b, wgs=None, drop_p=0.0, seed=0, off=0):
    """mpo_patch_fc_forward on operands carved out of NaN-filled buffers (64 guard rows behind X and behind H_bag) and a
    workspace carved out of a patterned one: returns H_bag after checking that nothing outside it was written."""
    dev, rows, width, embed = x_rows.device, x_rows.shape[0], x_rows.shape[1], w.shape[0]
    xbuf = torch.full((rows + 64, width), NAN, device=dev, dtype=torch.bfloat16)
    xbuf[:rows] = x_rows
    hbuf = torch.full((rows + 64, embed), NAN, device=dev, dtype=torch.bfloat16)
    nbytes = L.lib().mpo_patch_fc_workspace_bytes(embed, width)
    assert nbytes >= max(embed, 256) * width * 2                  # the packed bf16 weight: whole 256-row blocks
    wsbuf = torch.full((nbytes + 4096,), 0xA5, device=dev, dtype=torch.uint8)
    x, h, ws = xbuf[:rows], hbuf[:rows], wsbuf[:nbytes]
    with _Cut(wgs):
        batch = BagBatch(x, ops.make_cu(lengths, dev), list(lengths))
        plan = batch.plan()
    L.call("mpo_patch_fc_forward", L.ptr(x), L.ptr(batch.cu), batch.n_slides, batch.total_rows, batch.max_rows, width,
           L.ptr(w), L.ptr(b), embed, float(drop_p), seed, off, None, L.ptr(h), plan, L.ptr(ws), ws.numel(), L.stream_of(x))
    assert torch.isnan(hbuf[rows:]).all() and torch.isnan(xbuf[rows:]).all()
    assert bool((wsbuf[nbytes:] == 0xA5).all())
    assert torch.isfinite(h.float()).all()
    return h


# ------------------------------------------------------------------------------------ the layer's forward
@pytest.mark.parametrize("lengths", [[1], [127], [128], [129], [385], [2200], RAGGED], ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("embed", EMBEDS)
@pytest.mark.parametrize("width", WIDTHS)
def test_layer_forward_equals_fp64_of_the_rounded_operands(dev, width, embed, lengths):
    """Bar of tests/test_gpu_patch_coattn.py (the 1024 layer): 2^-7 of the largest entry -- H_bag is bf16.  2200 rows are 18
    chunks: past the rotation's wrap at both widths.  One workgroup per chunk (the plan's own cut at this size), one
    workgroup for everything and three for the window: the same bits."""
    w, b, x_all, ref_all = _layer(dev, width, embed)
    rows = sum(lengths)
    x, ref = x_all[:rows], ref_all[:rows]
    h = _raw_forward(x, lengths, w, b)
    err = relmax(h.double(), ref)
    print(f"[patch widths] {width} -> {embed} rows {lengths}: {err:.3e} of the largest entry (bar {2.0 ** -7:.3e})")
    assert err < 2.0 ** -7
    for wgs in (1, 3):
        assert torch.equal(_raw_forward(x, lengths, w, b, wgs=wgs), h), wgs


@pytest.mark.parametrize("embed", EMBEDS)
@pytest.mark.parametrize("width", WIDTHS)
def test_window_equals_slide_by_slide(dev, width, embed):
    """ops.patch_fc on the ragged window against every slide on its own, bit for bit, in eval mode; in training mode at a
    fixed ops._rng_calls the dropout counter is (window row x embed / 16 + column group), so a slide on its own draws the
    mask of the window's FIRST rows: the first slide is equal outright, the others in every element both runs kept (the
    values under the mask), and the whole window -- mask included -- is equal under every cut into workgroups."""
    w, b, x, _ = _layer(dev, width, embed)
    batch = BagBatch(x, ops.make_cu(RAGGED, dev), list(RAGGED))
    for drop_p in (0.0, 0.25):
        ops._rng_calls = 4100
        h = ops.patch_fc(x, w, b, drop_p, batch=batch)
        assert h.shape == (sum(RAGGED), embed) and h.dtype == torch.bfloat16
        ops._rng_calls = 4100
        assert torch.equal(_raw_forward(x, RAGGED, w, b, drop_p=drop_p, seed=torch.initial_seed() & (2 ** 64 - 1), off=4100), h)
        r0 = 0
        for i, m in enumerate(RAGGED):
            ops._rng_calls = 4100
            alone = ops.patch_fc(x[r0:r0 + m].contiguous(), w, b, drop_p)
            part = h[r0:r0 + m]
            if drop_p == 0.0 or i == 0:
                assert torch.equal(alone, part), (drop_p, i)
            else:
                both = (alone != 0) & (part != 0)
                assert int(both.sum()) > 0.2 * both.numel() or m == 1
                assert torch.equal(alone[both], part[both]), (drop_p, i)
            r0 += m
        for wgs in (1, 3):
            with _Cut(wgs):
                cut = BagBatch(x, ops.make_cu(RAGGED, dev), list(RAGGED))
                ops._rng_calls = 4100
                assert torch.equal(ops.patch_fc(x, w, b, drop_p, batch=cut), h), (drop_p, wgs)


# ------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("embed", EMBEDS)
@pytest.mark.parametrize("width", WIDTHS)
def test_dropout_masks(dev, width, embed):
    """test_fused_dropout_masks' checks at its bars: same stream -> same mask, the next -> another; realised rate within
    0.005 of 0.25 (2781 x embed / 2 positives: sigma <= 1.1e-3), kept / eval = 4 / 3 within 0.02 (both sides bf16), every
    column's rate within 0.06 (~1400 positives per column: sigma 0.012), and the keep scale on the tensor."""
    w, b, x, ref = _layer(dev, width, embed)
    batch = BagBatch(x, ops.make_cu(RAGGED, dev), list(RAGGED))
    h0 = ops.patch_fc(x, w, b, 0.0, batch=batch)
    ops._rng_calls = 900
    h1 = ops.patch_fc(x, w, b, 0.25, batch=batch)
    ops._rng_calls = 900
    h2 = ops.patch_fc(x, w, b, 0.25, batch=batch)
    assert torch.equal(h1, h2)
    h3 = ops.patch_fc(x, w, b, 0.25, batch=batch)                # next offset -> another mask
    assert not torch.equal(h1, h3)
    assert abs(h1._mpo_keep_scale - 1.0 / 0.75) < 1e-12
    pos = h0 > 0
    dropped = pos & (h1 == 0)
    rate = float(dropped.sum()) / float(pos.sum())
    assert abs(rate - 0.25) < 0.005, rate
    kept = pos & (h1 != 0)
    ratio = h1[kept].float() / h0[kept].float()
    assert float((ratio - 4.0 / 3.0).abs().max()) < 0.02
    col_rate = dropped.float().sum(0) / pos.float().sum(0).clamp_min(1)
    assert float((col_rate - 0.25).abs().max()) < 0.06, float((col_rate - 0.25).abs().max())
    assert not bool(((h1 != 0) & ~pos).any())                    # nothing appears where the layer is zero


# ------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("embed", EMBEDS)
@pytest.mark.parametrize("width", WIDTHS)
def test_backward_equals_fp64(dev, width, embed):
    """dW_H and db_H through ops.patch_fc (csrc/patch_wgrad.hip, which has taken these widths all along) at the 5e-3 of the
    1024 layer's test: the incoming gradient reaches the layer in bf16, so the fp64 side takes the rounded probe."""
    w0, b0, x, ref = _layer(dev, width, embed)
    w, b = w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    batch = BagBatch(x, ops.make_cu(RAGGED, dev), list(RAGGED))
    h = ops.patch_fc(x, w, b, 0.0, batch=batch)
    gen = torch.Generator(device=dev).manual_seed(width + embed)
    probe = torch.randn(h.shape, device=dev, generator=gen) * 0.01
    gw, gb = torch.autograd.grad((h.float() * probe).sum(), [w, b])
    g = probe.bfloat16().double() * (ref > 0)
    gw_ref, gb_ref = g.t() @ x.double(), g.sum(0)
    e_w, e_b = relmax(gw.double(), gw_ref), relmax(gb.double(), gb_ref)
    print(f"[patch widths] backward {width} -> {embed}: dW {e_w:.3e} db {e_b:.3e} (bar 5e-3)")
    assert gw.shape == (embed, width) and e_w < 5e-3 and e_b < 5e-3, (e_w, e_b)


# ------------------------------------------------------------------------------------ whole models
OMIC_SIZES = [64, 100, 256, 31, 8, 300]
MODEL_ROWS = [300, 65, 515]


def _fusion_model(kind, width, dev, bag_dtype, seed=4242, sizes=OMIC_SIZES):
    cls = MultimodalCoAttentionTransformer if kind == "mcat" else NarrowContextualAttentionGateTransformer
    model = cls(omic_sizes=sizes, bag_dtype=bag_dtype, patch_dim=width)
    shapes = C.model_shapes(sizes, kind == "nacagat")
    shapes["H.0.weight"] = (256, width)
    sd = syn.fill_state_dict(shapes, seed)
    model.load_state_dict(sd, strict=True)
    return model.to(dev).eval(), sd


def _ge_model(width, dev, bag_dtype, seed=4343):
    model = GeneExprNarrowContextualAttentionGateTransformer(bag_dtype=bag_dtype, patch_dim=width)
    shapes = C.ge_model_shapes()
    shapes["H.0.weight"] = (256, width)
    sd = syn.fill_state_dict(shapes, seed)
    model.load_state_dict(sd, strict=True)
    return model.to(dev).eval(), sd


def _fusion_inputs(width, dev, dtype, seed, rows=MODEL_ROWS, sizes=OMIC_SIZES):
    g = syn.rng(seed)
    wsis = [syn.normal(g, (m, width)) for m in rows]
    omics = [[syn.normal(g, (s,)) for s in sizes] for _ in rows]
    bags = BagBatch.from_list([x.to(dev).to(dtype) for x in wsis])
    om_w = [torch.stack([omics[b][i] for b in range(len(rows))]).to(dev) for i in range(len(sizes))]
    return wsis, omics, bags, om_w


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
@pytest.mark.parametrize("width", WIDTHS)
def test_fusion_models_equal_the_oracle(dev, width, kind, dtype):
    """One eval-mode window per model and width against the oracle slide by slide.  bf16 window: the oracle stores what the
    kernels store (bag_storage=bf16) and the bar is tests/test_gpu_models.py's for that comparison, 2e-4 on hazards and
    survival.  fp32 window (ops.linear + dropout, as for the small / big models): that file's fp32 bars, 1e-4 on hazards /
    survival / Y, 1e-3 on the pooling scores and element-wise on the co-attention map."""
    model, sd = _fusion_model(kind, width, dev, dtype)
    wsis, omics, bags, om_w = _fusion_inputs(width, dev, dtype, 515 + width)
    hz, sv, y, att = model.forward_window(bags, om_w, inference=True)
    fwd = O.mcat_forward if kind == "mcat" else O.nacagat_forward
    kw = dict(inference=True) if kind == "mcat" else {}
    if dtype == torch.bfloat16:
        kw["bag_storage"] = torch.bfloat16
    for i in range(len(MODEL_ROWS)):
        hz_o, sv_o, y_o, att_o = fwd(sd, wsis[i], omics[i], **kw)
        e_h, e_s, e_y = (float((a[i].detach().cpu() - o[0]).abs().max()) for a, o in ((hz, hz_o), (sv, sv_o), (y, y_o)))
        print(f"[patch widths] {kind} {width} {dtype} slide {i}: hazards {e_h:.2e} survs {e_s:.2e} Y {e_y:.2e}")
        if dtype == torch.bfloat16:
            assert e_h < 2e-4 and e_s < 2e-4, (i, e_h, e_s)
        else:
            assert e_h < 1e-4 and e_s < 1e-4 and e_y < 1e-4, (i, e_h, e_s, e_y)
            assert relerr(att["path"][i], att_o["path"]) < 1e-3 and relerr(att["omic"][i], att_o["omic"]) < 1e-3
            a, a_o = att["coattn"][i].cpu(), att_o["coattn"]
            assert ((a - a_o).abs() / a_o.clamp_min(1e-30)).max().item() < 1e-3, i


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("width", WIDTHS)
def test_gene_expression_model_equals_the_oracle(dev, width, dtype):
    """tests/test_gpu_bag_selfattn.py's bars: bf16 storage 2e-4 on Y and 2e-3 on the pooling scores against the oracle with
    the same storage; fp32 1e-4 on Y, 1e-3 on the pooling scores and element-wise on the M x M map."""
    model, sd = _ge_model(width, dev, dtype)
    g = syn.rng(616 + width)
    wsis = [syn.normal(g, (m, width)) for m in MODEL_ROWS]
    bags = BagBatch.from_list([x.to(dev).to(dtype) for x in wsis])
    y, att = model.forward_window(bags, need_maps=True)
    for i, wsi in enumerate(wsis):
        kw = dict(bag_storage=torch.bfloat16) if dtype == torch.bfloat16 else {}
        y_o, att_o = O.ge_nacagat_forward(sd, wsi, **kw)
        e_y, e_p = float((y[i].cpu() - y_o).abs().max()), relerr(att["path"][i], att_o["path"])
        print(f"[patch widths] ge {width} {dtype} slide {i}: Y {e_y:.2e} path {e_p:.2e}")
        if dtype == torch.bfloat16:
            assert e_y < 2e-4 and e_p < 2e-3, (i, e_y, e_p)
        else:
            assert e_y < 1e-4 and e_p < 1e-3, (i, e_y, e_p)
            a, a_o = att["attn"][i].cpu(), att_o["attn"]
            assert ((a - a_o).abs() / a_o.clamp_min(1e-30)).max().item() < 1e-3, i


# ------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
@pytest.mark.parametrize("width", WIDTHS)
def test_training_window_equals_per_slide_accumulation(dev, width, kind):
    """test_full_size_bf16_training_window_equals_per_slide at these widths and [300, 65, 515] rows: harness.train_window
    against the slides one at a time through forward() and the separate loss, at that test's bars (loss 2e-5, risk 1e-5,
    gradients 5e-4 of the largest entry; H.*: the pre-activation gradient travels in bf16 and one element landing on the
    other bf16 neighbour moves a row of dW_H by up to 2^-8 of a dominant element -- 4e-3 there; NaCAGaT's K2 gradient has
    been seen at 1.7e-3 against MCAT's 4.7e-4, and its bar here is 5e-3)."""
    model, _ = _fusion_model(kind, width, dev, torch.bfloat16, seed=991)
    n = len(MODEL_ROWS)
    wsis, omics, bags, om_w = _fusion_inputs(width, dev, torch.bfloat16, 992 + width)
    labels = (torch.arange(n) % 4).to(dev)
    cens = (torch.arange(n) % 2).float().to(dev)
    per_slide, risk = harness.train_window(model, bags, om_w, labels, cens, grad_acc_step=n)
    grads_w = {k: p.grad.clone() for k, p in model.named_parameters()}
    assert grads_w["H.0.weight"].shape == (256, width)
    model.zero_grad()
    r0 = 0
    for b, m in enumerate(MODEL_ROWS):
        hz, sv, y, att = model(wsi=bags.data[r0:r0 + m], omics=[o.to(dev) for o in omics[b]])
        loss = ces_loss(hz, sv, labels[b:b + 1], cens[b:b + 1])
        assert abs(float(loss) - float(per_slide[b])) < 2e-5 * max(1.0, abs(float(loss))), (b, float(loss), float(per_slide[b]))
        assert abs(float(-sv.sum()) - float(risk[b])) < 1e-5
        (loss / n).backward()
        r0 += m
    h_bar = 5e-3 if kind == "nacagat" else 4e-3
    for k, p in model.named_parameters():
        scale = max(float(p.grad.abs().max()), 1e-3)
        err = float((grads_w[k] - p.grad).abs().max()) / scale
        assert err < (h_bar if k.startswith("H.") else 5e-4), (k, err)


# ------------------------------------------------------------------------------------ graphed step, checkpoint
def _train_objects(dev, width, seed):
    sizes = [64] * 6
    model, _ = _fusion_model("mcat", width, dev, torch.bfloat16, seed=seed, sizes=sizes)
    window = harness.make_window(syn.make_cohort(6, 200, 700, sizes, 56, patch_dim=width), dev, torch.bfloat16)
    bucket = FlatGradBucket(list(model.parameters()))
    return model, bucket, window


def test_graphed_step_at_width_512_equals_eager_steps(dev):
    """tests/test_gpu_graph.py's rule (losses rtol 2e-3 / atol 2e-4, parameters rtol 5e-3 / atol 5e-4, the device-side step
    count) for three replays of a captured window step with Adam against three eager steps from the same state."""
    ops.set_rng_epoch(None)
    model_e, bucket_e, window_e = _train_objects(dev, 512, 55)
    assert window_e[0].data.shape[1] == 512
    opt_e = FlatAdam(bucket_e, lr=1e-3, weight_decay=1e-5)
    losses_e = []
    for _ in range(3):
        bucket_e.begin()
        loss, _ = harness.train_window(model_e, *window_e, 6)
        bucket_e.finish()
        opt_e.step()
        losses_e.append(loss.clone())
    ops.set_rng_epoch(None)
    model_g, bucket_g, window_g = _train_objects(dev, 512, 55)
    opt_g = FlatAdam(bucket_g, lr=1e-3, weight_decay=1e-5)
    step = harness.GraphedWindowStep(model_g, bucket_g, window_g, 6, opt=opt_g, warmup=0)
    losses_g = [step()[0].clone() for _ in range(3)]
    for a, b in zip(losses_e, losses_g):
        torch.testing.assert_close(a, b, rtol=2e-3, atol=2e-4)
    torch.testing.assert_close(opt_e.flat_p, opt_g.flat_p, rtol=5e-3, atol=5e-4)
    assert int(opt_g.t_dev) == 3
    assert float(losses_g[-1].mean()) < float(losses_g[0].mean())        # it trains
    torch.cuda.synchronize()
    ops.set_rng_epoch(None)


def test_checkpoint_round_trip_at_width_2048(dev, tmp_path):
    """checkpoint.save / load of a width-2048 MCAT after two Adam steps into new objects with other weights: parameters and
    both moments bit-equal, the patch weight (256, 2048) among them."""
    ops.set_rng_epoch(None)
    model, bucket, window = _train_objects(dev, 2048, 55)
    opt = FlatOptimizer(bucket, "adam", lr=1e-3, weight_decay=1e-5)
    for _ in range(2):
        bucket.begin()
        harness.train_window(model, *window, 6)
        bucket.finish()
        opt.step()
    path = tmp_path / "ck.pt"
    checkpoint.save(path, model, opt, 0, 0.0)
    assert tuple(checkpoint.peek(path)["model_state_dict"]["H.0.weight"].shape) == (256, 2048)
    model2, bucket2, _ = _train_objects(dev, 2048, 77)
    opt2 = FlatOptimizer(bucket2, "adam", lr=1e-3, weight_decay=1e-5)
    assert not torch.equal(opt2.flat_p, opt.flat_p)
    checkpoint.load(path, model2, opt2)
    assert int(opt2.t_dev) == 2
    moments = list(zip(opt.state_tensors(), opt2.state_tensors()))
    assert len(moments) >= 3 and all(torch.equal(a, b) for a, b in moments)
    assert any(float(a.abs().max()) > 0 for a, _ in moments[1:])
    for (k, a), (_, b) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert torch.equal(a, b), k
    # a model of another width does not take the file
    model3, _, _ = _train_objects(dev, 512, 77)
    with pytest.raises(RuntimeError, match="H.0.weight"):
        model3.load_state_dict(checkpoint.peek(path)["model_state_dict"])


# ------------------------------------------------------------------------------------ refusals
def test_refusals(dev):
    for kind in ("mcat", "nacagat"):
        model, _ = _fusion_model(kind, 512, dev, torch.bfloat16)
        _, _, bags, om_w = _fusion_inputs(1024, dev, torch.bfloat16, 5, rows=[40, 33])
        with pytest.raises(ValueError, match="patch_dim=512"):        # a window of another width than the model's
            model.forward_window(bags, om_w)
        with pytest.raises(ValueError, match="patch_dim=512"):
            model(wsi=bags.data[:40], omics=[o[0] for o in om_w])
    ge, _ = _ge_model(2048, dev, torch.bfloat16)
    bags = BagBatch.from_list([torch.zeros(40, 512, device=dev, dtype=torch.bfloat16)])
    with pytest.raises(ValueError, match="patch_dim=2048"):
        ge.forward_window(bags)
    with pytest.raises(ValueError, match="patch_dim=2048"):
        ge(bags.data)
    with pytest.raises(ValueError, match=r"patch_dim 768.*512.*1024.*2048"):
        MultimodalCoAttentionTransformer(omic_sizes=OMIC_SIZES, patch_dim=768)
    x = torch.zeros(100, 768, device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=r"patch layer.*512.*1024.*2048"):
        ops.patch_fc(x, torch.zeros(256, 768, device=dev), torch.zeros(256, device=dev), 0.0)
    with pytest.raises(ValueError, match="patch layer"):              # the window is not as wide as the weight
        ops.patch_fc(x, torch.zeros(256, 512, device=dev), torch.zeros(256, device=dev), 0.0)
    # the C entry itself names the set
    h = torch.empty(100, 256, device=dev, dtype=torch.bfloat16)
    ws = torch.empty(1 << 20, device=dev, dtype=torch.uint8)
    cu = ops.make_cu([100], dev)
    with pytest.raises(RuntimeError, match=r"\{512, 1024, 2048\}"):
        L.call("mpo_patch_fc_forward", L.ptr(x), L.ptr(cu), 1, 100, 100, 768, L.ptr(torch.zeros(256, 768, device=dev)),
               L.ptr(torch.zeros(256, device=dev)), 256, 0.0, 0, 0, None, L.ptr(h), None, L.ptr(ws), ws.numel(), L.stream_of(x))
