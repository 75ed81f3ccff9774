"""The gated-concat head on the GPU (csrc/fusion_next.hip + K6, include/mpo_fusion_next.h): the C-ABI entries against the fp64
restatement of tests/fusion_replay.py (itself pinned to the oracle and to fusion_next.npz by tests/test_fusion_next_cpu.py), the
fused training-step loss against the composed one on whole models, and the path a training step takes."""
import os
import re

import pytest
import torch

import cases as C
import fusion_replay as F
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import harness, ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.models import MultimodalCoAttentionTransformer, NarrowContextualAttentionGateTransformer
from tail_helpers import Guarded

pytestmark = pytest.mark.gpu

# bars (the project's own): outputs 1e-4 absolute (hazards / survs / Y are probabilities), fused output and per-slide loss
# 1e-4 relative (tests/test_gpu_tail.py:374), gradients 2e-3 of the reference gradient's max (tests/test_gpu_tail.py:420)
OUT_ATOL, REL_TOL, GRAD_TOL = 1e-4, 1e-4, 2e-3


def _kernel_constant(name):
    with open(os.path.join(os.path.dirname(ops.__file__), "csrc", "fusion_next.hip")) as f:
        return int(re.search(rf"constexpr int {name} = (\d+);", f.read()).group(1))


# The two row kernels give one wave to a (slide, branch) row, kGateWaves rows to a workgroup: a slide tile is kGateWaves / 2
# slides.  The parameter-gradient kernel loops over the slides (no tile).
SLIDE_TILE = _kernel_constant("kGateWaves") // 2
N_SLIDES = sorted({1,                                            # one row pair, half a workgroup
                   SLIDE_TILE - 1, SLIDE_TILE, SLIDE_TILE + 1,      # below, at and above one workgroup of the row kernels
                   2 * SLIDE_TILE, 2 * SLIDE_TILE + 1,              # ... and the second tile boundary (a ragged last workgroup)
                   33} - {0})                                       # many workgroups; K6's GEMMs past their 32-row tile


def _case(d, b, c, seed):
    g = syn.rng(seed)
    sd = syn.fill_state_dict(F.gated_concat_shapes(d, c), seed + 1)
    h = syn.normal(g, (2, b, d))
    label = torch.arange(b) % c
    cens = ((torch.arange(b) // 2) % 2).float()
    probes = [syn.normal(g, (b, c)) for _ in range(3)]
    w = torch.rand(b, generator=torch.Generator().manual_seed(seed)) * 0.5 + 0.1
    return sd, h, label, cens, probes, w


def _reference(sd, h, form, label, cens, probes, w):
    """fp64: outputs and the gradients of what the entry differentiates -> (dict of outputs, [d_h_path, d_h_omic, 10 grads])."""
    p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    hp, ho = (h[i].double().requires_grad_(True) for i in range(2))
    if form == "plain":
        fused, hz, sv, y = F.gated_concat_head(hp, ho, p)
        out = {"hazards": hz, "survs": sv, "y": y}
        scalar = sum((t * pr.double()).sum() for t, pr in zip((hz, sv, y), probes))
    else:
        loss, risk, hz, sv, y = F.gated_concat_head_loss(hp, ho, p, label, cens, form)
        out = {"hazards": hz, "survs": sv, "y": y, "loss": loss, "risk": risk}
        scalar = (loss * w.double()).sum()
    grads = torch.autograd.grad(scalar, [hp, ho] + [p[k] for k in sd], allow_unused=True)
    grads = [g if g is not None else torch.zeros_like(t) for g, t in zip(grads, [hp, ho] + [p[k] for k in sd])]
    return {k: v.detach() for k, v in out.items()}, grads


def _run_entry(dev, sd, h, form, label, cens, probes, w, interleaved):
    """One forward + backward through the C ABI with every output, `saved`, the workspace and every gradient in NaN-filled
    buffers between NaN guards.  interleaved: rows (B, [h_path | h_omic]) with stride 2 d, else (2, B, d) with stride d."""
    lib = L.lib()
    _, b, d = h.shape
    c = sd["classifier.weight"].shape[0]
    G = Guarded(dev)
    rows = (torch.cat([h[0], h[1]], dim=1) if interleaved else h).contiguous()
    hbuf = G.buf(rows.numel(), rows)
    ld, omic = (2 * d, d) if interleaved else (d, b * d)
    params = [v.to(dev).contiguous() for v in sd.values()]
    pa = L.ptr_array(params)
    hz, sv, y = (G.buf(b * c) for _ in range(3))
    loss, risk = G.buf(b), G.buf(b)
    with_loss = form != "plain"
    saved = G.buf((lib.mpo_gated_concat_head_loss_saved_floats if with_loss else lib.mpo_gated_concat_head_saved_floats)(b, d, c))
    ws_bytes = lib.mpo_gated_concat_head_workspace_bytes(b, d, c)
    ws = G.buf(ws_bytes // 4)
    d_h = G.buf(rows.numel())
    grads = [G.buf(p.numel()) for p in params]
    ga = L.ptr_array(grads)
    s = L.stream_of(hbuf)
    hp = L.ptr(hbuf)
    if not with_loss:
        L.call("mpo_gated_concat_head_forward", hp, hp + 4 * omic, ld, b, d, c, pa, L.ptr(hz), L.ptr(sv), L.ptr(y), L.ptr(saved), s)
        dprobe = [pr.to(dev).contiguous() for pr in probes]
        L.call("mpo_gated_concat_head_backward", hp, hp + 4 * omic, ld, b, d, c, pa, L.ptr(saved), L.ptr(hz), L.ptr(sv), L.ptr(y),
               L.ptr(dprobe[0]), L.ptr(dprobe[1]), L.ptr(dprobe[2]), L.ptr(d_h), L.ptr(d_h) + 4 * omic, ga, L.ptr(ws), ws_bytes, s)
    else:
        lab, cen, wd = label.to(dev), cens.to(dev), w.to(dev)
        L.call("mpo_gated_concat_head_loss_forward", hp, hp + 4 * omic, ld, b, d, c, pa, L.ptr(lab), L.ptr(cen), L.ptr(wd), 0.75, 1e-7,
               ("ces", "sct").index(form), L.ptr(hz), L.ptr(sv), L.ptr(y), L.ptr(loss), L.ptr(risk), L.ptr(saved), s)
        L.call("mpo_gated_concat_head_loss_backward", hp, hp + 4 * omic, ld, b, d, c, pa, L.ptr(saved), L.ptr(d_h),
               L.ptr(d_h) + 4 * omic, ga, L.ptr(ws), ws_bytes, s)
    G.check(f"{form} b={b} d={d} interleaved={interleaved}")            # nothing written outside any buffer
    out = {"hazards": hz.view(b, c), "survs": sv.view(b, c), "y": y.view(b, c)}
    if with_loss:
        out.update(loss=loss, risk=risk)
    dh = d_h.view(b, 2 * d) if interleaved else d_h.view(2, b, d)
    d_hp, d_ho = (dh[:, :d], dh[:, d:]) if interleaved else (dh[0], dh[1])
    return out, [d_hp, d_ho] + [g.view(p.shape) for g, p in zip(grads, params)]


def _compare(tag, got, ref, names):
    out, grads = got
    out_ref, grads_ref = ref
    for k, want in out_ref.items():
        have = out[k].double().cpu()
        assert bool(torch.isfinite(have).all()), f"{tag}: {k} has unwritten (NaN) elements"
        err = float((have - want).abs().max())
        bar = OUT_ATOL if k in ("hazards", "survs", "y") else REL_TOL * max(float(want.abs().max()), 1.0)
        assert err < bar, (tag, k, err, bar)
    for n, have, want in zip(names, grads, grads_ref):
        have = have.double().cpu()
        assert bool(torch.isfinite(have).all()), f"{tag}: gradient of {n} has unwritten (NaN) elements"
        err = float((have - want).abs().max()) / max(float(want.abs().max()), 1e-5)
        assert err < GRAD_TOL, (tag, n, err)


def _check(dev, d, b, c, form, seed):
    sd, h, label, cens, probes, w = _case(d, b, c, seed)
    ref = _reference(sd, h, form, label, cens, probes, w)
    names = ["h_path", "h_omic"] + list(sd)
    for interleaved in (True, False):                               # row stride 2 d, then d
        got = _run_entry(dev, sd, h, form, label, cens, probes, w, interleaved)
        _compare(f"{form} d={d} b={b} c={c} interleaved={interleaved}", got, ref, names)


@pytest.mark.parametrize("form", ["plain", "ces", "sct"])
@pytest.mark.parametrize("b", N_SLIDES)
@pytest.mark.parametrize("d", F.D_BUILT)
def test_entries_match_fp64_at_every_slide_tile_edge(dev, d, b, form):
    _check(dev, d, b, 4, form, 5000 + 7 * d + b)


@pytest.mark.parametrize("form", ["plain", "ces", "sct"])
@pytest.mark.parametrize("c", [1, F.MAX_CLASSES])
def test_entries_match_fp64_at_the_class_range_edges(dev, c, form):
    """n_classes 1 and 16: the smallest and the largest the head kernels accept."""
    _check(dev, 256, 3, c, form, 6000 + c)


@pytest.mark.parametrize("form", ["plain", "ces"])
def test_entries_match_fp64_at_300_slides(dev, form):
    """The largest window the layout goldens exercise K6 at: nothing in the new kernels assumes a tile count."""
    _check(dev, 128, 300, 4, form, 6100)


def test_entry_matches_fp64_on_the_golden_case(dev):
    """The inputs and weights of tests/golden/fusion_next.npz (d = 256): the CPU suite holds the fp64 restatement to that
    file's outputs and gradients, this holds the kernels to the restatement on the same rows."""
    sd = syn.fill_state_dict(C.GATED_CONCAT_SHAPES, 720)
    sd.update(syn.fill_state_dict({"classifier.weight": (4, C.E), "classifier.bias": (4,)}, 721))
    hp, ho, _ = C.fusion_inputs()
    h = torch.stack([torch.stack([hp, ho * 0.5, -hp]), torch.stack([ho, hp, ho * 2.0])])
    _, _, label, cens, probes, w = _case(C.E, 3, 4, 6200)
    for form in ("plain", "ces", "sct"):
        ref = _reference(sd, h, form, label, cens, probes, w)
        for interleaved in (True, False):
            got = _run_entry(dev, sd, h, form, label, cens, probes, w, interleaved)
            _compare(f"golden rows {form} interleaved={interleaved}", got, ref, ["h_path", "h_omic"] + list(sd))


def test_gate_gradients_are_bit_equal_from_run_to_run(dev):
    """dw and db of the gates are summed over the slides in a fixed order (no atomics)."""
    sd, h, label, cens, probes, w = _case(256, 33, 4, 6300)
    runs = [_run_entry(dev, sd, h, "ces", label, cens, probes, w, True)[1] for _ in range(2)]
    for a, b in zip(runs[0][2:6], runs[1][2:6]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------- whole models
OMIC_SIZES, ROWS, SLIDES = [64, 100, 256, 31, 8, 300], 900, 3


def _model(dev, kind, seed, bag_dtype=torch.float32):
    cls = MultimodalCoAttentionTransformer if kind == "mcat" else NarrowContextualAttentionGateTransformer
    model = cls(omic_sizes=OMIC_SIZES, fusion="gated_concat", bag_dtype=bag_dtype)
    model.load_state_dict(syn.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed), strict=True)
    return model.to(dev).eval()


def _window(dev, seed, bag_dtype=torch.float32):
    slides = syn.make_cohort(SLIDES, ROWS, ROWS, OMIC_SIZES, seed)
    return harness.make_window(slides, dev, bag_dtype)


@pytest.mark.parametrize("kind,loss", [("mcat", "ces"), ("mcat", "sct"), ("nacagat", "ces")])
def test_fused_loss_equals_the_composed_one(dev, kind, loss):
    """forward_window(ces_targets=...) against forward_window() + ops.ces_loss / ops.sct_loss: per-slide loss, risk and every
    parameter gradient.  Both run the same kernels up to the head, so the bars above are generous here."""
    model = _model(dev, kind, 7300)
    bags, omics, labels, cens = _window(dev, 7301)
    w = torch.full((SLIDES,), 0.25, device=dev)
    before = dict(ops.stats)
    _, _, _, att = model.forward_window(bags, omics, ces_targets=(labels, cens, w), fused_loss=loss)
    att["loss"].backward(w)
    assert ops.stats["head_loss_" + loss] == before["head_loss_" + loss] + 1
    assert ops.stats["gated_concat_head"] == before["gated_concat_head"] + 1
    fused = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    hz, sv, y, _ = model.forward_window(bags, omics)
    if loss == "ces":
        ref_loss, ref_risk = ops.ces_loss(hz, sv, labels, cens)
    else:
        ref_loss, ref_risk = ops.sct_loss(y, labels, cens), harness.risk_score(sv.detach())
    ref_loss.backward(w)
    assert float((att["loss"].detach() - ref_loss.detach()).abs().max()) < REL_TOL * max(float(ref_loss.detach().abs().max()), 1.0)
    assert float((att["risk"] - ref_risk).abs().max()) < OUT_ATOL * SLIDES
    for n, p in model.named_parameters():
        scale = max(float(p.grad.abs().max()), 1e-5)
        assert float((fused[n] - p.grad).abs().max()) / scale < GRAD_TOL, n


@pytest.mark.parametrize("loss", ["ces", "sct"])
def test_training_step_takes_the_fused_path(dev, loss):
    model = _model(dev, "mcat", 7400)
    window = _window(dev, 7401)
    before = dict(ops.stats)
    per_slide, risk = harness.train_window(model, *window, 4, loss=loss)
    assert ops.stats["gated_concat_head"] == before["gated_concat_head"] + 1
    assert ops.stats["head_loss_" + loss] == before["head_loss_" + loss] + 1
    assert per_slide.shape == (SLIDES,) and risk.shape == (SLIDES,) and bool(torch.isfinite(per_slide).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def test_reference_call_goes_through_the_gated_concat_head(dev):
    """model(wsi, omics), the reference's one-slide call, follows forward_window."""
    model = _model(dev, "mcat", 7500)
    wsi, omics, _, _ = C.model_inputs(ROWS, OMIC_SIZES, 7501)
    before = ops.stats["gated_concat_head"]
    hz, sv, y, _ = model(wsi=wsi.to(dev), omics=[o.to(dev) for o in omics])
    assert ops.stats["gated_concat_head"] == before + 1 and hz.shape == (1, 4)


def test_graphed_gated_concat_step_equals_eager_steps(dev):
    """A captured window step with fusion="gated_concat" (the head inside the graph, Adam too) replays what the eager steps
    compute; the bars are those tests/test_gpu_graph.py holds the `concat` step to."""
    from multimodal_path_omic_amd.dp import FlatAdam, FlatGradBucket

    def setup():
        ops.set_rng_epoch(None)
        model = _model(dev, "mcat", 7600, torch.bfloat16)              # (a bf16 window: the form the graphed step is run in)
        bucket = FlatGradBucket(list(model.parameters()))
        return model, bucket, FlatAdam(bucket, lr=1e-3, weight_decay=1e-5), _window(dev, 7601, torch.bfloat16)

    model_e, bucket_e, opt_e, window_e = setup()
    eager = []
    for _ in range(3):
        bucket_e.begin()
        loss, _ = harness.train_window(model_e, *window_e, SLIDES)
        bucket_e.finish()
        opt_e.step()
        eager.append(loss.clone())
    model_g, bucket_g, opt_g, window_g = setup()
    before = ops.stats["gated_concat_head"]
    step = harness.GraphedWindowStep(model_g, bucket_g, window_g, SLIDES, opt=opt_g, warmup=0)
    assert ops.stats["gated_concat_head"] == before + 1                 # the capture ran the head's call once
    graphed = [step()[0].clone() for _ in range(3)]
    ops.set_rng_epoch(None)
    for a, b in zip(eager, graphed):
        torch.testing.assert_close(a, b, rtol=2e-3, atol=2e-4)
    torch.testing.assert_close(opt_e.flat_p, opt_g.flat_p, rtol=5e-3, atol=5e-4)


# =============================================================================================== bilinear head
import functools                                                                            # noqa: E402

from tail_helpers import FWD_TOL, GRAD_TOL as TRAIN_GRAD_TOL, OFF, P, SEED, _pin            # noqa: E402  (test_gpu_train_dropout.py's bars)


def _bilinear_slide_tile(d):
    """Slides a workgroup of the pass over the bilinear weights keeps in LDS: the TB of bilinear_z_*_kernel<NS, TB> as
    mpo_launch_bilinear_z_fwd / _bwd instantiate it (d <= 256: <1, 16>; d = 512: <2, 8>)."""
    with open(os.path.join(os.path.dirname(ops.__file__), "csrc", "fusion_next.hip")) as f:
        src = f.read()
    small, big = (int(re.search(rf"bilinear_z_{w}_kernel<{ns}, (\d+)><<<", src).group(1)) for w, ns in (("bwd", 1), ("bwd", 2)))
    assert (small, big) == tuple(int(re.search(rf"bilinear_z_fwd_kernel<{ns}, (\d+)><<<", src).group(1)) for ns in (1, 2))
    return small if d <= 256 else big


def _bilinear_n_slides(d):
    tb = _bilinear_slide_tile(d)
    # 1; one below, at and one above the slide tile of the W pass; 33: more than one tile at every d (3 at TB = 16, 5 at TB = 8),
    # a ragged last one, and K6's GEMMs past their 32-row tile
    return sorted({1, tb - 1, tb, tb + 1, 33})


@functools.lru_cache(maxsize=None)
def _bilinear_weights(d, c):
    # gain 1 = the layer's own initialisation scale (N(0, 1 / sqrt(fan_in))).  Larger weights saturate the head: at gain 2 the
    # fp64 reference has survs down to 2e-11, under the `ces` loss's eps clamp of 1e-7, where -log(S) turns a 1e-4-relative
    # error of the fused output (the bar it is held to) into 1e-3 of loss -- the loss bar below would then say nothing about
    # the kernels.  The golden case further down keeps the reference fixture's gain of 3.
    return syn.fill_state_dict(F.bilinear_shapes(d, c), 8000 + d + c)


def _bilinear_case(d, b, c, seed):
    g = syn.rng(seed)
    h = syn.normal(g, (2, b, d))
    label = torch.arange(b) % c
    cens = ((torch.arange(b) // 2) % 2).float()
    probes = [syn.normal(g, (b, c)) for _ in range(3)]
    w = torch.rand(b, generator=torch.Generator().manual_seed(seed)) * 0.5 + 0.1
    return _bilinear_weights(d, c), h, label, cens, probes, w


def _bilinear_reference(sd, h, form, label, cens, probes, w, keeps=None):
    p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    hp, ho = (h[i].double().requires_grad_(True) for i in range(2))
    if form == "plain":
        _, hz, sv, y = F.bilinear_head(hp, ho, p, keeps)
        out = {"hazards": hz, "survs": sv, "y": y}
        scalar = sum((t * pr.double()).sum() for t, pr in zip((hz, sv, y), probes))
    else:
        loss, risk, hz, sv, y = F.bilinear_head_loss(hp, ho, p, label, cens, form, keeps)
        out = {"hazards": hz, "survs": sv, "y": y, "loss": loss, "risk": risk}
        scalar = (loss * w.double()).sum()
    leaves = [hp, ho] + [p[k] for k in sd]
    grads = torch.autograd.grad(scalar, leaves, allow_unused=True)
    return {k: v.detach() for k, v in out.items()}, [g if g is not None else torch.zeros_like(t) for g, t in zip(grads, leaves)]


def _run_bilinear_entry(dev, sd, h, form, label, cens, probes, w, interleaved, rng=(0.0, 0, 0), epoch=None):
    """As _run_entry: every output, `saved`, the workspace and every gradient NaN-filled between NaN guards."""
    lib = L.lib()
    _, b, d = h.shape
    c = sd["classifier.weight"].shape[0]
    G = Guarded(dev)
    rows = (torch.cat([h[0], h[1]], dim=1) if interleaved else h).contiguous()
    hbuf = G.buf(rows.numel(), rows)
    ld, omic = (2 * d, d) if interleaved else (d, b * d)
    params = [v.to(dev).contiguous() for v in sd.values()]
    pa = L.ptr_array(params)
    hz, sv, y = (G.buf(b * c) for _ in range(3))
    loss, risk = G.buf(b), G.buf(b)
    with_loss = form != "plain"
    saved = G.buf((lib.mpo_bilinear_head_loss_saved_floats if with_loss else lib.mpo_bilinear_head_saved_floats)(b, d, c))
    ws_bytes = lib.mpo_bilinear_head_workspace_bytes(b, d, c)
    ws = G.buf(ws_bytes // 4)
    d_h = G.buf(rows.numel())
    grads = [G.buf(p.numel()) for p in params]
    ga = L.ptr_array(grads)
    s, hp, ep = L.stream_of(hbuf), L.ptr(hbuf), L.ptr(epoch)
    head = (hp, hp + 4 * omic, ld, b, d, 32, 64, c, pa, float(rng[0]), int(rng[1]), int(rng[2]), ep)
    if not with_loss:
        L.call("mpo_bilinear_head_forward", *head, L.ptr(hz), L.ptr(sv), L.ptr(y), L.ptr(saved), s)
        dprobe = [pr.to(dev).contiguous() for pr in probes]
        L.call("mpo_bilinear_head_backward", *head, L.ptr(saved), L.ptr(hz), L.ptr(sv), L.ptr(y), L.ptr(dprobe[0]), L.ptr(dprobe[1]),
               L.ptr(dprobe[2]), L.ptr(d_h), L.ptr(d_h) + 4 * omic, ga, L.ptr(ws), ws_bytes, s)
    else:
        lab, cen, wd = label.to(dev), cens.to(dev), w.to(dev)
        L.call("mpo_bilinear_head_loss_forward", *head, L.ptr(lab), L.ptr(cen), L.ptr(wd), 0.75, 1e-7, ("ces", "sct").index(form),
               L.ptr(hz), L.ptr(sv), L.ptr(y), L.ptr(loss), L.ptr(risk), L.ptr(saved), s)
        L.call("mpo_bilinear_head_loss_backward", *head, L.ptr(saved), L.ptr(d_h), L.ptr(d_h) + 4 * omic, ga, L.ptr(ws), ws_bytes, s)
    G.check(f"bilinear {form} b={b} d={d} interleaved={interleaved}")
    out = {"hazards": hz.view(b, c), "survs": sv.view(b, c), "y": y.view(b, c)}
    if with_loss:
        out.update(loss=loss, risk=risk)
    dh = d_h.view(b, 2 * d) if interleaved else d_h.view(2, b, d)
    d_hp, d_ho = (dh[:, :d], dh[:, d:]) if interleaved else (dh[0], dh[1])
    return out, [d_hp, d_ho] + [g.view(p.shape) for g, p in zip(grads, params)]


def _bilinear_check(dev, d, b, c, form, seed):
    sd, h, label, cens, probes, w = _bilinear_case(d, b, c, seed)
    ref = _bilinear_reference(sd, h, form, label, cens, probes, w)
    for interleaved in (True, False):
        got = _run_bilinear_entry(dev, sd, h, form, label, cens, probes, w, interleaved)
        _compare(f"bilinear {form} d={d} b={b} c={c} interleaved={interleaved}", got, ref, ["h_path", "h_omic"] + list(sd))


BILINEAR_EDGES = [(d, b) for d in F.D_BUILT for b in _bilinear_n_slides(d)]


@pytest.mark.parametrize("form", ["plain", "ces", "sct"])
@pytest.mark.parametrize("d,b", BILINEAR_EDGES)
def test_bilinear_entries_match_fp64_at_every_slide_tile_edge(dev, d, b, form):
    _bilinear_check(dev, d, b, 4, form, 8100 + 7 * d + b)


@pytest.mark.parametrize("form", ["plain", "ces", "sct"])
@pytest.mark.parametrize("c", [1, F.MAX_CLASSES])
def test_bilinear_entries_match_fp64_at_the_class_range_edges(dev, c, form):
    _bilinear_check(dev, 256, 3, c, form, 8200 + c)


def test_bilinear_entry_matches_fp64_on_the_golden_case(dev):
    """Inputs and weights of tests/golden/fusion_next.npz (d = 256, weight gain 3): see the gated-concat twin above."""
    sd = syn.fill_state_dict(C.BILINEAR_SHAPES, 710, gain=3.0)
    sd.update(syn.fill_state_dict({"classifier.weight": (4, C.E), "classifier.bias": (4,)}, 721))
    hp, ho, _ = C.fusion_inputs()
    h = torch.stack([torch.stack([hp, ho * 0.5, -hp]), torch.stack([ho, hp, ho * 2.0])])
    _, _, label, cens, probes, w = _case(C.E, 3, 4, 6200)
    for form in ("plain", "ces", "sct"):
        ref = _bilinear_reference(sd, h, form, label, cens, probes, w)
        for interleaved in (True, False):
            got = _run_bilinear_entry(dev, sd, h, form, label, cens, probes, w, interleaved)
            _compare(f"bilinear golden rows {form} interleaved={interleaved}", got, ref, ["h_path", "h_omic"] + list(sd))


def test_bilinear_gradients_are_bit_equal_from_run_to_run(dev):
    sd, h, label, cens, probes, w = _bilinear_case(256, 33, 4, 8300)
    runs = [_run_bilinear_entry(dev, sd, h, "ces", label, cens, probes, w, True)[1] for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- training mode: masks replayed on the host
def _train_errs(got, ref):
    out, grads = got
    out_ref, grads_ref = ref
    e_out = max(float((out[k].double().cpu() - v).abs().max() / v.abs().max().clamp_min(1e-30)) for k, v in out_ref.items())
    e_grad = max(float((g.double().cpu() - r).abs().max()) / max(float(r.abs().max()), 1e-5) for g, r in zip(grads, grads_ref))
    return e_out, e_grad


@pytest.mark.parametrize("b", [1, 33])
@pytest.mark.parametrize("form", ["plain", "ces"])
def test_bilinear_training_equals_fp64_with_replayed_masks(dev, b, form):
    """One training-mode call at d = 256, p = 0.25: the five masks rebuilt on the host from (seed, offset, epoch) reproduce
    outputs and gradients (forward and backward of the call therefore used the same masks) at the bars
    tests/test_gpu_train_dropout.py holds the pooling head to; the masks of offset + 1 miss them by more than 100 x."""
    d, epoch = 256, 3
    sd, h, label, cens, probes, w = _bilinear_case(d, b, 4, 8400 + b)
    ep = torch.tensor([epoch], dtype=torch.int64, device=dev)
    got = _run_bilinear_entry(dev, sd, h, form, label, cens, probes, w, True, rng=(P, SEED, OFF), epoch=ep)
    keeps = F.bilinear_keeps(SEED, OFF, b, d, P, epoch)
    e_out, e_grad = _train_errs(got, _bilinear_reference(sd, h, form, label, cens, probes, w, keeps))
    assert e_out < FWD_TOL and e_grad < TRAIN_GRAD_TOL, (e_out, e_grad)
    wrong = F.bilinear_keeps(SEED, OFF + 1, b, d, P, epoch)
    c_out, c_grad = _train_errs(got, _bilinear_reference(sd, h, form, label, cens, probes, w, wrong))
    assert c_out >= 100 * FWD_TOL and c_grad >= 100 * TRAIN_GRAD_TOL, (c_out, c_grad)
    # realised keep rates: a binomial 5 sigma band around 1 - p for each site's element count
    for name, k in keeps.items():
        n = k.numel()
        rate = float((k != 0).double().mean())
        assert abs(rate - (1 - P)) <= 5 * (P * (1 - P) / n) ** 0.5, (name, n, rate)


def test_bilinear_second_call_draws_other_masks(dev):
    """Through ops (one _reserve(span) per call): the second call's masks are those of the next offset."""
    d, b = 256, 5
    sd, h, *_ = _bilinear_case(d, b, 4, 8500)
    from multimodal_path_omic_amd.fusion import BilinearFusion
    fus = BilinearFusion(dim1=d, dim2=d, output_size=d)
    fus.load_state_dict({k: v for k, v in sd.items() if not k.startswith("classifier")}, strict=True)
    cls = torch.nn.Linear(d, 4)
    cls.load_state_dict({"weight": sd["classifier.weight"], "bias": sd["classifier.bias"]})
    fus.to(dev).train()
    cls.to(dev)
    ops.set_rng_epoch(None)
    _pin()
    rows = torch.cat([h[0], h[1]], dim=1).to(dev)
    span = L.lib().mpo_bilinear_head_rng_span(b, d)
    outs = [ops.bilinear_head(rows, fus, cls, True)[0].detach().double().cpu() for _ in range(2)]
    assert ops._rng_calls == OFF + 2 * (span + 1)
    assert not torch.equal(outs[0], outs[1])
    p = {k: v.double() for k, v in sd.items()}
    for i, off in enumerate((OFF, OFF + span + 1)):
        _, hz, _, _ = F.bilinear_head(h[0].double(), h[1].double(), p, F.bilinear_keeps(SEED, off, b, d, P))
        assert float((outs[i] - hz).abs().max()) < OUT_ATOL


# ---- contract: rng_state, graph replays, rng_base
def _bilinear_model(dev, seed, bag_dtype=torch.float32):
    model = MultimodalCoAttentionTransformer(omic_sizes=OMIC_SIZES, fusion="bilinear", bag_dtype=bag_dtype)
    model.load_state_dict(syn.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed), strict=True)
    return model.to(dev)


def test_rng_state_reproduces_bilinear_training_steps(dev):
    model = _bilinear_model(dev, 8600).train()
    window = _window(dev, 8601)
    ops.set_rng_epoch(None)
    _pin()
    state = ops.rng_state()

    def two_steps():
        out = []
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            out.append(harness.train_window(model, *window, SLIDES)[0].clone())
        return out
    first = two_steps()
    ops.set_rng_state(state, device=dev)
    second = two_steps()
    assert not torch.equal(first[0], first[1])                       # the two steps drew different masks
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_graphed_bilinear_step_draws_fresh_masks_and_replays_from_its_rng_base(dev):
    from multimodal_path_omic_amd.dp import FlatGradBucket

    def capture(rng_base=None):
        model = _bilinear_model(dev, 8700, torch.bfloat16).train()
        bucket = FlatGradBucket(list(model.parameters()))
        return harness.GraphedWindowStep(model, bucket, _window(dev, 8701, torch.bfloat16), SLIDES, opt=None, warmup=1,
                                         rng_base=rng_base)
    ops.set_rng_epoch(None)
    _pin()
    step = capture()
    epoch0 = int(ops._rng_epoch_tensor)
    first = [step()[0].clone() for _ in range(2)]
    assert not torch.equal(first[0], first[1])                       # consecutive replays: the device epoch moved the masks
    ops._rng_epoch_tensor.fill_(epoch0)
    step2 = capture(rng_base=step.rng_base)
    assert step2.rng_base == step.rng_base
    ops._rng_epoch_tensor.fill_(epoch0)
    second = [step2()[0].clone() for _ in range(2)]
    ops.set_rng_epoch(None)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


@pytest.mark.parametrize("loss", ["ces", "sct"])
def test_bilinear_fused_loss_equals_the_composed_one_and_takes_the_fused_path(dev, loss):
    model = _bilinear_model(dev, 8800).eval()
    bags, omics, labels, cens = _window(dev, 8801)
    w = torch.full((SLIDES,), 0.25, device=dev)
    before = dict(ops.stats)
    _, _, _, att = model.forward_window(bags, omics, ces_targets=(labels, cens, w), fused_loss=loss)
    att["loss"].backward(w)
    assert ops.stats["head_loss_" + loss] == before["head_loss_" + loss] + 1
    assert ops.stats["bilinear_head"] == before["bilinear_head"] + 1
    fused = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    hz, sv, y, _ = model.forward_window(bags, omics)
    if loss == "ces":
        ref_loss, ref_risk = ops.ces_loss(hz, sv, labels, cens)
    else:
        ref_loss, ref_risk = ops.sct_loss(y, labels, cens), harness.risk_score(sv.detach())
    ref_loss.backward(w)
    assert float((att["loss"].detach() - ref_loss.detach()).abs().max()) < REL_TOL * max(float(ref_loss.detach().abs().max()), 1.0)
    assert float((att["risk"] - ref_risk).abs().max()) < OUT_ATOL * SLIDES
    for n, p in model.named_parameters():
        scale = max(float(p.grad.abs().max()), 1e-5)
        assert float((fused[n] - p.grad).abs().max()) / scale < GRAD_TOL, n
    # ... and a train_window step moves the same counters
    before = dict(ops.stats)
    harness.train_window(model, bags, omics, labels, cens, 4, loss=loss)
    assert ops.stats["bilinear_head"] == before["bilinear_head"] + 1
    assert ops.stats["head_loss_" + loss] == before["head_loss_" + loss] + 1


# =============================================================================================== the Python layer's refusals
class _KeepsItsGradient(torch.autograd.Function):
    """Passes `y` on and sends no gradient back to `x`: what reaches x's producer is an undefined gradient."""

    @staticmethod
    def forward(ctx, x, y):
        return y.clone()

    @staticmethod
    def backward(ctx, g):
        return None, g


def _head_callers(dev, fusion, d, c):
    """-> (plain(h), with_loss(h, label, cens, w, **kw), the modules' parameters) of ops' public functions of one fusion."""
    from multimodal_path_omic_amd.fusion import BilinearFusion, ConcatFusion, GatedConcatFusion
    cls = torch.nn.Linear(d, c).to(dev)
    if fusion == "concat":
        fus = ConcatFusion(dims=[d, d], hidden_size=d, output_size=d).to(dev).eval()
        plain = lambda h: ops.fusion_head_cat(h, fus, cls)                                               # noqa: E731
        with_loss = lambda h, *t, **kw: ops.fusion_head_loss_cat(h, fus, cls, *t, **kw)                  # noqa: E731
    elif fusion == "gated_concat":
        fus = GatedConcatFusion(dims=[d, d], hidden_size=d, output_size=d).to(dev).eval()
        plain = lambda h: ops.gated_concat_head(h, fus, cls)                                             # noqa: E731
        with_loss = lambda h, *t, **kw: ops.gated_concat_head_loss(h, fus, cls, *t, **kw)                # noqa: E731
    else:
        fus = BilinearFusion(dim1=d, dim2=d, output_size=d).to(dev).eval()
        plain = lambda h: ops.bilinear_head(h, fus, cls, False)                                          # noqa: E731
        with_loss = lambda h, *t, **kw: ops.bilinear_head_loss(h, fus, cls, *t, False, **kw)             # noqa: E731
    return plain, with_loss, list(fus.parameters()) + list(cls.parameters())


@pytest.mark.parametrize("fusion", ["concat", "gated_concat", "bilinear"])
def test_python_layer_refusals(dev, fusion):
    """What ops refuses on its own side of the C ABI, the same for the three fusions, and the one backward that does nothing."""
    b, d, c = 2, min(F.D_BUILT), 4
    name = {"concat": "fusion_head_loss", "gated_concat": "gated_concat_head_loss", "bilinear": "bilinear_head_loss"}[fusion]
    plain, with_loss, params = _head_callers(dev, fusion, d, c)
    h = syn.normal(syn.rng(9000), (b, 2 * d)).to(dev).requires_grad_(True)
    label, cens = torch.arange(b, device=dev) % c, torch.zeros(b, device=dev)
    w = torch.full((b,), 0.5, device=dev)
    # backward is driven with the slide_weight tensor itself, nothing else
    loss, *_ = with_loss(h, label, cens, w)
    with pytest.raises(RuntimeError, match=name + r": backward\(\) must be driven with the slide_weight tensor"):
        loss.backward(w.clone())
    assert h.grad is None and all(p.grad is None for p in params)
    # slide_weight: fp32, one value per slide
    for bad in (w.double(), torch.full((b + 1,), 0.5, device=dev)):
        with pytest.raises(ValueError, match=name + ": slide_weight must be a contiguous fp32 tensor of one value per slide"):
            with_loss(h, label, cens, bad)
    with pytest.raises(ValueError, match=name + r"\w*: loss 'nll' has no fused head launch"):
        with_loss(h, label, cens, w, loss="nll")
    # h is read in place by the two-pointer fusions: another shape or a strided view is refused; concat takes a copy instead
    wide = syn.normal(syn.rng(9001), (b, 4 * d)).to(dev)
    wide[:, :2 * d] = h.detach()
    if fusion == "concat":
        for got, want in zip(plain(wide[:, :2 * d]), plain(h.detach())):
            assert torch.equal(got, want)
    else:
        for call in (plain, lambda t: with_loss(t, label, cens, w)):
            with pytest.raises(ValueError, match="h must be contiguous"):
                call(wide[:, :2 * d])
            with pytest.raises(ValueError, match=r"is not \(B, 2 d\)"):
                call(wide[:, :2 * d + 1].contiguous())
            with pytest.raises(ValueError, match=r"is not \(B, 2 d\)"):
                call(h.detach().view(2, b, d))
    # a loss whose consumer sends no gradient back: the head's backward runs with none, launches nothing and returns none
    loss, *_ = with_loss(h, label, cens, w)
    probe = torch.ones(b, device=dev, requires_grad=True)
    _KeepsItsGradient.apply(loss, probe).sum().backward()
    assert probe.grad is not None and h.grad is None and all(p.grad is None for p in params)
