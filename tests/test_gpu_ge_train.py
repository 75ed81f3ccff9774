"""The gene-expression model's training step through the harness: the head + `ce` loss kernels against fp64, the
reference's golden values through forward_window, a window as the sum of its bags, no M x M map in a training step, the
flat gradient bucket and optimiser (with the L1 fold) against a stock-torch loop, and the captured step.

Dropout stays off wherever two paths are compared (they draw different masks); the training-mode cases check properties."""
import pytest
import torch
import torch.nn.functional as F

import cases as C
from multimodal_path_omic_amd import harness, ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.dp import FlatGradBucket, FlatOptimizer
from multimodal_path_omic_amd.models import GeneExprNarrowContextualAttentionGateTransformer
from multimodal_path_omic_amd.ops import BagBatch
from oracle import mpo_oracle as O

pytestmark = pytest.mark.gpu
sub = syn.subsample

# The bars tests/test_gpu_sct_loss.py holds the fp32 `sct` entries to against fp64 (restated, not imported): loss and Y are
# softmax / log of O(1) values, a few ulps relative; gradient entries are O(w) with a few fp32 roundings.
LOSS_RTOL, GRAD_ATOL = 1e-5, 1e-6
# loss and Y of a whole model on an fp32 window (test_forward_window_with_targets_matches_reference_golden below); Y on a bf16 window
# against the oracle fed the same stored values (tests/test_gpu_bag_selfattn.py::test_ge_model_bf16_bag_against_the_oracle)
GOLDEN_ABS, BF16_SAME_STORAGE_ABS = 1e-4, 2e-4
# tests/test_gpu_graph.py: replayed against eager steps
GRAPH_LOSS_TOL, GRAPH_PARAM_TOL = dict(rtol=2e-3, atol=2e-4), dict(rtol=5e-3, atol=5e-4)
# tests/test_gpu_train_options.py: the first window (no optimiser step yet) and a trajectory behind Adam steps.  That file
# holds OUTPUTS to its bars, not parameters: Adam's early update is sign-like, so a last-bit difference of a near-zero
# gradient entry moves that parameter by 2 lr whatever the arithmetic.
FIRST_WINDOW_TOL, ADAM_TRAJ_TOL = 1e-3, 5e-3


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def build_ge(dev, seed, bag_dtype=torch.float32, size="medium", d=256):
    model = GeneExprNarrowContextualAttentionGateTransformer(model_size=size, bag_dtype=bag_dtype)
    sd = syn.fill_state_dict(C.ge_model_shapes(d=d), seed)
    model.load_state_dict(sd, strict=True)
    return model.to(dev).eval(), sd


# ------------------------------------------------------------------------------------------------ 4. the head kernels
@pytest.mark.parametrize("b", [1, 5, 32])
@pytest.mark.parametrize("c", [2, 3, 8])
@pytest.mark.parametrize("d", [128, 256, 512])
def test_head_and_ce_loss_match_fp64(dev, d, c, b):
    g = torch.Generator(device="cpu").manual_seed(1000 * d + 10 * c + b)
    h = torch.randn(b, d, generator=g).to(dev)
    cls = torch.nn.Linear(d, c).to(dev)
    with torch.no_grad():
        cls.weight.copy_(torch.randn(c, d, generator=g) / d ** 0.5)
        cls.bias.copy_(torch.randn(c, generator=g) * 0.1)
    label = torch.randint(0, c, (b,), generator=g).to(dev)
    w = (torch.rand(b, generator=g) + 0.1).to(dev)
    hd = h.clone().requires_grad_(True)
    loss, y = ops.ge_head_loss(hd, cls, label)
    assert loss.shape == (b,) and y.shape == (b, c) and not y.requires_grad
    loss.backward(w)
    h64 = h.double().clone().requires_grad_(True)
    w64, b64 = cls.weight.detach().double().requires_grad_(True), cls.bias.detach().double().requires_grad_(True)
    y64 = torch.softmax(h64 @ w64.t() + b64, dim=1)
    ref = F.cross_entropy(y64, label, reduction="none")            # the reference's quirk: CE of the soft-maxed Y
    ref.backward(w.double())
    errs = dict(loss=float((loss.detach().double() - ref.detach()).abs().max()), y=float((y.double() - y64.detach()).abs().max()),
                d_h=float((hd.grad.double() - h64.grad).abs().max()), dW=float((cls.weight.grad.double() - w64.grad).abs().max()),
                db=float((cls.bias.grad.double() - b64.grad).abs().max()))
    print(f"[ge head d={d} C={c} B={b}] " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    torch.testing.assert_close(loss.double(), ref.detach(), rtol=LOSS_RTOL, atol=1e-6)
    torch.testing.assert_close(y.double(), y64.detach(), rtol=LOSS_RTOL, atol=1e-6)
    torch.testing.assert_close(hd.grad.double(), h64.grad, rtol=0, atol=GRAD_ATOL)
    torch.testing.assert_close(cls.weight.grad.double(), w64.grad, rtol=0, atol=GRAD_ATOL)
    torch.testing.assert_close(cls.bias.grad.double(), b64.grad, rtol=0, atol=GRAD_ATOL)


def test_head_broadcast_gradient_bad_label_and_refused_geometry(dev):
    g = torch.Generator(device="cpu").manual_seed(5)
    h = torch.randn(4, 256, generator=g).to(dev)
    cls = torch.nn.Linear(256, 3).to(dev)
    label = torch.tensor([0, 2, 1, 1], device=dev)
    # loss.sum().backward(): a broadcast (stride-0) upstream gradient
    hd = h.clone().requires_grad_(True)
    ops.ge_head_loss(hd, cls, label)[0].sum().backward()
    h64 = h.double().clone().requires_grad_(True)
    F.cross_entropy(torch.softmax(h64 @ cls.weight.detach().double().t() + cls.bias.detach().double(), 1), label,
                    reduction="sum").backward()
    torch.testing.assert_close(hd.grad.double(), h64.grad, rtol=0, atol=GRAD_ATOL)
    # a label outside [0, C) is flagged: NaN loss for that bag, Y still the softmax, no gradient from it, the others untouched
    dw_good = cls.weight.grad.clone()
    cls.zero_grad()
    bad = label.clone()
    bad[1] = 3
    hb = h.clone().requires_grad_(True)
    loss, y = ops.ge_head_loss(hb, cls, bad)
    assert bool(torch.isnan(loss[1])) and bool(torch.isfinite(loss[[0, 2, 3]]).all()) and bool(torch.isfinite(y).all())
    loss.backward(torch.ones(4, device=dev))
    assert float(hb.grad[1].abs().max()) == 0.0 and bool(torch.isfinite(cls.weight.grad).all())
    torch.testing.assert_close(hb.grad[[0, 2, 3]], hd.grad[[0, 2, 3]], rtol=0, atol=GRAD_ATOL)
    assert float((cls.weight.grad - dw_good).abs().max()) > 0          # bag 1 no longer contributes
    with pytest.raises(RuntimeError, match="d = 192"):
        ops.ge_head_loss(torch.zeros(2, 192, device=dev), torch.nn.Linear(192, 3).to(dev), label[:2])
    with pytest.raises(RuntimeError, match="9 classes"):
        ops.ge_head_loss(torch.zeros(2, 256, device=dev), torch.nn.Linear(256, 9).to(dev), label[:2])


# ------------------------------------------------------------------------------------------------ 5. golden parity
@pytest.mark.parametrize("case", list(C.GE_MODEL_CASES))
def test_forward_window_with_targets_matches_reference_golden(dev, golden, case):
    """One bag through forward_window(ce_targets=...) + backward, held to the bars of test_ge_model_matches_reference_golden."""
    g = golden("ge_models")
    m, seed = C.GE_MODEL_CASES[case]
    model, _ = build_ge(dev, seed)
    wsi, target = C.ge_model_inputs(m, seed + 1)
    w = torch.ones(1, device=dev)
    before = ops.stats["head_loss_ce"]
    y, att = model.forward_window(BagBatch.from_list([wsi.to(dev)]), ce_targets=(target.to(dev), w))
    assert ops.stats["head_loss_ce"] == before + 1
    assert y.shape == (1, 3) and att["attn"] is None and att["path"][0].shape == (1, m) and att["loss"].shape == (1,)
    e_loss = abs(att["loss"].item() - float(g[f"{case}/loss"]))
    e_y = float((y[0].detach().cpu() - g[f"{case}/Y"]).abs().max())
    print(f"[ge golden {case}] |loss - ref| {e_loss:.1e}, |Y - ref| {e_y:.1e}")
    assert e_loss < GOLDEN_ABS and e_y < GOLDEN_ABS
    att["loss"].backward(w)
    for n, prm in model.named_parameters():
        ref = g[f"{case}/grad/{n}"]
        got = sub(prm.grad if prm.grad is not None else torch.zeros_like(prm), 256).cpu()
        scale = max(float(ref.abs().max()), 1e-5)      # shift-invariant biases have ~1e-8 'gradients'
        assert float((got - ref).abs().max()) / scale < 5e-3, (n, float((got - ref).abs().max()) / scale)


# ------------------------------------------------------------------------------------------------ 6. window = sum of bags
LENGTHS = [300, 65, 2048, 515]


@pytest.mark.parametrize("bag_dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_window_is_the_sum_of_its_bags(dev, bag_dtype):
    model, _ = build_ge(dev, 611, bag_dtype)
    g = syn.rng(612)
    wsis = [syn.normal(g, (m, 1024)).to(dev).to(bag_dtype) for m in LENGTHS]
    labels = (torch.arange(len(LENGTHS)) % 3).to(dev)
    acc = len(LENGTHS)
    bags = BagBatch.from_list(wsis)
    # need_maps=True first (no targets): the maps and Y of the window against forward()
    with torch.no_grad():
        y_m, att_m = model.forward_window(bags, need_maps=True)
    per_bag = harness.train_ge_window(model, bags, labels, acc)
    grads_w = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad()
    with torch.no_grad():
        y_w, att_w = model.forward_window(bags, ce_targets=(labels, torch.full((acc,), 1.0 / acc, device=dev)))
    assert att_w["attn"] is None
    for b, wsi in enumerate(wsis):
        y, att = model(wsi=wsi)
        assert relerr(y_w[b], y) < 1e-5 and relerr(y_m[b], y) < 1e-5
        assert att_m["attn"][b].shape == (LENGTHS[b], LENGTHS[b]) and att_m["path"][b].shape == (1, LENGTHS[b])
        assert relerr(att_m["attn"][b], att["attn"]) < 1e-4
        assert relerr(att_m["path"][b], att["path"]) < 1e-4 and relerr(att_w["path"][b], att["path"]) < 1e-4
        loss = F.cross_entropy(y.unsqueeze(0), labels[b:b + 1])                      # models/ge_nacagat/main.py:33
        assert abs(float(loss) - float(per_bag[b])) < 2e-5 * max(1.0, abs(float(loss))), (b, float(loss), float(per_bag[b]))
        (loss / acc).backward()                                                    # main.py:51
    worst = {}
    for n, p in model.named_parameters():
        scale = max(float(p.grad.abs().max()), 1e-3)            # shift-invariant biases: ~1e-8 noise
        err = float((grads_w[n] - p.grad).abs().max()) / scale
        bar = 2e-4 if bag_dtype == torch.float32 else (4e-3 if n.startswith("H.") else 5e-4)
        worst[n.startswith("H.")] = max(worst.get(n.startswith("H."), 0.0), err)
        assert err < bar, (n, err)
    print(f"[ge window {bag_dtype}] worst scaled gradient error: H.* {worst.get(True, 0):.1e}, others {worst.get(False, 0):.1e}")


def test_forward_window_refuses_short_bags(dev):
    """Bags of at most 16 rows take the token tail's short-axis kernels; the window form refuses them with a message."""
    model, _ = build_ge(dev, 613)
    bags = BagBatch.from_list([torch.zeros(100, 1024, device=dev), torch.zeros(16, 1024, device=dev)])
    with pytest.raises(ValueError, match="at least 17 rows"):
        model.forward_window(bags)


# ------------------------------------------------------------------------------------------------ 7. no map in training
def test_training_step_allocates_no_map_at_15000_rows(dev):
    m, seed = 15000, 4444
    model, _ = build_ge(dev, seed, torch.bfloat16)
    model.train()
    bags = BagBatch.from_list([syn.make_bag(m, seed + 1).to(dev).to(torch.bfloat16)])
    label, w = torch.tensor([1], device=dev), torch.ones(1, device=dev)

    def step(need_maps):
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        y, att = model.forward_window(bags, need_maps=need_maps, ce_targets=(label, w))
        att["loss"].backward(w)
        torch.cuda.synchronize(dev)
        assert bool(torch.isfinite(att["loss"]).all()) and abs(float(y.sum()) - 1.0) < 1e-5
        assert (att["attn"] is not None) == need_maps
        peak = torch.cuda.max_memory_allocated(dev)
        del y, att
        return peak

    step(False)                                          # allocator warm-up
    lean, full = step(False), step(True)
    print(f"[ge 15k] peak allocated: step {lean / 2**20:.0f} MiB, step with the map {full / 2**20:.0f} MiB "
          f"(map alone {m * m * 4 / 2**20:.0f} MiB)")
    assert full - lean >= 0.8 * m * m * 4
    for n, prm in model.named_parameters():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), n


# ------------------------------------------------------------------------------------------------ 8. bucket + optimiser
def _three_bags(dev, bag_dtype=torch.float32, seed=701):
    g = syn.rng(seed)
    slides = [{"wsi": syn.normal(g, (m, 1024)), "gene_expr_class": i % 3} for i, m in enumerate([120, 65, 300])]
    return slides, harness.make_ge_window(slides, dev, bag_dtype)


def test_bucket_receives_the_gradients_of_the_eager_path(dev):
    slides, (bags, labels) = _three_bags(dev)
    model, sd = build_ge(dev, 702)
    bucket = FlatGradBucket(list(model.parameters()))
    bucket.begin()
    harness.train_ge_window(model, bags, labels, 3)
    bucket.finish()
    for p in (model.classifier.weight, model.classifier.bias):          # written in place by the head's backward
        assert p.grad.data_ptr() == p._mpo_grad_view.data_ptr()
    ref, _ = build_ge(dev, 702)
    for s in slides:
        y, _ = ref(wsi=s["wsi"].to(dev))
        (F.cross_entropy(y.unsqueeze(0), torch.tensor([s["gene_expr_class"]], device=dev)) / 3).backward()
    for (n, p), off, q in zip(model.named_parameters(), bucket.offsets, ref.parameters()):
        got = bucket.flat[off:off + p.numel()].view_as(p)
        scale = max(float(q.grad.abs().max()), 1e-3)
        assert float((got - q.grad).abs().max()) / scale < 2e-4, n
    # a second window before the optimiser step accumulates into the same slices
    harness.train_ge_window(model, bags, labels, 3)
    bucket.finish()
    for (n, p), off, q in zip(model.named_parameters(), bucket.offsets, ref.parameters()):
        got = bucket.flat[off:off + p.numel()].view_as(p)
        scale = max(float(q.grad.abs().max()), 1e-3)
        assert float((got - 2 * q.grad).abs().max()) / scale < 4e-4, n


def test_adam_steps_with_l1_fold_track_the_stock_torch_loop(dev):
    """Three windows of train_ge_window + FlatOptimizer('adam', l1_lambda) against models/ge_nacagat/main.py:24-56 spelled
    with stock torch on the CPU oracle: (loss / acc + lambda * l1_reg).backward() per bag, torch.optim.Adam; the reported
    loss is loss + lambda * l1_reg."""
    lam, lr, wd, acc = 1e-5, 1e-3, 1e-5, 3
    slides, (bags, labels) = _three_bags(dev)
    model, sd = build_ge(dev, 703)
    o = harness.training_options(dict(loss="ce", optimizer="adam", lr=lr, weight_decay=wd, grad_acc_step=acc, scheduler=None,
                                      gamma=1.0, **{"lambda": lam}), "ge_nacagat")
    bucket = FlatGradBucket(list(model.parameters()))
    opt = o.make_optimizer(bucket)
    start = opt.flat_p.clone()
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    opt_ref = torch.optim.Adam(list(p.values()), lr=lr, weight_decay=wd)
    for step in range(3):
        bucket.begin()
        got = harness.train_ge_window(model, bags, labels, acc, l1=o.l1).cpu()
        bucket.finish()
        opt.step(l1_slides=bags.n_slides)
        opt_ref.zero_grad()
        want = []
        for s in slides:
            y, _ = O.ge_nacagat_forward(p, s["wsi"])
            loss = O.ge_ce_loss(y, torch.tensor([s["gene_expr_class"]]))
            reg = lam * sum(v.abs().sum() for v in p.values())
            (loss / acc + reg).backward()
            want.append(float(loss + reg))
        opt_ref.step()
        err = float((got - torch.tensor(want)).abs().max())
        print(f"[ge adam + l1] step {step}: reported loss {got.tolist()} |err| {err:.1e}")
        assert err < (FIRST_WINDOW_TOL if step == 0 else ADAM_TRAJ_TOL)
    moved = float((opt.flat_p - start).abs().max())
    assert moved > lr                                             # it stepped: Adam moves a parameter by ~lr per step
    with torch.no_grad():
        y_w, _ = model.forward_window(bags)
        for b, s in enumerate(slides):
            y_o, _ = O.ge_nacagat_forward(p, s["wsi"])
            assert float((y_w[b].cpu() - y_o).abs().max()) < ADAM_TRAJ_TOL
    dev_p = max(float((prm.detach().cpu() - p[n].detach()).abs().max()) for n, prm in model.named_parameters())
    print(f"[ge adam + l1] after 3 steps: max |p - p_ref| {dev_p:.1e} (moved {moved:.1e}; reported, not held -- see the bars above)")


# ------------------------------------------------------------------------------------------------ 9. the captured step
def _graph_setup(dev, train_mode, lam=0.0):
    model, _ = build_ge(dev, 801, torch.bfloat16)
    model.train(train_mode)
    _, window = _three_bags(dev, torch.bfloat16, 802)
    bucket = FlatGradBucket(list(model.parameters()))
    opt = FlatOptimizer(bucket, "adam", lr=1e-3, weight_decay=1e-5, l1_lambda=lam)
    return model, bucket, opt, window


@pytest.mark.parametrize("lam", [0.0, 1e-5])
def test_graphed_ge_step_equals_eager_steps(dev, lam):
    ops.set_rng_epoch(None)
    model_e, bucket_e, opt_e, (bags_e, labels_e) = _graph_setup(dev, False, lam)
    losses_e = []
    for _ in range(3):
        bucket_e.begin()
        loss = harness.train_ge_window(model_e, bags_e, labels_e, 3, l1=lam)
        bucket_e.finish()
        opt_e.step(l1_slides=3) if lam else opt_e.step()
        losses_e.append(loss.clone())
    ops.set_rng_epoch(None)
    model_g, bucket_g, opt_g, window_g = _graph_setup(dev, False, lam)
    state = [t.clone() for t in opt_g.state_tensors()]
    step = harness.GraphedWindowStep(model_g, bucket_g, window_g, 3, opt=opt_g, warmup=1)
    for t, k in zip(opt_g.state_tensors(), state):                 # construction does not train
        assert torch.equal(t, k)
    assert int(opt_g.t_dev) == 0
    losses_g = [step().clone() for _ in range(3)]
    for a, b in zip(losses_e, losses_g):
        torch.testing.assert_close(a, b, **GRAPH_LOSS_TOL)
    torch.testing.assert_close(opt_e.flat_p, opt_g.flat_p, **GRAPH_PARAM_TOL)
    assert int(opt_g.t_dev) == 3
    assert float((opt_g.flat_p - state[0]).abs().max()) > 1e-3       # three Adam steps of lr 1e-3 moved the parameters
    ops.set_rng_epoch(None)


def test_graphed_ge_step_draws_fresh_dropout_masks_and_refuses_the_split(dev):
    ops.set_rng_epoch(None)
    model, bucket, _, window = _graph_setup(dev, True)
    with pytest.raises(ValueError, match="not for the gene-expression model"):
        harness.GraphedWindowStep(model, bucket, window, 3, opt=None, split_patch_grad=True)
    step = harness.GraphedWindowStep(model, bucket, window, 3, opt=None, warmup=1)
    l1 = step().clone()
    l2 = step().clone()
    assert not torch.equal(l1, l2)                                  # same weights, the epoch advanced inside the graph
    assert bool(torch.isfinite(l1).all()) and bool(torch.isfinite(l2).all()) and bool(torch.isfinite(bucket.flat).all())
    torch.cuda.synchronize()
    ops.set_rng_epoch(None)
