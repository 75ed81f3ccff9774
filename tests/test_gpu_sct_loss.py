"""The `sct` loss (SurvivalClassificationTobitLoss, models/loss.py:62-85, on Y = softmax(logits)): the standalone HIP pair
(ops.sct_loss through the survival head) and the fused training-step head (mpo_fusion_head_sct_loss_forward + the unchanged
mpo_fusion_head_loss_backward) against an fp64 torch restatement and against the reference's own values
(tests/golden/train_options.npz): B = 1..64 slides, every label, both censorings, peaky logits with Y[y] ~ 1e-9, per-slide
and broadcast upstream gradients, an absolute bar where the exact gradient is 0 (censored at label 0), and the concat
training step taking the fused path."""
import numpy as np
import pytest
import torch

import cases as C
from multimodal_path_omic_amd import harness, ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.models import MultimodalCoAttentionTransformer

pytestmark = pytest.mark.gpu
EPS = 1e-7


def sct_fp64(logits, label, cens, eps=EPS):
    y = torch.softmax(logits.double(), dim=1)
    idx = torch.arange(y.shape[1], device=y.device)[None, :]
    lab = label.view(-1, 1)
    keep = torch.where(cens.view(-1, 1) != 0, idx >= lab, idx == lab)
    return -torch.log((y * keep).sum(1) + eps)


def _case(dev, b, seed, peaky=False):
    g = torch.Generator(device="cpu").manual_seed(seed)
    logits = torch.randn(b, 4, generator=g) * 2.0
    label = torch.arange(b) % 4
    cens = ((torch.arange(b) // 4) % 2).float()
    if peaky:
        logits[:, :] = 0.0
        logits[torch.arange(b), (label + 1) % 4] = 21.0
    return logits.to(dev), label.to(dev), cens.to(dev)


# bars: the fp32 kernels against fp64.  Loss: softmax and log of O(1) values, a few ulps relative (|loss| up to ~21 on the
# peaky cases, so 1e-5 relative); gradient entries are O(w) with a few fp32 roundings -> 1e-6 absolute at w <= 1.
LOSS_RTOL, GRAD_ATOL = 1e-5, 1e-6


@pytest.mark.parametrize("b", [1, 3, 8, 17, 64])
@pytest.mark.parametrize("peaky", [False, True])
def test_standalone_sct_matches_fp64(dev, b, peaky):
    logits, label, cens = _case(dev, b, 100 + b, peaky)
    lg = logits.clone().requires_grad_(True)
    _, _, y = ops.survival_head(lg)
    loss = ops.sct_loss(y, label, cens)
    w = torch.rand(b, device=dev) + 0.1
    loss.backward(w)
    lg64 = logits.double().clone().requires_grad_(True)
    ref = sct_fp64(lg64, label, cens)
    ref.backward(w.double())
    torch.testing.assert_close(loss.double(), ref.detach(), rtol=LOSS_RTOL, atol=1e-6)
    torch.testing.assert_close(lg.grad.double(), lg64.grad, rtol=0, atol=GRAD_ATOL)
    # broadcast upstream gradient (loss.sum().backward())
    lg2 = logits.clone().requires_grad_(True)
    ops.sct_loss(ops.survival_head(lg2)[2], label, cens).sum().backward()
    lg64.grad = None
    sct_fp64(lg64, label, cens).sum().backward()
    torch.testing.assert_close(lg2.grad.double(), lg64.grad, rtol=0, atol=GRAD_ATOL)


def _fused(dev, logits, label, cens, w):
    """The fused head on a fusion MLP whose last layer passes `logits` through exactly: hcat = logits in the first 4
    columns, identity-like weights, zero biases (ReLU layers see logits + 30 so nothing is clipped)."""
    b, c = logits.shape
    from multimodal_path_omic_amd.fusion import ConcatFusion
    d = 8
    fus = ConcatFusion(dims=[d // 2, d // 2], hidden_size=d, output_size=d).to(dev)
    cls = torch.nn.Linear(d, c).to(dev)
    with torch.no_grad():
        for lin in (fus.fusion_layer[0], fus.fusion_layer[2]):
            lin.weight.zero_()
            lin.weight[:c, :c] = torch.eye(c)
            lin.bias.zero_()
        cls.weight.zero_()
        cls.weight[:, :c] = torch.eye(c)
        cls.bias.fill_(-30.0)
    hcat = torch.zeros(b, d, device=dev)
    hcat[:, :c] = logits + 30.0
    hcat.requires_grad_(True)
    loss, risk, hz, sv, y = ops.fusion_head_loss_cat(hcat, fus, cls, label, cens, w, loss="sct")
    loss.backward(w)
    return loss, risk, sv, hcat.grad[:, :c]


@pytest.mark.parametrize("b", [1, 5, 16, 64])
@pytest.mark.parametrize("peaky", [False, True])
def test_fused_sct_head_matches_fp64(dev, b, peaky):
    logits, label, cens = _case(dev, b, 200 + b, peaky)
    w = torch.full((b,), 0.125, device=dev)
    before = ops.stats["head_loss_sct"]
    loss, risk, sv, dlog = _fused(dev, logits, label, cens, w)
    assert ops.stats["head_loss_sct"] == before + 1
    lg64 = logits.double().clone().requires_grad_(True)
    ref = sct_fp64(lg64, label, cens)
    ref.backward(w.double())
    # the logits went through +30 / -30 in fp32: ~2e-6 absolute on them
    torch.testing.assert_close(loss.double(), ref.detach(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(dlog.double(), lg64.grad, rtol=0, atol=1e-6)
    torch.testing.assert_close(risk, -sv.sum(1))
    assert torch.isfinite(dlog).all()


def test_exact_zero_gradient_censored_at_label_zero(dev):
    """Censored at y = 0: P = 1 for every logit vector, the exact gradient is 0 -- the fused kernel forms 1 - P as the sum
    of the classes below the label (none), so it returns exact zeros; the standalone pair stays within ulps of 0."""
    b = 32
    g = torch.Generator(device="cpu").manual_seed(9)
    logits = (torch.randn(b, 4, generator=g) * 8.0).to(dev)
    label = torch.zeros(b, dtype=torch.int64, device=dev)
    cens = torch.ones(b, device=dev)
    w = torch.ones(b, device=dev)
    _, _, _, dlog = _fused(dev, logits, label, cens, w)
    assert float(dlog.abs().max()) == 0.0
    lg = logits.clone().requires_grad_(True)
    ops.sct_loss(ops.survival_head(lg)[2], label, cens).backward(w)
    assert float(lg.grad.abs().max()) < 1e-6


def test_sct_matches_reference_golden(dev, golden):
    g = golden("train_options")
    logits, label, cens = g["sct/logits"].to(dev), g["sct/label"].to(dev), g["sct/censorship"].to(dev)
    ref_loss, ref_grad = g["sct/loss"].double(), g["sct/dlogits"].double()
    b = logits.shape[0]
    # the reference runs in fp32 too: bars are twice the fp32 restatement's own distance to fp64 plus a few ulps
    lg = logits.clone().requires_grad_(True)
    loss = ops.sct_loss(ops.survival_head(lg)[2], label, cens)
    loss.backward(torch.ones(b, device=dev))
    torch.testing.assert_close(loss.double().cpu(), ref_loss, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lg.grad.double().cpu(), ref_grad, rtol=0, atol=2e-6)
    loss_f, _, _, dlog = _fused(dev, logits, label, cens, torch.ones(b, device=dev))
    torch.testing.assert_close(loss_f.double().cpu(), ref_loss, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(dlog.double().cpu(), ref_grad, rtol=0, atol=2e-6)
    # control: the ces loss on the same inputs is nowhere near
    hz, sv, _ = ops.survival_head(logits)
    ces, _ = ops.ces_loss(hz, sv, label, cens)
    assert float((ces.double().cpu() - ref_loss).abs().max()) > 0.1


def test_concat_training_step_takes_fused_sct_path(dev):
    sizes = [64] * 6
    model = MultimodalCoAttentionTransformer(omic_sizes=sizes)
    model.load_state_dict(syn.fill_state_dict(C.model_shapes(sizes, False), 77))
    model.to(dev).eval()
    slides = syn.make_cohort(4, 200, 500, sizes, 78)
    window = harness.make_window(slides, dev)
    before = dict(ops.stats)
    loss, risk = harness.train_window(model, *window, 4, loss="sct")
    assert ops.stats["head_loss_sct"] == before["head_loss_sct"] + 1
    assert ops.stats["head_loss_ces"] == before["head_loss_ces"]
    # same values as the unfused path (forward_window + ops.sct_loss)
    with torch.no_grad():
        _, sv, y, _ = model.forward_window(*window[:2])
        ref = ops.sct_loss(y, window[2], window[3])
    torch.testing.assert_close(loss, ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(risk, harness.risk_score(sv), rtol=1e-5, atol=1e-5)


def test_sct_entries_refuse_bad_arguments(dev):
    from multimodal_path_omic_amd import _lib as L
    x = torch.zeros(16, device=dev)
    lab = torch.zeros(1, dtype=torch.int64, device=dev)
    lib = L.lib()
    assert lib.mpo_sct_loss_forward(L.ptr(x), L.ptr(lab), L.ptr(x), 1, 17, 1e-7, L.ptr(x), L.stream_of(x)) != 0
    assert lib.mpo_sct_loss_forward(None, L.ptr(lab), L.ptr(x), 1, 4, 1e-7, L.ptr(x), L.stream_of(x)) != 0
    assert lib.mpo_sct_loss_backward(L.ptr(x), L.ptr(lab), L.ptr(x), 1, 0, 1e-7, L.ptr(x), 0, L.ptr(x), L.stream_of(x)) != 0
    with pytest.raises(ValueError):
        ops.fusion_head_loss_cat(x.view(2, 8), None, None, lab, x, x, loss="ce")
