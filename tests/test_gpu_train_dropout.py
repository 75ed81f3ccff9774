"""Training-mode parity of the tail's fused entries against the fp64 oracle run with the SAME dropout masks.

The kernels draw every mask from a pure function of (seed, counter); tests/dropout_replay.py rebuilds them on the host
from the kernels' indexing and stream layout.  With torch.manual_seed and ops._rng_calls pinned, each test runs an op
with p = 0.25, rebuilds its masks and compares the forward output, dx and every parameter gradient with
oracle/mpo_oracle.py in fp64 -- at the bars of the eval-mode test of that op (forward 1e-4 of the reference's max,
gradients 2e-3 of each tensor's max).  A dropout at the wrong place, a wrong keep scale, two sites or branches drawing
the same counters, or a gate that indexes its stream differently from the forward fails here.  The sensitivity controls
at the end replay deliberately wrong masks to show the comparison can fail."""
import numpy as np
import pytest
import torch

import cases as C
import dropout_replay as R
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.transformer import make_set_transformer
from oracle import mpo_oracle as O
from tail_helpers import (FF, FWD_TOL, HEADS, LAYERS, OFF, P, SEED, SNN_SIZES, _encoder_check, _encoder_oracle, _pin, _pool_check,
                          _pool_oracle, _pool_setup, _snn_check, _snn_setup, _t, grad_errs, relerr)

pytestmark = pytest.mark.gpu


@pytest.fixture
def fast_path():
    was = L.lib().mpo_set_gemm_fast_path(1)
    yield lambda on: L.lib().mpo_set_gemm_fast_path(int(on))
    L.lib().mpo_set_gemm_fast_path(was)


@pytest.fixture
def epoch_tensor(dev):
    def install(e):
        t = torch.full((1,), e, dtype=torch.int64, device=dev)
        ops.set_rng_epoch(t)
        return t
    yield install
    ops.set_rng_epoch(None)


# ------------------------------------------------------------------------------------------- encoder
@pytest.mark.parametrize("fast", [True, False], ids=["fast", "general"])
@pytest.mark.parametrize("d", [128, 256, 512])
@pytest.mark.parametrize("ns", [1, 5, 32])
def test_encoder_token_tail_training_equals_fp64_oracle(dev, fast_path, fast, d, ns):
    """ops.encoder_stacked, 2 branches x 2 layers, T = 6 (mha_small's counter stream) with the fast GEMM bodies and
    the general ones."""
    fast_path(fast)
    _encoder_check(dev, 2, ns, C.N_OMIC, d, 100 + d + ns)


@pytest.mark.parametrize("T", [17, 200, 2050])
def test_encoder_bag_rows_training_equals_fp64_oracle(dev, T):
    """T > 16: the bag self-attention's block hash for the attention probabilities; at T = 2050 the forward and dx
    products run on gemm_f32_rows.hip, the weight gradients on gemm_f32_longk.hip, both with RNG and ReLU gates.
    T = 2050 runs the attention on its fp32 kernels: one of this input's 10^6 FFN pre-activations of layer 1 sits at
    2e-8 of their maximum, and the three-term bf16 attention (1e-6 relative, covered at T = 17 and 200 and by the
    gene-expression model below) moves it across the ReLU kink -- a different gate, not a different mask."""
    was = L.lib().mpo_set_bag_self_attention_bf16x3(0 if T == 2050 else 1)
    try:
        _encoder_check(dev, 2 if T < 2050 else 1, 1, T, 256, 300 + T)
    finally:
        L.lib().mpo_set_bag_self_attention_bf16x3(was)


@pytest.mark.parametrize("ff", [100, 102])
def test_encoder_irregular_ff_training_equals_fp64_oracle(dev, ff):
    """FFN widths off the 4- and 16-grid at d = 128, 5 slides x 6 tokens (30 rows: the general GEMM body throughout).
    ff = 100: K % 16 != 0 in linear2 and its gradients, leading dimension still % 4 == 0 (whole-quad draws).  ff = 102:
    lda % 4 != 0, so linear1's epilogue dropout and the regenerated gate of linear2's backward pair draw per element,
    and no operand row of width ff is 16-byte aligned.  mpo_encoder_forward has no check on ff: both widths run, at the
    bars of the ff = 512 cases."""
    _encoder_check(dev, 2, 5, C.N_OMIC, 128, 1200 + ff, ff=ff)


def test_encoder_refuses_narrow_heads_in_training(dev):
    """64 heads of width 2 at T = 16 would draw 64 * 16 counters per row for the attention mask, more than the
    max(ff, 3 d) = 512 its stream slot holds: refused in training, before any launch."""
    enc = make_set_transformer(128, P, nhead=64, dim_feedforward=FF, num_layers=1).to(dev)
    x = torch.randn(1, 2, 16, 128, device=dev)
    with pytest.raises(RuntimeError, match="heads \\* T"):
        ops.encoder_stacked(x, [list(enc.layers)], training=True)


# ------------------------------------------------------------------------------------------- gated pool
@pytest.mark.parametrize("interleave", [False, True], ids=["plain", "interleaved"])
@pytest.mark.parametrize("L_,ns", [(6, 1), (6, 32), (64, 1), (64, 32), (65, 1), (65, 32), (2050, 1)])
def test_gated_pool_training_equals_fp64_oracle(dev, L_, ns, interleave):
    """ops.gated_pool_stacked, 2 branches: the scorer is fused into the pooling kernels up to L = 64 and a many-row
    product from 65 on; rho's dropout over the [branch][slide][d] or the interleaved [slide][branch][d] rows."""
    _pool_check(dev, ns, L_, interleave, 500 + L_ + ns)


def test_pool_rho_zeros_are_exactly_the_dropped_elements(dev):
    """With rho's bias at +10 its ReLU never outputs zero, so h == 0 exactly where the mask dropped -- element by
    element, in both layouts."""
    nb, ns, L_, d = 2, 32, 6, 256
    sds, heads, rhos, x, _, _ = _pool_setup(dev, nb, ns, L_, d, 610, rho_bias=10.0)
    for interleave in (False, True):
        _pin()
        with torch.no_grad():
            _, h = ops.gated_pool_stacked(x.to(dev), heads, rhos, training=True, interleave=interleave)
        h = (h.view(ns, nb, d).transpose(0, 1) if interleave else h).cpu().numpy()
        kr = R.pool_keeps(SEED, OFF, nb, ns, L_, d, P, P, interleave)[2]
        assert ((h == 0) == (kr == 0)).all(), int(((h == 0) != (kr == 0)).sum())
        assert 0.2 < float((kr == 0).mean()) < 0.3


# ------------------------------------------------------------------------------------------- omic SNN
@pytest.mark.parametrize("ns", [1, 5, 32])
def test_omic_snn_training_equals_fp64_oracle(dev, ns):
    _snn_check(dev, ns, 700 + ns)


def test_omic_snn_alpha_constant_is_exactly_the_dropped_elements(dev):
    """ELU >= -1 never reaches alpha' = -1.758, so G_bag equals the AlphaDropout constant a alpha' + b exactly where
    the second site's host mask says 'dropped' -- element by element."""
    ns = 32
    G, xs, _ = _snn_setup(dev, ns, 780)
    _pin()
    with torch.no_grad():
        y = ops.omic_snn([x.to(dev) for x in xs], G, training=True).cpu().double().numpy()
    a = 1.0 / ((1 - P) * (1 + P * R.ALPHA_PRIME ** 2)) ** 0.5
    const = a * R.ALPHA_PRIME - a * R.ALPHA_PRIME * P
    is_const = np.abs(y - const) < 1e-5                                   # (ns, N, d)
    keeps = R.snn_keeps(SEED, OFF, ns, len(SNN_SIZES), C.E, P)
    dropped = np.stack([~k2 for _, k2 in keeps], axis=1)
    assert (is_const == dropped).all(), int((is_const != dropped).sum())


# ------------------------------------------------------------------------------------------- epoch (graph replay path)
def test_device_epoch_shifts_every_stream_by_epoch_times_2_pow_40(dev, epoch_tensor):
    """ops.set_rng_epoch(t) with t = 3: the kernels add 3 * 2^40 to every stream offset (what a captured graph's
    replay does); encoder (both attention paths), pool and SNN match the oracle fed masks drawn at that offset."""
    epoch_tensor(3)
    _encoder_check(dev, 2, 5, C.N_OMIC, 256, 810, epoch=3)
    _encoder_check(dev, 1, 1, 200, 256, 811, epoch=3)
    _pool_check(dev, 32, 6, True, 812, epoch=3)
    _pool_check(dev, 1, 65, False, 813, epoch=3)
    _snn_check(dev, 5, 814, epoch=3)


# ------------------------------------------------------------------------------------------- gene-expression model
def test_ge_model_training_step_equals_fp64_oracle(dev, monkeypatch):
    """GeneExprNarrowContextualAttentionGateTransformer in train() at M = 2050 (fp32 bag): forward + cross-entropy
    backward against ge_nacagat_forward with every mask -- the patch layer's (read back from H_bag: ReLU zeros and
    dropped elements both carry zero value and zero gradient), the set-Transformer's over the M rows (block hash) and
    the pooling head's.  The self-attention module's own dropout is 0 (nn.MultiheadAttention's default)."""
    from multimodal_path_omic_amd.models import GeneExprNarrowContextualAttentionGateTransformer
    m, seed = 2050, 909
    sd = syn.fill_state_dict(C.ge_model_shapes(), seed)
    model = GeneExprNarrowContextualAttentionGateTransformer()
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).train()
    assert model.self_attention.dropout == 0.0
    wsi, target = C.ge_model_inputs(m, seed + 1)
    captured = {}
    patch_fc = model._patch_fc

    def capture(bags):
        out = patch_fc(bags)
        captured["h"] = out.data.detach().float().cpu()
        return out
    model._patch_fc = capture
    reserved = []
    reserve = ops._reserve

    def record(span):
        seed_, off = reserve(span)
        reserved.append((int(span), off))
        return seed_, off
    monkeypatch.setattr(ops, "_reserve", record)
    _pin()
    y, att = model(wsi=wsi.to(dev))
    torch.nn.functional.cross_entropy(y.unsqueeze(0), target.to(dev)).backward()

    d = C.E
    enc_off = [o for s, o in reserved if s == R.encoder_span(1, m, d, FF, LAYERS)]
    pool_off = [o for s, o in reserved if s == R.pool_span(1, m, d)]
    assert len(enc_off) == 1 and len(pool_off) == 1, reserved
    enc_keeps = [tuple(_t(k[0, 0]) for k in layer)
                 for layer in R.encoder_keeps(SEED, enc_off[0], 1, 1, m, d, FF, HEADS, LAYERS, P)]
    ka, kb, kr = R.pool_keeps(SEED, pool_off[0], 1, 1, m, d, P, P, False)
    h = captured["h"]
    keep_h = (h > 0).double() / (1 - P)
    assert 0.3 < float((h == 0).double().mean()) < 0.8
    p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    yo, atto = O.ge_nacagat_forward(p, wsi.double(), keep_h=keep_h, enc_keeps=enc_keeps,
                                    pool_keeps=(_t(ka[0, 0]), _t(kb[0, 0]), _t(kr[0, 0])))
    O.ge_ce_loss(yo, target).backward()
    e_y = float((y.detach().double().cpu() - yo.detach()).abs().max())
    e_a = relerr(att["path"], atto["path"])
    errs = {n: grad_errs([prm.grad], [p[n].grad])[0] for n, prm in model.named_parameters()}
    worst = max(errs, key=errs.get)
    print(f"GE model M={m}: Y {e_y:.1e} path scores {e_a:.1e} grads max {errs[worst]:.1e} ({worst})")
    assert e_y < 1e-4, e_y
    assert e_a < 1e-3, e_a
    for n, e in errs.items():
        assert e < 5e-3, (n, e)


# ------------------------------------------------------------------------------------------- sensitivity controls
def _control(label, err, bar):
    print(f"  control {label}: error {err:.2e} = {err / bar:.0f} x the bar {bar:.0e}")
    assert err >= 100 * bar, (label, err)


def test_encoder_controls_wrong_masks_fail_by_100x(dev):
    """The oracle with a deliberately wrong mask set misses the GPU output by >= 100x the forward bar."""
    r = _encoder_check(dev, 2, 5, C.N_OMIC, 256, 900)
    sds, x, probe, y, keeps = r["sds"], r["x"], r["probe"], r["y"], r["keeps"]

    def err(ks):
        return relerr(y, _encoder_oracle(sds, x, probe, ks)[0])
    swapped = [(a, k3, f, k1) for a, k1, f, k3 in keeps]                      # out-proj and FFN-out masks swapped
    _control("encoder: sites 1 and 3 swapped", err(swapped), FWD_TOL)
    no_attn = [(None, k1, f, k3) for a, k1, f, k3 in keeps]
    _control("encoder: attention mask omitted", err(no_attn), FWD_TOL)
    rescaled = [(a, k1 / (1 - P), f, k3) for a, k1, f, k3 in keeps]           # 1 / (1-p)^2 at site 1
    _control("encoder: keep scale 1/(1-p)^2 at site 1", err(rescaled), FWD_TOL)
    same_br = [tuple(np.stack([k[0], k[0]]) for k in layer) for layer in keeps]
    _control("encoder: branch 1 drawing branch 0's counters", err(same_br), FWD_TOL)


def test_pool_controls_wrong_masks_fail_by_100x(dev):
    r = _pool_check(dev, 32, 64, False, 950)
    ka, kb, kr = r["keeps"]

    def err(ks):
        sco, ho, _, _ = _pool_oracle(r["sds"], r["x"], r["ph"], r["pa"], ks)
        return max(relerr(r["sc"], sco), relerr(r["h"], ho))
    # (a and b enter the scores as a product: swapping their masks is invisible, drawing the same counters is not)
    _control("pool: attention_b drawing attention_a's counters", err((ka, ka, kr)), FWD_TOL)
    _control("pool: attention_a mask omitted", err((None, kb, kr)), FWD_TOL)
    _control("pool: rho mask omitted", err((ka, kb, None)), FWD_TOL)
    _control("pool: keep scale 1/(1-p)^2 on attention_b", err((ka, kb / (1 - P), kr)), FWD_TOL)
    _control("pool: branch 1 drawing branch 0's counters", err((np.stack([ka[0], ka[0]]), kb, kr)), FWD_TOL)
