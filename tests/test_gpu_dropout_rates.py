"""Every dropout site at rates other than 0.25, against the fp64 oracle under the same masks.

Three threshold widths coexist in the kernels (tests/rate_cases.py; DESIGN.md, "Dropout sites"): 8 bit with scale
256 / (256 - round(256 p)) (patch layer, bag self-attention), 16 bit (the bf16 patch epilogue, fed the 8-bit site's realised rate)
and 24 bit with scale 1 / (1 - p) (everything else).  At 0.25 = 64 / 256 all three drop the same elements and scale by the same
4/3, so a site that draws under one width and scales under the other, a backward that regenerates its gate under the other width,
two rates handed to each other's site, or a host restatement that models the wrong width is invisible there.  Here: 0.1 (26 / 256,
realised above p), 0.2 (51 / 256, below), 0.5 (exact; another rate than the constructors' default), 0.001 (round(256 p) = 0)
and the upper end (0.99 runs, 0.999 is refused).

Bars: the ones the same operation has at 0.25 -- tail_helpers.FWD_TOL / GRAD_TOL, test_gpu_train_step._bars, and for the patch
layer and K2 the bars of their own files, named where used.  The scale criteria of the patch layer are the issue's: fp32 storage
element-wise within 2e-4 relative; bf16 storage the mean ratio within a quarter of the gap between the two candidate scales
(bf16 rounding is 2^-9 per element and averages to ~1e-6 over 3e5 elements; the gap is 1.9e-3 at 0.1, 1.2e-3 at 0.2).

Controls (host only, no kernel is altered): each family's comparison is repeated with the oracle's masks or scale under the OTHER
convention -- the 8-bit rule where the site is 24-bit, 1 / (1 - p) where the site scales by 256 / (256 - thr8), head and rho rates
swapped -- and must fail; the factor by which it misses is printed (NOTES.md records them).  tests/test_dropout_rates_cpu.py
asserts that every replayed site has an element in the band between the two rules at these shapes and streams."""
import contextlib
import itertools

import numpy as np
import pytest
import torch

import cases as C
import dropout_replay as R
import fusion_replay as F
import rate_cases as T
import step_replay as S
import test_gpu_train_step as STEP
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.blocks import PreGatingContextualAttention
from multimodal_path_omic_amd.ops import BagBatch, make_cu
from oracle import mpo_oracle as O
from tail_helpers import (FWD_TOL, GRAD_TOL, OFF, SEED, SNN_SIZES, _encoder_check, _encoder_oracle, _pin, _pool_check, _pool_oracle,
                          _pool_setup, _snn_gpu, _snn_oracle, _snn_setup, grad_errs, relerr)
from test_gpu_coattn_nacagat import GRAD_TOL_BF16_BAG, GRAD_TOL_BF16_PARAM
from test_gpu_fusion_next import _bilinear_case, _bilinear_reference, _run_bilinear_entry, _train_errs

pytestmark = pytest.mark.gpu
E = C.E


@pytest.fixture
def fast_path():
    was = L.lib().mpo_set_gemm_fast_path(1)
    yield lambda on: L.lib().mpo_set_gemm_fast_path(int(on))
    L.lib().mpo_set_gemm_fast_path(was)


@pytest.fixture
def generator_restored():
    """The dropout generator's three values as the test found them, whatever it pinned."""
    ops.set_rng_epoch(None)
    keep = ops.rng_state()
    yield
    ops.set_rng_epoch(None)
    ops.set_rng_state(keep)


def _fails(label, err, bar):
    """A control: the comparison under the other convention must miss its bar.  -> the factor."""
    print(f"  control {label}: error {err:.2e} = {err / bar:.1f} x the bar {bar:.1e}")
    assert err > bar, (label, err, bar)
    return err / bar


def _scales(keep):
    return sorted(set(np.unique(np.asarray(keep)).tolist()) - {0.0})


# ------------------------------------------------------------------------------------------- encoder
@pytest.mark.parametrize("fast", [True, False], ids=["fast", "general"])
@pytest.mark.parametrize("p", [0.1, 0.2, 0.5])
def test_encoder_rates_equal_fp64_oracle(dev, fast_path, generator_restored, p, fast):
    """ops.encoder_stacked, 2 branches x 2 layers x 5 slides x 6 tokens at d = 256: every site on the 24-bit stream."""
    fast_path(fast)
    e = T.ENCODER
    _encoder_check(dev, e["nb"], e["ns"], e["T"], e["d"], 2100 + int(1000 * p), p=p)


@pytest.mark.parametrize("p", [0.1, 0.2, 0.5])
def test_encoder_long_axis_mixes_the_8bit_hash_with_the_24bit_stream(dev, generator_restored, p):
    """T = 17, one sequence, three-term bf16 attention on: the attention probabilities are dropped by the bag self-attention's
    8-bit block hash (scale 256 / (256 - thr8)), every other site by the 24-bit stream (1 / (1 - p)) -- two scales in one layer."""
    e = T.ENCODER_LONG
    was = L.lib().mpo_set_bag_self_attention_bf16x3(1)
    try:
        r = _encoder_check(dev, e["nb"], e["ns"], e["T"], e["d"], 2300 + int(1000 * p), p=p)
    finally:
        L.lib().mpo_set_bag_self_attention_bf16x3(was)
    for attn, out, ff, ff_out in r["keeps"]:
        assert _scales(attn) == [T.scale8(p)]
        assert _scales(out) == _scales(ff) == _scales(ff_out) == [T.scale24(p)]


def test_encoder_control_8bit_rule_at_the_24bit_sites_fails(dev, generator_restored):
    e, p = T.ENCODER, 0.1
    r = _encoder_check(dev, e["nb"], e["ns"], e["T"], e["d"], 2400, p=p)
    wrong = R.encoder_keeps(SEED, OFF, e["nb"], e["ns"], e["T"], e["d"], 512, 8, 2, T.keeps_under_8bit_rule(p))
    flipped = sum(int(((a != 0) != (b != 0)).sum()) for la, lb in zip(r["keeps"], wrong) for a, b in zip(la, lb))
    assert flipped >= 1
    err = relerr(r["y"], _encoder_oracle(r["sds"], r["x"], r["probe"], wrong)[0])
    _fails(f"encoder: masks of the 8-bit rule at p = {p} ({flipped} elements flipped, scale {T.scale8(p):.5f})", err, FWD_TOL)


# ------------------------------------------------------------------------------------------- pooling heads
@pytest.mark.parametrize("interleave", [False, True], ids=["plain", "interleaved"])
@pytest.mark.parametrize("L_,ns", T.POOL_SHAPES)
@pytest.mark.parametrize("p_head,p_rho", T.POOL_PAIRS)
def test_pool_head_and_rho_rates_equal_fp64_oracle(dev, generator_restored, p_head, p_rho, L_, ns, interleave):
    """ops.gated_pool_stacked passes the scorer's rate and rho's separately: each site must receive its own."""
    _pool_check(dev, ns, L_, interleave, 2500 + L_ + ns, p_head=p_head, p_rho=p_rho)


@pytest.mark.parametrize("p_head,p_rho", T.POOL_PAIRS)
def test_pool_rho_zeros_are_the_elements_dropped_at_rhos_rate(dev, generator_restored, p_head, p_rho):
    """test_gpu_train_dropout.py::test_pool_rho_zeros_are_exactly_the_dropped_elements with two rates: rho's bias at +10, so
    h == 0 exactly where the 24-bit rule at p_rho (not p_head, not round(256 p_rho) / 256) dropped."""
    nb, ns, L_, d = 2, 32, 6, 256
    sds, heads, rhos, x, _, _ = _pool_setup(dev, nb, ns, L_, d, 2610, rho_bias=10.0, p_head=p_head, p_rho=p_rho)
    for interleave in (False, True):
        _pin()
        with torch.no_grad():
            _, h = ops.gated_pool_stacked(x.to(dev), heads, rhos, training=True, interleave=interleave)
        h = (h.view(ns, nb, d).transpose(0, 1) if interleave else h).cpu().numpy()
        kr = R.pool_keeps(SEED, OFF, nb, ns, L_, d, p_head, p_rho, interleave)[2]
        assert ((h == 0) == (kr == 0)).all(), int(((h == 0) != (kr == 0)).sum())
        for other in (p_head, T.realised(p_rho)):
            ko = R.pool_keeps(SEED, OFF, nb, ns, L_, d, p_head, other, interleave)[2]
            assert ((h == 0) != (ko == 0)).any(), other


def test_pool_control_swapped_rates_fail(dev, generator_restored):
    p_head, p_rho, ns, L_ = 0.1, 0.2, 32, 6
    r = _pool_check(dev, ns, L_, True, 2650, p_head=p_head, p_rho=p_rho)
    wrong = R.pool_keeps(SEED, OFF, 2, ns, L_, 256, p_rho, p_head, True)
    sco, ho, _, _ = _pool_oracle(r["sds"], r["x"], r["ph"], r["pa"], wrong)
    _fails("pool: head and rho rates swapped", max(relerr(r["sc"], sco), relerr(r["h"], ho)), FWD_TOL)
    wrong = R.pool_keeps(SEED, OFF, 2, ns, L_, 256, T.realised(p_head), T.realised(p_rho), True)
    sco, ho, _, _ = _pool_oracle(r["sds"], r["x"], r["ph"], r["pa"], wrong)
    _fails("pool: masks of the 8-bit rule", max(relerr(r["sc"], sco), relerr(r["h"], ho)), FWD_TOL)


# ------------------------------------------------------------------------------------------- omic SNN
def _snn_run(dev, p, seed):
    G, xs, probe = _snn_setup(dev, T.SNN_NS, seed, p)
    y, grads = _snn_gpu(dev, G, xs, probe)
    keeps = R.snn_keeps(SEED, OFF, T.SNN_NS, len(SNN_SIZES), E, p)
    return G, xs, probe, y, grads, keeps


def _snn_errs(G, xs, probe, y, grads, keeps, p):
    yo, go = _snn_oracle(G, xs, probe, keeps, p)
    return relerr(y, yo), max(grad_errs(grads, go))


@pytest.mark.parametrize("p", [0.1, 0.2, 0.5])
def test_omic_snn_rates_equal_fp64_oracle(dev, generator_restored, p):
    """ns = 5, ragged widths: both AlphaDropout sites at rate p, whose constants a(p), b(p) are right only at that p."""
    G, xs, probe, y, grads, keeps = _snn_run(dev, p, 2700 + int(1000 * p))
    e_y, e_g = _snn_errs(G, xs, probe, y, grads, keeps, p)
    print(f"omic SNN p={p}: y {e_y:.1e} grads max {e_g:.1e}")
    assert e_y < FWD_TOL and e_g < GRAD_TOL, (e_y, e_g)
    if p == 0.1:
        # the dropped elements of the second site hold a alpha' + b; formed in fp64 here, in float32 on the device (one sqrtf,
        # one division, four products: a few ulp of 1.46, i.e. < 1e-6)
        a = 1.0 / ((1 - p) * (1 + p * R.ALPHA_PRIME ** 2)) ** 0.5
        const = a * R.ALPHA_PRIME - a * R.ALPHA_PRIME * p
        dropped = np.stack([~k2 for _, k2 in keeps], axis=1)                  # (ns, N, d)
        yd = y.double().numpy()
        worst = float(np.abs(yd[dropped] - const).max())
        print(f"omic SNN p={p}: dropped elements against a alpha' + b = {const:.7f}: max |diff| {worst:.1e}")
        assert worst < 1e-6, worst
        assert ((np.abs(yd - const) < 1e-5) == dropped).all()                 # ELU >= -1 never reaches the constant
        at_default = 1.0 / (0.75 * (1 + 0.25 * R.ALPHA_PRIME ** 2)) ** 0.5 * R.ALPHA_PRIME * 0.75
        assert abs(const - at_default) > 0.1                                  # (the constant of p = 0.25 is another number)


def test_omic_snn_control_8bit_rule_fails(dev, generator_restored):
    p = 0.1
    G, xs, probe, y, grads, keeps = _snn_run(dev, p, 2790)
    wrong = R.snn_keeps(SEED, OFF, T.SNN_NS, len(SNN_SIZES), E, T.keeps_under_8bit_rule(p))
    flipped = sum(int((a != b).sum()) for ka, kb in zip(keeps, wrong) for a, b in zip(ka, kb))
    assert flipped >= 1
    e_y, _ = _snn_errs(G, xs, probe, y, grads, wrong, p)
    _fails(f"omic SNN: masks of the 8-bit rule ({flipped} elements flipped)", e_y, FWD_TOL)
    e_y, _ = _snn_errs(G, xs, probe, y, grads, keeps, 0.25)
    _fails("omic SNN: the right masks with AlphaDropout's constants of p = 0.25", e_y, FWD_TOL)


# ------------------------------------------------------------------------------------------- patch layer
ROUTES = ["patch_fc_bf16", "fused_mcat", "epilogue", "patch_fc_f32"]


def _patch_operands(dev, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(T.PATCH_ROWS, 1024, generator=gen)
    w = (torch.rand(E, 1024, generator=gen) - 0.5) / 16
    b = torch.randn(E, generator=gen) * 0.1
    return x, w, b, gen


def _stream():
    torch.manual_seed(SEED)
    ops._rng_calls = OFF


def _gap(p):
    return abs(T.scale8(p) - T.scale24(p))


def _hold_mean_scale(what, estimate, p, expect=None):
    """Criterion (b) / (c): within a quarter of the gap between the two candidate scales of the realised one.  expect: what the
    estimate comes to under (the realised scale, 1 / (1 - p)) where it is not the scale itself (_bf16_gate)."""
    gap = _gap(p)
    right, other = expect or (T.scale8(p), T.scale24(p))
    print(f"  {what}: {estimate:.6f} (under the realised scale {right:.6f}, under 1 / (1 - p) {other:.6f}, a quarter of the gap {gap / 4:.1e})")
    assert abs(estimate - right) < gap / 4, (what, estimate, right)
    return abs(estimate - other) / (gap / 4)                   # the factor by which the other convention misses


def _bf16_gate(d, kept, p):
    """(c) where the gated gradient is STORED in bf16: sum(g) / sum(d) over the kept elements with g = bf16(d x fp32(scale)),
    under the realised scale and under 1 / (1 - p).  A bf16 upstream gradient has 128 mantissa patterns, and the relative
    rounding error of d x scale depends on the pattern alone, so it does not average out over the elements: for the scale
    256 / 205 the mean sits 2.4e-4 above the scale itself (measured 1.24908 on both bf16 routes), four fifths of the bar.  The
    expectation is therefore formed with that rounding, as tests/test_gpu_patch_epilogue.py forms its reference."""
    dk = d[kept].float()
    return tuple(float((dk * torch.tensor(s, dtype=torch.float32, device=d.device)).bfloat16().double().sum() / dk.double().sum())
                 for s in (T.scale8(p), T.scale24(p)))


def _realised_rate(what, kept, pos, p):
    n = int(pos.sum())
    rate = 1.0 - float((kept & pos).sum()) / n
    sigma = (T.realised(p) * (1 - T.realised(p)) / n) ** 0.5
    print(f"  {what}: dropped {rate:.5f} of {n} positive elements (thr8 / 256 = {T.realised(p):.5f}, p = {p}, sigma {sigma:.1e})")
    assert abs(rate - T.realised(p)) < 4 * sigma, (what, rate)


def _patch_fc_bf16(dev, p):
    """ops.patch_fc on a bf16 window, embed 256, patch_dim 1024: mpo_patch_fc_forward (8 bit), backward through
    mpo_patch_epilogue_backward, which ops feeds the realised rate."""
    x, w, b, gen = _patch_operands(dev, 3100)
    xd = x.to(dev).bfloat16()
    wp, bp = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    h0 = ops.patch_fc(xd, wp, bp, 0.0).detach()
    _stream()
    h = ops.patch_fc(xd, wp, bp, p)
    assert h._mpo_keep_scale == T.scale8(p)
    _stream()
    again = ops.patch_fc(xd, wp, bp, p).detach()
    # an upstream gradient of positive bf16 values: g = bf16(d * gate) rounds every element on its own, and the column sums
    # average that out (with all ones every element of g would be the ONE number bf16(gate): 1.1094 for 1.11304 and for 1.11111)
    d = (torch.rand(h.shape, generator=gen) + 0.5).bfloat16().float().to(dev)
    _, db_pos = torch.autograd.grad((h.float() * d).sum(), [wp, bp], retain_graph=True)
    probe = (torch.randn(h.shape, generator=gen) * 0.01).bfloat16().float().to(dev)
    dw, db = torch.autograd.grad((h.float() * probe).sum(), [wp, bp])
    kept = h.detach() != 0
    g = (probe.double() * kept * T.scale8(p)).cpu()
    xs = xd.double().cpu()
    return dict(h0=h0.float(), h=h.detach().float(), again=again.float(), gate=float(db_pos.double().sum() / d[kept].double().sum()),
                gate_expect=_bf16_gate(d, kept, p), dw=dw.cpu(), db=db.cpu(), dw_ref=g.t() @ xs, db_ref=g.sum(0),
                bar=5e-3)        # test_gpu_patch_coattn.py::test_patch_layer_alone_is_the_fused_kernel_without_its_co_attention


def _patch_fc_f32(dev, p):
    """ops.patch_fc_f32: mpo_patch_fc_f32_forward (host scale) and, on the same stream, mpo_patch_fc_f32_forward_dev; the
    one-pass backward takes the gate 256 / (256 - thr8) by value."""
    x, w, b, gen = _patch_operands(dev, 3200)
    xd = x.to(dev)
    wp, bp = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    h0 = ops.patch_fc_f32(xd, wp, bp, 0.0).detach()
    _stream()
    h = ops.patch_fc_f32(xd, wp, bp, p)
    x2 = xd.clone()
    x2._mpo_feature_scale_dev = ops.feature_scale_device(x2)
    _stream()
    again = ops.patch_fc_f32(x2, wp, bp, p).detach()
    _, db_ones = torch.autograd.grad(h.sum(), [wp, bp], retain_graph=True)
    probe = torch.randn(h.shape, generator=gen).to(dev)
    dw, db = torch.autograd.grad((h * probe).sum(), [wp, bp])
    kept = h.detach() > 0
    # all-ones upstream: the bias gradient is gate x (kept positive elements of the column), column by column
    per_column = (db_ones.double() / kept.double().sum(0)).cpu()
    g = (probe.double() * kept * T.scale8(p)).cpu()
    return dict(h0=h0, h=h.detach(), again=again, gate=float(db_ones.double().sum() / kept.double().sum()), per_column=per_column,
                dw=dw.cpu(), db=db.cpu(), dw_ref=g.t() @ xd.double().cpu(), db_ref=g.sum(0),
                bar=1e-4, bar_b=1e-5)   # test_gpu_patch_fc_f32.py::test_dropout_mask_lives_in_the_output_and_gates_the_backward


def _mcat_params(seed):
    return syn.fill_state_dict({"H.0.weight": (E, 1024), "H.0.bias": (E,), **C.MCAT_COATTN_SHAPES}, seed)


def _fused_call(dev, prm, x, query, p):
    batch = BagBatch.from_list([x.to(dev).bfloat16()])
    d = {k: v.to(dev).requires_grad_(True) for k, v in prm.items()}
    out, _, h, _ = ops.patch_coattn_mcat(batch.data, batch, d["H.0.weight"], d["H.0.bias"], p, query.to(dev).requires_grad_(True),
                                         d["co_attention.in_proj_weight"], d["co_attention.in_proj_bias"],
                                         d["co_attention.out_proj.weight"], d["co_attention.out_proj.bias"], False)
    return out, h, d


def _fused_oracle(prm, x, query, kept, scale):
    """fp64 gradients of sum(out) on the stored operands (bf16 X and W_H, H_bag rounded once to bf16) with the mask read off
    H_bag and the given keep scale."""
    pr = {k: v.double().requires_grad_(True) for k, v in prm.items()}
    w = pr["H.0.weight"] + (pr["H.0.weight"].bfloat16().double() - pr["H.0.weight"]).detach()
    h = torch.relu(x.bfloat16().double() @ w.t() + pr["H.0.bias"]) * (kept.double() * scale)
    h = h + (h.bfloat16().double() - h).detach()
    out, _ = O.mcat_coattention(query.double(), h, pr, need_weights=False)
    out.sum().backward()
    return pr["H.0.weight"].grad, pr["H.0.bias"].grad


def _fused_mcat(dev, p):
    """ops.patch_coattn_mcat: the patch layer inside mpo_patch_coattn_mcat_forward (8 bit); K1's backward finishes d(H_bag) with
    the gate 256 / (256 - thr8) it is handed by value."""
    x, _, _, gen = _patch_operands(dev, 3300)
    prm = _mcat_params(3301)
    query = syn.normal(syn.rng(3302), (6, E))
    _, h0, _ = _fused_call(dev, prm, x, query, 0.0)
    _stream()
    out, h, d = _fused_call(dev, prm, x, query, p)
    _stream()
    _, again, _ = _fused_call(dev, prm, x, query, p)
    out.sum().backward()
    dw, db = d["H.0.weight"].grad.cpu(), d["H.0.bias"].grad.cpu()
    kept = (h.detach() != 0).cpu()
    dw_ref, db_ref = _fused_oracle(prm, x, query, kept, T.scale8(p))
    res = dict(h0=h0.detach().float(), h=h.detach().float(), again=again.detach().float(), dw=dw, db=db, dw_ref=dw_ref, db_ref=db_ref,
               bar=2e-2)         # test_gpu_patch_coattn.py::test_fused_dropout_masks
    if T.thr8(p):
        # (c) where no upstream gradient can be set on H_bag: the bias gradient against the oracle's under the two scales,
        # as the fraction of the way from the realised-scale gradient to the 1 / (1 - p) one (0 = realised, 1 = the other)
        _, db_other = _fused_oracle(prm, x, query, kept, T.scale24(p))
        step = (db_other - db_ref).double()
        res["fraction"] = float(((db.double() - db_ref) * step).sum() / (step * step).sum())
    return res


def _epilogue(dev, p):
    """mpo_patch_epilogue_forward / _backward (the 16-bit site) fed ops._realised_drop(p), as PatchFcFn.backward feeds the
    backward entry: threshold 65536 thr8 / 256 exactly, scale 1 / (1 - thr8 / 256) = 256 / (256 - thr8)."""
    lib = L.lib()
    fed = ops._realised_drop(p)
    gen = torch.Generator().manual_seed(3400)
    prod = (torch.rand(T.PATCH_ROWS, E, generator=gen) + 0.1).bfloat16().to(dev)
    b = (torch.rand(E, generator=gen) * 0.5).to(dev)                           # relu(prod + b) > 0 everywhere: zeros are drops

    def forward(drop):
        h = prod.clone()
        L.check(lib.mpo_patch_epilogue_forward(L.ptr(h), L.ptr(b), h.shape[0], h.shape[1], float(drop), SEED, OFF, None, L.stream_of(h)),
                "mpo_patch_epilogue_forward")
        return h
    h0, h, again = forward(0.0), forward(fed), forward(fed)
    dy = (torch.rand(h.shape, generator=gen) + 0.5).bfloat16().to(dev)
    g = torch.empty_like(dy)
    db = torch.full((E,), float("nan"), device=dev)
    ws = torch.empty(max(256, lib.mpo_patch_epilogue_backward_workspace_bytes(h.numel(), E)), dtype=torch.uint8, device=dev)
    L.check(lib.mpo_patch_epilogue_backward(L.ptr(h), L.ptr(dy), L.ptr(g), h.numel(), E, float(fed), L.ptr(db), L.ptr(ws), ws.numel(),
                                            L.stream_of(h)), "mpo_patch_epilogue_backward")
    kept = h != 0
    scale = torch.tensor(1.0 / (1.0 - fed), dtype=torch.float32, device=dev)      # as the kernel forms it
    pre = torch.relu(prod.float() + b)
    # the existing bars of tests/test_gpu_patch_epilogue.py: bit equality of the survivors and of the gated gradient
    assert torch.equal(h[kept], (pre * scale).bfloat16()[kept])
    assert torch.equal(g, torch.where(kept, (dy.float() * scale).bfloat16(), torch.zeros_like(dy)))
    return dict(h0=h0.float(), h=h.float(), again=again.float(), gate=float(db.double().sum() / dy[kept].double().sum()),
                gate_expect=_bf16_gate(dy, kept, p) if T.thr8(p) else None, db=db.cpu(), db_ref=g.double().sum(0).cpu(), bar_b=1e-6)


_ROUTE = {"patch_fc_bf16": _patch_fc_bf16, "fused_mcat": _fused_mcat, "epilogue": _epilogue, "patch_fc_f32": _patch_fc_f32}


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def _hold_patch_route(route, p, r):
    """(a) - (d) of one route's run `r`.  -> the factor by which 1 / (1 - p) misses the scale criteria (the control)."""
    h0, h = r["h0"], r["h"]
    kept, pos = h != 0, h0 > 0.05
    # (a) a second call on the same stream drops the same elements (the backward gates by H_bag's zeros: the forward's mask)
    assert torch.equal(r["again"] != 0, kept), route
    _realised_rate(f"{route} p={p}", kept, pos, p)
    ratio = h[kept & pos].double() / h0[kept & pos].double()
    factors = []
    if route == "patch_fc_f32":                                               # (b) fp32 storage: element by element
        worst = float((ratio / T.scale8(p) - 1).abs().max())
        print(f"  {route} p={p}: survivors / base against the realised scale, worst relative {worst:.1e}")
        assert worst < 2e-4, worst
        factors.append(float((ratio / T.scale24(p) - 1).abs().min()) / 2e-4)
        per_column = float((r["per_column"] / T.scale8(p) - 1).abs().max())    # (a), (c): the gate, and the forward's mask, per column
        assert per_column < 2e-4, per_column
    factors.append(_hold_mean_scale(f"{route} p={p}: mean survivors / base", float(ratio.mean()), p))        # (b)
    if "gate" in r:                                                                                             # (c)
        factors.append(_hold_mean_scale(f"{route} p={p}: bias gradient / upstream over the kept elements", r["gate"], p,
                                        r.get("gate_expect")))
    if "fraction" in r:
        print(f"  {route} p={p}: db sits at {r['fraction']:+.3f} of the way from the realised-scale oracle to the 1 / (1 - p) one")
        assert abs(r["fraction"]) < 0.25, r["fraction"]
        factors.append(abs(1.0 - r["fraction"]) / 0.25)
    if "dw" in r:                                                                                               # (d)
        e_w, e_b = _rel(r["dw"], r["dw_ref"]), _rel(r["db"], r["db_ref"])
        print(f"  {route} p={p}: dW {e_w:.1e} db {e_b:.1e} against fp64 under H_bag's mask and the realised scale")
        assert e_w < r["bar"] and e_b < r.get("bar_b", r["bar"]), (e_w, e_b)
    else:
        e_b = float((r["db"].double() - r["db_ref"]).abs().max() / r["db_ref"].abs().max())
        assert e_b < r["bar_b"], e_b
    return min(factors)


@pytest.mark.parametrize("p", T.INEXACT)
@pytest.mark.parametrize("route", ROUTES)
def test_patch_layer_routes_hold_the_realised_scale(dev, generator_restored, route, p):
    """3 000 rows through each of the four ways to the patch layer.  The control is on the same figures: every scale estimate
    must ALSO miss 1 / (1 - p) by more than its bar (the two scales are 1.7e-3 / 9.8e-4 apart; a gradient bar of 5e-3 cannot
    tell them apart, the mean ratios can)."""
    factor = _hold_patch_route(route, p, _ROUTE[route](dev, p))
    print(f"  control {route} p={p}: the same estimates against 1 / (1 - p) miss their bars by >= {factor:.1f} x")
    assert factor > 1.0, factor


@pytest.mark.parametrize("route", ROUTES)
def test_patch_layer_rate_below_1_512_is_no_dropout_bit_for_bit(dev, generator_restored, route):
    """p = 0.001: round(256 p) = 0, so the 8-bit sites keep every element at scale 1 -- output and every gradient equal the
    eval-mode call's bit for bit; ops still reserves the call's counters (the rate is positive) and tags the keep scale 1.0."""
    p = T.SMALL
    x, w, b, gen = _patch_operands(dev, 3500)
    if route == "epilogue":
        r = _epilogue(dev, p)
        assert ops._realised_drop(p) == 0.0 and torch.equal(r["h"], r["h0"])
        return
    probe = torch.randn(T.PATCH_ROWS, E, generator=gen).to(dev)
    got = []
    for rate in (0.0, p):
        _stream()
        if route == "fused_mcat":
            out, h, d = _fused_call(dev, _mcat_params(3501), x, syn.normal(syn.rng(3502), (6, E)), rate)
            out.sum().backward()
            got.append([h.detach(), out.detach()] + [v.grad for v in d.values()])
        else:
            bf16 = route == "patch_fc_bf16"
            xd = x.to(dev).bfloat16() if bf16 else x.to(dev)
            wp, bp = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
            h = ops.patch_fc(xd, wp, bp, rate) if bf16 else ops.patch_fc_f32(xd, wp, bp, rate)
            if bf16:
                assert getattr(h, "_mpo_keep_scale", None) == (1.0 if rate else None)
            got.append([h.detach()] + list(torch.autograd.grad((h.float() * probe).sum(), [wp, bp])))
        assert ops._rng_calls == OFF + ((T.PATCH_ROWS * E // 16 + 2) + 1 if rate else 0)
    for a, c in zip(*got):
        assert torch.equal(a, c)


# ------------------------------------------------------------------------------------------- the upper end
def test_rate_that_rounds_to_256_is_refused_and_0_99_runs(dev, generator_restored):
    x, w, b, _ = _patch_operands(dev, 3600)
    xd, x16 = x.to(dev), x.to(dev).bfloat16()
    wp, bp = w.to(dev), b.to(dev)
    calls = ops._rng_calls
    words = r"realised as round\(256 p\) / 256 = 256/256"
    for call in (lambda: ops.patch_fc(x16, wp, bp, 0.999), lambda: ops.patch_fc_f32(xd, wp, bp, 0.999),
                 lambda: _fused_call(dev, _mcat_params(3601), x, syn.normal(syn.rng(3602), (6, E)), 0.999)):
        with pytest.raises(ValueError, match=words):
            call()
    assert ops._rng_calls == calls                                            # nothing was reserved
    # the C entries themselves, on output buffers that must keep their contents
    lib = L.lib()
    h32 = torch.full((T.PATCH_ROWS, E), 7.0, device=dev)
    ws = ops._workspace(lib.mpo_patch_fc_f32_workspace_bytes(0), dev)
    with pytest.raises(RuntimeError, match=words):
        L.call("mpo_patch_fc_f32_forward", L.ptr(xd), xd.shape[0], 1024, L.ptr(wp), L.ptr(bp), E, 0.999, 1, 2, None, ops.feature_scale(xd),
               L.ptr(h32), L.ptr(ws), ws.numel(), L.stream_of(xd))
    scale = ops.feature_scale_device(xd)
    with pytest.raises(RuntimeError, match=words):
        L.call("mpo_patch_fc_f32_forward_dev", L.ptr(xd), xd.shape[0], 1024, L.ptr(wp), L.ptr(bp), E, 0.999, 1, 2, None, L.ptr(scale),
               L.ptr(h32), L.ptr(ws), ws.numel(), L.stream_of(xd))
    h16 = torch.full((T.PATCH_ROWS, E), 7.0, device=dev, dtype=torch.bfloat16)
    batch = BagBatch(x16, make_cu([x16.shape[0]], dev), [x16.shape[0]])
    ws = ops._workspace(lib.mpo_patch_fc_workspace_bytes(E, 1024), dev)
    with pytest.raises(RuntimeError, match=words):
        L.call("mpo_patch_fc_forward", L.ptr(x16), L.ptr(batch.cu), 1, batch.total_rows, batch.max_rows, 1024, L.ptr(wp), L.ptr(bp), E,
               0.999, 1, 2, None, L.ptr(h16), batch.plan(), L.ptr(ws), ws.numel(), L.stream_of(x16))
    prm = {k: v.to(dev) for k, v in _mcat_params(3601).items()}
    query = syn.normal(syn.rng(3602), (6, E)).to(dev)
    out = torch.full((6, E), 7.0, device=dev)
    saved = torch.empty(lib.mpo_coattn_saved_floats(1, 6, E), device=dev)
    ws = ops._workspace(lib.mpo_patch_coattn_workspace_bytes(1, 6, E, 1024), dev)
    with pytest.raises(RuntimeError, match=words):
        L.call("mpo_patch_coattn_mcat_forward", L.ptr(x16), L.ptr(batch.cu), 1, batch.total_rows, batch.max_rows, 1024,
               L.ptr(prm["H.0.weight"]), L.ptr(prm["H.0.bias"]), 0.999, 1, 2, None, L.ptr(query), 6, E,
               L.ptr(prm["co_attention.in_proj_weight"]), L.ptr(prm["co_attention.in_proj_bias"]),
               L.ptr(prm["co_attention.out_proj.weight"]), L.ptr(prm["co_attention.out_proj.bias"]), L.ptr(h16), L.ptr(out), None,
               L.ptr(saved), batch.plan(), L.ptr(ws), ws.numel(), L.stream_of(query))
    torch.cuda.synchronize()
    assert bool((h32 == 7.0).all()) and bool((h16 == 7.0).all()) and bool((out == 7.0).all())
    # 0.99: thr8 = 253, three bytes of 256 keep, scale 256 / 3 -- the fp32 route's scale check, element by element
    p = 0.99
    assert T.thr8(p) == 253
    wq, bq = wp.clone().requires_grad_(True), bp.clone().requires_grad_(True)
    h0 = ops.patch_fc_f32(xd, wq, bq, 0.0).detach()
    h = ops.patch_fc_f32(xd, wq, bq, p)
    kept, pos = h.detach() != 0, h0 > 0.05
    _realised_rate("patch_fc_f32 p=0.99", kept, pos, p)
    ratio = h.detach()[kept & pos].double() / h0[kept & pos].double()
    worst = float((ratio / T.scale8(p) - 1).abs().max())
    print(f"  patch_fc_f32 p={p}: {int((kept & pos).sum())} survivors, survivors / base against 256 / 3: worst relative {worst:.1e}")
    assert worst < 2e-4 and int((kept & pos).sum()) > 1000, worst
    _, db_ones = torch.autograd.grad(h.sum(), [wq, bq])
    gate = float(db_ones.double().sum() / (h.detach() > 0).double().sum())
    assert abs(gate / T.scale8(p) - 1) < 2e-4 and abs(gate / T.scale24(p) - 1) > 0.1, gate


# ------------------------------------------------------------------------------------------- K2 map (NaCAGaT co-attention)
def _k2_module(dev, seed, p):
    sd = syn.fill_state_dict(C.NACAGAT_COATTN_SHAPES, seed)
    mod = PreGatingContextualAttention(embed_dim=E, num_heads=1, dropout_p=p)
    mod.load_state_dict({k[len("co_attention."):]: v for k, v in sd.items()}, strict=True)
    return mod.to(dev), sd


def _k2_run(dev, lengths, p, dtype, seed):
    mod, sd = _k2_module(dev, seed, p)
    n_q, rows = T.MAP_N_Q, sum(lengths)
    cases = [C.coattn_inputs(m, seed + 1 + b) for b, m in enumerate(lengths)]           # per slide (q, bag, p_out, p_a)
    query = torch.stack([c[0] for c in cases])
    bags = torch.cat([c[1] for c in cases]).to(dtype)
    qd = query.to(dev).requires_grad_(True)
    bd = bags.to(dev).requires_grad_(True)
    batch = BagBatch(bd, make_cu(lengths, dev), list(lengths))
    mod.eval()
    with torch.no_grad():
        _, maps_eval = mod.forward_window(qd, batch)
    mod.train()
    torch.manual_seed(SEED)
    ops._rng_calls = T.MAP_OFF
    with S.recording() as records:
        out, maps = mod.forward_window(qd, batch)
    assert records == [(R.map_span(n_q, rows), T.MAP_OFF)], records
    loss = sum((out[b] * c[2].to(dev)).sum() + (maps[b] * c[3].to(dev)).sum() for b, c in enumerate(cases))
    params = dict(mod.named_parameters())
    grads = torch.autograd.grad(loss, [qd, bd] + [params[k[len("co_attention."):]] for k in sd])
    return dict(sd=sd, cases=cases, bags=bags.float(), out=out.detach().cpu(), maps=[a.detach().cpu() for a in maps],
                maps_eval=[a.cpu() for a in maps_eval], grads=[g.float().cpu() for g in grads])


def _k2_errs(run, keeps, dtype):
    """Worst miss of (out, map, each gradient) against the fp64 oracle under `keeps`, each over its bar of
    tests/test_gpu_coattn_nacagat.py's training replay: out 2e-4, map 1e-3, gradients 2e-3 (bf16 bags: 7e-3 the bag's, 5e-3)."""
    prm = {k: v.double().requires_grad_(True) for k, v in run["sd"].items()}
    qs = [c[0].double().requires_grad_(True) for c in run["cases"]]
    bo = run["bags"].double().requires_grad_(True)
    loss, outs, maps, row = 0, [], [], 0
    for b, c in enumerate(run["cases"]):
        m = c[1].shape[0]
        o, a = O.pregating_contextual_attention(qs[b], bo[row:row + m], prm, keep=torch.from_numpy(np.ascontiguousarray(keeps[b])))
        loss = loss + (o * c[2].double()).sum() + (a * c[3].double()).sum()
        outs.append(o.detach())
        maps.append(a.detach())
        row += m
    g = torch.autograd.grad(loss, qs + [bo] + list(prm.values()), allow_unused=True)
    g_ref = [torch.stack(g[:len(qs)]), g[len(qs)]] + [x if x is not None else torch.zeros_like(t) for x, t in zip(g[len(qs) + 1:], prm.values())]
    f32 = dtype == torch.float32
    figures = {"out": (relerr(run["out"], torch.stack(outs)), 2e-4),
               "map": (max(relerr(a, ao) for a, ao in zip(run["maps"], maps)), 1e-3)}
    for name, got, ref in zip(["query", "bag"] + list(prm), run["grads"], g_ref):
        bar = 2e-3 if f32 else (GRAD_TOL_BF16_BAG if name == "bag" else GRAD_TOL_BF16_PARAM)
        figures["grad/" + name] = (relerr(got, ref), bar)
    return figures


def _k2_check(dev, p, lengths, dtype):
    run = _k2_run(dev, lengths, p, dtype, 3700 + sum(lengths))
    keeps = R.map_keeps(SEED, T.MAP_OFF, T.MAP_N_Q, lengths, p)
    dropped = 0
    for a, a_eval, k in zip(run["maps"], run["maps_eval"], keeps):
        assert bool((a_eval > 0).all())
        diff = (a.numpy() == 0) != (k == 0)
        assert not diff.any(), int(diff.sum())
        kept = a != 0
        ratio = a[kept].double() / a_eval[kept].double()
        assert float((ratio * (1 - p) - 1).abs().max()) < 1e-5, float((ratio * (1 - p) - 1).abs().max())
        dropped += int((~kept).sum())
    figures = _k2_errs(run, keeps, dtype)
    print(f"K2 map p={p} lengths={lengths} {dtype}: {dropped} dropped; " + " ".join(f"{k} {e:.1e}" for k, (e, _) in figures.items()))
    for k, (e, bar) in figures.items():
        assert e < bar, (k, e, bar)
    return dropped


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("lengths", T.MAP_LENGTHS, ids=["33_5", "777"])
@pytest.mark.parametrize("p", T.INEXACT)
def test_k2_map_rates_mask_scale_and_fp64_oracle(dev, generator_restored, p, lengths, dtype):
    """The co-attention map's dropout (csrc/bag_maps.hip map_keep4, 24 bit) at the module's own rate: the zero pattern of the
    returned map equals the host restatement dropout_replay.map_keeps element for element (the softmax is positive before
    dropout), the kept elements are the eval-mode map times 1 / (1 - p), and output, map and every gradient match the oracle
    under the HOST masks -- a kernel dropping at another rate, identically forward and backward, fails all three."""
    _k2_check(dev, p, lengths, dtype)


def test_k2_map_still_drops_at_a_rate_below_1_512(dev, generator_restored):
    """p = 0.001 on one slide of 777 rows (4 662 elements): the 24-bit site still drops, and still matches fp64."""
    assert _k2_check(dev, T.SMALL, [777], torch.float32) >= 1


def test_k2_map_control_8bit_rule_fails(dev, generator_restored):
    for lengths in T.MAP_LENGTHS:
        p, dtype = 0.1, torch.float32
        run = _k2_run(dev, lengths, p, dtype, 3700 + sum(lengths))
        wrong = R.map_keeps(SEED, T.MAP_OFF, T.MAP_N_Q, lengths, T.keeps_under_8bit_rule(p))
        right = R.map_keeps(SEED, T.MAP_OFF, T.MAP_N_Q, lengths, p)
        flipped = sum(int(((a != 0) != (b != 0)).sum()) for a, b in zip(right, wrong))
        assert flipped >= 1
        figures = _k2_errs(run, wrong, dtype)
        worst = max(figures, key=lambda k: figures[k][0] / figures[k][1])
        _fails(f"K2 map {lengths}: masks of the 8-bit rule ({flipped} flipped; {worst})", *figures[worst])


# ------------------------------------------------------------------------------------------- bilinear head
@pytest.mark.parametrize("form", ["plain", "ces"])
def test_bilinear_head_rate_equals_fp64_oracle(dev, generator_restored, form):
    """b = 4 at rate 0.1: the head's five sites through tests/fusion_replay.py (24 bit); the 8-bit rule's masks must fail."""
    d, b, p, epoch = 256, 4, 0.1, 3
    sd, h, label, cens, probes, w = _bilinear_case(d, b, 4, 3800)
    ep = torch.tensor([epoch], dtype=torch.int64, device=dev)
    got = _run_bilinear_entry(dev, sd, h, form, label, cens, probes, w, True, rng=(p, SEED, OFF), epoch=ep)
    keeps = F.bilinear_keeps(SEED, OFF, b, d, p, epoch)
    e_out, e_grad = _train_errs(got, _bilinear_reference(sd, h, form, label, cens, probes, w, keeps))
    print(f"bilinear head {form} p={p}: outputs {e_out:.1e} gradients {e_grad:.1e}")
    assert e_out < FWD_TOL and e_grad < GRAD_TOL, (e_out, e_grad)
    wrong = F.bilinear_keeps(SEED, OFF, b, d, T.keeps_under_8bit_rule(p), epoch)
    flipped = sum(int(((keeps[k] != 0) != (wrong[k] != 0)).sum()) for k in keeps)
    assert flipped >= 1
    c_out, _ = _train_errs(got, _bilinear_reference(sd, h, form, label, cens, probes, w, wrong))
    _fails(f"bilinear head {form}: masks of the 8-bit rule ({flipped} flipped)", c_out, FWD_TOL)


# ------------------------------------------------------------------------------------------- 24-bit sites at 0.001
def test_24bit_sites_still_drop_at_a_rate_below_1_512(dev, generator_restored):
    e = T.ENCODER
    r = _encoder_check(dev, e["nb"], e["ns"], e["T"], e["d"], 3900, p=T.SMALL)
    dropped = sum(int((k == 0).sum()) for layer in r["keeps"] for k in layer)
    assert dropped >= 10, dropped                                            # 368 640 draws at 0.001


# ------------------------------------------------------------------------------------------- the whole step
# A ReLU whose pre-activation is within the forward's own fp32 error of zero has no determined gate: the device may put it on
# the other side than fp64 does, and the gradients of that one FFN column (its row of linear1.weight, its element of
# linear1.bias) then differ by one token's contribution while every other element agrees to 1e-9.  (MCAT fp32 at dropout 0.1,
# epoch 2: column 142 of path_transformer.layers.0.linear1 has a pre-activation of 2.65e-6 beside a layer maximum of 3.61 --
# 7e-7 relative, the tail's measured forward error is 3e-7; GPU against fp64 3.7e-3 of the bias gradient's maximum at that one
# element, 3e-9 at the next; the CPU oracle run in fp32 under the same masks stays on fp64's side: 7e-7.)  As
# test_gpu_patch_fc_f32.py compares under the gate the kernel used, the step below is compared under fp64's gates and, only if
# that misses and only for pre-activations below KINK_BAND of their layer's maximum, under the other gate for those elements.
KINK_BAND = 1e-5           # a tenth of FWD_TOL, the forward bar the tail is held to; 30 x its measured forward error


@contextlib.contextmanager
def _ffn_relu_taps(flips=None):
    """Inside: the oracle's encoder FFNs report every fp64 pre-activation of linear1 below KINK_BAND of its call's largest as
    (parameter prefix, call index, flat index, value), and negate those named in `flips` {(prefix, call index): [flat indices]}
    (a change of value below 2e-5 of the layer's maximum, which puts the ReLU's gate on the other side)."""
    lin, seen, calls = O._lin, [], {}

    def tap(x, p, name):
        y = lin(x, p, name)
        if not name.endswith(".linear1") or y.dtype != torch.float64:
            return y
        i = calls[name] = calls.get(name, -1) + 1
        flat = y.detach().reshape(-1)
        near = torch.nonzero(flat.abs() < KINK_BAND * float(flat.abs().max())).reshape(-1).tolist()
        seen.extend((name, i, j, float(flat[j])) for j in near)
        other_side = [j for j in (flips or {}).get((name, i), []) if j in near]      # (under a control's masks it may not be marginal)
        if other_side:
            shift = torch.zeros(y.numel(), dtype=y.dtype)
            shift[other_side] = -2.0 * flat[other_side]
            y = y + shift.view(y.shape)                    # (the value changes sign, the derivative with respect to it stays 1)
        return y
    O._lin = tap
    try:
        yield seen
    finally:
        O._lin = lin


def _flips(subset):
    flips = {}
    for name, i, j, _ in subset or ():
        flips.setdefault((name, i), []).append(j)
    return flips


def _step_errors(kind, dtype, run, keep_maps):
    """STEP._compare against the fp64 oracle -> (errors, marginal ReLU pre-activations, those taken on the other side or None)."""
    with _ffn_relu_taps() as marginal:
        errs = STEP._compare(run, STEP._oracle(kind, dtype, run, keep_maps=keep_maps), dtype)
    if STEP._factor(errs) < 1.0 or not 1 <= len(marginal) <= 3:
        return errs, marginal, None
    for n in range(1, len(marginal) + 1):
        for subset in itertools.combinations(marginal, n):
            with _ffn_relu_taps(_flips(subset)):
                other = STEP._compare(run, STEP._oracle(kind, dtype, run, keep_maps=keep_maps), dtype)
            print(f"  with {[m[:3] for m in subset]} on the other side: {STEP._line(other)}")
            if STEP._factor(other) < 1.0:
                return other, marginal, subset
    return errs, marginal, None


STEP_CASES = [("mcat", torch.bfloat16, (0.1, 0.25)), ("nacagat", torch.float32, (0.1, 0.25)), ("mcat", torch.float32, (0.1, 0.2)),
              ("nacagat", torch.bfloat16, (0.1, 0.25))]


@pytest.mark.parametrize("kind,dtype,rates", STEP_CASES, ids=["mcat_bf16_0.1", "nacagat_fp32_0.1", "mcat_fp32_0.1_heads_0.2",
                                                               "nacagat_bf16_0.1"])
def test_whole_step_gives_every_site_its_own_rate(dev, kind, dtype, rates):
    """test_gpu_train_step.py's eager step (463 rows, 4 slides, 6 groups, d 256, epoch tensor = 2) with the model built at
    dropout = 0.1 -- patch layer (8 bit: 26 / 256), SNN, both encoders, rho -- while the pooling heads keep their hard-wired
    0.25 (or are set to 0.2) and NaCAGaT's map its own 0.25: up to three rates in one step.  Same bars (STEP._bars); the K2 map's
    mask comes from the host restatement.  Control: the oracle with two sites' rates exchanged (head <-> rho), or with the
    encoders' masks under the 8-bit rule, misses them."""
    p, p_head = rates
    with STEP._generator_restored():
        run = STEP._eager_run(dev, kind, dtype, 2, rates=rates)
        assert set(run["sites"]) == {"snn", "patch", "encoder", "pool"} | ({"map"} if kind == "nacagat" else set())
        assert not S.ranges_overlap(run["records"])
        keep_maps = None
        if kind == "nacagat":
            keep_maps = [torch.from_numpy(np.ascontiguousarray(k)) for k in run["host"]["map"]]
            for host, dev_keep in zip(keep_maps, run["keep_maps"]):
                assert torch.equal(host != 0, dev_keep != 0) and _scales(host) in ([], [T.scale24(S.MAP_P)])
        kept = run["keep_h"] != 0
        assert _scales(run["keep_h"]) == [T.scale8(p)] and 0.3 < float(kept.double().mean()) < 0.6
        errs, marginal, other_side = _step_errors(kind, dtype, run, keep_maps)
        print(f"[train step] {kind} {dtype} dropout={p} heads={p_head} map={S.MAP_P}: {STEP._line(errs)}")
        print(f"  FFN pre-activations below {KINK_BAND:.0e} of their layer's maximum: {marginal}; compared on the other side: {other_side}")
        for k, v in errs.items():
            assert v[0] < v[1], (k, v)
        sites, B, N, D = run["sites"], STEP.B, STEP.N, STEP.D
        wrong = {"pool: head and rho rates exchanged":
                 dict(run["host"], pool=R.pool_keeps(STEP.SEED, sites["pool"], 2, B, N, D, p, p_head, True, 2)),
                 "encoders: masks of the 8-bit rule":
                 dict(run["host"], encoder=R.encoder_keeps(STEP.SEED, sites["encoder"], 2, B, N, D, S.FF, S.HEADS, S.LAYERS,
                                                           T.keeps_under_8bit_rule(p), 2)),
                 "SNN: masks of the heads' rate":
                 dict(run["host"], snn=R.snn_keeps(STEP.SEED, sites["snn"], B, N, D, p_head, 2))}
        for label, host in wrong.items():
            with _ffn_relu_taps(_flips(other_side)):
                bad = STEP._compare(run, STEP._oracle(kind, dtype, run, host=host, keep_maps=keep_maps), dtype)
            print(f"  control [{kind} {dtype}] {label}: {STEP._factor(bad):.1f} x the bar (the right masks: {STEP._factor(errs):.2f} x)")
            assert STEP._factor(bad) > 1.0, (label, bad)
        # the patch layer's scale: 1 / (1 - p) where the site scales by 256 / (256 - thr8).  The two are 1.7e-3 apart and every
        # activation of H_bag moves by that: the forward bars (1e-4 fp32, 2e-4 bf16 window) see it on either storage
        with _ffn_relu_taps(_flips(other_side)):
            bad = STEP._compare(run, STEP._oracle(kind, dtype, run, keep_h=kept.double() * T.scale24(p), keep_maps=keep_maps), dtype)
        print(f"  control [{kind} {dtype}] patch layer scaled by 1 / (1 - p): {STEP._factor(bad):.1f} x the bar")
        assert STEP._factor(bad) > 1.0, bad
