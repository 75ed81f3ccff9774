"""The K1 and K2 bag kernels at many tiles per wave.

A window of a few thousand rows is cut into one or two 32-row tiles per workgroup, so the loops that carry state from trip to
trip -- the forward's double-buffered image and hand-counted waits, its online softmax, the backward's image refilled under
the previous tile's stores, the load-ahead / write-late Stage loops, accumulators kept over tiles, a ragged last tile after
full ones, idle waves beside busy ones in the LDS merge -- do not run at test sizes the way they run in the benchmark (59
tiles per workgroup).  `ops.plan_workgroups` = 1 / 3 / 7 / 9 gives a workgroup up to 94 tiles; tests/test_plan_cuts_cpu.py
shows which depth every case reaches for every kernel.  Every check below is the body of an existing test, run again with
the batches built under a coarser plan, against the same reference and at the same bar (named at each test); the worst
error per cut is printed (pytest -rA) and quoted in NOTES.md.

Bags the test allocates itself carry 64 NaN rows behind them: a read past a slide's end is clamped by the kernels, so the
rows must stay NaN and every output finite."""
import pytest
import torch

import cases as C
import test_gpu_coattn_mcat as K1
import test_gpu_coattn_nacagat as K2
import test_gpu_models as M
import test_gpu_patch_coattn as F1
import test_plan_cuts_cpu as P
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.ops import BagBatch
from oracle import mpo_oracle as O

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 64
# golden case -> cuts (None: the plan's own cut, one or two tiles per workgroup)
SLIDE_CUTS = [("m2000_peaky", None), ("m2000_peaky", 1), ("m2000_peaky", 3), ("m2000_peaky", 7), ("m777_ragged", 1)]
WINDOW_CUTS = [1, 9]
relerr = K1.relerr


class _Cut:
    """ops.plan_workgroups for the plans built inside the block."""

    def __init__(self, wgs):
        self.wgs = wgs

    def __enter__(self):
        self.old, ops.plan_workgroups = ops.plan_workgroups, self.wgs

    def __exit__(self, *exc):
        ops.plan_workgroups = self.old


class _Switch:
    """One of the library's kernel-choice switches (mpo_set_*), restored on the way out."""

    def __init__(self, name, value):
        self.fn, self.value = getattr(L.lib(), name), int(value)

    def __enter__(self):
        self.prev = self.fn(self.value)

    def __exit__(self, *exc):
        self.fn(self.prev)


class _Guarded:
    """Places a bag on the device with GUARD NaN rows behind it; check() after the kernels have run."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def __call__(self, t):
        buf = torch.full((t.shape[0] + GUARD, t.shape[1]), NAN, device=self.dev, dtype=t.dtype)
        buf[:t.shape[0]] = t.to(self.dev)
        self.bufs.append((buf, t.shape[0]))
        return buf[:t.shape[0]]

    def check(self):
        assert self.bufs
        for buf, rows in self.bufs:
            assert bool(torch.isnan(buf[rows:].float()).all()) and bool(torch.isfinite(buf[:rows].float()).all())


def _report(tag, cut, worst):
    print(f"[plan cuts] {tag} cut {cut}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------ the plan itself
def test_real_plan_equals_the_restatement(dev):
    windows = list(P.CASES) + [(lengths, None) for lengths, _ in P.CASES] + [([15000] * 6, None), ([15000] * 32, None),
                                                                               ([30000] + [40] * 15 + [7] * 16, None)]
    assert L.lib().mpo_coattn_target_workgroups() == P.TARGET_WORKGROUPS
    for lengths, wgs in windows:
        with _Cut(wgs):
            batch = BagBatch(torch.empty(sum(lengths), 1, device=dev), ops.make_cu(lengths, dev), list(lengths))
            batch.plan()
        wg, c = batch._plan
        starts, n_wg, rpw = P.plan(lengths, wgs)
        assert wg.tolist() == starts and int(c.n_wg) == n_wg and int(c.rows_per_wg) == rpw, (lengths, wgs)
    assert ops.plan_workgroups is None


# ------------------------------------------------------------------------------------ K1
@pytest.mark.parametrize("case,cut", SLIDE_CUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("alt", [0, 1], ids=["general_bwd", "special_bwd"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_k1_module_under_cuts(dev, golden, dtype, alt, case, cut):
    """test_coattn_forward_backward's body and bars (out 1e-4, map element-wise 1e-3 and rows summing to 1, both gradient
    sets 1e-3, a bf16 d_bag 1.5e-2), with the backward on the general matrix-pipe kernel and on the special one of the
    storage mode (fp32 bag: the vector-ALU kernel; bf16 bag: the two-wave kernel)."""
    switch = "mpo_set_coattn_bwd_f32_vector" if dtype == torch.float32 else "mpo_set_coattn_bwd_two_wave"
    place = _Guarded(dev)
    with _Switch(switch, alt), _Cut(cut):
        worst = K1.check_coattn_forward_backward(dev, golden, case, dtype, to_dev=place)
    place.check()
    _report(f"K1 module {case} {str(dtype)[6:]} {switch[8:]}={alt}", cut, worst)


@pytest.mark.parametrize("cut", WINDOW_CUTS)
@pytest.mark.parametrize("alt", [0, 1], ids=["general_bwd", "special_bwd"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_k1_window_under_cuts_equals_its_slides(dev, dtype, alt, cut):
    """test_coattn_ragged_window_equals_per_slide's body and bars (window against each slide's own call 1e-5, the summed
    weight gradient 1e-4, each slide against the oracle 1e-4 / map 1e-3): the window runs under the cut, the slides under
    their own one-slide plans."""
    switch = "mpo_set_coattn_bwd_f32_vector" if dtype == torch.float32 else "mpo_set_coattn_bwd_two_wave"
    place = _Guarded(dev)
    with _Switch(switch, alt):
        worst = K1.check_coattn_ragged_window(dev, dtype, P.RAGGED, window_plan=_Cut(cut), place=place)
    place.check()
    _report(f"K1 window {str(dtype)[6:]} {switch[8:]}={alt} (window against slide)", cut, worst)
    assert ops.plan_workgroups is None


# ------------------------------------------------------------------------------------ patch layer + K1
@pytest.mark.parametrize("lengths,gain", [([2000], 4.0), ([777], 2.0)], ids=["m2000_peaky", "m777_ragged"])
def test_patch_layer_with_k1_under_cuts(dev, lengths, gain):
    """test_fused_forward_and_gradients_match_oracle's body and bars in eval mode (mpo_patch_coattn_mcat_forward, the gated
    backward through coattn_bwd8 with the ReLU gate on); H_bag does not depend on the bag plan's cut of the co-attention
    slices, so it must come out bit for bit under every cut."""
    base = None
    for cut in ((None, 1, 3, 7) if lengths == [2000] else (None, 1)):
        with _Cut(cut):
            h, worst = F1.check_fused_forward_and_gradients(dev, lengths, gain)
        assert bool(torch.isfinite(h.float()).all())
        _report(f"patch layer + K1 {lengths}", cut, worst)
        base = h if base is None else base
        assert torch.equal(h, base), cut


@pytest.mark.parametrize("lengths,cuts", [([2000], (None, 1, 3, 7)), (P.RAGGED, (None, 1, 9))], ids=["m2000", "ragged"])
def test_patch_layer_with_k1_training_mode_under_cuts(dev, lengths, cuts):
    """Training mode at test_fused_dropout_masks' checks: the dropout counter of the patch layer is (window row, 16-column
    group) with the stream in the key (csrc/patch_fc_fwd.hip), so at one ops._rng_calls the kept / dropped pattern of H_bag
    -- the whole tensor -- is identical under every cut; and the backward (two-wave kernel, gate = keep scale) sees that
    mask: dW_H and db_H against the oracle with the mask replayed, 2e-2."""
    p = F1._params(841)
    bags, query = F1._inputs(lengths, 842)
    ops.set_rng_epoch(None)
    _, _, h0, *_ = F1._fused(p, bags, query, dev, need_weights=False, drop_p=0.0)
    base, ref = None, None
    for cut in cuts:
        saved_calls = ops._rng_calls
        try:
            with _Cut(cut):
                ops._rng_calls = 7700
                out, _, h, d, q, _ = F1._fused(p, bags, query, dev, need_weights=False, drop_p=0.25)
                out.sum().backward()
        finally:
            ops._rng_calls = saved_calls
        assert bool(torch.isfinite(h.float()).all()) and bool(torch.isfinite(out).all())
        base = h.detach() if base is None else base
        assert torch.equal(h.detach(), base), cut
        ref = ref or F1.replayed_mask_gradients(p, bags, query, h0, base)
        e_w = F1.relmax(d["H.0.weight"].grad.cpu(), ref["H.0.weight"].grad)
        e_b = F1.relmax(d["H.0.bias"].grad.cpu(), ref["H.0.bias"].grad)
        _report(f"patch layer + K1 training {lengths}", cut, {"dW_H": e_w, "db_H": e_b})
        assert e_w < 2e-2 and e_b < 2e-2, (cut, e_w, e_b)
        assert bool(torch.isfinite(q.grad).all())
    pos = h0 > 0
    rate = float((pos & (base == 0)).sum()) / float(pos.sum())
    assert abs(rate - 0.25) < 0.01, rate                           # (~5e5 positives: sigma 6e-4)


# ------------------------------------------------------------------------------------ K2
@pytest.mark.parametrize("case,cut", SLIDE_CUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("one_pass", [0, 1], ids=["two_pass_key_grad", "one_pass_key_grad"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_k2_module_under_cuts(dev, golden, dtype, one_pass, case, cut):
    """test_nacagat_forward_backward's body and bars in eval mode, with the key-side gradient in one pass
    (bag_key_grad_kernel) and in two (bag_colacc / bag_outer)."""
    place = _Guarded(dev)
    with _Switch("mpo_set_nacagat_one_pass_key_grad", one_pass), _Cut(cut):
        worst = K2.check_nacagat_forward_backward(dev, golden, case, dtype, to_dev=place)
    place.check()
    _report(f"K2 module {case} {str(dtype)[6:]} one_pass={one_pass}", cut, worst)


@pytest.mark.parametrize("one_pass", [0, 1], ids=["two_pass_key_grad", "one_pass_key_grad"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_k2_module_training_mode_under_cuts(dev, dtype, one_pass):
    """test_nacagat_training_dropout_replays_through_oracle's body and bars (a bf16 bag: the bf16 gradient bars of
    test_nacagat_forward_backward) on 2000 rows.  The map's dropout is drawn by the softmax kernel, one block per (query,
    slide), with the counter = flat map index / 4 (csrc/bag_maps.hip): it does not see the plan, so at one ops._rng_calls
    the zero pattern of the post-dropout map is identical under every cut."""
    base = None
    for cut in (None, 1, 3, 7):
        place = _Guarded(dev)
        with _Switch("mpo_set_nacagat_one_pass_key_grad", one_pass), _Cut(cut):
            worst, a = K2.check_nacagat_training_replay(dev, 2000, 1.0, 909, to_dev=place, rng_calls=5300, dtype=dtype)
        place.check()
        _report(f"K2 training {str(dtype)[6:]} one_pass={one_pass}", cut, worst)
        base = a if base is None else base
        assert torch.equal(a == 0, base == 0), cut


def _window_against_oracle(dev, kind, dtype, cut):
    """A ragged window through the module under a cut against the oracle slide by slide, fed the same stored values: output,
    map (element-wise relative, rows summing to one), d_query / d_bag per slide and the summed parameter gradients."""
    lengths = P.RAGGED
    n, e = len(lengths), C.E
    mod, p = (K1.make_module(77, 2.0, dev) if kind == "K1" else K2.make_module(205, 1.5, dev))
    mod.eval()
    g = syn.rng(79)
    bags = [torch.clamp(syn.normal(g, (m, e)), min=0).to(dtype) for m in lengths]
    query = syn.normal(g, (n, C.N_OMIC, e))
    probe = syn.normal(g, (n, C.N_OMIC, e))
    probe_a = [syn.normal(g, (C.N_OMIC, m)) for m in lengths]
    place = _Guarded(dev)
    qd = query.to(dev).requires_grad_(True)
    with _Cut(cut):
        data = place(torch.cat(bags)).requires_grad_(True)
        batch = BagBatch(data, ops.make_cu(lengths, dev), list(lengths))
        out, maps = mod.forward_window(qd, batch, need_weights=True) if kind == "K1" else mod.forward_window(qd, batch)
        loss = (out * probe.to(dev)).sum()
        for a, pa in zip(maps, probe_a):
            loss = loss + (a * pa.to(dev)).sum()
        params = dict(mod.named_parameters())
        names = list(p)
        gs = torch.autograd.grad(loss, [qd, data] + [params[k[len("co_attention."):]] for k in names])
    place.check()
    qo = [query[i].clone().requires_grad_(True) for i in range(n)]
    bo = [b.float().clone().requires_grad_(True) for b in bags]
    loss_o, outs, maps_o = 0.0, [], []
    for i in range(n):
        if kind == "K1":
            o, a = O.mcat_coattention(qo[i], bo[i], p, need_weights=True)
        else:
            o, a = O.pregating_contextual_attention(qo[i], bo[i], p)
        outs.append(o)
        maps_o.append(a)
        loss_o = loss_o + (o * probe[i]).sum() + (a * probe_a[i]).sum()
    go = torch.autograd.grad(loss_o, qo + bo + [p[k] for k in names], allow_unused=True)
    worst = {"out": 0.0, "map": 0.0, "d_query": 0.0, "d_bag": 0.0, "grads": 0.0}
    off = 0
    for i, m in enumerate(lengths):
        a, a_o = maps[i].detach().cpu(), maps_o[i].detach()
        torch.testing.assert_close(a.sum(1), torch.ones(C.N_OMIC), rtol=1e-4, atol=1e-4)
        worst["out"] = max(worst["out"], relerr(out[i], outs[i]))
        worst["map"] = max(worst["map"], float(((a - a_o).abs() / a_o.clamp_min(1e-30)).max()))
        worst["d_bag"] = max(worst["d_bag"], relerr(gs[1][off:off + m], go[n + i]))
        off += m
    # (of the window's largest entry: a one-row slide's softmax is 1 whatever the query, its d_query is zero in the oracle)
    worst["d_query"] = relerr(gs[0], torch.stack(go[:n]))
    for k, gr, ref in zip(names, gs[2:], go[2 * n:]):
        if ref is not None and float(ref.abs().max()) > 0:
            worst["grads"] = max(worst["grads"], relerr(gr, ref))
        assert bool(torch.isfinite(gr).all()), k
    return worst


@pytest.mark.parametrize("cut", WINDOW_CUTS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_k1_window_under_cuts_equals_the_oracle(dev, dtype, cut):
    """forward_window on the ragged case at test_coattn_forward_backward's bars (the m777_ragged weights, gain 2)."""
    worst = _window_against_oracle(dev, "K1", dtype, cut)
    _report(f"K1 window {str(dtype)[6:]} (against the oracle)", cut, worst)
    assert worst["out"] < 1e-4 and worst["map"] < 1e-3 and worst["d_query"] < 1e-3 and worst["grads"] < 1e-3, worst
    assert worst["d_bag"] < (1e-3 if dtype == torch.float32 else 1.5e-2), worst


@pytest.mark.parametrize("cut", WINDOW_CUTS)
@pytest.mark.parametrize("one_pass", [0, 1], ids=["two_pass_key_grad", "one_pass_key_grad"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_k2_window_under_cuts_equals_the_oracle(dev, dtype, one_pass, cut):
    """forward_window on the ragged case at test_nacagat_forward_backward's bars for a fixture that is not peaky (the
    m777_ragged weights, gain 1.5): out 2e-4, map 1e-3, gradients 2e-3 for an fp32 bag, GRAD_TOL_BF16_BAG /
    GRAD_TOL_BF16_PARAM for a bf16 one."""
    with _Switch("mpo_set_nacagat_one_pass_key_grad", one_pass):
        worst = _window_against_oracle(dev, "K2", dtype, cut)
    _report(f"K2 window {str(dtype)[6:]} one_pass={one_pass} (against the oracle)", cut, worst)
    f32 = dtype == torch.float32
    assert worst["out"] < 2e-4 and worst["map"] < 1e-3, worst
    assert worst["d_bag"] < (2e-3 if f32 else K2.GRAD_TOL_BF16_BAG), worst
    assert max(worst["d_query"], worst["grads"]) < (2e-3 if f32 else K2.GRAD_TOL_BF16_PARAM), worst


# ------------------------------------------------------------------------------------ the patch-side gradient entries
@pytest.mark.parametrize("lengths,cuts", [([2000], (None, 1, 3, 7)), ([777], (None, 1)), (P.RAGGED, (None, 1, 9))],
                         ids=["m2000", "m777", "ragged"])
@pytest.mark.parametrize("gate", [0.0, 4.0 / 3.0])
def test_patch_grad_entries_under_cuts(dev, gate, lengths, cuts):
    """mpo_nacagat_patch_grad and mpo_nacagat_patch_grad_fused at the definitions and bars of test_patch_grad_one_pass and
    test_fused_patch_side_gradient_matches_torch, 64 NaN guard rows behind the output.  Every output row is made of its own
    inputs alone (no sum across tiles), so the rows are bit-identical between cuts -- the existing test asks this of the
    fused entry for window against slide."""
    base = {}
    for cut in cuts:
        with _Cut(cut):
            got = {"one_pass": K2.check_patch_grad_one_pass(dev, lengths, gate, 256, guard=GUARD)}
            for n_q in (6, 16):
                got[f"fused n_q={n_q}"] = K2.check_fused_patch_side_gradient(dev, n_q, gate, lengths, guard=GUARD)
        for k, v in got.items():
            assert torch.equal(v, base.setdefault(k, v)), (k, cut)
    assert ops.plan_workgroups is None


# ------------------------------------------------------------------------------------ widths 128 and 512
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_small_models_with_one_workgroup_per_slide(dev, kind, dtype):
    """test_small_model_size_matches_oracle's body and bars on 800 rows under plan_workgroups = 1: 25 tiles, 7 / 6 per wave of
    the E = 128 instantiations."""
    with _Cut(1):
        e_h, worst = M.check_small_model(dev, kind, dtype, m=800)
    _report(f"small {kind} {str(dtype)[6:]}", 1, {"hazards": e_h, "grads / bar": worst})


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_big_mcat_with_one_workgroup_per_slide(dev, dtype):
    """test_big_mcat_matches_oracle's body and bars on 800 rows under plan_workgroups = 1: the two-wave and one-wave
    E = 512 instantiations of K1 walk 13 / 12 and all 25 tiles."""
    with _Cut(1):
        e_h, e_a, worst = M.check_big_mcat(dev, dtype, m=800)
    _report(f"big mcat {str(dtype)[6:]}", 1, {"hazards": e_h, "map": e_a, "grads / bar": worst})


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_big_nacagat_with_one_workgroup_per_slide(dev, dtype):
    """test_big_nacagat_matches_oracle's body and bars on [800, 77] rows with one workgroup per slide."""
    with _Cut(1):
        e_a, worst = M.check_big_nacagat(dev, dtype, lengths=(800, 77))
    _report(f"big nacagat {str(dtype)[6:]}", 1, {"map": e_a, "grads / bar": worst})


def test_the_knob_is_back_at_its_default():
    assert ops.plan_workgroups is None
