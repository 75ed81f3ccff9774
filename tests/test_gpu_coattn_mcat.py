"""GPU parity of K1 (MCAT co-attention, HIP) against the oracle and the reference's golden vectors.

Calls go through the drop-in module -> autograd Function -> C ABI (libmpo_hip.so).
Tolerances: north star = 1e-3 in fp32.  Attention maps are compared RELATIVELY.
For a bf16-stored bag the oracle is fed the same bf16-rounded values (bf16 is a storage format of
the INPUT; arithmetic stays fp32-accurate through hi/lo operand splitting), the bag gradient is
rounded to bf16 by construction and gets a bf16-sized tolerance.
"""
import contextlib
import math

import pytest
import torch

import cases as C
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.blocks import CoAttention
from multimodal_path_omic_amd.ops import BagBatch, linear
from oracle import mpo_oracle as O

pytestmark = pytest.mark.gpu
sub = syn.subsample
# check_coattn_forward_backward's bars: the output against its largest entry, the map element by element and relative, every
# gradient against its largest entry; a bf16 bag's gradient is emitted in bf16
OUT_TOL, MAP_REL_TOL, GRAD_TOL, BAG_GRAD_TOL_BF16 = 1e-4, 1e-3, 1e-3, 1.5e-2


def relerr(a, b):
    a, b = a.detach().float().cpu().reshape(-1), b.detach().float().cpu().reshape(-1)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def make_module(seed, gain, dev):
    sd = syn.fill_state_dict(C.MCAT_COATTN_SHAPES, seed, gain)
    mod = CoAttention(C.E, 1)
    mod.load_state_dict({k[len("co_attention."):]: v for k, v in sd.items()}, strict=True)
    return mod.to(dev), {k: v.clone().requires_grad_(True) for k, v in sd.items()}


def oracle_grads(loss, named):
    gs = torch.autograd.grad(loss, [t for _, t in named], allow_unused=True, retain_graph=True)
    return {n: (torch.zeros_like(t) if g is None else g) for (n, t), g in zip(named, gs)}


@pytest.mark.parametrize("act", ["none", "relu", "elu", "tanh", "sigmoid"])
@pytest.mark.parametrize("rows,i,o", [(6, 256, 256), (192, 256, 768), (7, 100, 256), (33, 512, 4)])
def test_linear_matches_torch(dev, act, rows, i, o):
    g = syn.rng(11)
    x = syn.normal(g, (rows, i)).to(dev).requires_grad_(True)
    w = syn.normal(g, (o, i), 0.1).to(dev).requires_grad_(True)
    b = syn.normal(g, (o,)).to(dev).requires_grad_(True)
    probe = syn.normal(g, (rows, o)).to(dev)
    y = linear(x, w, b, act)
    f = {"none": lambda t: t, "relu": torch.relu, "elu": torch.nn.functional.elu, "tanh": torch.tanh,
         "sigmoid": torch.sigmoid}[act]
    x64, w64, b64 = (t.detach().double().requires_grad_(True) for t in (x, w, b))
    y64 = f(x64 @ w64.t() + b64)
    assert relerr(y, y64) < 1e-5
    gy = torch.autograd.grad((y * probe).sum(), [x, w, b])
    g64 = torch.autograd.grad((y64 * probe.double()).sum(), [x64, w64, b64])
    for a, r in zip(gy, g64):
        assert relerr(a, r) < 1e-5


@pytest.mark.parametrize("case", list(C.COATTN_CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_coattn_forward_backward(dev, golden, case, dtype):
    check_coattn_forward_backward(dev, golden, case, dtype)


def check_coattn_forward_backward(dev, golden, case, dtype, to_dev=None):
    """The body of test_coattn_forward_backward (tests/test_gpu_plan_cuts.py runs it again under coarser work plans).
    `to_dev` places the bag on the device (default: a plain copy); returns the worst error per quantity."""
    m, gain, seed = C.COATTN_CASES[case]
    mod, p = make_module(seed, gain, dev)
    q, bag, p_out, p_a = C.coattn_inputs(m, seed + 1)
    bag_in = bag.to(dtype)                                    # what the kernel stores/reads
    to_dev = to_dev or (lambda t: t.to(dev))
    worst = {}
    # ---- oracle on exactly the values the kernel sees
    qo = q.clone().requires_grad_(True)
    bo = bag_in.float().clone().requires_grad_(True)
    out_o, a_o = O.mcat_coattention(qo, bo, p, need_weights=True)
    named = [("query", qo), ("bag", bo)] + list(p.items())
    g1_o = oracle_grads((out_o * p_out).sum() + (a_o * p_a).sum(), named)
    g0_o = oracle_grads((out_o * p_out).sum(), named)

    qd = q.to(dev).requires_grad_(True)
    bd = to_dev(bag_in).requires_grad_(True)
    # training-style call (no map), models/mcat/mcat.py:97 with inference=False
    out0, a0 = mod(query=qd, key=bd, value=bd, need_weights=False)
    assert a0 is None
    out1, a1 = mod(query=qd, key=bd, value=bd, need_weights=True)
    assert a1.shape == (C.N_OMIC, m)
    assert relerr(out0, out_o) < OUT_TOL, relerr(out0, out_o)
    assert relerr(out1, out_o) < OUT_TOL
    worst["out"] = max(relerr(out0, out_o), relerr(out1, out_o))
    # attention map: relative, element-wise
    rel_a = ((a1.detach().cpu() - a_o.detach()).abs() / a_o.detach().clamp_min(1e-30)).max().item()
    # The score operand enters the MFMA in THREE bf16 terms (all 24 mantissa bits; two terms left the deliberately peaky
    # fixture, |logit| ~ 130, at 1.1e-3): the north_star bar holds for every case (the fp32 oracle itself is 6e-5 from
    # fp64 on the peaky one; an fp32 bag keeps a 2^-17 residual of its own hi + lo split).
    print(f"[K1 map] {case} {str(dtype)[6:]}: rel err {rel_a:.2e}")
    assert rel_a < MAP_REL_TOL, rel_a
    worst["map"] = rel_a
    torch.testing.assert_close(a1.sum(1).cpu(), torch.ones(C.N_OMIC), rtol=1e-4, atol=1e-4)

    params = dict(mod.named_parameters())
    tensors = [qd, bd] + [params[k[len("co_attention."):]] for k in p]
    names = ["query", "bag"] + list(p)
    bag_tol = GRAD_TOL if dtype == torch.float32 else BAG_GRAD_TOL_BF16       # d_bag is emitted in the bag's dtype
    for tag, loss, ref in (("grad0", (out0 * p_out.to(dev)).sum(), g0_o),
                           ("grad1", (out1 * p_out.to(dev)).sum() + (a1 * p_a.to(dev)).sum(), g1_o)):
        gs = torch.autograd.grad(loss, tensors, retain_graph=True)
        for n, gr in zip(names, gs):
            tol = bag_tol if n == "bag" else GRAD_TOL
            e = relerr(gr, ref[n]) if ref[n].abs().max() > 0 else float(gr.abs().max())
            assert e < tol, (tag, n, e)
            key = "d_bag" if n == "bag" else "grads"
            worst[key] = max(worst.get(key, 0.0), e)
            assert bool(torch.isfinite(gr.float()).all()), (tag, n)

    if dtype == torch.float32:
        # the reference's own numbers (golden vectors), fp32 bag only
        g = golden("coattn_mcat")
        assert relerr(out1, g[f"{case}/out"]) < 1e-3
        ga = g[f"{case}/A_sub"]
        assert ((sub(a1).cpu() - ga).abs() / ga.clamp_min(1e-30)).max().item() < 1e-3
        gs = torch.autograd.grad((out1 * p_out.to(dev)).sum() + (a1 * p_a.to(dev)).sum(), tensors)
        for n, gr in zip(names, gs):
            ref = g[f"{case}/grad1/{n}"]
            if ref.abs().max() > 0:
                assert relerr(sub(gr), ref) < 2e-3, (n, relerr(sub(gr), ref))
    return worst


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_coattn_ragged_window_equals_per_slide(dev, dtype):
    """A window of slides in ONE ragged launch gives each slide the result of its own call."""
    check_coattn_ragged_window(dev, dtype, [1, 31, 32, 33, 500, 4097, 129])


def check_coattn_ragged_window(dev, dtype, lengths, window_plan=contextlib.nullcontext(), place=None):
    """The body of test_coattn_ragged_window_equals_per_slide; the window's batch is built, run and differentiated inside
    `window_plan` (tests/test_gpu_plan_cuts.py: a coarser work plan for the window, the slides keep their own); `place` puts
    the window's concatenated rows where the caller wants them (default: a clone).  Returns the worst window-against-slide
    differences."""
    mod, p = make_module(77, 2.0, dev)
    g = syn.rng(78)
    bags = [torch.clamp(syn.normal(g, (m, C.E)), min=0).to(dtype).to(dev) for m in lengths]
    query = syn.normal(g, (len(lengths), C.N_OMIC, C.E)).to(dev).requires_grad_(True)
    probe = syn.normal(g, (len(lengths), C.N_OMIC, C.E)).to(dev)
    with window_plan:
        batch = BagBatch.from_list(bags)
        data = (place(batch.data) if place else batch.data.clone()).requires_grad_(True)
        out_w, maps = mod.forward_window(query, batch.with_data(data), need_weights=True)
        gq, gb, gw = torch.autograd.grad((out_w * probe).sum(), [query, data, mod.in_proj_weight])
    assert all(bool(torch.isfinite(t.float()).all()) for t in (out_w, gq, gb, gw, *maps))
    off = 0
    worst = {"out": 0.0, "map": 0.0, "d_query": 0.0, "d_bag": 0.0}
    gw_sum = torch.zeros_like(gw)
    for i, bag in enumerate(bags):
        qi = query[i].detach().clone().requires_grad_(True)
        bi = bag.clone().requires_grad_(True)
        o_i, a_i = mod(query=qi, key=bi, value=bi, need_weights=True)
        assert relerr(out_w[i], o_i) < 1e-5
        assert relerr(maps[i], a_i) < 1e-5
        # and against the oracle
        o_o, a_o = O.mcat_coattention(qi.detach().cpu(), bag.float().cpu(), {k: v.detach() for k, v in p.items()})
        assert relerr(o_i, o_o) < 1e-4
        assert ((a_i.cpu() - a_o).abs() / a_o.clamp_min(1e-30)).max().item() < 1e-3
        gqi, gbi, gwi = torch.autograd.grad((o_i * probe[i]).sum(), [qi, bi, mod.in_proj_weight])
        for k, v in (("out", relerr(out_w[i], o_i)), ("map", relerr(maps[i], a_i)), ("d_query", relerr(gq[i], gqi)),
                     ("d_bag", relerr(gb[off:off + lengths[i]], gbi))):
            worst[k] = max(worst[k], v)
        assert relerr(gq[i], gqi) < 1e-5
        assert relerr(gb[off:off + lengths[i]], gbi) < 1e-5
        gw_sum += gwi
        off += lengths[i]
    worst["d_in_proj_weight"] = relerr(gw, gw_sum)
    assert relerr(gw, gw_sum) < 1e-4
    return worst


def test_coattn_rejects_bad_arguments(dev):
    mod, _ = make_module(1, 1.0, dev)
    q = torch.zeros(C.N_OMIC, C.E, device=dev)
    bag = torch.zeros(10, C.E, device=dev)
    with pytest.raises(NotImplementedError):
        mod(query=q, key=bag, value=bag.clone())
    with pytest.raises(RuntimeError):
        mod(query=q.cpu(), key=bag.cpu(), value=bag.cpu())          # no CPU fallback
    with pytest.raises(RuntimeError):
        mod(query=torch.zeros(17, C.E, device=dev), key=bag, value=bag)   # > 16 queries


@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_full_slide_100k_patches_fp32(dev, kind):
    """BASELINE cfg 5: one 100 000-patch fp32 bag (102.4 MB) through the co-attention of either model -- the split-M
    partials over ~260 workgroups, the ragged map at full length and the gradients, against the oracle on the CPU."""
    from multimodal_path_omic_amd.blocks import PreGatingContextualAttention
    from oracle import mpo_oracle as O
    m, seed = 100_000, 4321
    q, bag, p_out, p_a = C.coattn_inputs(m, seed)
    if kind == "mcat":
        mod, p = make_module(seed, 1.0, dev)
    else:
        sd = syn.fill_state_dict(C.NACAGAT_COATTN_SHAPES, seed)
        mod = PreGatingContextualAttention(embed_dim=C.E, num_heads=1)
        mod.load_state_dict({k[len("co_attention."):]: v for k, v in sd.items()}, strict=True)
        mod.to(dev).eval()
        p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    qo, bo = q.clone().requires_grad_(True), bag.clone().requires_grad_(True)
    if kind == "mcat":
        out_o, a_o = O.mcat_coattention(qo, bo, p, need_weights=True)
    else:
        out_o, a_o = O.pregating_contextual_attention(qo, bo, p)
    named = [("query", qo), ("bag", bo)] + list(p.items())
    # the map probe is scaled up: 100 000 entries of ~1e-5 each would otherwise not register against the output term
    g_o = oracle_grads((out_o * p_out).sum() + 1e3 * (a_o * p_a).sum(), named)
    qd, bd = q.to(dev).requires_grad_(True), bag.to(dev).requires_grad_(True)
    out, a = mod(query=qd, key=bd, value=bd, need_weights=True) if kind == "mcat" else mod(query=qd, key=bd, value=bd)
    assert a.shape == (C.N_OMIC, m)
    assert relerr(out, out_o) < 2e-4
    assert ((a.detach().cpu() - a_o.detach()).abs() / a_o.detach().clamp_min(1e-30)).max().item() < 1e-3
    torch.testing.assert_close(a.sum(1).cpu(), torch.ones(C.N_OMIC), rtol=1e-4, atol=1e-4)
    params = dict(mod.named_parameters())
    tensors = [qd, bd] + [params[k[len("co_attention."):]] for k in p]
    gs = torch.autograd.grad((out * p_out.to(dev)).sum() + 1e3 * (a * p_a.to(dev)).sum(), tensors)
    for (n, _), gr in zip(named, gs):
        assert relerr(gr, g_o[n]) < 3e-3, (n, relerr(gr, g_o[n]))


@pytest.mark.parametrize("n_q", [1, 6, 8])
@pytest.mark.parametrize("gate", [0.0, 4.0 / 3.0])
def test_two_wave_backward_equals_the_general_kernel(dev, n_q, gate):
    """K1's backward bag pass for a bf16 bag at embed 256 / <= 8 queries runs on csrc/coattn_bwd8.hip (two waves per SIMD,
    operands in LDS, both MFMA orientations in one pass, 16-byte dH stores); every other geometry on the general kernel.  Same
    mathematics: on a ragged window whose bags straddle every tile / workgroup edge the two must agree to the rounding both
    share -- the dH product takes its Z^T = [dctx | qk] operand as ONE bf16 term in both (2^-9 per term; the two-wave kernel
    rounds Z x gate, the general one Z), and d_bag is emitted in bf16 -- and to fp32 summation order elsewhere; with the
    patch layer's ReLU/dropout gate fused (zeros of the bag switch the gradient off, column sums = bias gradient) and
    without.  (Each kernel is held to the oracle separately by test_coattn_forward_backward and the model tests.)"""
    from multimodal_path_omic_amd import _lib as L
    from multimodal_path_omic_amd import ops
    lengths = [1, 31, 32, 33, 255, 700, 3000, 5000]
    g = syn.rng(77 + n_q)
    sd = syn.fill_state_dict(C.MCAT_COATTN_SHAPES, 78)
    p = {k[len("co_attention."):]: v.to(dev) for k, v in sd.items()}
    bags = [torch.relu(syn.normal(g, (m, C.E))).to(dev).to(torch.bfloat16) for m in lengths]
    query = syn.normal(g, (len(lengths) * n_q, C.E)).to(dev)
    probe = syn.normal(g, (len(lengths) * n_q, C.E)).to(dev)
    from multimodal_path_omic_amd.dp import FlatGradBucket
    bias = torch.nn.Parameter(torch.zeros(C.E, device=dev))           # stands in for the patch layer's bias (colsum receiver)
    bucket = FlatGradBucket([bias])                                   # the kernel writes the column sums into its slice

    def run(two_wave):
        prev = L.lib().mpo_set_coattn_bwd_two_wave(int(two_wave))
        try:
            batch = BagBatch.from_list(bags)
            data = batch.data.detach().requires_grad_(True)
            bucket.begin()
            bucket.flat.fill_(float("nan"))
            if gate:
                data._mpo_bias_param = bias
            q = query.clone().requires_grad_(True)
            w = {k: v.clone().requires_grad_(True) for k, v in p.items()}
            out, _ = ops.coattn_mcat(q, batch.with_data(data), w["in_proj_weight"], w["in_proj_bias"], w["out_proj.weight"],
                                     w["out_proj.bias"], False, gate)
            (out * probe).sum().backward()
            cs = bucket.flat[:C.E].clone() if gate else None
            return data.grad.float(), q.grad, {k: v.grad for k, v in w.items()}, cs
        finally:
            L.lib().mpo_set_coattn_bwd_two_wave(prev)
    db8, dq8, dw8, cs8 = run(True)
    db1, dq1, dw1, cs1 = run(False)
    scale = float(db1.abs().max())
    assert float((db8 - db1).abs().max()) < 1e-2 * scale
    assert float((db8 - db1).abs().mean()) < 5e-3 * float(db1.abs().mean())
    if gate:
        zero = torch.cat(bags).float() == 0
        assert float(db8[zero].abs().max()) == 0.0                    # the gate switches the gradient off where H = 0
        assert relerr(cs8, cs1) < 2e-2                               # (sums of thousands of signed bf16 values that differ in the last place)
        assert relerr(cs8, db8.sum(0)) < 1e-4                        # column sums of the rows it wrote
    assert relerr(dq8, dq1) < 1e-4
    for k in dw1:
        if dw1[k] is not None:
            assert relerr(dw8[k], dw1[k]) < 1e-4 or float(dw1[k].abs().max()) < 1e-12, k


@pytest.mark.parametrize("n_q", [1, 6, 8])
def test_fp32_bag_vector_backward_equals_the_general_kernel_and_fp64(dev, n_q):
    """K1 backward of an fp32 bag on the vector ALUs (csrc/coattn_bwd_f32.hip, plain fp32) against the general matrix-pipe kernel
    (three-term split) on a ragged window -- one-row slides, rows around every tile / step boundary, several tiles per wave --
    and both against a torch fp64 restatement of the folded co-attention (models/mcat/mcat.py:97): the vector kernel must
    be at least as close."""
    from multimodal_path_omic_amd import _lib as L
    from multimodal_path_omic_amd import ops
    lengths = [1, 15, 16, 17, 31, 32, 33, 255, 700, 3000, 5000]
    g = syn.rng(177 + n_q)
    sd = syn.fill_state_dict(C.MCAT_COATTN_SHAPES, 178)
    p = {k[len("co_attention."):]: v.to(dev) for k, v in sd.items()}
    bags = [syn.normal(g, (m, C.E)).to(dev) for m in lengths]
    query = syn.normal(g, (len(lengths) * n_q, C.E)).to(dev)
    probe = syn.normal(g, (len(lengths) * n_q, C.E)).to(dev)

    def run(vector):
        prev = L.lib().mpo_set_coattn_bwd_f32_vector(int(vector))
        try:
            batch = BagBatch.from_list(bags)
            data = batch.data.detach().requires_grad_(True)
            q = query.clone().requires_grad_(True)
            w = {k: v.clone().requires_grad_(True) for k, v in p.items()}
            out, _ = ops.coattn_mcat(q, batch.with_data(data), w["in_proj_weight"], w["in_proj_bias"], w["out_proj.weight"],
                                     w["out_proj.bias"], False, 0.0)
            (out * probe).sum().backward()
            return data.grad, q.grad, {k: v.grad for k, v in w.items()}
        finally:
            L.lib().mpo_set_coattn_bwd_f32_vector(prev)
    dbv, dqv, dwv = run(True)
    dbm, dqm, dwm = run(False)
    # fp64 restatement
    e = C.E
    w64 = {k: v.double().cpu().requires_grad_(True) for k, v in p.items()}
    q64 = query.double().cpu().requires_grad_(True)
    b64 = [b.double().cpu().requires_grad_(True) for b in bags]
    wq, wk, wv = w64["in_proj_weight"][:e], w64["in_proj_weight"][e:2 * e], w64["in_proj_weight"][2 * e:]
    bq, bk, bv = w64["in_proj_bias"][:e], w64["in_proj_bias"][e:2 * e], w64["in_proj_bias"][2 * e:]
    outs = []
    for i, hb in enumerate(b64):
        qq = q64[i * n_q:(i + 1) * n_q] @ wq.T + bq
        a = torch.softmax(qq @ (hb @ wk.T + bk).T / math.sqrt(e), dim=-1)
        outs.append((a @ (hb @ wv.T + bv)) @ w64["out_proj.weight"].T + w64["out_proj.bias"])
    (torch.cat(outs) * probe.double().cpu()).sum().backward()
    db64 = torch.cat([b.grad for b in b64])
    ev, em = relerr(dbv, db64), relerr(dbm, db64)
    print(f"[K1 fp32 backward] n_q={n_q}: d_bag vs fp64: vector {ev:.2e}, matrix pipe {em:.2e}; query {relerr(dqv, q64.grad):.2e}")
    assert ev < 2e-5 and ev <= em * 1.5 + 1e-6, (ev, em)
    assert relerr(dqv, q64.grad) < 2e-5
    for k in dwv:
        assert relerr(dwv[k], w64[k].grad) < 5e-5, k
    assert relerr(dbv, dbm) < 1e-4 and relerr(dqv, dqm) < 1e-4


@pytest.mark.parametrize("n_q", [1, 6, 8])
def test_fp32_bag_vector_backward_with_a_gradient_on_the_map(dev, n_q):
    """The `cesar` loss puts a gradient on the co-attention map (models/loss.py:88-101).  For an fp32 bag the vector-ALU backward
    takes it too (r04: the map's gradient enters on the folded registers, a step's 16 rows x 8 queries fetched as two coalesced
    loads and broadcast along the lane rows; the general kernel -- 1 KB of scratch per lane in this geometry -- keeps 9..16
    queries): against the general kernel and a torch fp64 restatement on a ragged window with full and ragged 16-row steps."""
    from multimodal_path_omic_amd import _lib as L
    from multimodal_path_omic_amd import ops
    lengths = [1, 15, 16, 17, 33, 255, 700, 3000, 5000]
    g = syn.rng(277 + n_q)
    sd = syn.fill_state_dict(C.MCAT_COATTN_SHAPES, 278)
    p = {k[len("co_attention."):]: v.to(dev) for k, v in sd.items()}
    bags = [syn.normal(g, (m, C.E)).to(dev) for m in lengths]
    query = syn.normal(g, (len(lengths) * n_q, C.E)).to(dev)
    probe = syn.normal(g, (len(lengths) * n_q, C.E)).to(dev)
    probe_map = [syn.normal(g, (n_q, m)).to(dev) for m in lengths]

    def run(vector):
        prev = L.lib().mpo_set_coattn_bwd_f32_vector(int(vector))
        try:
            batch = BagBatch.from_list(bags)
            data = batch.data.detach().requires_grad_(True)
            q = query.clone().requires_grad_(True)
            w = {k: v.clone().requires_grad_(True) for k, v in p.items()}
            out, amap = ops.coattn_mcat(q, batch.with_data(data), w["in_proj_weight"], w["in_proj_bias"], w["out_proj.weight"],
                                        w["out_proj.bias"], True, 0.0)
            maps = batch.split_map(amap, n_q)
            loss = (out * probe).sum()
            for a, pm in zip(maps, probe_map):
                loss = loss + (a * pm).sum()
            loss.backward()
            return data.grad, q.grad, {k: v.grad for k, v in w.items()}
        finally:
            L.lib().mpo_set_coattn_bwd_f32_vector(prev)
    dbv, dqv, dwv = run(True)
    dbm, dqm, dwm = run(False)
    e = C.E
    w64 = {k: v.double().cpu().requires_grad_(True) for k, v in p.items()}
    q64 = query.double().cpu().requires_grad_(True)
    b64 = [b.double().cpu().requires_grad_(True) for b in bags]
    wq, wk, wv = w64["in_proj_weight"][:e], w64["in_proj_weight"][e:2 * e], w64["in_proj_weight"][2 * e:]
    bq, bk, bv = w64["in_proj_bias"][:e], w64["in_proj_bias"][e:2 * e], w64["in_proj_bias"][2 * e:]
    loss = 0.0
    for i, hb in enumerate(b64):
        qq = q64[i * n_q:(i + 1) * n_q] @ wq.T + bq
        a = torch.softmax(qq @ (hb @ wk.T + bk).T / math.sqrt(e), dim=-1)
        o = (a @ (hb @ wv.T + bv)) @ w64["out_proj.weight"].T + w64["out_proj.bias"]
        loss = loss + (o * probe[i * n_q:(i + 1) * n_q].double().cpu()).sum() + (a * probe_map[i].double().cpu()).sum()
    loss.backward()
    db64 = torch.cat([b.grad for b in b64])
    ev, em = relerr(dbv, db64), relerr(dbm, db64)
    print(f"[K1 fp32 backward, map gradient] n_q={n_q}: d_bag vs fp64: vector {ev:.2e}, matrix pipe {em:.2e}; query {relerr(dqv, q64.grad):.2e}")
    assert ev < 2e-5 and ev <= em * 1.5 + 1e-6, (ev, em)
    assert relerr(dqv, q64.grad) < 2e-5
    for k in dwv:
        assert relerr(dwv[k], w64[k].grad) < 5e-5, k
    assert relerr(dbv, dbm) < 1e-4 and relerr(dqv, dqm) < 1e-4
