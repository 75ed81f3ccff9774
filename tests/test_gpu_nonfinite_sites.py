"""Non-finite propagation, site by site: a NaN, a +Inf and a -Inf planted in one element of a feature, activation, parameter
or upstream-gradient tensor, at the first unit, the last unit and a unit of a partial tile (tests/nonfinite_cases.py), against
the fp64 restatement of the same operation on the same stored inputs.

  1. nothing is swallowed: where the oracle is non-finite the kernel's unit is (hazards, survs, Y, loss, risk: element by
     element); a parameter whose oracle gradient holds a non-finite element has one here (tensor level)
  2. nothing leaks: a unit without a plant whose oracle output is finite is finite here, within the bar the site's own test
     file holds it to (imported from that file), and -- forward outputs, which have no cross-unit state -- bit-equal to the
     run without a plant
  3. finite where the oracle is finite: a planted unit that the plant leaves finite in the oracle (a -inf logit is a weight
     of 0, relu(-inf + b) is 0) is finite here and within the same bar

Sites: the three linear entries on every GEMM body with every epilogue activation, the bf16 patch epilogue and patch layer, MCAT
co-attention (bf16 / fp32 bags, n_q 6 and 8, with and without a gradient on the map), NaCAGaT on every key route, bag
self-attention in both arithmetics, encoder, gated pool with rho (fused, short, long), omic SNN, CAG, survival head, `ces`,
`sct`, the fused head + loss, the gene-expression head, the three fusion heads in three forms, and the map-block entries.

Sites run at p = 0; the pool and the SNN add one training-mode rate (0.25, masks replayed), where the kernels select
(keep ? v * s : 0) and torch multiplies: a dropped element of a NaN unit is 0 here and NaN there, the unit is non-finite in both.

Each case prints its findings before it asserts that there are none."""
import pytest
import torch
import torch.nn as nn

import nonfinite_cases as N
import selfattn_helpers as SH
import tail_helpers as H
import test_gpu_bag_selfattn as SA
import test_gpu_coattn_mcat as K1
import test_gpu_coattn_nacagat as K2
import test_gpu_fusion_next as FN
import test_gpu_ge_train as GE
import test_gpu_gemm_routes as RT
import test_gpu_patch_epilogue as PE
import test_gpu_tail_edges as TE
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import ops
from multimodal_path_omic_amd.fusion import ConcatFusion
from multimodal_path_omic_amd.ops import BagBatch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _rng_calls_put_back():
    calls = ops._rng_calls
    yield
    ops._rng_calls = calls


# ---------------------------------------------------------------------------------------------------------------- bars
def rel_to_max(tol, floor=1e-30):
    """max |got - ref| / max |ref| (tail_helpers.relerr, test_gpu_gemm_routes._err) against tol"""
    return lambda g, r: (float((g - r).abs().max() / r.abs().max().clamp_min(floor)), tol)


def grad_to_max(tol):
    """tail_helpers.grad_errs' measure: the scale is at least 1e-5"""
    return rel_to_max(tol, 1e-5)


def absolute(tol):
    return lambda g, r: (float((g - r).abs().max()), tol)


def close(rtol, atol):
    """torch.testing.assert_close's rule as (excess over rtol |ref|, atol)"""
    return lambda g, r: (float(((g - r).abs() - rtol * r.abs()).max()), atol if atol > 0 else 1e-300)


# ---------------------------------------------------------------------------------------------------------------- runners
def run_linear(dev, site, inp):
    R, I, O = site.R, site.I, site.O
    x, w, b, dy = (inp[k].to(dev).contiguous() for k in ("x", "w", "b", "dy"))
    y, dx, dw, db = torch.empty(R, O, device=dev), torch.empty(R, I, device=dev), torch.empty(O, I, device=dev), torch.empty(O, device=dev)
    s, lib = L.stream_of(x), L.lib()
    routes = []
    L.call("mpo_linear_forward", L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), R, I, O, 1.0, L.ACT[site.act], s)
    routes.append(lib.mpo_gemm_last_route())
    L.call("mpo_linear_backward_input", L.ptr(dy), L.ptr(w), L.ptr(dx), R, I, O, 1.0, 0, s)
    routes.append(lib.mpo_gemm_last_route())
    L.call("mpo_linear_backward_weight", L.ptr(dy), L.ptr(x), L.ptr(dw), L.ptr(db), R, I, O, 1.0, s)
    routes.append(lib.mpo_gemm_last_route())
    assert routes == [L.GEMM_ROUTE[r] for r in site.bodies], (routes, site.bodies)
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, b))
    g = torch.autograd.grad((ops.linear(xa, wa, ba, site.act) * dy).sum(), [xa, wa, ba])
    return N.Result(dict(act=y), dict(dx=g[0], dx_raw=dx), dict(dw=g[1], db=g[2], dw_raw=dw, db_raw=db))


def bars_linear(site, inp):
    tol_w = RT.TOL_LONG_K if site.R >= 2048 else RT.TOL
    return dict(act=rel_to_max(RT.TOL), dx=rel_to_max(RT.TOL), dx_raw=rel_to_max(RT.TOL), dw=rel_to_max(tol_w), db=rel_to_max(tol_w),
                dw_raw=rel_to_max(tol_w), db_raw=rel_to_max(tol_w))


def run_epilogue(dev, site, inp):
    h, dy = inp["h"].to(dev).bfloat16().contiguous(), inp["dy"].to(dev).bfloat16().contiguous()
    b = inp["b"].to(dev)
    PE._epilogue(h, b, 0.0)
    g, db = torch.empty_like(dy), torch.full((site.cols,), 7.0, device=dev)
    PE._epilogue_backward(h, dy, g, 0.0, db)
    return N.Result(dict(act=h.float()), dict(g=g.float()), dict(db=db))


def bars_epilogue(site, inp):
    # test_gpu_patch_epilogue.py holds the p = 0 epilogue to bit-equality with fp32 torch, which has no bar to import: against
    # fp64 that is one rounding to bf16 (8 significant bits: within 2^-8 relative); the bit comparison with the clean run is made
    # beside it.  Column sums: that file's COLSUM_REL of sum |g|
    ulp = lambda g, r: (float(((g - r).abs() / r.abs().clamp_min(1e-30)).max()), 2.0 ** -8)                  # noqa: E731
    scale = ((inp["h"] + inp["b"] > 0) * inp["dy"].abs()).double().sum(0)
    return dict(act=ulp, g=ulp, db=lambda g, r: (float(((g - r).abs() / scale.clamp_min(1e-30)).max()), PE.COLSUM_REL))


def run_head(dev, site, inp):
    lg = inp["logits"].to(dev).requires_grad_(True)
    hz, sv, y = ops.survival_head(lg)
    out = dict(hazards=hz, survs=sv, y=y)
    if site.form == "plain":
        scalar = sum((t * p.to(dev)).sum() for t, p in zip((hz, sv, y), inp["probes"]))
    else:
        if site.form == "ces":
            loss, risk = ops.ces_loss(hz, sv, inp["label"].to(dev), inp["cens"].to(dev))
        else:
            loss, risk = ops.sct_loss(y, inp["label"].to(dev), inp["cens"].to(dev)), -sv.sum(1)
        out.update(loss=loss, risk=risk)
        scalar = (loss * inp["w"].to(dev)).sum()
    scalar.backward()
    return N.Result(out, dict(dlogits=lg.grad), {})


def bars_head(site, inp):
    loss = TE.CES_LOSS if site.form == "ces" else TE.SCT_LOSS
    return dict(hazards=absolute(TE.HEAD_ABS), survs=absolute(TE.HEAD_ABS), y=absolute(TE.HEAD_ABS), loss=close(**loss),
                risk=close(**TE.RISK), dlogits=close(**TE.SCT_GRAD) if site.form == "sct" else grad_to_max(H.GRAD_TOL))


def run_loss(dev, site, inp):
    lab, cens, w = (inp[k].to(dev) for k in ("label", "cens", "w"))
    if site.kind == "ces":
        hz, sv = inp["hazards"].to(dev).requires_grad_(True), inp["survs"].to(dev).requires_grad_(True)
        loss, risk = ops.ces_loss(hz, sv, lab, cens)
        (loss * w).sum().backward()
        return N.Result(dict(loss=loss, risk=risk), dict(d_hazards=hz.grad, d_survs=sv.grad), {})
    y = inp["y"].to(dev).requires_grad_(True)
    loss = ops.sct_loss(y, lab, cens)
    (loss * w).sum().backward()
    return N.Result(dict(loss=loss), dict(d_y=y.grad), {})


def bars_loss(site, inp):
    if site.kind == "ces":
        return dict(loss=close(**TE.CES_LOSS), risk=close(**TE.RISK), d_hazards=close(**TE.CES_GRAD), d_survs=close(**TE.CES_GRAD))
    # d_Y = -w / (Y[y] + eps): no test holds d Y itself (test_sct_loss_edges holds d logits, behind the softmax).  It is one
    # fp32 sum of at most C terms and one division of O(1) values -- a few ulps of 6e-8 relative -- so the loss's own rule
    # (rtol 1e-5, atol 1e-6) is the bar set here, from the format's precision
    return dict(loss=close(**TE.SCT_LOSS), d_y=close(**TE.SCT_LOSS))


def run_fusion(dev, site, inp):
    sd = site.params(inp)
    h, label, cens, w = inp["h"], inp["label"], inp["cens"], inp["w"]
    probes = list(inp["probes"])
    b, d = site.b, site.d
    if site.fusion != "concat":
        entry = FN._run_entry if site.fusion == "gated_concat" else FN._run_bilinear_entry
        out, grads = entry(dev, sd, h, site.form, label, cens, probes, w, False)
        return N.Result(out, dict(d_h=torch.stack(grads[:2], 1)), dict(zip(sd, grads[2:])))
    fus = ConcatFusion(dims=[d, d], hidden_size=d, output_size=d)
    cls = nn.Linear(d, site.c)
    fus.load_state_dict({k: v for k, v in sd.items() if k.startswith("fusion_layer.")}, strict=True)
    cls.load_state_dict({k[len("classifier."):]: v for k, v in sd.items() if k.startswith("classifier.")}, strict=True)
    fus.to(dev), cls.to(dev)
    hcat = torch.cat([h[0], h[1]], 1).to(dev).requires_grad_(True)
    params = [dict(fus.named_parameters())[k] if k.startswith("fusion_layer.") else dict(cls.named_parameters())[k[len("classifier."):]]
              for k in sd]
    if site.form == "plain":
        hz, sv, y = ops.fusion_head_cat(hcat, fus, cls)
        out = dict(hazards=hz, survs=sv, y=y)
        grads = torch.autograd.grad(sum((t * p.to(dev)).sum() for t, p in zip((hz, sv, y), probes)), [hcat] + params)
    else:
        wd = w.to(dev)
        loss, risk, hz, sv, y = ops.fusion_head_loss_cat(hcat, fus, cls, label.to(dev), cens.to(dev), wd, loss=site.form)
        out = dict(hazards=hz, survs=sv, y=y, loss=loss, risk=risk)
        grads = torch.autograd.grad(loss, [hcat] + params, grad_outputs=wd)
    return N.Result(out, dict(d_h=grads[0].view(b, 2, d)), dict(zip(sd, grads[1:])))


def bars_fusion(site, inp):
    # test_gpu_fusion_next._compare: outputs 1e-4 absolute, loss and risk 1e-4 of max(|ref|, 1), gradients 2e-3 of max |ref|
    rel1 = lambda g, r: (float((g - r).abs().max()), FN.REL_TOL * max(float(r.abs().max()), 1.0))             # noqa: E731
    bars = dict(hazards=absolute(FN.OUT_ATOL), survs=absolute(FN.OUT_ATOL), y=absolute(FN.OUT_ATOL), loss=rel1, risk=rel1,
                d_h=grad_to_max(FN.GRAD_TOL))
    bars.update({k: grad_to_max(FN.GRAD_TOL) for k in site.params(inp)})
    return bars


def run_ge(dev, site, inp):
    h = inp["h"].to(dev).requires_grad_(True)
    cls = nn.Linear(site.d, site.c).to(dev)
    with torch.no_grad():
        cls.weight.copy_(inp["weight"])
        cls.bias.copy_(inp["bias"])
    loss, y = ops.ge_head_loss(h, cls, inp["label"].to(dev))
    loss.backward(inp["w"].to(dev))
    return N.Result(dict(y=y, loss=loss), dict(d_h=h.grad), dict(weight=cls.weight.grad, bias=cls.bias.grad))


def bars_ge(site, inp):
    return dict(y=close(GE.LOSS_RTOL, 1e-6), loss=close(GE.LOSS_RTOL, 1e-6), d_h=absolute(GE.GRAD_ATOL), weight=absolute(GE.GRAD_ATOL),
                bias=absolute(GE.GRAD_ATOL))


def _branch_names(sds):
    return [f"br{br}.{k}" for br, sd in enumerate(sds) for k in sd]


def run_pool(dev, site, inp):
    sc, h, dx, grads = H._pool_gpu(dev, inp["_sds"], inp["_heads"], inp["_rhos"], inp["x"], inp["ph"], inp["pa"], False, site.p > 0)
    n = site.nb * site.ns
    return N.Result(dict(scores=sc.reshape(n, -1), h=h.reshape(n, -1)), dict(dx=dx.reshape(n, -1)), dict(zip(_branch_names(inp["_sds"]), grads)))


def bars_pool(site, inp):
    bars = dict(scores=rel_to_max(H.FWD_TOL), h=rel_to_max(H.FWD_TOL), dx=grad_to_max(H.GRAD_TOL))
    bars.update({k: grad_to_max(H.GRAD_TOL) for k in _branch_names(inp["_sds"])})
    return bars


def run_encoder(dev, site, inp):
    y, dx, grads = H._encoder_gpu(dev, inp["_sds"], inp["_encs"], inp["x"], inp["probe"], training=False)
    n = site.nb * site.ns
    return N.Result(dict(tokens=y.reshape(n, -1)), dict(dx=dx.reshape(n, -1)), dict(zip(_branch_names(inp["_sds"]), grads)))


def bars_encoder(site, inp):
    bars = dict(tokens=rel_to_max(H.FWD_TOL), dx=grad_to_max(H.GRAD_TOL))
    bars.update({k: grad_to_max(H.GRAD_TOL) for k in _branch_names(inp["_sds"])})
    return bars


def run_snn(dev, site, inp):
    y, grads = H._snn_gpu(dev, inp["_G"], [inp[f"x{i}"] for i in range(len(H.SNN_SIZES))], inp["probe"])
    return N.Result(dict(g_bag=y.reshape(site.ns, -1)), {}, dict(zip([k for k, _ in inp["_G"].named_parameters()], grads)))


def bars_snn(site, inp):
    bars = dict(g_bag=rel_to_max(H.FWD_TOL))
    bars.update({k: grad_to_max(H.GRAD_TOL) for k, _ in inp["_G"].named_parameters()})
    return bars


def run_cag(dev, site, inp):
    q, qh = inp["q"].to(dev).requires_grad_(True), inp["q_hat"].to(dev).requires_grad_(True)
    mod = inp["_mod"]
    out = ops.contextual_gate(q, qh, mod)
    params = dict(mod.named_parameters())
    grads = torch.autograd.grad((out * inp["probe"].to(dev)).sum(), [q, qh] + [params[n] for n in site.NAMES])
    return N.Result(dict(out=out), dict(d_q=grads[0], d_q_hat=grads[1]), dict(zip(site.NAMES, grads[2:])))


def bars_cag(site, inp):
    bars = dict(out=rel_to_max(TE.CAG_FWD), d_q=rel_to_max(TE.CAG_GRAD), d_q_hat=rel_to_max(TE.CAG_GRAD))
    bars.update({k: rel_to_max(TE.CAG_GRAD) for k in site.NAMES})
    return bars


def run_coattn(dev, site, inp):
    n_q, E = site.n_q, site.E
    data = inp["bag"].to(site.dtype).to(dev).requires_grad_(True)
    leaves = [inp[k].to(dev).requires_grad_(True) for k in ("query", "in_w", "in_b", "out_w", "out_b")]
    batch = BagBatch.from_lengths(data, N.BAG_LENGTHS)
    p_out, p_q, p_map = (inp[k].to(dev) for k in ("p_out", "p_q", "p_map"))
    fused = ops.k2_fused_patch_grad
    try:
        ops.k2_fused_patch_grad = site.fused
        if site.kind == "mcat":
            out, amap = ops.coattn_mcat(leaves[0], batch, *leaves[1:], True)
            res, scalar = dict(out=out), (out * p_out).sum()
        else:
            want = {"key_projection": "kernel", "gemm": "gemm_" + str(site.dtype)[6:9].replace("flo", "f32").replace("bfl", "bf16"),
                    "split_halves": "halves"}[site.route.replace("_unfused_finish", "").replace("_bf16", "").replace("_f32", "")]
            assert ops._key_route(site.dtype, E, 0.0) == want, (site.route, ops._key_route(site.dtype, E, 0.0))
            q_proj, out, amap = ops.coattn_nacagat(leaves[0], batch, *leaves[1:], 0.0)
            res, scalar = dict(out=out, q_proj=q_proj), (out * p_out).sum() + (q_proj * p_q).sum()
        if site.map_grad:
            scalar = scalar + (amap * p_map).sum()
        g = torch.autograd.grad(scalar, [data] + leaves)
    finally:
        ops.k2_fused_patch_grad = fused
    ns = len(N.BAG_LENGTHS)
    res = {k: v.reshape(ns, -1) for k, v in res.items()}
    res["map"] = N.pad_maps(amap.detach().cpu(), N.BAG_LENGTHS, n_q)
    return N.Result(res, dict(d_query=g[1].reshape(ns, -1), d_bag=N.pad_slides(g[0].float().cpu(), N.BAG_LENGTHS, E)),
                    dict(zip(("in_w", "in_b", "out_w", "out_b"), g[2:])))


def bars_coattn(site, inp):
    """The bars of test_gpu_coattn_mcat.check_coattn_forward_backward and test_gpu_coattn_nacagat.check_nacagat_forward_backward,
    by their names there: the output against its largest entry, the map element by element and relative, gradients against
    their largest entry (a bf16 bag's own bars)."""
    bf16 = site.dtype == torch.bfloat16
    own = K1 if site.kind == "mcat" else K2
    rel_each = lambda g, r: (float(((g - r).abs() / r.abs().clamp_min(1e-30)).max()), own.MAP_REL_TOL)       # noqa: E731
    if site.kind == "mcat":
        grad, bag = K1.GRAD_TOL, (K1.BAG_GRAD_TOL_BF16 if bf16 else K1.GRAD_TOL)
        bars = dict(out=rel_to_max(K1.OUT_TOL), map=rel_each)
    else:
        grad, bag = (K2.GRAD_TOL_BF16_PARAM, K2.GRAD_TOL_BF16_BAG) if bf16 else (K2.GRAD_TOL, K2.GRAD_TOL)
        bars = dict(out=rel_to_max(K2.OUT_TOL), q_proj=rel_to_max(K2.OUT_TOL), map=rel_each)
    bars.update(d_query=rel_to_max(grad), d_bag=rel_to_max(bag), in_w=rel_to_max(grad), in_b=rel_to_max(grad), out_w=rel_to_max(grad),
                out_b=rel_to_max(grad))
    return bars


def run_selfattn(dev, site, inp):
    with SH.bf16x3(site.mode):
        x = inp["qkv"].to(dev).requires_grad_(True)
        out, amap = ops.BagSelfAttentionFn.apply(x, site.heads, 0.0, True)
        (out * inp["probe"].to(dev)).sum().backward()
    return N.Result(dict(out=out.reshape(site.n, -1), map=amap), dict(d_qkv=x.grad.reshape(site.n, -1)), {})


def bars_selfattn(site, inp):
    """test_gpu_bag_selfattn.test_attention_core_equals_torch: the bars of the arithmetic in use (selfattn_helpers._b3_modes), dq /
    dk / dv each against its own scale (part_scale); the map 1e-3 element by element where the reference is above 1e-30."""
    out_bar, grad_bar = next((o, g) for hook, o, g in SH._b3_modes(site.d, site.heads) if hook == site.mode)
    d = site.d

    def parts(g, r):
        g, r = g.reshape(-1, site.m, 3 * d), r.reshape(-1, site.m, 3 * d)
        return max(SH.relmax(g[..., sl], r[..., sl], SH.part_scale(r)(sl)) for sl in (slice(i * d, (i + 1) * d) for i in range(3))), grad_bar

    def each(g, r):
        big = r > 1e-30
        return float(((g - r).abs() / r.clamp_min(1e-30))[big].max()), SA.MAP_REL_TOL
    return dict(out=rel_to_max(out_bar), d_qkv=parts, map=each)


RUN = {N.LinearSite: (run_linear, bars_linear), N.EpilogueSite: (run_epilogue, bars_epilogue), N.HeadSite: (run_head, bars_head),
       N.LossSite: (run_loss, bars_loss), N.FusionSite: (run_fusion, bars_fusion), N.GeHeadSite: (run_ge, bars_ge),
       N.PoolSite: (run_pool, bars_pool), N.EncoderSite: (run_encoder, bars_encoder), N.SnnSite: (run_snn, bars_snn),
       N.CagSite: (run_cag, bars_cag), N.CoattnSite: (run_coattn, bars_coattn),
       N.SelfAttnSite: (run_selfattn, bars_selfattn)}
ON_DEVICE = (N.PoolSite, N.EncoderSite, N.SnnSite, N.CagSite)               # make(dev): their modules live on the device


def _bits(t):
    return t.detach().float().contiguous().view(torch.int32).cpu()


@pytest.mark.parametrize("name", list(N.SITES))
def test_site_propagates_planted_values_as_the_oracle_does(dev, name):
    site = N.SITES[name]
    run, bars_of = RUN[type(site)]
    inp = site.make(dev) if isinstance(site, ON_DEVICE) else site.make()
    clean = run(dev, site, inp)
    torch.cuda.synchronize(dev)
    found = [("clean", f) for f in N.clean_units_hold(clean, site.oracle(inp), [], bars_of(site, inp))]
    clean_bits = {k: _bits(v) for k, v in clean.out.items()}
    n_held = 0
    for row in N.rows_of(site):
        index, units = N.where(site, inp, row)
        pin = N.planted(inp, row.tensor, index, row.plant)
        ref = site.oracle(pin)
        got = run(dev, site, pin)
        torch.cuda.synchronize(dev)
        found += [(tuple(row[1:]), f) for f in N.covers(got, ref) + N.clean_units_hold(got, ref, units, bars_of(site, pin))]
        ok = N.clean_units(ref, units)
        n_held += int(ok.sum())
        for k, v in got.out.items():                      # forward outputs of clean units: no cross-unit state, the same bits
            b = _bits(v).reshape(ok.shape[0], -1)[ok]
            if not torch.equal(b, clean_bits[k].reshape(ok.shape[0], -1)[ok]):
                found.append((tuple(row[1:]), f"out {k}: a clean unit differs in bits from the run without a plant"))
    print(f"[non-finite] {name}: {len(N.rows_of(site))} plants, {n_held} clean units held, {len(found)} findings")
    for f in found[:40]:
        print("   ", f)
    assert not found, found[:8]


# ---------------------------------------------------------------------------------------------------------------- map blocks
def _maps(n_q, seed):
    g = torch.Generator().manual_seed(seed)
    n = n_q * sum(N.MAP_LENGTHS)
    return torch.randn(n, generator=g), torch.randn(n, generator=g)


def _batch(dev):
    rows = sum(N.MAP_LENGTHS)
    return BagBatch.from_lengths(torch.zeros(rows, 1, device=dev), N.MAP_LENGTHS)


@pytest.mark.parametrize("n_q", N.MAP_NQ)
def test_map_block_dot_and_scale_match_fp64(dev, n_q):
    """mpo_map_block_dot and mpo_map_block_scale on finite data, lengths one below, at and one above the 256-thread trip:
    every (slide, query) dot product within the fp32 worst-case bound of a sum of M_b products, computed from the data; the
    scaled map is one fp32 product per element: bit-equal to fp32 torch."""
    a, b = _maps(n_q, 9100 + n_q)
    batch = _batch(dev)
    ad, bd = a.to(dev), b.to(dev)
    out = torch.full((batch.n_slides * n_q,), float("nan"), device=dev)
    L.call("mpo_map_block_dot", L.ptr(ad), L.ptr(bd), L.ptr(batch.cu), batch.n_slides, n_q, L.ptr(out), L.stream_of(ad))
    dots, mags = N.map_block_fp64(a, b, N.MAP_LENGTHS, n_q)
    got = out.view(batch.n_slides, n_q).double().cpu()
    for i, m in enumerate(N.MAP_LENGTHS):
        err, bound = (got[i] - dots[i]).abs(), N.fp32_dot_bound(m, mags[i])
        print(f"[map blocks] n_q={n_q} M={m}: dot error {float(err.max()):.2e}, bound {float(bound.min()):.2e}")
        assert bool((err <= bound).all()), (m, err, bound)
    scale = torch.randn(batch.n_slides, generator=torch.Generator().manual_seed(5))
    scaled = torch.full_like(ad, float("nan"))
    L.call("mpo_map_block_scale", L.ptr(ad), L.ptr(scale.to(dev)), L.ptr(batch.cu), batch.n_slides, n_q, L.ptr(scaled), L.stream_of(ad))
    per_element = torch.cat([scale[i].expand(n_q * m) for i, m in enumerate(N.MAP_LENGTHS)])
    assert torch.equal(scaled.cpu(), per_element * a)


@pytest.mark.parametrize("plant", list(N.PLANTS))
@pytest.mark.parametrize("n_q", N.MAP_NQ)
def test_map_block_norm_keeps_a_planted_value_in_its_slide(dev, n_q, plant):
    """ops.map_block_norm with one element of one slide's block non-finite (first, last and the 257-row slide): that slide's
    norm and its block of the gradient are non-finite, as in fp64 torch; every other slide's norm is bit-equal to the clean
    run's and its gradient block finite and bit-equal."""
    a, _ = _maps(n_q, 9200 + n_q)
    batch = _batch(dev)
    probe = torch.rand(batch.n_slides, generator=torch.Generator().manual_seed(6)) + 0.5
    starts = [n_q * sum(N.MAP_LENGTHS[:i]) for i in range(len(N.MAP_LENGTHS) + 1)]

    def run(flat):
        fd = flat.to(dev).requires_grad_(True)
        norm = ops.MapBlockNormFn.apply(fd, batch, n_q)
        (norm * probe.to(dev)).sum().backward()
        return norm.detach().cpu(), fd.grad.cpu()

    def oracle(flat):
        f64 = flat.double().requires_grad_(True)
        norm = torch.stack([f64[starts[i]:starts[i + 1]].pow(2).sum().sqrt() for i in range(batch.n_slides)])
        (norm * probe.double()).sum().backward()
        return norm.detach(), f64.grad

    norm0, grad0 = run(a)
    for slide in (0, 3, len(N.MAP_LENGTHS) - 1):
        flat = a.clone()
        flat[starts[slide + 1] - 1] = N.PLANTS[plant]                         # the last element of the slide's last query row
        norm, grad = run(flat)
        norm_o, grad_o = oracle(flat)
        for i in range(batch.n_slides):
            blk = slice(starts[i], starts[i + 1])
            if i == slide:
                assert not bool(torch.isfinite(norm_o[i])) and not bool(torch.isfinite(norm[i])), (slide, norm[i])
                assert not bool(torch.isfinite(grad_o[blk]).all()) and not bool(torch.isfinite(grad[blk]).all()), slide
            else:
                assert bool(torch.isfinite(norm_o[i])) and torch.equal(norm[i], norm0[i]), (slide, i)
                assert torch.equal(grad[blk], grad0[blk]) and bool(torch.isfinite(grad[blk]).all()), (slide, i)


# ---------------------------------------------------------------------------------------------------------------- patch layer
@pytest.mark.parametrize("plant", list(N.PLANTS))
def test_patch_fc_bf16_keeps_a_planted_feature_in_its_row(dev, plant):
    """mpo_patch_fc_forward (bf16 window, 129 rows: one row past the 128-row tile) with one feature of the first row, of the
    tile's last row and of the lone row behind it non-finite: where the fp64 restatement on the same bf16 values has a
    non-finite row the kernel's row holds one (its deliberate superset -- the whole row -- is allowed); every other row is
    finite and bit-equal to the run without a plant."""
    from multimodal_path_omic_amd import synthetic as syn
    from oracle import mpo_oracle as O
    rows, g = 129, syn.rng(9300)
    x = syn.normal(g, (rows, 1024)).bfloat16()
    w, b = syn.normal(g, (256, 1024), 1 / 32), syn.normal(g, (256,), 0.1)
    wd, bd = w.to(dev), b.to(dev)
    with torch.no_grad():
        clean = ops.patch_fc(x.to(dev), wd, bd, 0.0)
        assert clean.dtype == torch.bfloat16 and bool(torch.isfinite(clean.float()).all())
        for r in (0, 127, 128):
            x2 = x.clone()
            x2[r, 100] = N.PLANTS[plant]
            h = ops.patch_fc(x2.to(dev), wd, bd, 0.0).float().cpu()
            ref = O.patch_fc(x2.double(), {"H.0.weight": w.double(), "H.0.bias": b.double()}, storage=torch.bfloat16, round_gemm_out=False)
            swallowed = N.unit_nonfinite(ref) & ~N.unit_nonfinite(h)
            assert not bool(swallowed.any()), (r, swallowed.nonzero().flatten().tolist())
            assert bool(N.unit_nonfinite(ref)[r]) or plant != "nan"
            others = torch.ones(rows, dtype=torch.bool)
            others[r] = False
            assert bool(torch.isfinite(h[others]).all()), r
            assert torch.equal(h[others], clean.float().cpu()[others]), r


# ---------------------------------------------------------------------------------------------------------------- bag self-attention
@pytest.mark.parametrize("plant", list(N.PLANTS))
@pytest.mark.parametrize("store", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("m", [33, 40])
def test_bag_self_attention_with_its_projections_on_both_storage_types(dev, m, store, plant):
    """ops.bag_self_attention (in projection, attention core, out projection) on three bags of m rows stored in bf16 or fp32,
    one element of a bag's first or last row non-finite, against O.bag_self_attention in fp64 on the stored values: where a
    query row of the oracle's output or map is non-finite the bag's is; the other bags are finite, within the bars of
    tests/test_gpu_bag_selfattn.py (the arithmetic's output bar, the map's MAP_REL_TOL) and bit-equal to the run without
    the plant."""
    from multimodal_path_omic_amd import synthetic as syn
    from oracle import mpo_oracle as O
    d, n, g = 256, 3, syn.rng(9500 + m)
    x = syn.normal(g, (n, m, d)).to(store)
    sd = syn.fill_state_dict({"self_attention.in_proj_weight": (3 * d, d), "self_attention.in_proj_bias": (3 * d,),
                              "self_attention.out_proj.weight": (d, d), "self_attention.out_proj.bias": (d,)}, 9501)
    mha = nn.MultiheadAttention(d, 1)
    mha.load_state_dict({k[len("self_attention."):]: v for k, v in sd.items()}, strict=True)
    mha.to(dev).eval()
    p = {k: v.double() for k, v in sd.items()}
    out_bar = max(o for _, o, _ in SH._b3_modes(d, 1))
    with torch.no_grad():
        out0, map0 = ops.bag_self_attention(x.to(dev), mha, training=False)
        for bag, row in ((0, 0), (1, m - 1), (n - 1, m - 1)):
            x2 = x.clone()
            x2[bag, row, 7] = N.PLANTS[plant]
            out, amap = ops.bag_self_attention(x2.to(dev), mha, training=False)
            for b in range(n):
                o_r, a_r = O.bag_self_attention(x2[b].double(), p)
                o, a = out[b].double().cpu(), amap[b].double().cpu()
                for name, got, ref in (("out", o, o_r), ("map", a, a_r)):
                    swallowed = ~torch.isfinite(ref).all(1) & torch.isfinite(got).all(1)
                    assert not bool(swallowed.any()), (name, bag, b, swallowed.nonzero().flatten().tolist()[:6])
                if b == bag:
                    assert not bool(torch.isfinite(o_r).all()) or plant != "nan"
                    continue
                assert bool(torch.isfinite(o_r).all()) and bool(torch.isfinite(o).all()) and bool(torch.isfinite(a).all()), (bag, b)
                assert SH.relmax(o, o_r) < out_bar, (bag, b, SH.relmax(o, o_r))
                big = a_r > 1e-30
                assert float(((a - a_r).abs() / a_r.clamp_min(1e-30))[big].max()) < SA.MAP_REL_TOL, (bag, b)
                assert torch.equal(out[b], out0[b]) and torch.equal(amap[b], map0[b]), (bag, b)
