"""Drivers of the token tail's two composite entries -- the set-Transformer encoder and the gated pooling head -- shared by
tests/test_gpu_train_dropout.py and tests/test_gpu_tail_edges.py.  Plain module (not a conftest).

Two ways to the same kernels:
  * the `ops` path (`_encoder_gpu`, `_pool_gpu`): autograd Functions, torch-allocated buffers;
  * the guarded path (`encoder_guarded`, `pool_guarded`): the C ABI through `L.call` on buffers the test owns -- input,
    output, `saved`, dx, every gradient and the workspace, each sized exactly by the entry's own size query, each between
    two runs of 64 NaN floats, outputs starting as NaN.  Afterwards every guard run must still be NaN and every output
    finite: a size query or carve that is short at an odd geometry shows here before any comparison.

Both are compared with oracle/mpo_oracle.py in fp64 (`_encoder_oracle`, `_pool_oracle`), in training mode under the masks
tests/dropout_replay.py rebuilds from (SEED, OFF).  Bars: forward 1e-4 of the reference's largest entry, dx and every parameter
gradient 2e-3 of that tensor's largest entry.  Every check takes the rate(s) of its sites (`p`; the pooling helpers `p_head`
and `p_rho` separately), P = 0.25 by default; the omic SNN's check lives here too (`_snn_check`)."""
import numpy as np
import torch
import torch.nn as nn

import cases as C
import dropout_replay as R
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.blocks import AttentionNetGated
from multimodal_path_omic_amd.transformer import make_set_transformer
from oracle import mpo_oracle as O

P = 0.25
SEED = 20261016
OFF = 4321
FF, HEADS, LAYERS = 512, 8, 2
FWD_TOL, GRAD_TOL = 1e-4, 2e-3
GUARD = 64                       # floats of NaN before and after every guarded buffer (256 bytes: 16-byte alignment is kept)


def relerr(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def grad_errs(got, ref):
    """max |got - ref| / max |ref| per tensor (check_grads' measure)."""
    out = []
    for g, r in zip(got, ref):
        scale = max(float(r.abs().max()), 1e-5)
        out.append(float((g.detach().double().cpu() - r).abs().max()) / scale)
    return out


def _pin():
    torch.manual_seed(SEED)
    ops._rng_calls = OFF
    assert torch.initial_seed() == SEED


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


class Guarded:
    """Device buffers between NaN runs.  buf(numel, fill, shift): `shift` floats of extra offset (a view one float into its
    storage is contiguous and not 16-byte aligned)."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def buf(self, numel, fill=None, shift=0):
        numel = int(numel)
        parent = torch.full((numel + 2 * GUARD + shift,), float("nan"), device=self.dev, dtype=torch.float32)
        view = parent[GUARD + shift:GUARD + shift + numel]
        if fill is not None:
            view.copy_(fill.reshape(-1))
        self.bufs.append((parent, GUARD + shift, numel))
        return view

    def check(self, what):
        torch.cuda.synchronize()
        for i, (parent, lo, numel) in enumerate(self.bufs):
            assert bool(torch.isnan(parent[:lo]).all()) and bool(torch.isnan(parent[lo + numel:]).all()), f"{what}: guard of buffer {i}"

    def all_nan(self, views):
        torch.cuda.synchronize()
        return all(bool(torch.isnan(v).all()) for v in views)


def _finite(what, **tensors):
    for name, t in tensors.items():
        for i, u in enumerate(t if isinstance(t, (list, tuple)) else [t]):
            assert bool(torch.isfinite(u).all()), f"{what}: {name}[{i}] has non-finite entries"


# ------------------------------------------------------------------------------------------- encoder
def _encoder_setup(dev, nb, ns, T, d, seed, ff=FF, heads=HEADS, training=True, p=P):
    sds, encs = [], []
    for br in range(nb):
        sd = syn.fill_state_dict(C.encoder_shapes("enc", d=d, ff=ff), seed + br)
        enc = make_set_transformer(d, p, nhead=heads, dim_feedforward=ff, num_layers=LAYERS)
        enc.load_state_dict({k[len("enc."):]: v for k, v in sd.items()}, strict=True)
        sds.append(sd)
        encs.append(enc.to(dev).train() if training else enc.to(dev).eval())
    g = syn.rng(seed + 50)
    x = syn.normal(g, (nb, ns, T, d))
    probe = syn.normal(g, (nb, ns, T, d))
    return sds, encs, x, probe


def _encoder_gpu(dev, sds, encs, x, probe, training=True):
    _pin()
    xd = x.to(dev).requires_grad_(True)
    y = ops.encoder_stacked(xd, [list(e.layers) for e in encs], training=training)
    params = [dict(e.named_parameters())[k[len("enc."):]] for e, sd in zip(encs, sds) for k in sd]
    grads = torch.autograd.grad((y * probe.to(dev)).sum(), [xd] + params)
    return y.detach().cpu(), grads[0].cpu(), [g.cpu() for g in grads[1:]]


def encoder_guarded(dev, sds, x, probe, ff=FF, heads=HEADS, training=True, unaligned=(), p=P):
    """mpo_encoder_forward + mpo_encoder_backward on guarded buffers; in training mode at rate p with (SEED, OFF) as the stream,
    which is what `_pin` gives the ops path.  unaligned: (branch, parameter name) pairs placed one float into their storage.
    -> (y, dx, [grads]) on the CPU, like _encoder_gpu."""
    lib = L.lib()
    nb, ns, T, d = x.shape
    bt = nb * ns
    G = Guarded(dev)
    xb = G.buf(x.numel(), x)
    params = [G.buf(v.numel(), v, shift=1 if (br, k) in unaligned else 0) for br, sd in enumerate(sds) for k, v in sd.items()]
    shapes = [tuple(v.shape) for sd in sds for v in sd.values()]
    y = G.buf(x.numel())
    saved = G.buf(lib.mpo_encoder_saved_floats(bt, T, d, ff, heads, LAYERS))
    p, seed, off = (p, SEED, OFF) if training else (0.0, 0, 0)
    pa = L.ptr_array(params)
    L.call("mpo_encoder_forward", L.ptr(xb), nb, ns, T, d, ff, heads, LAYERS, pa, float(p), seed, off, ops._epoch(), L.ptr(y),
           L.ptr(saved), L.stream_of(xb))
    dy = G.buf(x.numel(), probe)
    dx = G.buf(x.numel())
    grads = [G.buf(v.numel()) for v in params]
    ws_bytes = lib.mpo_encoder_workspace_bytes(bt, T, d, ff)
    ws = G.buf((ws_bytes + 3) // 4)
    ga = L.ptr_array(grads)
    L.call("mpo_encoder_backward", L.ptr(xb), nb, ns, T, d, ff, heads, LAYERS, pa, float(p), seed, off, ops._epoch(), L.ptr(saved),
           L.ptr(dy), L.ptr(dx), ga, L.ptr(ws), ws_bytes, L.stream_of(xb))
    G.check("encoder")
    _finite("encoder", y=y, dx=dx, grads=grads)
    return y.view(x.shape).cpu(), dx.view(x.shape).cpu(), [g.view(s).cpu() for g, s in zip(grads, shapes)]


def _encoder_oracle(sds, x, probe, keeps, heads=HEADS):
    """fp64 set_transformer per branch with that branch's masks (keeps = None: eval) -> y (nb, ns, T, d), dx, [param grads]
    (branch-major)."""
    ys, dxs, gs = [], [], []
    for br, sd in enumerate(sds):
        p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        xo = x[br].double().requires_grad_(True)
        kb = None if keeps is None else [tuple(None if k is None else _t(k[br]) for k in layer) for layer in keeps]
        yo = O.set_transformer(xo, p, "enc", LAYERS, heads, keeps=kb)
        (yo * probe[br].double()).sum().backward()
        ys.append(yo.detach())
        dxs.append(xo.grad)
        gs += [p[k].grad for k in sd]
    return torch.stack(ys), torch.stack(dxs), gs


def encoder_compare(tag, got, ref, sds):
    """Prints the worst figures of one run against the oracle, then asserts them at the bars.  -> (e_y, e_dx, worst gradient)"""
    (y, dx, grads), (yo, dxo, go) = got, ref
    e_y, e_dx = relerr(y, yo), grad_errs([dx], [dxo])[0]
    e_g = grad_errs(grads, go)
    names = [f"br{br}.{k}" for br, sd in enumerate(sds) for k in sd]
    worst = int(np.argmax(e_g))
    print(f"{tag}: y {e_y:.1e} dx {e_dx:.1e} grads max {e_g[worst]:.1e} ({names[worst]})")
    assert e_y < FWD_TOL, e_y
    assert e_dx < GRAD_TOL, e_dx
    for n, e in zip(names, e_g):
        assert e < GRAD_TOL, (n, e)
    return e_y, e_dx, e_g[worst]


def _encoder_check(dev, nb, ns, T, d, seed, epoch=0, ff=FF, heads=HEADS, training=True, p=P):
    """p: the rate of every dropout site of the encoder (the modules are built with it)."""
    sds, encs, x, probe = _encoder_setup(dev, nb, ns, T, d, seed, ff, heads, training, p)
    y, dx, grads = _encoder_gpu(dev, sds, encs, x, probe, training)
    keeps = R.encoder_keeps(SEED, OFF, nb, ns, T, d, ff, heads, LAYERS, p, epoch) if training else None
    ref = _encoder_oracle(sds, x, probe, keeps, heads)
    encoder_compare(f"encoder nb={nb} ns={ns} T={T} d={d} heads={heads} ff={ff} epoch={epoch} training={training} p={p}",
                    (y, dx, grads), ref, sds)
    return dict(sds=sds, x=x, probe=probe, y=y, keeps=keeps)


# ------------------------------------------------------------------------------------------- gated pool
def _pool_setup(dev, nb, ns, L_, d, seed, rho_bias=None, training=True, p_head=P, p_rho=P):
    """p_head: the scorer's two dropouts (AttentionNetGated.drop_p, hard-wired to 0.25 by the constructor and set here);
    p_rho: rho's nn.Dropout."""
    sds, heads, rhos = [], [], []
    for br in range(nb):
        sd = syn.fill_state_dict(C.pool_shapes("head", "rho", d=d), seed + br)
        if rho_bias is not None:
            sd["rho.0.bias"] = torch.full((d,), float(rho_bias))
        head = AttentionNetGated(n_classes=1, input_dim=d, hidden_dim=d)
        head.drop_p = float(p_head)
        rho = nn.Sequential(nn.Linear(d, d), nn.ReLU(), nn.Dropout(p_rho))
        head.load_state_dict({k[len("head."):]: v for k, v in sd.items() if k.startswith("head.")})
        rho.load_state_dict({k[len("rho."):]: v for k, v in sd.items() if k.startswith("rho.")})
        sds.append(sd)
        heads.append(head.to(dev).train() if training else head.to(dev).eval())
        rhos.append(rho.to(dev).train() if training else rho.to(dev).eval())
    g = syn.rng(seed + 50)
    x = syn.normal(g, (nb, ns, L_, d))
    probe_h = syn.normal(g, (nb, ns, d))
    probe_a = syn.normal(g, (nb, ns, L_))
    return sds, heads, rhos, x, probe_h, probe_a


def _pool_params(sd, head, rho):
    hp, rp = dict(head.named_parameters()), dict(rho.named_parameters())
    return [hp[k[len("head."):]] if k.startswith("head.") else rp[k[len("rho."):]] for k in sd]


def _pool_gpu(dev, sds, heads, rhos, x, probe_h, probe_a, interleave, training=True):
    nb, ns, L_, d = x.shape
    _pin()
    xd = x.to(dev).requires_grad_(True)
    sc, h = ops.gated_pool_stacked(xd, heads, rhos, training=training, interleave=interleave)
    h_std = h.view(ns, nb, d).transpose(0, 1) if interleave else h           # -> (nb, ns, d)
    loss = (h_std * probe_h.to(dev)).sum() + (sc[:, :, 0] * probe_a.to(dev)).sum()
    params = [q for sd, hd, rh in zip(sds, heads, rhos) for q in _pool_params(sd, hd, rh)]
    grads = torch.autograd.grad(loss, [xd] + params)
    return sc[:, :, 0].detach().cpu(), h_std.detach().cpu(), grads[0].cpu(), [g.cpu() for g in grads[1:]]


def pool_guarded(dev, sds, x, probe_h, probe_a, interleave, training=True, backward=True, p_head=P, p_rho=P):
    """mpo_gated_pool_forward (+ mpo_gated_pool_backward) on guarded buffers -> (scores, h (nb, ns, d), dx, [grads]) on the
    CPU like _pool_gpu; without `backward` dx and grads are None and the guarded set is returned for a refusal test:
    (scores, h, None, None, state)."""
    lib = L.lib()
    nb, ns, L_, d = x.shape
    bt = nb * ns
    G = Guarded(dev)
    xb = G.buf(x.numel(), x)
    params = [G.buf(v.numel(), v) for sd in sds for v in sd.values()]
    shapes = [tuple(v.shape) for sd in sds for v in sd.values()]
    scores = G.buf(bt * L_)
    h = G.buf(bt * d)
    saved = G.buf(lib.mpo_gated_pool_saved_floats(bt, L_, d))
    (p_head, p_rho), seed, off = ((p_head, p_rho), SEED, OFF) if training else ((0.0, 0.0), 0, 0)
    pa = L.ptr_array(params)
    L.call("mpo_gated_pool_forward", L.ptr(xb), nb, ns, L_, d, pa, float(p_head), float(p_rho), seed, off, ops._epoch(), L.ptr(scores),
           L.ptr(h), int(interleave), L.ptr(saved), L.stream_of(xb))
    h_std = (h.view(ns, nb, d).transpose(0, 1) if interleave else h.view(nb, ns, d))
    dh = G.buf(bt * d, probe_h.transpose(0, 1).contiguous() if interleave else probe_h)
    d_ext = G.buf(bt * L_, probe_a)
    dx = G.buf(x.numel())
    grads = [G.buf(v.numel()) for v in params]
    ws_bytes = lib.mpo_gated_pool_workspace_bytes(bt, L_, d)
    ws = G.buf((ws_bytes + 3) // 4)
    ga = L.ptr_array(grads)

    def run_backward():
        L.call("mpo_gated_pool_backward", L.ptr(xb), nb, ns, L_, d, pa, float(p_head), float(p_rho), L.ptr(saved), L.ptr(h), L.ptr(dh),
               int(interleave), L.ptr(d_ext), L.ptr(dx), ga, L.ptr(ws), ws_bytes, L.stream_of(xb))
    if not backward:
        G.check("gated pool forward")
        _finite("gated pool", scores=scores, h=h)
        return (scores.view(nb, ns, L_).cpu(), h_std.cpu(), None, None,
                dict(G=G, run_backward=run_backward, untouched=[dx, ws] + grads))
    run_backward()
    G.check("gated pool")
    _finite("gated pool", scores=scores, h=h, dx=dx, grads=grads)
    return scores.view(nb, ns, L_).cpu(), h_std.cpu(), dx.view(x.shape).cpu(), [g.view(s).cpu() for g, s in zip(grads, shapes)]


def _pool_oracle(sds, x, probe_h, probe_a, keeps):
    ka, kb, kr = keeps if keeps is not None else (None, None, None)
    nb, ns = x.shape[:2]
    scs, hs, dxs, gs = [], [], [], []
    for br, sd in enumerate(sds):
        p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        xo = x[br].double().requires_grad_(True)
        loss = 0
        sc_b, h_b = [], []
        for s in range(ns):
            a, h = O.gated_mil_pool(xo[s], p, "head", "rho", None if ka is None else _t(ka[br, s]),
                                    None if kb is None else _t(kb[br, s]), None if kr is None else _t(kr[br, s]))
            loss = loss + (h * probe_h[br, s].double()).sum() + (a[0] * probe_a[br, s].double()).sum()
            sc_b.append(a[0].detach())
            h_b.append(h.detach())
        loss.backward()
        scs.append(torch.stack(sc_b))
        hs.append(torch.stack(h_b))
        dxs.append(xo.grad)
        gs += [p[k].grad for k in sd]
    return torch.stack(scs), torch.stack(hs), torch.stack(dxs), gs


def pool_compare(tag, got, ref, sds, forward_only=False):
    """Prints the worst figures of one run against the oracle, then asserts them at the bars.
    -> (e_scores, e_h, e_dx, worst gradient)"""
    (sc, h, dx, grads), (sco, ho, dxo, go) = got, ref
    e_sc, e_h = relerr(sc, sco), relerr(h, ho)
    if forward_only:
        print(f"{tag}: scores {e_sc:.1e} h {e_h:.1e}")
        assert e_sc < FWD_TOL and e_h < FWD_TOL, (e_sc, e_h)
        return e_sc, e_h, None, None
    e_dx = grad_errs([dx], [dxo])[0]
    e_g = grad_errs(grads, go)
    names = [f"br{br}.{k}" for br, sd in enumerate(sds) for k in sd]
    worst = int(np.argmax(e_g))
    print(f"{tag}: scores {e_sc:.1e} h {e_h:.1e} dx {e_dx:.1e} grads max {e_g[worst]:.1e} ({names[worst]})")
    assert e_sc < FWD_TOL and e_h < FWD_TOL, (e_sc, e_h)
    assert e_dx < GRAD_TOL, e_dx
    for n, e in zip(names, e_g):
        assert e < GRAD_TOL, (n, e)
    return e_sc, e_h, e_dx, e_g[worst]


def _pool_check(dev, ns, L_, interleave, seed, epoch=0, nb=2, d=256, training=True, p_head=P, p_rho=P):
    sds, heads, rhos, x, ph, pa = _pool_setup(dev, nb, ns, L_, d, seed, training=training, p_head=p_head, p_rho=p_rho)
    sc, h, dx, grads = _pool_gpu(dev, sds, heads, rhos, x, ph, pa, interleave, training)
    keeps = R.pool_keeps(SEED, OFF, nb, ns, L_, d, p_head, p_rho, interleave, epoch) if training else None
    ref = _pool_oracle(sds, x, ph, pa, keeps)
    pool_compare(f"pool nb={nb} ns={ns} L={L_} d={d} interleave={interleave} epoch={epoch} training={training} p_head={p_head} p_rho={p_rho}",
                 (sc, h, dx, grads), ref, sds)
    return dict(sds=sds, x=x, ph=ph, pa=pa, sc=sc, h=h, keeps=keeps)


# ------------------------------------------------------------------------------------------- omic SNN
SNN_SIZES = [100, 31, 256, 8, 300, 64]          # ragged widths (test_gpu_tail.py's)


def _snn_setup(dev, ns, seed, p=P):
    torch.manual_seed(seed)
    G = nn.ModuleList([nn.Sequential(
        nn.Sequential(nn.Linear(s, C.E), nn.ELU(), nn.AlphaDropout(p=p, inplace=False)),
        nn.Sequential(nn.Linear(C.E, C.E), nn.ELU(), nn.AlphaDropout(p=p, inplace=False))) for s in SNN_SIZES]).to(dev)
    G.train()
    g = syn.rng(seed + 1)
    xs = [syn.normal(g, (ns, s)) for s in SNN_SIZES]
    probe = syn.normal(g, (ns, len(SNN_SIZES), C.E))
    return G, xs, probe


def _snn_gpu(dev, G, xs, probe):
    _pin()
    y = ops.omic_snn([x.to(dev) for x in xs], G, training=True)
    grads = torch.autograd.grad((y * probe.to(dev)).sum(), list(G.parameters()))
    return y.detach().cpu(), [g.cpu() for g in grads]


def _snn_oracle(G, xs, probe, keeps, p=P):
    prm = {"G." + k: v.detach().double().cpu().requires_grad_(True) for k, v in G.state_dict().items()}
    ns = xs[0].shape[0]
    ys = []
    for s in range(ns):
        ad = [(_t(k1[s]), _t(k2[s])) for k1, k2 in keeps]
        ys.append(O.omic_fc([x[s].double() for x in xs], prm, "G", ad_keeps=ad, drop_p=p))
    yo = torch.stack(ys)                                   # (ns, N, d)
    (yo * probe.double()).sum().backward()
    return yo.detach(), [prm["G." + k].grad for k, _ in G.named_parameters()]


def _snn_check(dev, ns, seed, epoch=0, p=P):
    G, xs, probe = _snn_setup(dev, ns, seed, p)
    y, grads = _snn_gpu(dev, G, xs, probe)
    keeps = R.snn_keeps(SEED, OFF, ns, len(SNN_SIZES), C.E, p, epoch)
    yo, go = _snn_oracle(G, xs, probe, keeps, p)
    e_y = relerr(y, yo)
    e_g = grad_errs(grads, go)
    names = [k for k, _ in G.named_parameters()]
    worst = int(np.argmax(e_g))
    print(f"omic SNN ns={ns} epoch={epoch} p={p}: y {e_y:.1e} grads max {e_g[worst]:.1e} ({names[worst]})")
    assert e_y < FWD_TOL, e_y
    for n, e in zip(names, e_g):
        assert e < GRAD_TOL, (n, e)
    return y, keeps
