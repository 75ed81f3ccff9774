"""The flat optimisers' gradient guard on the device (csrc/grad_guard.hip through ops.grad_norm_flat /
ops.optim_step_flat_guarded / dp.FlatOptimizer(max_grad_norm=, skip_nonfinite=)): the norm against fp64 and its
determinism, non-finite detection at every path's edge, clipping as the composition "unguarded pass on coef * g", coef == 1
bit for bit, what is clipped (the L1 term yes, weight decay no) with three controls that must miss, the skipped step, and
both inside a captured window step.  u = 2^-24 throughout."""
import numpy as np
import pytest
import torch

import cases as C
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import harness, ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.dp import FlatGradBucket, FlatOptimizer
from multimodal_path_omic_amd.models import MultimodalCoAttentionTransformer, NarrowContextualAttentionGateTransformer

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
N_NORM = 1024 * 256 * 4 + 4 * 1000 + 3      # past one trip of the norm's fixed grid, and a 3-element scalar tail
N = 2048 * 256 * 4 + 4 * 1000 + 3           # past one trip of the optimiser's grid (test_gpu_flat_optim.py's N)
SMALL = [1, 3, 4, 5, 1027]
ALGS = ["adam", "adamax", "adadelta", "sgd"]


def f32(v):
    return float(np.float32(v))


LR = {"adam": f32(1e-3), "adamax": f32(2e-3), "adadelta": f32(1.0), "sgd": f32(1e-3)}


def _grads(n, dev, seed, steps):
    """test_gpu_flat_optim.py's gradients: 1e-6 .. 1e2 in magnitude, exact zeros, some elements zero at every step."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    never = torch.rand(n, device=dev, generator=gen) < 0.1
    out = []
    for _ in range(steps):
        mag = 10.0 ** (torch.rand(n, device=dev, generator=gen) * 8.0 - 6.0)
        sign = torch.where(torch.rand(n, device=dev, generator=gen) < 0.5, -1.0, 1.0)
        zero = never | (torch.rand(n, device=dev, generator=gen) < 0.1)
        out.append(torch.where(zero, torch.zeros_like(mag), sign * mag).float())
    return out


def _params(n, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    p = (torch.randn(n, device=dev, generator=gen) * 0.05).float()
    p[::97] = 0.0                                         # sign(0) = 0
    return p


def _bucket(dev, seed, n):
    p = torch.nn.Parameter(_params(n, dev, seed))
    return FlatGradBucket([p]), p


def _unaligned(t):
    """The same values in a view one element into a buffer: 4-byte but not 16-byte aligned, the all-scalar path."""
    raw = torch.zeros(t.numel() + 1, device=t.device, dtype=t.dtype)
    raw[1:].copy_(t)
    assert raw[1:].data_ptr() % 16 == 4
    return raw[1:]


def _ctl(dev):
    return torch.zeros(4, dtype=torch.int32, device=dev)


def _read(ctl):
    """(norm, coef, nonfinite, skipped) of a control block, on the host."""
    f = ctl.view(torch.float32)
    return float(f[0]), float(f[1]), int(ctl[2]), int(ctl[3])


def _norm64(g, p=None, l1=0.0):
    gp = g if not l1 else g + l1 * torch.sign(p)          # fp32, one rounding: what the optimiser applies
    return float(torch.linalg.vector_norm(gp.double()))


def _coef_ref(norm64, c):
    return f32(min(1.0, c / (norm64 + 1e-6)))


# ------------------------------------------------------------------------------------------------------------- 1. the norm
@pytest.mark.parametrize("n", SMALL + [N_NORM, N, "unaligned"])
def test_norm_matches_fp64_and_repeats_bit_for_bit(dev, n):
    """fp64 accumulation and one rounding to fp32 behind the square root: 4u relative."""
    unaligned = n == "unaligned"
    n = 1027 if unaligned else n
    g, p = _grads(n, dev, 100 + n % 89, 1)[0], _params(n, dev, 7)
    if n == 1:
        g.fill_(0.37)                                     # (the one element is not one of the exact zeros)
    if unaligned:
        g, p = _unaligned(g), _unaligned(p)
    l1 = f32(1e-3)
    for lam, pp in ((0.0, None), (l1, p)):
        ctl = _ctl(dev)
        ops.grad_norm_flat(g, ctl, pp, lam)
        norm, coef, bad, skipped = _read(ctl)
        ref = _norm64(g, p, lam)
        print(f"[grad norm n={n} unaligned={unaligned} l1={lam:g}] {norm:.9e} ref {ref:.9e} rel {abs(norm - ref) / max(ref, 1e-300):.2e}")
        assert abs(norm - ref) <= 4 * U * ref
        assert (coef, bad, skipped) == (1.0, 0, 0)
        again = _ctl(dev)
        ops.grad_norm_flat(g, again, pp, lam)
        assert torch.equal(again, ctl)
    if n > 1:
        assert _norm64(g, p, l1) != _norm64(g)            # the L1 term is in the reference it was held to


@pytest.mark.parametrize("n", [5, N_NORM])
def test_norm_of_a_finite_3e38_is_finite(dev, n):
    """3e38 squared overflows fp32, not fp64: the element is finite and so is the norm."""
    g = _grads(n, dev, 31, 1)[0]
    g[n // 2] = 3e38
    ctl = _ctl(dev)
    ops.grad_norm_flat(g, ctl, None, 0.0, max_norm=1e30, skip_nonfinite=True)
    norm, coef, bad, skipped = _read(ctl)
    ref = _norm64(g)
    assert ref >= 3e38 * (1 - U) and np.isfinite(norm) and abs(norm - ref) <= 4 * U * ref
    assert (bad, skipped) == (0, 0) and abs(coef - 1e30 / ref) <= 2 * U * 1e30 / ref


# ------------------------------------------------------------------------------------------------ 2. non-finite detection
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_one_nonfinite_element_is_seen_wherever_it_lies(dev, value):
    base = _grads(N_NORM, dev, 41, 1)[0]
    small = _unaligned(base[:1027])
    t = torch.full((1,), 5, dtype=torch.int32, device=dev)
    cases = [(base, 0), (base, N_NORM - 1), (base, 1024 * 256 * 4 + 5), (small, 0), (small, 1026)]
    for k, (g, at) in enumerate(cases):
        g = g.clone() if g is base else g
        ctl = _ctl(dev)
        ops.grad_norm_flat(g, ctl, None, 0.0, max_norm=1.0)
        assert _read(ctl)[2:] == (0, 0)
        keep = float(g[at])
        g[at] = value
        ops.grad_norm_flat(g, ctl, None, 0.0, max_norm=1.0, skip_nonfinite=True, step_dev=t)
        assert _read(ctl)[2:] == (1, 1), (value, at)
        assert int(t) == 5 - (k + 1)                      # the count the caller had advanced is taken back
        ops.grad_norm_flat(g, ctl, None, 0.0, max_norm=1.0, skip_nonfinite=False, step_dev=t)
        assert _read(ctl)[2:] == (1, 1) and int(t) == 5 - (k + 1)        # measured, not skipped: nothing counted
        g[at] = keep
        ops.grad_norm_flat(g, ctl, None, 0.0, max_norm=1.0, skip_nonfinite=True, step_dev=t)
        assert _read(ctl)[2:] == (0, 1)                   # the flag is the last gradient's, the count runs on


# ----------------------------------------------------------------------------------------------- 3. clipping by composition
def _optimisers(dev, alg, n, seed, wd, l1=0.0, **guard):
    kw = dict(lr=LR[alg], weight_decay=wd, l1_lambda=l1)
    ba, _ = _bucket(dev, seed, n)
    bb, _ = _bucket(dev, seed, n)
    return ba, FlatOptimizer(ba, alg, **kw, **guard), bb, FlatOptimizer(bb, alg, **kw)


def _assert_state(a, b, exact):
    for x, y in zip([a.flat_p, *a._moments()], [b.flat_p, *b._moments()]):
        if exact:
            assert torch.equal(x, y)
        else:
            torch.testing.assert_close(x, y, rtol=1e-6, atol=1e-9)
    assert int(a.t_dev) == int(b.t_dev)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("alg", ALGS)
def test_clipped_step_is_the_unguarded_step_on_the_scaled_gradient(dev, alg, wd):
    """FlatOptimizer(max_grad_norm=c) fed g against the unguarded optimiser fed g * coef_ref, coef_ref from the fp64 norm."""
    c = 100.0
    ba, guarded, bb, plain = _optimisers(dev, alg, N, 300, f32(wd), max_grad_norm=c)
    coefs = []
    for i, g in enumerate(_grads(N, dev, 301, 5)):
        g = g * (2.0 ** -10 if i % 2 else 1.0)            # every other gradient lies inside the ball
        coefs.append(_coef_ref(_norm64(g), c))
        ba.flat[:N].copy_(g)
        bb.flat[:N].copy_(g * coefs[-1])
        guarded.step()
        plain.step()
        assert abs(float(guarded.clip_coef) - coefs[-1]) <= 2 * U * coefs[-1]
    assert min(coefs) < 1.0 and max(coefs) == 1.0, coefs     # precondition: both sides of the clip were taken
    _assert_state(guarded, plain, exact=False)
    assert int(guarded.skipped_steps) == 0


@pytest.mark.parametrize("n", SMALL + ["unaligned"])
def test_guarded_entry_at_the_small_and_unaligned_sizes(dev, n):
    """ops.optim_step_flat_guarded on buffers of 1 .. 1027 elements and on views one element into theirs: coef == 1 gives the
    unguarded entry's bits, a clipped step its result on coef_ref * g."""
    unaligned = n == "unaligned"
    n = 1027 if unaligned else n
    wrap = _unaligned if unaligned else (lambda t: t.clone())
    for alg in ALGS:
        for c in (None, 1e-3):
            g = torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(n))
            coef = 1.0 if c is None else _coef_ref(_norm64(g), c)
            assert (coef < 1.0) == (c is not None)
            a = [wrap(_params(n, dev, 9)), wrap(g), wrap(torch.zeros(n, device=dev)), wrap(torch.zeros(n, device=dev))]
            b = [wrap(_params(n, dev, 9)), wrap(g * coef), wrap(torch.zeros(n, device=dev)), wrap(torch.zeros(n, device=dev))]
            ctl = _ctl(dev)
            kw = dict(lr=LR[alg], weight_decay=f32(1e-2))
            for _ in range(3):
                ops.grad_norm_flat(a[1], ctl, None, 0.0, c, True)
                ops.optim_step_flat_guarded(alg, *a, ctl, skip_nonfinite=True, **kw)
                ops.optim_step_flat(alg, *b, **kw)
            for x, y in zip(a[:1] + a[2:], b[:1] + b[2:]):
                if c is None:
                    assert torch.equal(x, y), (alg, n)
                else:
                    torch.testing.assert_close(x, y, rtol=1e-6, atol=1e-9)


# ------------------------------------------------------------------------------------------------------ 4. clip off is free
@pytest.mark.parametrize("alg", ALGS)
def test_a_guard_that_never_bites_changes_no_bit(dev, alg):
    """coef == 1 and no non-finite element: the guarded pass is the unguarded one bit for bit (weight decay and the L1 fold
    on, so that every term of g' is in play)."""
    l1 = f32(1e-4)
    ba, guarded, bb, plain = _optimisers(dev, alg, N, 400, f32(1e-2), l1, max_grad_norm=1e30, skip_nonfinite=True)
    for g in _grads(N, dev, 401, 5):
        ba.flat[:N].copy_(g)
        bb.flat[:N].copy_(g)
        guarded.step(l1_slides=2)
        plain.step(l1_slides=2)
    assert float(guarded.clip_coef) == 1.0 and int(guarded.skipped_steps) == 0
    _assert_state(guarded, plain, exact=True)


# ------------------------------------------------------------------------------------------------------ 5. what is clipped
def test_l1_term_is_clipped_and_weight_decay_is_not(dev):
    """SGD, one step: dp = -lr (coef (g + l1 sign p) + wd p) in fp64, per element within 8u |dp| + u |p| (eight roundings of a
    linear expression: coef, g', the product, the sum with wd p, the product with lr, the difference and its share of p).
    Controls that must each miss that bar 100-fold somewhere: the L1 term left out of the norm, weight decay clipped as
    well, norm and coefficient over g alone."""
    n, lr, wd, l1, c = 4099, f32(0.1), f32(0.1), f32(0.5), f32(5.0)
    bucket, p = _bucket(dev, 500, n)
    opt = FlatOptimizer(bucket, "sgd", lr=lr, weight_decay=wd, l1_lambda=l1, max_grad_norm=c)
    g = torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(501))
    bucket.flat[:n].copy_(g)
    p0 = opt.flat_p[:n].double().clone()
    opt.step(l1_slides=1)
    moved = opt.flat_p[:n].double() - p0
    gd, s = g.double(), torch.sign(p0)
    norm_full = float(torch.linalg.vector_norm(gd + l1 * s))
    norm_g = float(torch.linalg.vector_norm(gd))
    coef, coef_g = c / (norm_full + 1e-6), c / (norm_g + 1e-6)
    assert coef < 0.1 and abs(float(opt.last_grad_norm) - norm_full) <= 4 * U * norm_full
    ref = -lr * (coef * (gd + l1 * s) + wd * p0)
    bar = 8 * U * ref.abs() + U * p0.abs()
    worst = float(((moved - ref).abs() / bar.clamp_min(1e-300)).max())
    print(f"[grad guard sgd] coef {coef:.6f}: max |dp - ref| / bar {worst:.3f}")
    assert bool(((moved - ref).abs() <= bar).all())
    controls = {"l1 left out of the norm": -lr * (coef_g * (gd + l1 * s) + wd * p0),
                "weight decay clipped too": -lr * coef * (gd + l1 * s + wd * p0),
                "g alone measured and scaled": -lr * (coef_g * gd + l1 * s + wd * p0)}
    for name, wrong in controls.items():
        miss = float(((moved - wrong).abs() / bar.clamp_min(1e-300)).max())
        print(f"[grad guard sgd] control '{name}': err/bar {miss:.3e}")
        assert miss > 100, name
    assert float(opt.flat_p[n:].abs().max()) == 0.0       # the padding stays zero


# ------------------------------------------------------------------------------------------------------------------ 6. skip
@pytest.mark.parametrize("alg", ALGS)
def test_poisoned_step_is_skipped_and_leaves_no_trace(dev, alg):
    g1, g2, g3 = _grads(N, dev, 601, 3)
    g2[N - 1] = float("nan")
    (ba, _), (bb, _) = _bucket(dev, 600, N), _bucket(dev, 600, N)
    a = FlatOptimizer(ba, alg, lr=LR[alg], weight_decay=f32(1e-2), skip_nonfinite=True)
    b = FlatOptimizer(bb, alg, lr=LR[alg], weight_decay=f32(1e-2), skip_nonfinite=True)     # sees the finite gradients only
    ba.flat[:N].copy_(g1)
    a.step()
    before = [t.clone() for t in (a.flat_p, *a._moments(), a.t_dev)]
    ba.flat[:N].copy_(g2)
    a.step()
    for t, k in zip((a.flat_p, *a._moments(), a.t_dev), before):
        assert torch.equal(t, k)
    assert int(a.skipped_steps) == 1 and int(a.t_dev) == 1
    ba.flat[:N].copy_(g3)
    a.step()
    for g in (g1, g3):
        bb.flat[:N].copy_(g)
        b.step()
    _assert_state(a, b, exact=True)
    assert int(a.t_dev) == 2 and int(a.skipped_steps) == 1 and int(b.skipped_steps) == 0
    if alg == "adam":                                      # the guard is opt-in
        bc, _ = _bucket(dev, 600, N)
        plain = FlatOptimizer(bc, alg, lr=LR[alg], weight_decay=f32(1e-2))
        bc.flat[:N].copy_(g2)
        plain.step()
        assert bool(torch.isnan(plain.flat_p[N - 1])) and plain.grad_ctl is None


# ------------------------------------------------------------------------------------------------------ 7. inside the graph
def _window_setup(dev, kind, c):
    sizes = [64] * 6
    cls = MultimodalCoAttentionTransformer if kind == "mcat" else NarrowContextualAttentionGateTransformer
    model = cls(omic_sizes=sizes, bag_dtype=torch.bfloat16)
    model.load_state_dict(syn.fill_state_dict(C.model_shapes(sizes, kind == "nacagat"), 55))
    model.to(dev).eval()                                   # no masks to align between the twin and the graph
    window = harness.make_window(syn.make_cohort(3, 40, 70, sizes, 56), dev, torch.bfloat16)
    bucket = FlatGradBucket(list(model.parameters()))
    opt = FlatOptimizer(bucket, "adam", lr=1e-3, max_grad_norm=c, skip_nonfinite=True)
    return model, bucket, opt, window


@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_guard_inside_a_captured_window_step(dev, kind):
    ops.set_rng_epoch(None)
    c = 0.5
    model_e, bucket_e, opt_e, window_e = _window_setup(dev, kind, c)
    twin = []
    for _ in range(3):
        bucket_e.begin()
        harness.train_window(model_e, *window_e, 3)
        bucket_e.finish()
        opt_e.step()
        twin.append(opt_e.flat_p.clone())
    ops.set_rng_epoch(None)
    model, bucket, opt, window = _window_setup(dev, kind, c)
    step = harness.GraphedWindowStep(model, bucket, window, 3, opt=opt)
    assert int(opt.skipped_steps) == 0 and int(opt.t_dev) == 0       # warm-up and priming put both back
    step()
    step()
    print(f"[grad guard graph {kind}] norm {float(opt.last_grad_norm):.4e} coef {float(opt.clip_coef):.4e}")
    torch.testing.assert_close(opt.flat_p, twin[1], rtol=1e-6, atol=1e-9)
    before = [t.clone() for t in (opt.flat_p, *opt._moments(), opt.t_dev)]
    omic = window[1][0]
    keep = omic[0, 0].clone()
    omic[0, 0] = float("nan")                              # in place: the graph reads this tensor
    step()
    for t, k in zip((opt.flat_p, *opt._moments(), opt.t_dev), before):
        assert torch.equal(t, k)
    assert int(opt.skipped_steps) == 1 and int(opt.t_dev) == 2
    omic[0, 0] = keep
    step()
    torch.testing.assert_close(opt.flat_p, twin[2], rtol=1e-6, atol=1e-9)
    assert int(opt.t_dev) == 3 and int(opt.skipped_steps) == 1 and int(opt_e.skipped_steps) == 0
    ops.set_rng_epoch(None)


# ------------------------------------------------------------------------------------------------------ 8. entry refusals
def test_entries_refuse_bad_arguments_and_launch_nothing(dev):
    lib = L.lib()
    x = torch.ones(64, device=dev)
    ctl = _ctl(dev)
    ws = torch.zeros(256, dtype=torch.uint8, device=dev)
    need = lib.mpo_grad_norm_flat_workspace_bytes(64)
    s = L.stream_of(x)
    assert lib.mpo_grad_norm_flat(L.ptr(x), None, 64, 0.0, 1.0, 1, None, None, L.ptr(ws), need, s) != 0
    assert b"ctl" in lib.mpo_last_error()
    assert lib.mpo_grad_norm_flat(L.ptr(x), None, 64, 0.0, 1.0, 1, None, L.ptr(ctl), L.ptr(ws), need - 1, s) != 0
    assert b"workspace" in lib.mpo_last_error()
    step = (64, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 0.0, 1, None)
    assert lib.mpo_optim_step_flat_guarded(7, L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), *step, L.ptr(ctl), 1, s) != 0
    assert b"algorithm" in lib.mpo_last_error()
    assert lib.mpo_optim_step_flat_guarded(0, L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), *step, None, 1, s) != 0
    assert b"ctl" in lib.mpo_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, torch.ones_like(x)) and int(ctl.abs().sum()) == 0 and int(ws.sum()) == 0
