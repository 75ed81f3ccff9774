"""The flat optimisers of the reference's training.optimizer choices (csrc/optim.hip optim_flat_kernel through
mpo_optim_step_flat / dp.FlatOptimizer) against fp64 torch.optim driven by the same gradient sequence: 20 steps of Adam,
Adamax, Adadelta and SGD with and without weight decay, gradients spanning 1e-6 .. 1e2 with exact zeros, a parameter count
past one grid of threads (2048 x 256 x 4 elements) and an odd tail.  Also: the learning rate read from a device scalar and
changed between calls, the L1 fold against autograd of the reference's l1_reg, the deterministic |p| sum, and controls that
must miss the bar (Adam in place of Adamax, Adadelta's eps outside the square root, the L1 term divided by grad_acc_step, a
frozen learning rate)."""
import numpy as np
import pytest
import torch

from multimodal_path_omic_amd import ops
from multimodal_path_omic_amd.dp import FlatExponentialLR, FlatGradBucket, FlatOptimizer

pytestmark = pytest.mark.gpu
STEPS = 20
U = 2.0 ** -24
N = 2048 * 256 * 4 + 4 * 1000 + 3         # past one grid of float4 threads, and a 3-element scalar tail


def f32(v):
    return float(np.float32(v))


LR = {"adam": f32(1e-3), "adamax": f32(2e-3), "adadelta": f32(1.0), "sgd": f32(1e-3)}
B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-8)
RHO, EPS_AD = f32(0.9), f32(1e-6)


def _grads(n, dev, seed, steps=STEPS):
    gen = torch.Generator(device=dev).manual_seed(seed)
    never = torch.rand(n, device=dev, generator=gen) < 0.1
    out = []
    for _ in range(steps):
        mag = 10.0 ** (torch.rand(n, device=dev, generator=gen) * 8.0 - 6.0)
        sign = torch.where(torch.rand(n, device=dev, generator=gen) < 0.5, -1.0, 1.0)
        zero = never | (torch.rand(n, device=dev, generator=gen) < 0.1)
        out.append(torch.where(zero, torch.zeros_like(mag), sign * mag).float())
    return out


def _torch_opt(alg, param, lr, wd):
    if alg == "adam":
        return torch.optim.Adam([param], lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
    if alg == "adamax":
        return torch.optim.Adamax([param], lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
    if alg == "adadelta":
        return torch.optim.Adadelta([param], lr=lr, rho=RHO, eps=EPS_AD, weight_decay=wd, foreach=False)
    return torch.optim.SGD([param], lr=lr, weight_decay=wd, foreach=False)


class _Reference:
    """fp64 torch.optim plus a running per-element bound on the drift of an fp32 evaluation of the same recurrences.

    g' = g + l1 sign(p) + wd p is off by E_g = 2u(|g| + l1 + wd|p|) + wd E_p (the terms may cancel).  Each state is a
    convex recurrence: its error decays with the recurrence's factor and gains (1 - factor) times the input's error plus a
    few roundings of the same recurrence on magnitudes (A for first moments, the state itself for positive ones).  The
    update q (what p moves by) is then off by its sensitivity to those errors plus 8 roundings of |q|; for Adam/Adamax fp32
    powf adds u / (1 - b1^t) (and u / (2(1 - b2^t)) for Adam's second moment).  E_p sums the update errors and one
    rounding of p per step.  The tests allow 2x these bounds: a few fp32 ulps of each quantity -- a wrong algorithm, eps
    placement, L1 scale or learning rate moves the update at the percent level."""

    def __init__(self, alg, p0, lr, wd, l1=0.0):
        self.alg, self.lr, self.wd, self.l1 = alg, lr, wd, l1
        self.param = torch.nn.Parameter(p0.double().clone())
        self.opt = _torch_opt(alg, self.param, lr, wd)
        z = torch.zeros_like(self.param.detach())
        self.A, self.e1, self.e2, self.e_p = z.clone(), z.clone(), z.clone(), z.clone()
        self.t = 0

    def set_lr(self, lr):
        self.lr = lr
        for g in self.opt.param_groups:
            g["lr"] = lr

    def step(self, g):
        self.t += 1
        t, lr, wd = self.t, self.lr, self.wd
        p_old = self.param.detach().clone()
        gd = g.double() + self.l1 * torch.sign(p_old)
        gp = gd + wd * p_old
        e_g = 2 * U * (g.double().abs() + self.l1 + wd * p_old.abs()) + wd * self.e_p
        st_old = {k: v.clone() for k, v in self.opt.state[self.param].items() if torch.is_tensor(v)} if self.t > 1 else {}
        self.param.grad = gd.clone()
        self.opt.step()
        st = self.opt.state[self.param]
        p_new = self.param.detach()
        q = (p_new - p_old).abs()
        if self.alg == "adam":
            m, v = st["exp_avg"], st["exp_avg_sq"]
            self.A = B1 * self.A + (1 - B1) * gp.abs()
            self.e1 = B1 * self.e1 + (1 - B1) * e_g + 3 * U * self.A
            self.e2 = B2 * self.e2 + (1 - B2) * (2 * gp.abs() + e_g) * e_g + 5 * U * v
            bc1, bc2s = 1 - B1 ** t, (1 - B2 ** t) ** 0.5
            denom = v.sqrt() / bc2s + EPS
            rel = 8 * U + U / bc1 + U / (2 * (1 - B2 ** t)) + self.e2 / (2 * v).clamp_min(1e-300)
            e_q = (lr / bc1) * self.e1 / denom + q * rel
        elif self.alg == "adamax":
            m, u_inf = st["exp_avg"], st["exp_inf"]
            self.A = B1 * self.A + (1 - B1) * gp.abs()
            self.e1 = B1 * self.e1 + (1 - B1) * e_g + 3 * U * self.A
            self.e2 = torch.maximum(B2 * self.e2 + 2 * U * u_inf, e_g + 2 * U * u_inf)
            bc1 = 1 - B1 ** t
            e_q = (lr / bc1) * (self.e1 + m.abs() * self.e2 / u_inf) / u_inf + q * (8 * U + U / bc1)
        elif self.alg == "adadelta":
            v, a = st["square_avg"], st["acc_delta"]
            a_old = st_old.get("acc_delta", torch.zeros_like(a))
            self.e1 = RHO * self.e1 + (1 - RHO) * (2 * gp.abs() + e_g) * e_g + 5 * U * v
            ratio = (a_old + EPS_AD).sqrt() / (v + EPS_AD).sqrt()
            rel_d = 8 * U + self.e2 / (2 * (a_old + EPS_AD)) + self.e1 / (2 * (v + EPS_AD))
            d = q / lr
            e_d = d * rel_d + ratio * e_g
            self.e2 = RHO * self.e2 + (1 - RHO) * (2 * d + e_d) * e_d + 5 * U * a
            e_q = lr * e_d + q * 2 * U
        else:
            e_q = lr * e_g + q * 2 * U
        self.e_p = self.e_p + e_q + U * p_new.abs()

    def check(self, p, what=""):
        p = p[:self.param.numel()]                      # the bucket pads to 64 elements; the padding stays zero
        err = (p.double() - self.param.detach()).abs()
        bar = 2 * self.e_p + 1e-30
        ratio = float((err / bar).max())
        if what:
            print(f"[flat optim {self.alg}{what}] step {self.t}: max |p - ref| {float(err.max()):.3e}, max err/bar {ratio:.3f}")
        return ratio


def _bucket(dev, seed, n=N):
    gen = torch.Generator(device=dev).manual_seed(seed)
    p = torch.nn.Parameter((torch.randn(n, device=dev, generator=gen) * 0.05).float())
    p.data[::97] = 0.0                                    # sign(0) = 0 in the L1 fold
    return FlatGradBucket([p]), p


def _run(dev, alg, wd, seed, l1=0.0, n=N, ctl=None):
    bucket, p = _bucket(dev, seed, n)
    ref = _Reference(alg if ctl != "adam_for_adamax" else "adam", p.detach().clone(), LR[alg], wd, l1)
    opt = FlatOptimizer(bucket, alg, lr=LR[alg], weight_decay=wd, l1_lambda=l1,
                        **({"betas": (B1, B2), "eps": EPS} if alg in ("adam", "adamax") else {}))
    worst = 0.0
    for i, g in enumerate(_grads(n, dev, seed + 1)):
        bucket.flat[:g.numel()].copy_(g)
        opt.step(**({"l1_slides": 1} if l1 else {}))
        ref.step(g)
        worst = max(worst, ref.check(opt.flat_p, f" wd={wd} l1={l1}" if i == STEPS - 1 else ""))
    return worst


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("alg", ["adam", "adamax", "adadelta", "sgd"])
def test_flat_optimiser_matches_fp64_torch_optim(dev, alg, wd):
    assert _run(dev, alg, f32(wd), 1000 + 10 * len(alg)) <= 1.0


def test_adam_algorithm_matches_mpo_adam_step_flat(dev):
    """algorithm 'adam' of the new pass is the arithmetic of mpo_adam_step_flat (FlatAdam); the two kernels may contract
    different products into FMAs, so they agree to a few ulps rather than bit for bit."""
    from multimodal_path_omic_amd.dp import FlatAdam
    b1, p1 = _bucket(dev, 7)
    b2, p2 = _bucket(dev, 7)
    a = FlatAdam(b1, lr=1e-3, weight_decay=1e-2)
    o = FlatOptimizer(b2, "adam", lr=1e-3, weight_decay=1e-2)
    for g in _grads(N, dev, 8, steps=5):
        b1.flat[:g.numel()].copy_(g)
        b2.flat[:g.numel()].copy_(g)
        a.step()
        o.step()
    d = float((a.flat_p - o.flat_p).abs().max())
    print(f"[flat optim adam vs FlatAdam] max |p diff| {d:.2e}")
    torch.testing.assert_close(o.flat_p, a.flat_p, rtol=1e-6, atol=1e-9)


def test_l1_fold_matches_autograd_of_l1_reg(dev):
    """g' = g + lambda * S * sign(p): S slides each adding lambda * l1_reg(model) to their loss (models/utils.py:33-40,
    models/mcat/main.py:69), gradient by autograd of the reference's expression."""
    n, slides, lam = 4099, 8, 1e-3
    bucket, p = _bucket(dev, 21, n)
    w = p.detach().double().clone().requires_grad_(True)
    total = sum(lam * torch.abs(w).sum() for _ in range(slides))
    (g_l1,) = torch.autograd.grad(total, [w])
    opt = FlatOptimizer(bucket, "sgd", lr=1.0, l1_lambda=lam)
    p0 = opt.flat_p.clone()
    bucket.flat.zero_()
    opt.step(l1_slides=slides)
    moved = (p0 - opt.flat_p)[:n].double()
    torch.testing.assert_close(moved, g_l1, rtol=4 * U, atol=U * float(p0.abs().max()) * 2)
    assert float(opt.flat_p[n:].abs().max()) == 0.0           # padding untouched by the fold (sign(0) = 0)
    # control: the term divided by grad_acc_step (as the data loss is) is 8x too small
    assert float((moved / slides - g_l1).abs().max()) > 100 * 4 * U * lam * slides


def test_l1_fold_trajectory_and_control_scaled_by_grad_acc_step(dev):
    lam = f32(1e-4)
    assert _run(dev, "adamax", f32(1e-2), 3100, l1=lam, n=300_007) <= 1.0
    # control: folding lambda / grad_acc_step (8) instead of lambda
    bucket, p = _bucket(dev, 3100, 300_007)
    ref = _Reference("adamax", p.detach().clone(), LR["adamax"], f32(1e-2), lam)
    opt = FlatOptimizer(bucket, "adamax", lr=LR["adamax"], weight_decay=f32(1e-2), l1_lambda=lam / 8,
                        betas=(B1, B2), eps=EPS)
    for g in _grads(300_007, dev, 3101):
        bucket.flat[:g.numel()].copy_(g)
        opt.step(l1_slides=1)
        ref.step(g)
    assert ref.check(opt.flat_p, " control l1/8") > 100


def test_control_adam_in_place_of_adamax_misses(dev):
    assert _run(dev, "adamax", 0.0, 4000, n=300_007, ctl="adam_for_adamax") > 100


def test_control_adadelta_eps_outside_sqrt_misses(dev):
    """d = sqrt(a)+eps over sqrt(v)+eps instead of sqrt(a+eps)/sqrt(v+eps): the fp64 restatement of the wrong form against
    the kernel."""
    n = 300_007
    bucket, p = _bucket(dev, 5000, n)
    opt = FlatOptimizer(bucket, "adadelta", lr=LR["adadelta"])
    pw = p.detach().double().clone()
    v, a = torch.zeros_like(pw), torch.zeros_like(pw)
    ref = _Reference("adadelta", p.detach().clone(), LR["adadelta"], 0.0)
    for g in _grads(n, dev, 5001):
        bucket.flat[:g.numel()].copy_(g)
        opt.step()
        ref.step(g)
        gd = g.double()
        v = RHO * v + (1 - RHO) * gd * gd
        d = (a.sqrt() + EPS_AD) / (v.sqrt() + EPS_AD) * gd
        a = RHO * a + (1 - RHO) * d * d
        pw = pw - LR["adadelta"] * d
    assert ref.check(opt.flat_p, " (right form)") <= 1.0
    wrong = float(((opt.flat_p[:n].double() - pw).abs() / (2 * ref.e_p + 1e-30)).max())
    print(f"[flat optim adadelta] eps-outside-sqrt control: err/bar {wrong:.3e}")
    assert wrong > 100


@pytest.mark.parametrize("alg", ["adamax", "adam", "adadelta", "sgd"])
def test_device_lr_follows_schedule_and_frozen_lr_misses(dev, alg):
    """The pass reads lr from the optimiser's device scalar: FlatExponentialLR changes it between calls (as between the
    replays of a captured step); a pass that kept the first lr misses."""
    n, gamma = 300_007, 0.5
    bucket, p = _bucket(dev, 6000, n)
    ref = _Reference(alg, p.detach().clone(), LR[alg], 0.0)
    opt = FlatOptimizer(bucket, alg, lr=LR[alg], **({"betas": (B1, B2), "eps": EPS} if alg in ("adam", "adamax") else {}))
    sched = FlatExponentialLR(opt, gamma)
    frozen_b, _ = _bucket(dev, 6000, n)
    frozen = FlatOptimizer(frozen_b, alg, lr=LR[alg], **({"betas": (B1, B2), "eps": EPS} if alg in ("adam", "adamax") else {}))
    torch_sched = torch.optim.lr_scheduler.ExponentialLR(ref.opt, gamma)
    for i, g in enumerate(_grads(n, dev, 6001, steps=8)):
        bucket.flat[:g.numel()].copy_(g)
        frozen_b.flat[:g.numel()].copy_(g)
        opt.step()
        frozen.step()
        ref.step(g)
        if i % 2 == 1:                                # "epoch" boundary every 2 steps
            sched.step()
            torch_sched.step()
            ref.lr = ref.opt.param_groups[0]["lr"]
            assert sched.get_last_lr()[0] == ref.lr      # same Python-float chain as torch
    assert ref.check(opt.flat_p, " scheduled") <= 1.0
    assert float(((frozen.flat_p[:n].double() - ref.param.detach()).abs() / (2 * ref.e_p + 1e-30)).max()) > 100


def test_abs_sum_is_deterministic_and_matches_fp64(dev):
    for n, seed in ((1, 1), (5, 2), (4096, 3), (N, 4), (17_000_001, 5)):
        gen = torch.Generator(device=dev).manual_seed(seed)
        x = torch.randn(n, device=dev, generator=gen) * 0.1
        s = ops.flat_abs_sum(x)
        ref = float(x.double().abs().sum())
        # fp32 partial sums of ~n / 262144 terms, a 256-wide tree and an fp64 final pass: a few hundred ulps at most
        assert abs(float(s) - ref) <= 64 * U * ref * np.log2(max(n, 2)) + 1e-30, (n, float(s), ref)
        assert torch.equal(ops.flat_abs_sum(x), s)                     # no atomics: the same bits every time
    off = torch.randn(1001, device=dev)[1:]                            # 4-byte but not 16-byte aligned: scalar path
    assert abs(float(ops.flat_abs_sum(off)) - float(off.double().abs().sum())) <= 1e-4 * float(off.abs().sum())


def test_optim_entry_refuses_bad_arguments(dev):
    from multimodal_path_omic_amd import _lib as L
    x = torch.zeros(64, device=dev)
    lib = L.lib()
    assert lib.mpo_optim_step_flat(7, L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), 64, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 0.0, 1,
                                   None, L.stream_of(x)) != 0
    assert b"algorithm" in lib.mpo_last_error()
    assert lib.mpo_optim_step_flat(1, L.ptr(x), L.ptr(x), None, None, 64, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 0.0, 1,
                                   None, L.stream_of(x)) != 0
    assert lib.mpo_optim_step_flat(3, x.data_ptr() + 2, L.ptr(x), None, None, 8, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 0.0, 1,
                                   None, L.stream_of(x)) != 0
    assert lib.mpo_abs_sum_flat(L.ptr(x), 64, L.ptr(x), None, 0, L.stream_of(x)) != 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("alg", ["adamax", "adadelta"])
def test_unaligned_and_odd_buffers_take_the_same_arithmetic(dev, alg):
    """Buffers that are not 16-byte aligned, or an element count not a multiple of 4, run element by element: the same
    update as the 16-byte path, up to the compiler's FMA contraction (a few ulps of the parameter)."""
    n = 4099
    gen = torch.Generator(device=dev).manual_seed(77)
    base = [torch.randn(n + 1, device=dev, generator=gen) * s for s in (0.05, 1.0)]
    a = [t[:n].clone() for t in base] + [torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
    raw = [torch.zeros(n + 1, device=dev) for _ in range(4)]
    for r, t in zip(raw, a):
        r[1:].copy_(t)
    b = [r[1:] for r in raw]                                              # 4-byte offset: no 16-byte access possible
    for _ in range(3):
        for p, g, s1, s2 in (a, b):
            ops.optim_step_flat(alg, p, g, s1, s2, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, l1=1e-3)
    torch.testing.assert_close(a[0], b[0], rtol=1e-6, atol=1e-9)
