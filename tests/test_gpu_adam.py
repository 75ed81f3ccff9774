"""The optimiser of every training step, mpo_adam_step_flat (csrc/optim.hip adam_flat_kernel) and its wrapper dp.FlatAdam,
against fp64 torch.optim.Adam driven by the same gradient sequence: 20 steps, gradients spanning 1e-6 .. 1e2 with exact
zeros, with and without weight decay, both step-count paths (the device counter FlatAdam and captured graphs use, a
host step >= 1), and a parameter count past the launch's 2048 x 256 threads (the grid-stride loop)."""
import numpy as np
import pytest
import torch

from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd.dp import FlatAdam, FlatGradBucket

pytestmark = pytest.mark.gpu
STEPS = 20
U = 2.0 ** -24                  # unit roundoff of fp32


def f32(v):
    """The kernel takes its hyper-parameters as fp32: the reference uses the same rounded values."""
    return float(np.float32(v))


LR, B1, B2, EPS = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8)


def _grad_sequence(n, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    never = torch.rand(n, device=dev, generator=gen) < 0.1          # elements whose gradient is always exactly 0
    out = []
    for _ in range(STEPS):
        mag = 10.0 ** (torch.rand(n, device=dev, generator=gen) * 8.0 - 6.0)      # 1e-6 .. 1e2
        sign = torch.where(torch.rand(n, device=dev, generator=gen) < 0.5, -1.0, 1.0)
        zero = never | (torch.rand(n, device=dev, generator=gen) < 0.1)
        out.append(torch.where(zero, torch.zeros_like(mag), sign * mag).float())
    return out


class _Reference:
    """fp64 torch.optim.Adam plus a running bound on how far an fp32 evaluation of the same recurrences may drift.

    Per step the kernel rounds a handful of fp32 operations.  g' = g + wd p is off by E_g = u (|g| + wd |p|) (g and wd p
    may cancel) plus wd times the parameter's own drift E_p.  m = b1 m + (1-b1) g' is off by (1-b1) E_g plus ~3 roundings
    of A = b1 A + (1-b1) |g'| (the same recurrence on magnitudes; m itself may cancel to ~0), and older errors decay by b1:
    E_m = b1 E_m + (1-b1) E_g + 3u A.  v adds positive terms: E_v = b2 E_v + (1-b2)(2|g'| + E_g) E_g + 5u v.  The update
    lr/bc1 * m / (sqrt(v)/bc2 + eps) then carries E_m through the same factor, plus a relative error of a few u, of v's
    E_v/2V, and of fp32 powf in the bias corrections (one ulp of b^t against 1 - b^t: u/(1-b1^t), u/(2(1-b2^t))).  The
    parameter error sums those update errors and one rounding of p per step.  The tests hold the kernel to 2x these
    bounds: a few fp32 ulps of each quantity, far below what a wrong bias correction, weight-decay placement or step
    count would move (percent-level on the update)."""

    def __init__(self, p0, wd):
        self.p = p0.double().clone().requires_grad_(False)
        self.param = torch.nn.Parameter(self.p)
        self.opt = torch.optim.Adam([self.param], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
        self.wd = wd
        z = torch.zeros_like(self.p)
        self.A, self.V, self.e_m, self.e_v, self.e_p = z.clone(), z.clone(), z.clone(), z.clone(), z.clone()
        self.t = 0

    def step(self, g):
        self.t += 1
        t = self.t
        p_old = self.param.detach().clone()
        gp = g.double() + self.wd * p_old
        self.param.grad = g.double().clone()
        self.opt.step()
        st = self.opt.state[self.param]
        m, v = st["exp_avg"], st["exp_avg_sq"]
        # g' = g + wd p: one rounding of |g| + wd |p| (g and wd p may cancel), on the drifted fp32 parameter
        e_g = U * (g.double().abs() + self.wd * p_old.abs()) + self.wd * self.e_p
        self.A = B1 * self.A + (1 - B1) * gp.abs()
        self.e_m = B1 * self.e_m + (1 - B1) * e_g + 3 * U * self.A
        self.e_v = B2 * self.e_v + (1 - B2) * (2 * gp.abs() + e_g) * e_g + 5 * U * v
        bc1, bc2s = 1 - B1 ** t, (1 - B2 ** t) ** 0.5
        denom = v.sqrt() / bc2s + EPS
        upd = (LR / bc1) * m / denom
        rel = 8 * U + U / bc1 + U / (2 * (1 - B2 ** t)) + self.e_v / (2 * v).clamp_min(1e-300)
        self.e_p = self.e_p + (LR / bc1) * self.e_m / denom + upd.abs() * rel + U * self.param.detach().abs()

    def check(self, p, m, v):
        st = self.opt.state[self.param]
        for name, got, ref, bound in (("exp_avg", m, st["exp_avg"], self.e_m), ("exp_avg_sq", v, st["exp_avg_sq"], self.e_v),
                                      ("param", p, self.param.detach(), self.e_p)):
            err = (got.double() - ref).abs()
            worst = float((err / (2 * bound).clamp_min(1e-300)).max())
            assert bool((err <= 2 * bound).all()), (name, self.t, worst, float(err.max()))


@pytest.mark.parametrize("n", [1, 63, 2048 * 256 + 5])
@pytest.mark.parametrize("wd", [0.0, 1e-5])
@pytest.mark.parametrize("counter", ["device", "host"])
def test_adam_step_flat_matches_torch_adam(dev, n, wd, counter):
    wd = f32(wd)
    gen = torch.Generator(device=dev).manual_seed(n)
    p = torch.randn(n, device=dev, generator=gen)
    ref = _Reference(p, wd)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    t_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = L.lib()
    for t, g in enumerate(_grad_sequence(n, dev, n + 1), start=1):
        if counter == "device":
            t_dev += 1
            step, step_ptr = 0, L.ptr(t_dev)
        else:
            step, step_ptr = t, None
        L.check(lib.mpo_adam_step_flat(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, LR, B1, B2, EPS, wd, step, step_ptr,
                                       L.stream_of(p)), "mpo_adam_step_flat")
        ref.step(g)
        ref.check(p, m, v)


@pytest.mark.parametrize("wd", [0.0, 1e-5])
def test_flat_adam_matches_torch_adam(dev, wd):
    """FlatAdam over a bucket of parameters of several sizes (slices padded to 64 elements; the padding stays zero)."""
    wd = f32(wd)
    gen = torch.Generator(device=dev).manual_seed(3)
    sizes = [1, 63, 2048 * 256 + 5]
    params = [torch.nn.Parameter(torch.randn(k, device=dev, generator=gen)) for k in sizes]
    refs = [_Reference(q.detach(), wd) for q in params]
    bucket = FlatGradBucket(params)
    opt = FlatAdam(bucket, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd)
    seqs = [_grad_sequence(k, dev, 10 + i) for i, k in enumerate(sizes)]
    for t in range(STEPS):
        for q, seq in zip(params, seqs):
            q._mpo_grad_view.copy_(seq[t])
        opt.step()
        for q, r, off, seq in zip(params, refs, bucket.offsets, seqs):
            r.step(seq[t])
            k = q.numel()
            r.check(q.detach(), opt.exp_avg[off:off + k], opt.exp_avg_sq[off:off + k])
    assert int(opt.t_dev) == STEPS
    used = torch.zeros_like(opt.flat_p, dtype=torch.bool)
    for q, off in zip(params, bucket.offsets):
        used[off:off + q.numel()] = True
        assert q.data_ptr() == opt.flat_p[off:].data_ptr()        # parameters live in the flat buffer
    assert bool((opt.flat_p[~used] == 0).all() and (opt.exp_avg_sq[~used] == 0).all())


def test_adam_step_zero_without_device_counter_is_refused(dev):
    p = torch.ones(8, device=dev)
    g, m, v = torch.ones_like(p), torch.zeros_like(p), torch.zeros_like(p)
    with pytest.raises(RuntimeError, match="adam: step counts from 1"):
        L.check(L.lib().mpo_adam_step_flat(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), 8, LR, B1, B2, EPS, 0.0, 0, None,
                                           L.stream_of(p)), "mpo_adam_step_flat")
    torch.cuda.synchronize()
    assert bool((p == 1).all() and (m == 0).all())               # refused before any launch
