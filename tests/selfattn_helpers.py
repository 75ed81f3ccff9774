"""What tests/test_gpu_bag_selfattn.py and tests/test_gpu_bag_selfattn_edges.py share: the fp64 reference of the attention core
of csrc/bag_selfattn.hip, the error measures, the switch between its two arithmetics and the dropout-mask read-back."""
import math

import torch

from multimodal_path_omic_amd import ops
from multimodal_path_omic_amd import synthetic as syn


def relmax(a, b, scale=None):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).abs().max() / (b.abs().max().clamp_min(1e-30) if scale is None else scale))


def part_scale(ref):
    """Scale for one of dq / dk / dv: its own largest entry, but no smaller than 1e-2 of the whole gradient's (at M = 1 the
    true dq and dk are exactly zero)."""
    return lambda sl: max(float(ref[..., sl].abs().max()), 1e-2 * float(ref.abs().max()))


def attention_ref(qkv, heads, keep=None):
    """(n, M, 3d) fp64 on the CPU -> out (n, M, d), probabilities (n, h, M, M); keep: (n, h, M, M) scaled keep mask."""
    n, m, d3 = qkv.shape
    d, hd = d3 // 3, d3 // 3 // heads
    q, k, v = (qkv[..., i * d:(i + 1) * d].reshape(n, m, heads, hd).transpose(1, 2) for i in range(3))
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1)
    pd = p if keep is None else p * keep
    return (pd @ v).transpose(1, 2).reshape(n, m, d), p


def _b3_modes(d, heads):
    """Heads of width 32 (several) and 256 (one) run on three-term bf16 MFMAs by default (~16 mantissa bits per operand); the
    verification hook keeps them on the fp32 kernels.  -> [(hook value, output bar, gradient bar)]"""
    b3 = (heads > 1 and d == 32 * heads) or (heads == 1 and d == 256)
    return [(1, 1e-4, 1e-3), (0, 1e-5, 1e-4)] if b3 else [(1, 1e-5, 1e-4)]


class bf16x3:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from multimodal_path_omic_amd import _lib as L
        self.was = L.lib().mpo_set_bag_self_attention_bf16x3(self.on)

    def __exit__(self, *exc):
        from multimodal_path_omic_amd import _lib as L
        L.lib().mpo_set_bag_self_attention_bf16x3(self.was)


def realised_drop(p):
    """The kernels draw 8 bits per element (csrc/bag_selfattn.hip sa_drop): drop when byte < thr = round(256 p), capped at
    255; kept entries are scaled by 256 / (256 - thr).  -> thr / 256"""
    return min(int(p * 256.0 + 0.5), 255) / 256.0 if p > 0 else 0.0


def _recover_keep(dev, qkv, heads, p, offset):
    """The kernel's own (scaled) keep mask, read back through V = identity blocks: out[q][h hd + c] = P_drop[h][q][b hd + c]."""
    n, m, d3 = qkv.shape
    d, hd = d3 // 3, d3 // 3 // heads
    _, p_ref = attention_ref(qkv.double(), heads)
    keep = torch.zeros(n, heads, m, m, dtype=torch.float64)
    for b in range((m + hd - 1) // hd):
        probe = qkv.clone()
        v = torch.zeros(n, m, heads, hd)
        rows = torch.arange(b * hd, min(m, (b + 1) * hd))
        v[:, rows, :, rows - b * hd] = 1.0
        probe[..., 2 * d:] = v.reshape(n, m, d)
        ops._rng_calls = offset
        out, _ = ops.BagSelfAttentionFn.apply(probe.to(dev), heads, p, False)
        pd = out.cpu().double().reshape(n, m, heads, hd).permute(0, 2, 1, 3)          # (n, h, q, c)
        keep[..., rows] = pd[..., : len(rows)] / p_ref[..., rows].clamp_min(1e-300)
    return keep


def _dropout_mask_check(dev, m, d, heads, out_bar, grad_bar, p=0.25, n=1):
    """-> (keep, out, x.grad, reference gradient) for the callers that look further.  The kernels quantise p to
    pr = round(256 p) / 256: the recovered keep values must be {0, 1 / (1 - pr)} at rate pr (p = 0.25 is its own pr)."""
    g = syn.rng(7100 + m)
    qkv = syn.normal(g, (n, m, 3 * d)) * 0.5
    probe = syn.normal(g, (n, m, d))
    offset, pr = 12345, realised_drop(p)
    keep = _recover_keep(dev, qkv, heads, p, offset)
    vals = keep.round(decimals=4).unique()
    assert all(min(abs(float(v)), abs(float(v) - 1 / (1 - pr))) < 1e-3 for v in vals), vals
    rate = float((keep < 0.5).double().mean())
    assert abs(rate - pr) < 4 * math.sqrt(pr * (1 - pr) / keep.numel()) + 1e-3, rate
    if heads > 1 and m * m >= 64:
        assert not torch.equal(keep[0, 0] > 0.5, keep[0, 1] > 0.5)                    # heads draw their own masks
    elif heads > 1:      # a few bits per head (9 at M = 3; the seed is the process's): two heads may coincide, not all of them
        assert any(not torch.equal(keep[0, 0] > 0.5, keep[0, h] > 0.5) for h in range(1, heads))
    for i in range(1, n):
        assert not torch.equal(keep[0] > 0.5, keep[i] > 0.5), i                       # and so do sequences
    ops._rng_calls = offset
    x = qkv.to(dev).requires_grad_(True)
    out, _ = ops.BagSelfAttentionFn.apply(x, heads, p, False)
    (out * probe.to(dev)).sum().backward()
    xr = qkv.double().requires_grad_(True)
    out_r, _ = attention_ref(xr, heads, keep=(keep > 0.5).double() / (1 - pr))
    (out_r * probe.double()).sum().backward()
    assert relmax(out, out_r) < out_bar
    for part in range(3):
        sl = slice(part * d, (part + 1) * d)
        assert relmax(x.grad[..., sl], xr.grad[..., sl], part_scale(xr.grad)(sl)) < grad_bar, part
    # another offset = another mask
    ops._rng_calls = offset + 1
    out2, _ = ops.BagSelfAttentionFn.apply(qkv.to(dev), heads, p, False)
    assert not torch.equal(out2, out.detach())
    return keep, out.detach().cpu(), x.grad.cpu(), xr.grad
