"""Two C-ABI entries INTEGRATION.md offers to reference maintainers, called through ctypes as a caller of the library would:
mpo_colsum_bf16 (column sums of a bf16 matrix in fp32: the patch layer's bias gradient) and mpo_patch_epilogue_forward /
_backward (h = dropout_p(relu(h + b)) in place on a bf16 product, and its derivative).  References: fp64 sums, and bit-exact
fp32 element-wise arithmetic rounded once to bf16.  Operands are carved out of NaN-filled buffers (nothing outside the
rows may be read or written), and both entries move bf16 x 8 (16-byte) vectors: a misaligned pointer must be refused on
the host, before any launch."""
import pytest
import torch

from multimodal_path_omic_amd import _lib as L

pytestmark = pytest.mark.gpu
WIDTHS = [8 * d for d in (1, 2, 4, 8, 16, 32, 64, 128, 256)]       # 8 * every divisor of 256
COLSUM_REL = 1e-6                                                    # fp32 column sums against fp64, relative to sum |x|
PAD = 8                                                              # NaN rows either side (keeps 16-byte alignment)


def _padded(rows, cols, dev, dtype=torch.bfloat16):
    buf = torch.full((rows + 2 * PAD, cols), float("nan"), device=dev, dtype=dtype)
    return buf, buf[PAD:PAD + rows]


def _colsum(x, out):
    L.check(L.lib().mpo_colsum_bf16(L.ptr(x), L.ptr(out), x.shape[0], x.shape[1], L.stream_of(x)), "mpo_colsum_bf16")


def _rows_for(cols, edge):
    """edge 'grid': more rows than the launch's 2048 workgroups x (256 / (cols / 8)) rows cover in one trip."""
    return 2048 * (256 // (cols // 8)) + 5 if edge == "grid" else edge


@pytest.mark.parametrize("edge", [1, 7, 33, "grid"])
@pytest.mark.parametrize("cols", WIDTHS)
def test_colsum_bf16_matches_fp64(dev, cols, edge):
    rows = _rows_for(cols, edge)
    gen = torch.Generator(device=dev).manual_seed(cols * 7 + rows)
    buf, x = _padded(rows, cols, dev)
    x.copy_(torch.randn(rows, cols, device=dev, generator=gen) * 3.0)
    out = torch.full((cols,), float("nan"), device=dev)
    _colsum(x, out)
    ref = x.double().sum(0)
    scale = x.double().abs().sum(0)
    # fp32 partial sums (a thread's rows, a workgroup's 256 lanes, fp32 atomics across workgroups): rounding errors of
    # ~1e-8 of sum |x| with random signs; one row lost or counted twice moves a column by ~1 / rows of it
    err = float(((out.double() - ref).abs() / scale.clamp_min(1e-30)).max())
    assert err < COLSUM_REL, err
    # integer-valued entries: every partial sum is exact in fp32 (|sum| < 2^24), so the result must be too
    x.copy_(torch.randint(-8, 9, (rows, cols), device=dev, generator=gen).to(torch.bfloat16))
    _colsum(x, out)
    assert torch.equal(out.double(), x.double().sum(0))
    assert torch.isnan(buf[:PAD]).all() and torch.isnan(buf[PAD + rows:]).all()


def _epilogue(h, bias, drop_p, seed=0, offset=0):
    L.check(L.lib().mpo_patch_epilogue_forward(L.ptr(h), L.ptr(bias), h.shape[0], h.shape[1], float(drop_p), seed, offset,
                                               None, L.stream_of(h)), "mpo_patch_epilogue_forward")


def _epilogue_backward(h, dy, g, drop_p, d_bias=None):
    lib = L.lib()
    ws = torch.empty(max(256, lib.mpo_patch_epilogue_backward_workspace_bytes(h.numel(), h.shape[1])), dtype=torch.uint8,
                     device=h.device)
    L.check(lib.mpo_patch_epilogue_backward(L.ptr(h), L.ptr(dy), L.ptr(g), h.numel(), h.shape[1], float(drop_p), L.ptr(d_bias),
                                            L.ptr(ws), ws.numel(), L.stream_of(h)), "mpo_patch_epilogue_backward")


@pytest.mark.parametrize("edge", [1, 7, 33, "grid"])
@pytest.mark.parametrize("cols", [8, 64, 256, 2048])
def test_epilogue_without_dropout_is_bit_exact(dev, cols, edge):
    """p = 0: h = bf16(relu(fp32(h) + b)), one rounding -- bit for bit what torch computes from the same values.  'grid':
    more 8-element vectors than the launch's 8192 x 256 threads cover in one trip."""
    rows = 8192 * 256 * 8 // cols + 5 if edge == "grid" else edge
    gen = torch.Generator(device=dev).manual_seed(cols + rows)
    buf, h = _padded(rows, cols, dev)
    h.copy_(torch.randn(rows, cols, device=dev, generator=gen))
    b = torch.randn(cols, device=dev, generator=gen) * 0.5
    ref = torch.relu(h.float() + b).bfloat16()
    _epilogue(h, b, 0.0)
    assert torch.equal(h, ref)
    assert torch.isnan(buf[:PAD]).all() and torch.isnan(buf[PAD + rows:]).all()


def test_epilogue_dropout_rate_scale_and_backward_mask(dev):
    """p = 0.25: a quarter of the (all positive) activations dropped, the kept ones scaled by exactly fp32(1 / 0.75) = 4/3
    before the one rounding; the backward gates dy by the same mask (read off h) with the same scale, and its bias
    gradient is the column sums of that gated gradient."""
    rows, cols, p = 4096, 256, 0.25
    gen = torch.Generator(device=dev).manual_seed(5)
    h = (torch.rand(rows, cols, device=dev, generator=gen) + 0.1).bfloat16()
    b = torch.rand(cols, device=dev, generator=gen) * 0.5               # relu(h + b) > 0 everywhere: zeros are drops
    h_in = h.clone()
    pre = torch.relu(h.float() + b)
    scale = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)       # fp32(4/3), as the kernel forms 1 / (1 - p)
    _epilogue(h, b, p, seed=1234, offset=99)
    kept = h != 0
    rate = 1.0 - float(kept.float().mean())
    assert abs(rate - p) < 5e-3, rate                                  # 1M draws: sigma 4.3e-4
    assert torch.equal(h[kept], (pre * scale.to(dev)).bfloat16()[kept])
    # same (seed, offset): the same mask; another offset: another mask
    h2, h3 = h_in.clone(), h_in.clone()
    _epilogue(h2, b, p, seed=1234, offset=99)
    _epilogue(h3, b, p, seed=1234, offset=99 + rows * cols)
    assert torch.equal(h2 != 0, kept) and not torch.equal(h3 != 0, kept)
    dy = torch.randn(rows, cols, device=dev, generator=gen).bfloat16()
    g = torch.empty_like(dy)
    d_bias = torch.full((cols,), float("nan"), device=dev)
    _epilogue_backward(h, dy, g, p, d_bias)
    ref_g = torch.where(kept, (dy.float() * scale.to(dev)).bfloat16(), torch.zeros_like(dy))
    assert torch.equal(g, ref_g)
    ref_b = g.double().sum(0)
    assert float(((d_bias.double() - ref_b).abs() / g.double().abs().sum(0)).max()) < COLSUM_REL
    g0 = torch.empty_like(dy)
    _epilogue_backward(h, dy, g0, p)                                   # without the column sums
    assert torch.equal(g0, g)


def _misaligned(n, dev, dtype=torch.bfloat16):
    """A contiguous n-element tensor starting 2 bytes past a 16-byte boundary (and the buffer it lives in)."""
    buf = torch.full((n + 16,), 3.0, device=dev, dtype=dtype)
    t = buf[1:1 + n]
    assert t.data_ptr() % 16 != 0
    return buf, t


def test_misaligned_operands_are_refused_before_any_launch(dev):
    cols, rows = 256, 64
    _, x = _misaligned(rows * cols, dev)
    out = torch.full((cols,), 7.0, device=dev)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _colsum(x.view(rows, cols), out)
    hb, h = _misaligned(rows * cols, dev)
    b = torch.zeros(cols, device=dev)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _epilogue(h.view(rows, cols), b, 0.0)
    h_ok = torch.full((rows, cols), 3.0, device=dev, dtype=torch.bfloat16)
    bbuf = torch.zeros(cols + 4, device=dev)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _epilogue(h_ok, bbuf[1:1 + cols], 0.0)                          # fp32 bias 4 bytes off
    dy = torch.ones(rows, cols, device=dev, dtype=torch.bfloat16)
    gb, g = _misaligned(rows * cols, dev)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _epilogue_backward(h_ok, dy, g.view(rows, cols), 0.0)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all() and (hb == 3.0).all() and (h_ok == 3.0).all() and (gb == 3.0).all())
