"""The patch layer of an fp16-stored window on the hand-written kernels (mpo_patch_fc_f16_*, csrc/patch_fc_split.hip;
models/mcat/mcat.py:24-29,87 and its backward): the forward as two fp16 MFMA terms W_hi X + W_lo X against the fp64 product
of the SAME stored operands (X as fp16 stores it, W_H fp32), the one-pass backward (ReLU / dropout derivative read off H_bag,
dW_H = g^T X with X split exactly into bf16 hi + lo, db_H = colsum g) against fp64 as well.  The only rounding left is W's
dropped lo tail and the fp32 accumulation, so the bars are those tests/test_gpu_patch_fc_f32.py holds the fp32 window's
kernels to, on that file's seeded operands."""
import pytest
import torch

from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import ops

pytestmark = pytest.mark.gpu


def _operands(rows, dev, seed):
    """tests/test_gpu_patch_fc_f32.py's operands; x additionally as fp16 stores it."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(rows, 1024, device=dev, generator=gen)
    w = (torch.rand(256, 1024, device=dev, generator=gen) - 0.5) / 16
    b = torch.randn(256, device=dev, generator=gen) * 0.1
    return x.half(), w, b, gen


@pytest.mark.parametrize("rows", [1, 15, 127, 128, 129, 1000, 33001])
def test_forward_and_backward_match_fp64(dev, rows):
    x, w, b, gen = _operands(rows, dev, rows)
    wp, bp = torch.nn.Parameter(w.clone()), torch.nn.Parameter(b.clone())
    # operands carved out of NaN-padded buffers: nothing outside [0, rows) may leak into a sum
    xbuf = torch.full((rows + 200, 1024), float("nan"), device=dev, dtype=torch.float16)
    xbuf[:rows] = x
    h = ops.patch_fc_f16(xbuf[:rows], wp, bp, 0.0)
    assert h.dtype == torch.float32 and h.shape == (rows, 256)
    ref = torch.relu(x.double() @ w.double().t() + b.double())
    err = float((h.double() - ref).abs().max())
    print(f"rows {rows}: forward |err| {err:.2e}")
    assert err < 3e-6, err
    probe = torch.randn(rows, 256, device=dev, generator=gen)
    (h * probe).sum().backward()
    g = probe.double() * (ref > 0)
    g_k = probe.double() * (h.detach() > 0)                    # (dW against the mask the kernel itself used, as in the fp32 file)
    dw_ref, db_ref = g_k.t() @ x.double(), g_k.sum(0)
    flips = float((h.detach() > 0).ne(ref > 0).float().mean())
    e_w = float((wp.grad.double() - dw_ref).abs().max() / dw_ref.abs().max().clamp_min(1e-30))
    e_b = float((bp.grad.double() - db_ref).abs().max() / db_ref.abs().max().clamp_min(1e-30))
    print(f"rows {rows}: mask flips {flips:.2e}, dW rel {e_w:.2e}, db rel {e_b:.2e}")
    assert flips < 5e-6
    assert e_w < 1e-4 and e_b < 1e-5, (e_w, e_b)
    assert float(((g - g_k) != 0).float().mean()) < 5e-6


def _scaled_operands(dev, case):
    rows = 3000
    x, w, b, gen = _operands(rows, dev, 77)
    x_gain, w_gain = {"features_1e-4": (1e-4, 1.0), "features_1e4": (1e4, 1.0), "row_of_65504": (1.0, 1.0),
                      "weights_3000": (1.0, 3000.0), "weights_1e-3": (1.0, 1e-3)}[case]
    x = (x.float() * x_gain).half()
    if case == "row_of_65504":
        sign = torch.where(torch.rand(1024, device=dev, generator=gen) < 0.5, -1.0, 1.0)
        x[5] = (sign * 65504.0).half()
    return x, w * w_gain, b * (x_gain * w_gain)


@pytest.mark.parametrize("case", ["features_1e-4", "features_1e4", "row_of_65504", "weights_3000", "weights_1e-3"])
def test_forward_keeps_fp32_accuracy_at_any_operand_scale(dev, case):
    """tests/test_gpu_patch_fc_f32.py's normalisation (error over max |ref|, 3e-6; mask flips 2e-5).  features_1e-4: most
    stored features are fp16 SUBNORMALS (below 6.1e-5) and must reach the MFMA as operands like any other -- flushed to zero
    they would cost ~0.3 of the product; features_1e4 and the row of +-65504 sit at fp16's upper end (no feature scale, no
    clamp: the scaled weight's 2^15 times 65504 over 1024 terms stays far inside the fp32 accumulator)."""
    x, w, b = _scaled_operands(dev, case)
    assert torch.isfinite(x).all()
    if case == "features_1e-4":
        assert float((x.abs() < 6.1e-5).float().mean()) > 0.4
    h = ops.patch_fc_f16(x, torch.nn.Parameter(w), torch.nn.Parameter(b), 0.0)
    ref = torch.relu(x.double() @ w.double().t() + b.double())
    err = float((h.double() - ref).abs().max() / ref.abs().max())
    flips = float((h > 0).ne(ref > 0).float().mean())
    print(f"{case}: forward err / max|ref| {err:.2e}, mask flips {flips:.2e}")
    assert err < 3e-6, err
    assert flips < 2e-5


@pytest.mark.parametrize("p", [0.25, 0.1])
def test_dropout_is_the_fp32_kernels_stream_and_gates_the_backward(dev, p):
    """Same (seed, offset, epoch) as the fp32 kernel on x.float(): the same zero pattern wherever the fp64 pre-activation is
    clear of the ReLU kink; realised rate round(256 p) / 256, keep scale 256 / (256 - round(256 p)) -- at p = 0.1 neither is
    the nominal one (26 / 256, 1.11304 against 1.11111) -- and a backward gated by exactly that scale."""
    rows = 20000
    thr8 = int(p * 256.0 + 0.5)
    realised, scale = thr8 / 256.0, 256.0 / (256.0 - thr8)
    x, w, b, gen = _operands(rows, dev, 9)
    wp, bp = torch.nn.Parameter(w.clone()), torch.nn.Parameter(b.clone())
    torch.manual_seed(5)
    calls = ops._rng_calls
    try:
        h = ops.patch_fc_f16(x, wp, bp, p)
        span = ops._rng_calls - calls
        ops._rng_calls = calls
        h32 = ops.patch_fc_f32(x.float(), torch.nn.Parameter(w.clone()), torch.nn.Parameter(b.clone()), p)
        assert ops._rng_calls - calls == span                  # the fp32 Function's counter reservation
    finally:
        ops._rng_calls = calls + span
    pre = x.double() @ w.double().t() + b.double()
    clear = pre > 1e-4
    assert torch.equal((h == 0)[clear], (h32 == 0)[clear])
    # (each kernel within 3e-6 of the same fp64 product, times the keep scale of at most 4 / 3)
    assert float((h.detach() - h32.detach()).abs().max()) < 8e-6
    base = torch.relu(pre).float()
    pos = base > 0.05
    kept = (h > 0) & pos
    rate = 1.0 - float(kept.sum()) / float(pos.sum())
    ks = h[kept] / base[kept]
    print(f"p {p}: realised rate {rate:.5f} (round(256 p) / 256 = {realised:.5f}), keep scale off by {float((ks - scale).abs().max()):.1e}")
    assert abs(rate - realised) < (5e-3 if p == 0.25 else 1e-3), rate      # (0.1 against 26 / 256 differ by 1.6e-3: told apart)
    assert float((ks - scale).abs().max()) < 1e-3
    h2 = ops.patch_fc_f16(x, wp, bp, p)                        # a second call reserves new counters: a fresh mask
    assert float(((h > 0) != (h2 > 0)).float().mean()) > 0.05
    probe = torch.randn(rows, 256, device=dev, generator=gen)
    (h * probe).sum().backward()
    g = probe.double() * (h.detach() > 0) * scale
    dw_ref, db_ref = g.t() @ x.double(), g.sum(0)
    e_w = float((wp.grad.double() - dw_ref).abs().max() / dw_ref.abs().max())
    e_b = float((bp.grad.double() - db_ref).abs().max() / db_ref.abs().max())
    print(f"p {p}: gated dW rel {e_w:.2e}, db rel {e_b:.2e}")
    assert e_w < 1e-4 and e_b < 1e-5, (e_w, e_b)


def test_non_finite_features_stay_non_finite(dev):
    """A NaN or an infinity in a patch feature makes its row of H_bag non-finite -- no clamp, and no ReLU turning a -inf sum
    into a finite zero -- and leaves every other row alone."""
    rows = 500
    x, w, b, gen = _operands(rows, dev, 78)
    clean = ops.patch_fc_f16(x.clone(), torch.nn.Parameter(w), torch.nn.Parameter(b), 0.0)
    x2 = x.clone()
    x2[7, 100] = float("nan")
    x2[300, 5] = float("inf")
    x2[411, 1023] = float("-inf")
    h = ops.patch_fc_f16(x2, torch.nn.Parameter(w), torch.nn.Parameter(b), 0.0)
    keep = torch.ones(rows, dtype=torch.bool, device=dev)
    for r in (7, 300, 411):                                    # (the whole row, as from the fp32 window's kernel)
        assert not torch.isfinite(h[r]).any(), r
        keep[r] = False
    assert torch.isfinite(h[keep]).all()
    torch.testing.assert_close(h[keep], clean[keep], rtol=0, atol=5e-6)


def test_exactly_its_geometry_is_claimed(dev):
    h16 = dict(device=dev, dtype=torch.float16)
    w = torch.empty(256, 1024, device=dev)
    assert ops.patch_fc_f16_supported(torch.empty(4, 1024, **h16), w)
    assert not ops.patch_fc_f16_supported(torch.empty(4, 1024, device=dev), w)
    assert not ops.patch_fc_f16_supported(torch.empty(4, 1024, device=dev, dtype=torch.bfloat16), w)
    assert not ops.patch_fc_f16_supported(torch.empty(4, 1024, **h16), torch.empty(128, 1024, device=dev))
    assert not ops.patch_fc_f16_supported(torch.empty(4, 512, **h16), torch.empty(256, 512, device=dev))
    assert not ops.patch_fc_f16_supported(torch.empty(4, 2048, **h16)[:, ::2], w)
    assert not ops.patch_fc_f32_supported(torch.empty(4, 1024, **h16), w)
    with pytest.raises(ValueError, match="fp16 patch layer: built for"):
        ops.patch_fc_f16(torch.empty(4, 1024, device=dev), w, torch.empty(256, device=dev), 0.0)


def _rc(name, *args):
    lib = L.lib()
    rc = getattr(lib, name)(*args)
    return rc, (lib.mpo_last_error() or b"").decode()


def test_entries_refuse_in_the_fp32_entries_words(dev):
    """768 / 128-embed / p = 0.999 (round(256 p) = 256): refused before anything is launched, output untouched, no counters
    reserved -- by ops in _realised_drop's words, by the C entries in mpo_patch_fc_f32_*'s."""
    rows = 64
    x, w, b, _ = _operands(rows, dev, 3)
    words = r"realised as round\(256 p\) / 256 = 256/256"
    calls = ops._rng_calls
    with pytest.raises(ValueError, match=words):
        ops.patch_fc_f16(x, w, b, 0.999)
    assert ops._rng_calls == calls
    h = torch.full((rows, 256), 7.0, device=dev)
    dw, db = torch.full((256, 1024), 7.0, device=dev), torch.full((256,), 7.0, device=dev)
    lib = L.lib()
    ws = ops._workspace(lib.mpo_patch_fc_f16_workspace_bytes(1), dev)
    assert lib.mpo_patch_fc_f16_workspace_bytes(0) == lib.mpo_patch_fc_f32_workspace_bytes(0)
    assert lib.mpo_patch_fc_f16_workspace_bytes(1) == lib.mpo_patch_fc_f32_workspace_bytes(1)
    s = L.stream_of(x)

    def fwd(patch_dim, embed, drop_256, total=rows):
        return _rc("mpo_patch_fc_f16_forward", L.ptr(x), total, patch_dim, L.ptr(w), L.ptr(b), embed, drop_256, 1, 2, None, L.ptr(h),
                   L.ptr(ws), ws.numel(), s)

    def bwd(patch_dim, embed, drop_256, total=rows):
        return _rc("mpo_patch_fc_f16_backward", L.ptr(h), L.ptr(h), L.ptr(x), total, embed, patch_dim, drop_256, L.ptr(dw), L.ptr(db),
                   L.ptr(ws), ws.numel(), s)
    for call, fp32_words in ((lambda: fwd(768, 256, 0), "built for 1024 -> 256 (got 768 -> 256)"),
                             (lambda: fwd(1024, 128, 0), "built for 1024 -> 256 (got 1024 -> 128)"),
                             (lambda: bwd(768, 256, 0), "built for 256 x 1024 (got 256 x 768)"),
                             (lambda: bwd(1024, 128, 0), "built for 256 x 1024 (got 128 x 1024)"),
                             (lambda: fwd(1024, 256, 256), "realised as round(256 p) / 256 = 256/256: nothing would be kept (p must be below 1 - 1/512)"),
                             (lambda: bwd(1024, 256, 256), "realised as round(256 p) / 256 = 256/256"),
                             (lambda: fwd(1024, 256, -1), "patch-layer dropout p must be in [0,1)"),
                             (lambda: fwd(1024, 256, 257), "patch-layer dropout p must be in [0,1)"),
                             (lambda: fwd(1024, 256, 0, total=0), "total_rows 0")):
        rc, msg = call()
        assert rc != 0 and fp32_words in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((h == 7.0).all()) and bool((dw == 7.0).all()) and bool((db == 7.0).all())
    rc, msg = fwd(1024, 256, 255)                              # the largest rate that keeps anything: runs
    assert rc == 0, msg
