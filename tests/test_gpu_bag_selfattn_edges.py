"""csrc/bag_selfattn.hip at its tile, batch and map edges: both kernel families (fp32 and three-term bf16, "b3") against the
fp64 attention of selfattn_helpers.attention_ref on the CPU, over the case table of tests/test_bag_selfattn_edges_cpu.py --
every head width at lengths around one and two 64-row blocks, below one 16-row wave tile, on three sequences with their own
data and gains, with the map where one head allows it, and the map kernels at the smallest lengths at which a workgroup walks
more than one key block.  Bars are those of tests/test_gpu_bag_selfattn.py per arithmetic: output 1e-4 (b3) / 1e-5 (fp32) and
gradient 1e-3 / 1e-4 of the largest entry, dq / dk / dv separately; map 1e-3 elementwise relative.

The kernel-level tests call the C ABI with their own buffers: every buffer -- inputs too -- lies between two runs of NaN,
outputs start as NaN, and the runs must still be NaN afterwards (an input read past its end would show as a NaN result)."""
import pytest
import torch

import test_bag_selfattn_edges_cpu as E
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import ops
from multimodal_path_omic_amd import synthetic as syn
from selfattn_helpers import _b3_modes, _dropout_mask_check, attention_ref, bf16x3, part_scale, relmax

pytestmark = pytest.mark.gpu

GUARD = 64                       # floats of NaN before and after every buffer (256 bytes: the 16-byte alignment is kept)
MAP_BAR = 1e-3                   # elementwise relative, where the reference exceeds 1e-30 (tests/test_gpu_bag_selfattn.py)
ROWSUM_BAR = 1e-4                # |sum of a map row - 1| (same file)
GAINS = (1.0, 3.0, 0.5)          # query gain of sequence i: a kernel that reads sequence 0 for sequence 2 fails


@pytest.fixture(autouse=True)
def _rng_calls_put_back():
    was = ops._rng_calls
    yield
    ops._rng_calls = was


def make_inputs(n, m, d, seed):
    g = syn.rng(seed)
    qkv, probe = syn.normal(g, (n, m, 3 * d)), syn.normal(g, (n, m, d))
    for i in range(n):
        qkv[i, :, :d] *= GAINS[i % len(GAINS)]
    return qkv, probe


def reference(qkv, heads, probe=None):
    """-> (out, probabilities of head 0 (n, M, M), gradient | None), fp64"""
    if probe is None:
        with torch.no_grad():
            out, p = attention_ref(qkv.double(), heads)
        return out, p[:, 0], None
    xr = qkv.double().requires_grad_(True)
    out, p = attention_ref(xr, heads)
    (out * probe.double()).sum().backward()
    return out.detach(), p[:, 0].detach(), xr.grad


def run_core(dev, qkv, heads, need_map, probe=None, p=0.0, seed=0, off=0):
    """One forward (and backward) through the C ABI on guarded buffers -> (out, map | None, d_qkv | None) on the CPU."""
    lib = L.lib()
    n, m, d3 = qkv.shape
    d = d3 // 3
    bufs = []

    def buf(numel, fill=None):
        parent = torch.full((int(numel) + 2 * GUARD,), float("nan"), device=dev, dtype=torch.float32)
        view = parent[GUARD:GUARD + int(numel)]
        if fill is not None:
            view.copy_(fill.reshape(-1))
        bufs.append((parent, int(numel)))
        return view

    x = buf(n * m * d3, qkv)
    out = buf(n * m * d)
    saved = buf(lib.mpo_bag_self_attention_saved_floats(n, m, d, heads))
    amap = buf(n * m * m) if need_map else None
    L.call("mpo_bag_self_attention_forward", L.ptr(x), n, m, d, heads, float(p), seed, off, ops._epoch(), L.ptr(out), L.ptr(saved),
           L.ptr(amap), L.stream_of(x))
    dqkv = None
    if probe is not None:
        g = buf(n * m * d, probe)
        dqkv = buf(n * m * d3)
        ws_bytes = lib.mpo_bag_self_attention_workspace_bytes(n, m, d, heads)
        ws = buf((ws_bytes + 3) // 4)
        L.call("mpo_bag_self_attention_backward", L.ptr(x), L.ptr(out), L.ptr(saved), L.ptr(g), n, m, d, heads, float(p), seed, off,
               ops._epoch(), L.ptr(dqkv), L.ptr(ws), ws_bytes, L.stream_of(x))
    torch.cuda.synchronize()
    for i, (parent, numel) in enumerate(bufs):
        assert bool(torch.isnan(parent[:GUARD]).all()) and bool(torch.isnan(parent[GUARD + numel:]).all()), f"guard of buffer {i}"
    return (out.view(n, m, d).cpu(), amap.view(n, m, m).cpu() if need_map else None,
            dqkv.view(n, m, d3).cpu() if dqkv is not None else None)


def map_errors(amap, p_ref):
    """-> (largest elementwise relative error where the reference exceeds 1e-30, largest |row sum - 1|)"""
    got = amap.double()
    big = p_ref > 1e-30
    rel = ((got - p_ref).abs() / p_ref.clamp_min(1e-30))[big].max().item()
    return rel, float((got.sum(-1) - 1).abs().max())


def check(tag, res, ref, d, out_bar, grad_bar, map_bar=MAP_BAR):
    """Prints every figure, then asserts them."""
    (out, amap, dqkv), (out_r, p_r, grad_r) = res, ref
    fig = {"out": relmax(out, out_r)}
    if dqkv is not None:
        for part, name in enumerate(("dq", "dk", "dv")):
            sl = slice(part * d, (part + 1) * d)
            fig[name] = relmax(dqkv[..., sl], grad_r[..., sl], part_scale(grad_r)(sl))
    if amap is not None:
        fig["map"], fig["rowsum"] = map_errors(amap, p_r)
    print(f"[self-attention edges] {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert bool(torch.isfinite(out).all()) and fig["out"] < out_bar, (tag, fig)
    for name in ("dq", "dk", "dv"):
        assert name not in fig or fig[name] < grad_bar, (tag, name, fig)
    if amap is not None:
        assert fig["map"] < map_bar and fig["rowsum"] < ROWSUM_BAR, (tag, fig)
    return fig


def bars(d, heads, hook):
    return {h: (o, g) for h, o, g in _b3_modes(d, heads)}[hook]


def test_case_table_runs_the_kernels_the_cpu_file_says(dev):
    """The family is chosen inside the library (b3_applies); what this side can see is the size of the saved state: the b3 path
    keeps its operand forms (3 x 4 arrays of n Mp d bf16), the fp32 path the log-sum-exps alone -- whatever the hook says."""
    lib = L.lib()
    for d, heads in E.GEOMETRIES:
        n, m = 3, 65
        lse = (n * heads * m + 3) // 4 * 4
        want = lse + (3 * 4 * n * E.mp(m) * d // 2 if E.b3_geometry(d, heads) else 0)
        assert lib.mpo_bag_self_attention_saved_floats(n, m, d, heads) == want, (d, heads)


@pytest.mark.parametrize("n,m,d,heads", E.SMALL_CASES)
def test_small_edges(dev, n, m, d, heads):
    qkv, probe = make_inputs(n, m, d, 8000 + 7 * m + d + heads)
    ref = reference(qkv, heads, probe)
    for hook, out_bar, grad_bar in _b3_modes(d, heads):
        with bf16x3(hook):
            res = run_core(dev, qkv, heads, heads == 1, probe)
        check(f"{E.kernel_of(d, heads, hook)} n={n} M={m} d={d} heads={heads}", res, ref, d, out_bar, grad_bar)


@pytest.mark.parametrize("n,m,d,heads,hook,bwd", E.MAP_CASES)
def test_map_with_several_blocks_per_workgroup(dev, n, m, d, heads, hook, bwd):
    """Forward + map (+ backward on the two 256-wide kernels) at the smallest lengths at which a map workgroup walks two key
    blocks, one workgroup gets a single block and the trailing ones none; the WHOLE map against fp64."""
    family, hd = E.kernel_of(d, heads, hook)
    nblk, split, per, cut = E.map_cut(family, hd, m)
    assert per == 2 and any(b1 - b0 == 1 for b0, b1 in cut) and any(b0 >= nblk for b0, _ in cut)
    qkv, probe = make_inputs(n, m, d, 8500 + m + d)
    ref = reference(qkv, heads, probe if bwd else None)
    with bf16x3(hook):
        res = run_core(dev, qkv, heads, True, probe if bwd else None)
    check(f"{(family, hd)} n={n} M={m} map cut {nblk} blocks / {split} x {per}", res, ref, d, *bars(d, heads, hook))


# ---------------------------------------------------------------------------------------------------------------- dropout
@pytest.mark.parametrize("m,d,heads,p,n", [(96, 256, 8, 0.1, 1), (96, 256, 8, 0.5, 1), (200, 256, 1, 0.1, 1), (200, 256, 1, 0.5, 1),
                                           (70, 512, 1, 0.1, 1), (70, 512, 1, 0.5, 1), (96, 256, 8, 0.25, 2), (200, 256, 1, 0.25, 2)])
def test_dropout_rate_is_quantised_and_sequences_draw_their_own_masks(dev, m, d, heads, p, n):
    """p is realised as round(256 p) / 256 (26 / 256 for 0.1): keep values {0, 256 / (256 - round(256 p))} at that rate, the
    forward and all three gradients under exactly that mask; on two sequences the masks differ (stream seq * H + h)."""
    assert E.thr(0.1) == 26 and E.thr(0.25) == 64 and E.thr(0.5) == 128
    for hook, out_bar, grad_bar in _b3_modes(d, heads):
        with bf16x3(hook):
            _dropout_mask_check(dev, m, d, heads, out_bar, grad_bar, p=p, n=n)


def test_fully_dropped_rows(dev):
    """Three keys at p = 0.5: one row in eight loses every key.  Its output and its dq are exactly zero (no 0 / 0, no stale
    accumulator), and dk / dv equal the reference under the recovered mask (asserted inside _dropout_mask_check)."""
    m, d, heads, p, n = 3, 256, 8, 0.5, 4
    hd = d // heads
    for hook, out_bar, grad_bar in _b3_modes(d, heads):
        with bf16x3(hook):
            keep, out, grad, _ = _dropout_mask_check(dev, m, d, heads, out_bar, grad_bar, p=p, n=n)
        dead = (keep < 0.5).all(-1)                                                    # (n, h, q)
        assert 0 < int(dead.sum()) < dead.numel(), int(dead.sum())
        per_head = lambda t: t.reshape(n, m, heads, hd).permute(0, 2, 1, 3)             # noqa: E731  -> (n, h, q, c)
        o, dq = per_head(out), per_head(grad[..., :d])
        assert bool((o[dead] == 0).all()) and bool((dq[dead] == 0).all()), hook
        assert bool((o[~dead].abs().amax(-1) > 0).all())


@pytest.mark.parametrize("m,d,heads", [(96, 256, 8), (70, 256, 1), (70, 128, 1)])
def test_p_that_rounds_to_zero_is_no_dropout(dev, m, d, heads):
    """round(256 * 0.001) = 0: the no-dropout instantiation, bit for bit, forward and backward; 0.002 rounds to 1 / 256."""
    assert E.thr(0.001) == 0 and E.thr(0.002) == 1
    qkv, probe = make_inputs(1, m, d, 8700 + m)
    for hook, _, _ in _b3_modes(d, heads):
        with bf16x3(hook):
            got = []
            for p in (0.0, 0.001, 0.002):
                ops._rng_calls = 777
                x = qkv.to(dev).requires_grad_(True)
                out, _ = ops.BagSelfAttentionFn.apply(x, heads, p, False)
                (out * probe.to(dev)).sum().backward()
                got.append((out.detach(), x.grad))
        assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), hook
        assert not torch.equal(got[0][0], got[2][0]), hook


# ---------------------------------------------------------------------------------------------------------------- large logits
def test_large_logits(dev):
    """Largest |score| * scale = 80 (E.large_logit_input).  The map bar is not the file's alone: a plain torch fp32 attention has
    its own error at such logits (the exponent's argument error grows with |s|), measured on the CPU against the same fp64
    reference -- E.FP32_LARGE_LOGIT_MAP_ERR -- and the bar is the larger of 1e-3 and 4 x that (E.LARGE_LOGIT_MAP_BAR)."""
    qkv, probe = E.large_logit_input()
    d, heads = E.LARGE_LOGIT_SHAPE[1], 1
    ref = reference(qkv, heads, probe)
    peak = float((qkv[0, :, :d].double() @ qkv[0, :, d:2 * d].double().t()).abs().max()) / d ** 0.5
    assert 79.0 < peak < 81.0, peak
    for hook, out_bar, grad_bar in _b3_modes(d, heads):
        with bf16x3(hook):
            res = run_core(dev, qkv, heads, True, probe)
        check(f"{E.kernel_of(d, heads, hook)} large logits (peak {peak:.1f})", res, ref, d, out_bar, grad_bar, E.LARGE_LOGIT_MAP_BAR)


@pytest.mark.parametrize("m,d,heads", [(70, 256, 1), (70, 256, 8), (70, 128, 1)])
def test_all_zero_query_rows(dev, m, d, heads):
    """A query of zeros scores every key 0: its map row is 1 / M and its output the mean of V."""
    qkv, probe = make_inputs(2, m, d, 8900 + d + heads)
    rows = [0, 5, m - 1]
    qkv[:, rows, :d] = 0.0
    ref = reference(qkv, heads, probe)
    v_mean = qkv[..., 2 * d:].double().mean(1, keepdim=True).expand(-1, len(rows), -1)
    for hook, out_bar, grad_bar in _b3_modes(d, heads):
        with bf16x3(hook):
            res = run_core(dev, qkv, heads, heads == 1, probe)
        check(f"{E.kernel_of(d, heads, hook)} zero queries M={m}", res, ref, d, out_bar, grad_bar)
        out, amap, _ = res
        assert relmax(out[:, rows], v_mean, float(ref[0].abs().max())) < out_bar, hook
        if amap is not None:
            assert float((amap[:, rows].double() * m - 1).abs().max()) < MAP_BAR, hook


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_before_any_launch(dev):
    """Both are MPO_CHECKs of mpo_launch_bag_sa_fwd (csrc/bag_selfattn.hip:1217-1218), ahead of the dispatch: nothing runs."""
    m, d = 32, 256
    base = torch.zeros(1 + m * 3 * d + 3, device=dev)
    view = base[1:1 + m * 3 * d].view(1, m, 3 * d)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.BagSelfAttentionFn.apply(view, 1, 0.0, True)
    with pytest.raises(RuntimeError, match="one head only"):
        ops.BagSelfAttentionFn.apply(torch.zeros(1, m, 3 * d, device=dev), 8, 0.0, True)
