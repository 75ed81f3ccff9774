"""CPU-only: the dropout stream bookkeeping of the tail's fused entries (csrc/tail_api.hip).  For every geometry of a grid
the kernels accept, the counters each site draws (tests/dropout_replay.py, restated from the kernels' indexing) lie inside
the span the library reserves per call, and no two sites or branches of one call share a counter.  The span queries
are pure host functions; no kernel is launched."""
import itertools

import pytest

import dropout_replay as R
from multimodal_path_omic_amd import _lib as L

ENC_T = (1, 6, 16, 17, 200, 2050)
WIDTHS = ((128, 512), (256, 512), (512, 512))          # (d, ff): the small, medium and big models


def _disjoint(ranges, what):
    ranges = sorted((lo, hi, tag) for lo, hi, tag in ranges if hi > lo)
    for (lo0, hi0, t0), (lo1, hi1, t1) in zip(ranges, ranges[1:]):
        assert hi0 <= lo1, (what, t0, (lo0, hi0), t1, (lo1, hi1))


def _inside(ranges, off, span, what):
    for lo, hi, tag in ranges:
        assert off <= lo and hi <= off + span, (what, tag, (lo, hi), (off, off + span))


def _heads(d):
    return sorted({1, 8, d // 32, d // 16, d // 2})


def test_encoder_streams_stay_in_their_span_and_apart():
    lib = L.lib()
    off = 12345
    n = 0
    for (d, ff), T, nb, ns, layers in itertools.product(WIDTHS, ENC_T, (1, 2), (1, 5, 32, 64), (1, 2)):
        if T > 16 and ns > 1:
            continue                                     # long token axes: one bag per call (row f3)
        for heads in _heads(d):
            if T <= 16 and heads * T > max(ff, 3 * d):
                continue                                 # refused by mpo_encoder_forward (test below)
            if T > 16 and d // heads not in (16, 32, 64, 128, 256, 512):
                continue                                 # head dimensions the bag self-attention is built for
            span = lib.mpo_encoder_rng_span(nb * ns, T, d, ff, layers)
            assert span == R.encoder_span(nb * ns, T, d, ff, layers)
            sites = [(lo, hi, (l, s, br)) for l, s, br, lo, hi in R.encoder_sites(nb, ns, T, d, ff, heads, layers, off)]
            what = dict(d=d, ff=ff, T=T, branches=nb, slides=ns, layers=layers, heads=heads)
            _inside(sites, off, span, what)
            _disjoint(sites, what)
            n += 1
    assert n > 500


def test_narrow_heads_would_overlap_the_next_stream():
    """T <= 16 draws heads * T counters per token row for the attention probabilities, in a slot max(ff, 3 d) counters
    per row wide.  Narrow heads (d = 128 in 64 heads of 2) at T = 16 would run into the out-proj mask's stream, so
    mpo_encoder_forward refuses them (tests/test_gpu_train_dropout.py checks the refusal on the GPU)."""
    d, ff, T, heads = 128, 512, 16, 64
    sites = R.encoder_sites(1, 1, T, d, ff, heads, 1)
    s0 = next(s for s in sites if s[1] == 0)
    s1 = next(s for s in sites if s[1] == 1)
    assert s0[4] > s1[3]
    # the model's geometries are not affected: 8 heads at every T <= 16 and width
    for (d, ff), T in itertools.product(WIDTHS, range(1, 17)):
        assert 8 * T <= max(ff, 3 * d)


@pytest.mark.parametrize("interleave", [False, True])
def test_gated_pool_streams_stay_in_their_span_and_apart(interleave):
    lib = L.lib()
    off = 777
    for (d, _), L_, nb, ns in itertools.product(WIDTHS, (1, 6, 64, 65, 2050), (1, 2), (1, 5, 32, 64)):
        if L_ > 65 and ns > 1:
            continue
        span = lib.mpo_gated_pool_rng_span(nb * ns, L_, d)
        assert span == R.pool_span(nb * ns, L_, d)
        sites = [(lo, hi, (s, br)) for s, br, lo, hi in R.pool_sites(nb, ns, L_, d, interleave, off)]
        what = dict(d=d, L=L_, branches=nb, slides=ns, interleave=interleave)
        _inside(sites, off, span, what)
        _disjoint(sites, what)


def test_interleaved_rho_branches_draw_distinct_elements():
    """Interleaved rho: branch br's element (s, j) is element s * nb * d + br * d + j of one stream -- every element of
    the stream once, no two (branch, slide, column) triples alike."""
    for d, nb, ns in itertools.product((128, 256, 512), (1, 2), (1, 5, 64)):
        seen = set()
        for br in range(nb):
            for s in range(ns):
                first = 4 * (br * (d // 4)) + s * nb * d
                elems = range(first, first + d)
                assert not seen.intersection(elems)
                seen.update(elems)
        assert seen == set(range(ns * nb * d))


def test_omic_snn_streams_stay_in_their_span_and_apart():
    lib = L.lib()
    off = 4242
    for (d, _), ns, groups in itertools.product(WIDTHS, (1, 5, 32, 64), (1, 4, 6)):
        span = lib.mpo_omic_snn_rng_span(ns, groups, d)
        assert span == R.snn_span(ns, groups, d)
        sites = [(lo, hi, (g, l)) for g, l, lo, hi in R.snn_sites(ns, groups, d, off)]
        what = dict(d=d, slides=ns, groups=groups)
        _inside(sites, off, span, what)
        _disjoint(sites, what)


def test_successive_calls_and_epochs_do_not_share_counters():
    """ops._reserve hands out [off, off + span] per call; an epoch moves every stream by 2^40 counters, more than any
    geometry of the grid reserves, so epoch e's streams never reach epoch e + 1's."""
    from multimodal_path_omic_amd import ops
    was = ops._rng_calls
    try:
        ops._rng_calls = 100
        _, a = ops._reserve(R.encoder_span(2, 6, 256, 512, 2))
        _, b = ops._reserve(R.pool_span(2, 6, 256))
        assert a == 100 and b == a + R.encoder_span(2, 6, 256, 512, 2) + 1
    finally:
        ops._rng_calls = was
    assert R.encoder_span(64, 2050, 512, 512, 2) < R.EPOCH_STRIDE
    assert R.pool_span(2 * 64, 2050, 512) < R.EPOCH_STRIDE
