"""Harrell's C on the device (harness.concordance_index_device, csrc/concordance.hip) against integer counts formed here by
numpy from the pair predicates (EQUAL, not close: the kernel counts in integers) and against the two host forms
(oracle.mpo_oracle.concordance_index_censored, harness.concordance_index_censored; within 1e-15: one fp64 division of
exactly representable terms).  Sizes: 1, 2, 3; the kernel's tile T at T - 1, T, T + 1, 2 T + 1; 1000; and 4097, the first size
at which a workgroup walks more than one tile of j.  Inputs: integer months (many ties in time, with and without events at
the tied times), risks quantised to 1/8 (many exact ties), risks of magnitude 1e-9 spaced 3e-9 and 3e-8 apart (the tolerance
decides), all censored (no comparable pair: NaN), none censored, one NaN risk; censorship is 0.0 / 1.0 throughout."""
import warnings

import numpy as np
import pytest
import torch

from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import harness
from oracle import mpo_oracle as O

pytestmark = pytest.mark.gpu

T = L.lib().mpo_concordance_tile() if torch.cuda.is_available() else 256
SIZES = [1, 2, 3, T - 1, T, T + 1, 2 * T + 1, 1000, 4097]
KINDS = ["month_ties", "tolerance", "all_censored", "none_censored", "one_nan"]


def make_case(kind, n, seed=0):
    """-> censorship fp32, time fp64, risk fp32 (numpy)."""
    g = np.random.default_rng(1000 * n + seed)
    time = g.integers(1, 13, n).astype(np.float64)                       # months 1..12: ties from n = 13 on at the latest
    cens = (g.random(n) < 0.4).astype(np.float32)
    risk = (g.integers(-16, 17, n) / 8.0).astype(np.float32)
    if kind == "tolerance":
        # multiples of 3e-9 (even subjects) and of 3e-8 (odd): differences of 3e-9, 6e-9, 9e-9 tie, 1.2e-8 and up do not;
        # no difference comes nearer to 1e-8 than 1e-9, a million times fp32's rounding of these values
        k = g.integers(0, 7, n)
        risk = np.where(np.arange(n) % 2 == 0, k * 3e-9, k * 3e-8).astype(np.float32)
    elif kind == "all_censored":
        cens[:] = 1.0
    elif kind == "none_censored":
        cens[:] = 0.0
    elif kind == "one_nan":
        risk[n // 2] = np.nan
        cens[n // 2] = 0.0                                               # (the NaN subject starts pairs of its own)
    return cens, time, risk


def counts_by_numpy(cens, time, risk):
    """concordant, tied, comparable over every ordered pair, from the predicates as the header states them."""
    event = (np.float32(1.0) - cens) != 0
    r = risk.astype(np.float64)
    comparable = event[:, None] & ((time[None, :] > time[:, None]) | ((time[None, :] == time[:, None]) & ~event[None, :]))
    np.fill_diagonal(comparable, False)
    with np.errstate(invalid="ignore"):
        diff = r[:, None] - r[None, :]
        tie = np.abs(diff) <= 1e-8
        concordant = comparable & (diff > 0) & ~tie
    return [int(concordant.sum()), int((comparable & tie).sum()), int(comparable.sum())]


def on_device(dev, cens, time, risk):
    return torch.from_numpy(cens).to(dev), torch.from_numpy(time).to(dev), torch.from_numpy(risk).to(dev)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_counts_equal_numpy_and_the_index_equals_the_host_forms(dev, kind, n):
    cens, time, risk = make_case(kind, n)
    c_index, counts = harness.concordance_index_device(*on_device(dev, cens, time, risk))
    assert c_index.shape == (1,) and c_index.dtype == torch.float64 and c_index.is_cuda
    assert counts.shape == (3,) and counts.dtype == torch.int64 and counts.is_cuda
    want = counts_by_numpy(cens, time, risk)
    print(f"[concordance {kind} n={n}] counts {counts.tolist()} (numpy {want}), c_index {float(c_index)!r}")
    assert counts.tolist() == want
    event = (1 - cens).astype(bool)
    result = harness.EvalResult(*[None] * 6, c_index, counts)
    if want[2] == 0:
        assert bool(torch.isnan(c_index).all())
        for host in (O.concordance_index_censored, harness.concordance_index_censored):
            with pytest.raises(ValueError, match="no comparable pairs"):
                host(event, time, risk)
        with pytest.raises(ValueError, match="no comparable pairs"):
            result.c_index_value()
        return
    assert kind != "all_censored"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                   # (numpy on the NaN risk)
        refs = [O.concordance_index_censored(event, time, risk), harness.concordance_index_censored(event, time, risk)]
    for ref in refs:
        assert abs(float(c_index) - ref) <= 1e-15, (float(c_index), ref)
    assert result.c_index_value() == float(c_index)


def test_the_cases_hold_what_they_are_meant_to():
    """Ties in time with and without an event at the tied time, exact risk ties, tolerance-decided pairs on both sides."""
    cens, time, risk = make_case("month_ties", 1000)
    event = cens == 0
    same_time = time[:, None] == time[None, :]
    assert (same_time & event[:, None] & event[None, :]).sum() > 1000 and (same_time & event[:, None] & ~event[None, :]).sum() > 1000
    assert counts_by_numpy(cens, time, risk)[1] > 1000
    cens, time, risk = make_case("tolerance", 1000)
    diff = np.abs(risk.astype(np.float64)[:, None] - risk.astype(np.float64)[None, :])
    assert ((diff > 0) & (diff <= 1e-8)).sum() > 1000 and ((diff > 1e-8) & (diff < 2e-8)).sum() > 1000
    assert np.abs(diff - 1e-8).min() > 5e-10


def test_two_calls_return_identical_bits_and_time_is_converted(dev):
    cens, time, risk = on_device(dev, *make_case("month_ties", 4097, seed=1))
    a, b = harness.concordance_index_device(cens, time, risk), harness.concordance_index_device(cens, time, risk)
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[1], b[1])
    c = harness.concordance_index_device(cens.double(), time.float(), risk.double())      # integer months: exact in fp32
    assert torch.equal(a[0].view(torch.int64), c[0].view(torch.int64)) and torch.equal(a[1], c[1])


def test_no_host_sync_and_capturable(dev):
    cens, time, risk = on_device(dev, *make_case("month_ties", 1000, seed=2))
    harness.concordance_index_device(cens, time, risk)                    # (allocator warm)
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            int(probe)                                                    # the mode is honoured: a synchronising call raises
        c_index, counts = harness.concordance_index_device(cens, time, risk)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert counts.tolist() == counts_by_numpy(*make_case("month_ties", 1000, seed=2))
    # inside a HIP graph: the replay follows the risks it reads
    static_risk = risk.clone()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        harness.concordance_index_device(cens, time, static_risk)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        g_index, g_counts = harness.concordance_index_device(cens, time, static_risk)
    graph.replay()
    assert torch.equal(g_counts, counts) and torch.equal(g_index, c_index)
    static_risk.copy_(-risk)
    graph.replay()
    flipped = harness.concordance_index_device(cens, time, -risk)
    assert torch.equal(g_counts, flipped[1]) and torch.equal(g_index, flipped[0]) and not torch.equal(g_counts, counts)


def test_host_known_mistakes_raise(dev):
    cens, time, risk = on_device(dev, *make_case("month_ties", 10))
    with pytest.raises(ValueError, match="GPU"):
        harness.concordance_index_device(cens.cpu(), time, risk)
    with pytest.raises(ValueError, match="GPU"):
        harness.concordance_index_device(cens, time.cpu().numpy(), risk)
    with pytest.raises(ValueError, match="9 times"):
        harness.concordance_index_device(cens, time[:9], risk)
    with pytest.raises(ValueError, match="at least one"):
        harness.concordance_index_device(cens[:0], time[:0], risk[:0])
