"""For tests/test_stratify_cpu.py: the cases, an EXACT restatement of harness.risk_stratification's definition in
fractions.Fraction (integers, order statistics and rational arithmetic only: no rounding anywhere, so it is the measure for
any floating-point implementation, whatever the order of its sums and products) and the bars such an implementation is held to.

Bars (u = 2^-53, one rounding of fp64 to nearest):
  surv   a product of k factors is k divisions and k - 1 multiplications (1.0 * f is exact): 2k - 1 roundings, and the exact
         value is rounded once more to be an fp64 reference: within (2k + 1) u relative, first order; the second-order
         part, below (2k u)^2, is beneath one u of the bar's two spare for any k below 2^25.  Exactly 0 or 1 where the exact
         value is: a factor of 0 is the exact quotient 0 / n, and no factor means no operation.
  E1     one rounding per term (d * n_1 is an exact integer below 2^48, then one division); V: q, 1 - q, d * q, * (1 - q),
         * (n - d), / (n - 1): six per term.  Adding the m_u terms (every other
         summand is 0.0, exact) rounds at most m_u - 1 times whatever the order, all terms >= 0: within (m_u + 6) u of the
         sum, first order; the bar is (m_u + 8) u of the exact sum.
"""
import bisect
import math
import os
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["continuous", "month_ties", "all_censored", "all_events", "equal_times", "equal_risks", "nans"]
GIVEN_CUTOFF = 0.125                         # a value the quantised risks take: subjects AT the cut-off, which are low
MODES = [(kind, mode) for kind in KINDS for mode in ("median", "given")] + [("month_ties", "above_all")]


def freireich():
    """-> censorship fp32, weeks fp64, risk fp32 (placebo 1, 6-MP 0: the median, 0.5, cuts between the arms) of Freireich et
    al. 1963, 42 leukaemia patients (tests/golden/freireich_1963.csv)."""
    rows = np.loadtxt(os.path.join(ROOT, "tests", "golden", "freireich_1963.csv"), delimiter=",", skiprows=1)
    assert rows.shape == (42, 3)
    return rows[:, 1].astype(np.float32), rows[:, 0].astype(np.float64), rows[:, 2].astype(np.float32)


def make_case(kind, n, seed=0):
    """-> censorship fp32, time fp64, risk fp32 (numpy)."""
    g = np.random.default_rng(7000 * n + seed)
    time = g.integers(1, 13, n).astype(np.float64)                       # months 1..12: heavy ties
    cens = (g.random(n) < 0.4).astype(np.float32)
    risk = (g.integers(-16, 17, n) / 8.0).astype(np.float32)             # quantised: ties at the median and at GIVEN_CUTOFF
    risk[risk == 0] = np.where(g.random(int((risk == 0).sum())) < 0.5, np.float32(-0.0), np.float32(0.0))      # a +-0 mix
    if kind == "continuous":
        time = g.exponential(30.0, n)
        risk = g.standard_normal(n).astype(np.float32)
    elif kind == "all_censored":
        cens[:] = 1.0
    elif kind == "all_events":
        cens[:] = 0.0
    elif kind == "equal_times":
        time[:] = 7.0
    elif kind == "equal_risks":
        risk[:] = 0.375                                                  # nobody is above the median: the high group is empty
    elif kind == "nans":
        risk[[n // 2, n // 3]] = np.nan
        time[n - 1] = np.nan
    return cens, time, risk


def cutoff_of(mode, risk):
    """None (the median) or the given cut-off as a Python float."""
    if mode == "median":
        return None
    return GIVEN_CUTOFF if mode == "given" else float(np.nanmax(risk)) + 1.0 if not np.isnan(risk).all() else 1.0


def exact(cens, time, risk, cutoff=None):
    """harness.risk_stratification's definition in exact arithmetic -> dict: cutoff (float: the one rounding the definition makes), group,
    at_risk, deaths (lists / lists per group), sizes, o1, and as Fractions e1, v and per group `steps` = [(event time, S_g
    from it on, number of factors)] in ascending time."""
    n = len(risk)
    time = [float(x) for x in time]
    event = [bool((np.float32(1.0) - np.float32(c)) != 0) for c in cens]
    r = [float(np.float32(x)) + 0.0 for x in risk]
    valid = [not (math.isnan(r[i]) or math.isnan(time[i])) for i in range(n)]
    if cutoff is None:
        s = sorted(r[i] for i in range(n) if valid[i])
        m = len(s)
        cut = float((Fraction(s[(m - 1) // 2]) + Fraction(s[m // 2])) / 2) if m else float("nan")
    else:
        cut = float(cutoff)
    group = [(1 if r[i] > cut else 0) if valid[i] else -1 for i in range(n)]
    at_risk, deaths, steps, sorted_times, event_counts = [], [], [], [], []
    for g in (0, 1):
        times = sorted(time[i] for i in range(n) if group[i] == g)
        counts = {}
        for i in range(n):
            if group[i] == g and event[i]:
                counts[time[i]] = counts.get(time[i], 0) + 1
        at_risk.append([len(times) - bisect.bisect_left(times, time[i]) if valid[i] else 0 for i in range(n)])
        deaths.append([counts.get(time[i], 0) if valid[i] else 0 for i in range(n)])
        product, k, curve = Fraction(1), 0, []
        for u in sorted(counts):
            at = len(times) - bisect.bisect_left(times, u)
            product, k = product * Fraction(at - counts[u], at), k + 1
            curve.append((u, product, k))
        steps.append(curve)
        sorted_times.append(times)
        event_counts.append(counts)
    o1, e1, v = 0, Fraction(0), Fraction(0)
    pooled = sorted(set(event_counts[0]) | set(event_counts[1]))
    for u in pooled:
        n0, n1 = (len(t) - bisect.bisect_left(t, u) for t in sorted_times)
        d0, d1 = (c.get(u, 0) for c in event_counts)
        nn, dd = n0 + n1, d0 + d1
        o1 += d1
        e1 += Fraction(dd * n1, nn)
        if nn > 1:
            v += Fraction(dd * n1 * (nn - n1) * (nn - dd), nn * nn * (nn - 1))
    sizes = [group.count(0), group.count(1), group.count(-1), len(pooled)]
    return dict(cutoff=cut, group=group, at_risk=at_risk, deaths=deaths, steps=steps, sizes=sizes, o1=o1, e1=e1, v=v, time=time, valid=valid)


def surv_reference(ex):
    """-> (ref, bar): (2, n) fp64, the exact S_g(t_i) rounded once (NaN for an excluded subject) and the relative bar
    (2k + 1) u of every element (0 where the exact value is 0 or 1 with no factor)."""
    n = len(ex["group"])
    ref, bar = np.full((2, n), np.nan), np.zeros((2, n))
    for g in (0, 1):
        times = [u for u, _, _ in ex["steps"][g]]
        values = [(1.0, 0)] + [(float(p), k) for _, p, k in ex["steps"][g]]
        for i in range(n):
            if ex["valid"][i]:
                value, k = values[bisect.bisect_right(times, ex["time"][i])]
                ref[g, i], bar[g, i] = value, (2 * k + 1) * U if 0.0 < value < 1.0 else 0.0
    return ref, bar


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def check_against_exact(got, ex, what):
    """got: a harness.StratResult against exact() -> the relative difference of its p from libm's on its own chi2, or None."""
    assert bits(got.cutoff)[0] == bits([ex["cutoff"]])[0], (what, float(got.cutoff[0]), ex["cutoff"])
    assert got.group.dtype == np.int32 and got.group.tolist() == ex["group"], what
    assert got.at_risk.dtype == np.int32 and got.at_risk.tolist() == ex["at_risk"], what
    assert got.deaths.dtype == np.int32 and got.deaths.tolist() == ex["deaths"], what
    assert got.sizes.dtype == np.int64 and got.sizes.tolist() == ex["sizes"], what
    o1, e1, v, chi2, p = (float(x) for x in got.logrank)
    assert o1 == ex["o1"], what
    ref, bar = surv_reference(ex)
    assert got.surv.shape == ref.shape and np.array_equal(np.isnan(got.surv), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    err = np.abs(got.surv[ok] - ref[ok])
    assert (err <= bar[ok] * ref[ok]).all(), (what, float((err / np.maximum(ref[ok], 1e-300)).max()))
    m_u = ex["sizes"][3]
    for name, have, want in (("E1", e1, ex["e1"]), ("V", v, ex["v"])):
        assert abs(Fraction(have) - want) <= Fraction((m_u + 8) * U) * want, (what, name, have, float(want))
    if ex["sizes"][0] == 0 or ex["sizes"][1] == 0 or ex["v"] == 0:
        assert math.isnan(chi2) and math.isnan(p), what
        return None
    x = o1 - e1
    assert chi2 == (x * x) / v, (what, chi2, (x * x) / v)      # (O1 - E1)^2 / V from the result's OWN sums, the square one product
    want_p = math.erfc(math.sqrt(chi2 / 2.0))
    return abs(p - want_p) / want_p if want_p >= 1e-300 else None
