"""The non-finite tables (tests/nonfinite_cases.py) without a GPU: for every row the fp64 oracle alone behaves as
tests/test_gpu_nonfinite_sites.py assumes -- a NaN poisons the unit it is planted in, every unit without a plant stays finite,
a -inf logit is a weight of 0 and leaves its slide finite -- and the oracle's own primitives agree with the stock torch
modules on planted inputs.  The last tests hold the table to its axes: a row removed from it is reported."""
import pytest
import torch
import torch.nn as nn

import nonfinite_cases as N
from oracle import mpo_oracle as O

NAN, INF = float("nan"), float("inf")


def _finite(res, kinds=("out", "igrad", "pgrad")):
    return all(bool(torch.isfinite(t).all()) for k in kinds for t in getattr(res, k).values())


@pytest.mark.parametrize("name", list(N.SITES))
def test_oracle_behaves_as_the_gpu_test_assumes(name):
    site = N.SITES[name]
    inp = site.make()
    assert _finite(site.oracle(inp)), "the clean inputs already give a non-finite value"
    rows = N.rows_of(site)
    assert rows
    for row in rows:
        index, units = N.where(site, inp, row)
        assert inp[row.tensor].is_floating_point(), row
        ref = site.oracle(N.planted(inp, row.tensor, index, row.plant))
        # no leak: every unit without a plant is finite in every output and input gradient
        if units != N.ALL:
            n = next(iter(ref.out.values())).shape[0]
            others = torch.ones(n, dtype=torch.bool)
            others[units] = False
            for kind in ("out", "igrad"):
                for k, t in getattr(ref, kind).items():
                    assert not bool(N.unit_nonfinite(t)[others].any()), (row, kind, k)
            assert n == 1 or bool(N.clean_units(ref, units).any()), (row, "no clean unit is left to hold to a bar")
        # sigmoid(-inf) = 0 and exp(-inf) = 0: hazard 0, softmax weight 0, a finite slide (the eps clamps take the logs).  Not at
        # the label's own column under `ces`: hazard 0 there is surv 1, and log(1 - S[y]) = -inf in the oracle too.
        weight_zero = row.tensor == "logits" and row.plant == "-inf" and not (" ces " in row.site and row.pos.endswith("@label"))
        if weight_zero:
            assert _finite(ref, ("out", "igrad")), row
        elif row.plant == "nan":
            poisoned = [t for kind in ("out", "igrad") for t in getattr(ref, kind).values()]
            hit = torch.stack([N.unit_nonfinite(t) for t in poisoned]).any(0)
            if row.pos.endswith("@tail"):               # read only by a censored slide: the reference indexes predictions[label:]
                assert bool(hit[units[0]]) == bool(inp["cens"][units[0]]), row
                continue
            # (a parameter's element poisons its column in every unit)
            assert all(bool(hit[u]) for u in (range(len(hit)) if units == N.ALL else units)), (row, "the NaN does not reach the oracle's outputs")


def test_oracle_primitives_agree_with_stock_torch_modules_on_planted_inputs():
    """relu, clamp, elu, softmax, layer_norm and sigmoid: what the oracle is made of against nn modules, with a NaN, a +Inf
    and a -Inf planted, position by position (NaN == NaN here)."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 9, generator=g, dtype=torch.float64)
    for plant in N.PLANTS.values():
        xp = x.clone()
        xp[1, 3] = plant
        w, b = torch.randn(9, generator=g, dtype=torch.float64), torch.randn(9, generator=g, dtype=torch.float64)
        ln = nn.LayerNorm(9).double()
        with torch.no_grad():
            ln.weight.copy_(w)
            ln.bias.copy_(b)
        pairs = {"relu": (torch.relu(xp), nn.ReLU()(xp)), "elu": (O._elu(xp), nn.ELU()(xp)),
                 "sigmoid": (torch.sigmoid(xp), nn.Sigmoid()(xp)), "softmax": (torch.softmax(xp, 1), nn.Softmax(dim=1)(xp)),
                 "layer_norm": (O._layer_norm(xp, w, b), ln(xp).detach()),
                 "clamp": (xp.clamp(min=1e-7), torch.maximum(xp, torch.tensor(1e-7, dtype=torch.float64)))}
        for name, (a, r) in pairs.items():
            assert torch.equal(torch.isfinite(a), torch.isfinite(r)), (name, plant)
            torch.testing.assert_close(a, r, rtol=1e-12, atol=1e-12, equal_nan=True, msg=f"{name} {plant}")
            assert bool(torch.isfinite(a[[0, 2, 3]]).all()), (name, plant, "the plant left its row")
    # what the kernels are held to, spelled out once
    t = torch.tensor([NAN, INF, -INF], dtype=torch.float64)
    assert torch.isnan(torch.relu(t)[0]) and torch.relu(t)[1] == INF and torch.relu(t)[2] == 0
    assert torch.isnan(t.clamp(min=1e-7)[0]) and t.clamp(min=1e-7)[2] == 1e-7
    assert torch.isnan(O._elu(t)[0]) and O._elu(t)[2] == -1
    assert torch.isnan(torch.sigmoid(t)[0]) and torch.sigmoid(t)[1] == 1 and torch.sigmoid(t)[2] == 0
    sm = torch.softmax(torch.tensor([[0.0, -INF, 1.0], [0.0, INF, 1.0], [0.0, NAN, 1.0]], dtype=torch.float64), 1)
    assert bool(torch.isfinite(sm[0]).all()) and sm[0, 1] == 0 and bool(torch.isnan(sm[1:]).all())


def test_relu_backward_passes_a_gradient_at_a_nan():
    """Why backward is compared at tensor level only: torch's threshold backward sends the gradient through where the saved
    activation is NaN (NaN <= 0 is false); the kernels' gate (v > 0) sends 0."""
    x = torch.tensor([NAN, -1.0, 2.0], dtype=torch.float64, requires_grad=True)
    torch.relu(x).backward(torch.tensor([5.0, 5.0, 5.0], dtype=torch.float64))
    assert x.grad.tolist() == [5.0, 0.0, 5.0]


def test_table_reaches_every_axis_value_and_a_removed_row_is_noticed():
    assert {tuple(r) for r in N.ROWS} == N.wanted() and len(N.ROWS) == len(N.wanted())
    for i in (0, len(N.ROWS) // 2, len(N.ROWS) - 1):
        rest = N.ROWS[:i] + N.ROWS[i + 1:]
        assert N.wanted() - {tuple(r) for r in rest} == {tuple(N.ROWS[i])}
    # every site plants all three kinds at its first and last unit, and a unit of a partial tile where it has one
    for s in N.SITES.values():
        rows = N.rows_of(s)
        assert {r.plant for r in rows} == set(N.PLANTS), s.name
        pos = {r.pos.split("/")[0].split("@")[0] for r in rows}
        assert {"first", "last", "partial"} <= pos or {"b0", "b1", "b2"} <= pos, (s.name, pos)
    # one site per GEMM body and entry, per pool family, per fusion and form, per loss and censoring state
    bodies = {(e, b) for s in N.LINEAR_SITES for e, b in zip(("fwd", "dx", "dw"), s.bodies)}
    assert bodies >= ({(e, b) for e in ("fwd", "dx") for b in ("general_nb4", "general_nb8", "fast", "rows")}
                      | {("dw", b) for b in ("general_nb4", "general_nb8", "fast", "longk")})
    assert {(s.act) for s in N.LINEAR_SITES} == set(N.ACTS)
    assert {s.family for s in N.POOL_SITES} == {"fused", "short", "long"} and any(s.p > 0 for s in N.POOL_SITES)
    assert {(s.fusion, s.form) for s in N.FUSION_SITES} == {(f, m) for f in ("concat", "gated_concat", "bilinear")
                                                            for m in ("plain", "ces", "sct")}
    assert {(s.kind, s.cens) for s in N.LOSS_SITES} == {(k, c) for k in ("ces", "sct") for c in (0, 1)}
    assert set(N.HEAD_LABEL.tolist()) >= {0, 2} and all(set(c.tolist()) == {0.0, 1.0} for c in N.HEAD_CENS)


def test_predicates_report_a_swallowed_and_a_leaked_value():
    """covers and clean_units_hold on hand-made results: a swallowed NaN, a leak and an error over the bar are each found."""
    ref = N.Result(dict(h=torch.tensor([[1.0, NAN], [2.0, 3.0]]), loss=torch.tensor([NAN, 1.0])), {}, dict(w=torch.tensor([NAN, 1.0])))
    same = N.Result(dict(h=torch.tensor([[INF, 0.0], [2.0, 3.0]]), loss=torch.tensor([NAN, 1.0])), {}, dict(w=torch.tensor([INF, 1.0])))
    bars = dict(h=lambda g, r: (float((g - r).abs().max()), 1e-3), loss=lambda g, r: (float((g - r).abs().max()), 1e-3))
    assert N.covers(same, ref) == [] and N.clean_units_hold(same, ref, [0], bars) == []
    swallowed = N.Result(dict(h=torch.tensor([[1.0, 0.0], [2.0, 3.0]]), loss=torch.tensor([0.5, 1.0])), {}, dict(w=torch.tensor([0.0, 1.0])))
    assert len(N.covers(swallowed, ref)) == 3
    leaked = N.Result(dict(h=torch.tensor([[NAN, NAN], [NAN, 3.0]]), loss=torch.tensor([NAN, 1.5])), {}, dict(w=torch.tensor([NAN, 1.0])))
    found = N.clean_units_hold(leaked, ref, [0], bars)
    assert len(found) == 2 and "leak" in found[0] and "off by" in found[1]
    assert N.clean_units(ref, N.ALL).tolist() == [False, False]
    # rule 3: a planted unit that the oracle leaves finite is held like a clean one -- a NaN or a wrong number there is found
    fin = N.Result(dict(h=torch.tensor([[1.0, 0.0], [2.0, 3.0]]), loss=torch.tensor([4.0, 1.0])), {}, {})
    assert N.held_units(fin, [0]).tolist() == [True, True] and N.clean_units(fin, [0]).tolist() == [False, True]
    assert N.clean_units_hold(fin, fin, [0], bars) == [] and N.clean_units_hold(fin, fin, N.ALL, bars) == []
    nan_there = N.Result(dict(h=torch.tensor([[NAN, 0.0], [2.0, 3.0]]), loss=torch.tensor([4.0, 1.0])), {}, {})
    wrong_there = N.Result(dict(h=torch.tensor([[1.0, 0.0], [2.0, 3.0]]), loss=torch.tensor([4.5, 1.0])), {}, {})
    for units in ([0], N.ALL):
        assert len(N.clean_units_hold(nan_there, fin, units, bars)) == 1 and "planted" in N.clean_units_hold(nan_there, fin, units, bars)[0]
        assert len(N.clean_units_hold(wrong_there, fin, units, bars)) == 1 and "off by" in N.clean_units_hold(wrong_there, fin, units, bars)[0]
