"""Every body of the fp32 GEMM launcher (csrc/gemm_f32.hip) at the edges of its dispatch predicates, against fp64.

The launcher sends a product to one of five bodies ("fp32 GEMM routing"): general with 4 or 8 k-blocks in
flight, fast (branch-free), rows (32 x 64 tiles) and longk (K slices, atomic adds).  The three linear entries are called
directly through L.call, so that alpha, accumulate, a null bias, a null dbias and the pointer alignment are the test's:
    forward  y  = act(alpha (x W^T + b))     M = R, N = O, K = I     (layout 3)
    input    dx (+)= alpha dy W              M = R, N = I, K = O     (layout 2)
    weight   dW = alpha dy^T x, db = colsum  M = O, N = I, K = R     (layout 0)
Each case states the body it expects per entry and compares it with mpo_gemm_last_route(): a predicate that moves a case
to another body fails here, and the table below is then edited on purpose.  Every tensor lives inside a larger device
buffer filled with a sentinel; "unaligned" views start one float after a 16-byte boundary.  After the three calls the
surroundings of every tensor, and the inputs themselves, must be bit-unchanged.  The reference is the same product in fp64
on the CPU from the fp32 inputs.

Bars (max |got - ref| / max |ref| per tensor, those of test_linear_matches_torch and test_many_row_products_equal_torch):
1e-5 for y, dx and dW / db with K < 2048, 1e-4 for dW / db with K >= 2048.  Worst error per body over all cases of this
file, measured on an MI355X (printed by test_route_summary_covers_every_body_per_entry):
    general nb4 4.4e-07   general nb8 8.6e-07   fast 9.6e-07   rows 2.9e-07      (bar 1e-5; the two largest are tanh outputs)
    longk 3.2e-07 (bar 1e-4 from K = 2048 on)
    fusion head, 2048 / 2049 slides: forward 2.2e-07 (bar 1e-4), gradients 3.1e-07 (bar 2e-3)
The controls shift one column of the reference's weight (of x for the weight gradient) by one row and must miss the bar by
>= 100 x; measured 3.8e3 x (general nb8) to 4.2e4 x (general nb4).

Grouped launches whose members leave for rows / longk are driven through ops.fusion_head_cat at the end of the file.
"""
from collections import namedtuple

import pytest
import torch
import torch.nn as nn

from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.fusion import ConcatFusion

pytestmark = pytest.mark.gpu

NB4, NB8, FAST, ROWS, LONGK = "general_nb4", "general_nb8", "fast", "rows", "longk"
ENTRIES = ("fwd", "dx", "dw")
TOL, TOL_LONG_K = 1e-5, 1e-4
SENTINEL = 1.0e30
ACTS = {"none": lambda t: t, "relu": torch.relu, "elu": nn.functional.elu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}

# un: which tensors are only 4-byte aligned -- "x", "w", "dy", "dyx" (dy and x) or "out" (y, dx, dW and db)
Case = namedtuple("Case", "R I O fwd dx dw un act alpha acc bias dbias", defaults=(None, "none", 1.0, 0, True, True))


def _id(c):
    s = f"{c.R}x{c.I}x{c.O}"
    if c.un:
        s += f"-un_{c.un}"
    if c.act != "none":
        s += f"-{c.act}"
    if c.alpha != 1.0:
        s += f"-alpha{c.alpha:g}"
    return s + ("-acc" if c.acc else "") + ("" if c.bias else "-nobias") + ("" if c.dbias else "-nodbias")


CASES = [
    # ---- tiny / irregular: the general body ((7, 12, 20): K < 16 with lda % 4 == 0; (33, 512, 4) and (7, 20, 272): K > 256)
    Case(1, 1, 1, NB4, NB4, NB4), Case(1, 256, 1, NB4, NB4, NB4), Case(7, 12, 20, NB4, NB4, NB4),
    Case(15, 16, 16, NB4, NB4, NB4), Case(17, 16, 16, NB4, NB4, NB4), Case(16, 15, 16, NB4, NB4, NB4),
    Case(16, 16, 20, NB4, NB4, NB4), Case(33, 512, 4, NB8, NB4, NB4),
    Case(7, 20, 272, NB4, NB8, NB4),                       # (added: the only general nb8 product in the dx layout)
    # ---- fast, k-block edges: K = 16 leaves three waves without a block; 256 -> 272 switches 4 to 8 blocks in flight;
    #      per-wave block counts 5 (K = 272, last wave 2), 7 (448), 8 (512), 17 (1040, last wave 14)
    Case(16, 16, 16, FAST, FAST, FAST), Case(16, 256, 16, FAST, FAST, FAST), Case(16, 272, 16, FAST, FAST, FAST),
    Case(16, 448, 16, FAST, FAST, FAST), Case(16, 512, 16, FAST, FAST, FAST), Case(16, 1040, 16, FAST, FAST, FAST),
    Case(192, 256, 768, FAST, FAST, FAST),
    # ---- regular shapes, one operand 4-byte aligned: general for the entries that read it; only the outputs: still fast
    Case(16, 256, 16, NB4, FAST, NB4, un="x"), Case(16, 256, 16, NB4, NB4, FAST, un="w"),
    Case(16, 256, 16, FAST, NB4, NB4, un="dy"), Case(16, 256, 16, FAST, FAST, FAST, un="out"),
    Case(192, 256, 256, NB4, FAST, NB4, un="x"), Case(192, 256, 256, NB4, NB4, FAST, un="w"),
    Case(192, 256, 256, FAST, NB4, NB4, un="dy"), Case(192, 256, 256, FAST, FAST, FAST, un="out"),
    # ---- rows: M = 511 / 512 / 513 (the last workgroup owns one row), odd k-blocks per wave (K = 64, 192, 320),
    #      N or K off the 64-grid, unaligned operands (dx loads W as strided scalars: an unaligned W keeps it on rows)
    Case(511, 64, 64, NB4, NB4, NB8), Case(512, 64, 64, ROWS, ROWS, FAST), Case(513, 64, 64, ROWS, ROWS, NB8),
    Case(515, 192, 128, ROWS, ROWS, NB8), Case(1030, 320, 64, ROWS, ROWS, NB8),
    Case(512, 64, 48, FAST, FAST, FAST), Case(512, 48, 64, FAST, FAST, FAST),
    Case(512, 64, 64, NB4, ROWS, NB8, un="x"), Case(512, 64, 64, NB4, ROWS, FAST, un="w"),
    Case(512, 64, 64, ROWS, NB4, NB8, un="dy"), Case(513, 64, 64, ROWS, ROWS, NB8, un="out"),
    # ---- longk (dW, db): K = 2047 / 2048 / 2049 (the last slice holds one row), M or N it must refuse, scalar loads of
    #      unaligned operands; each with and without a bias gradient
    Case(2047, 64, 32, NB4, NB4, NB8), Case(2048, 64, 32, FAST, FAST, LONGK), Case(2049, 64, 32, NB4, NB4, LONGK),
    Case(2567, 128, 64, ROWS, ROWS, LONGK), Case(2048, 64, 48, FAST, FAST, FAST), Case(2048, 80, 32, FAST, FAST, FAST),
    Case(2049, 64, 32, NB4, NB4, LONGK, un="dyx"), Case(2049, 64, 32, NB4, NB4, LONGK, un="out"),
    Case(2047, 64, 32, NB4, NB4, NB8, dbias=False), Case(2048, 64, 32, FAST, FAST, LONGK, dbias=False),
    Case(2049, 64, 32, NB4, NB4, LONGK, dbias=False), Case(2567, 128, 64, ROWS, ROWS, LONGK, dbias=False),
    Case(2048, 64, 48, FAST, FAST, FAST, dbias=False), Case(2048, 80, 32, FAST, FAST, FAST, dbias=False),
    Case(2049, 64, 32, NB4, NB4, LONGK, un="dyx", dbias=False),
    # ---- a null bias, once per forward body
    Case(7, 12, 20, NB4, NB4, NB4, bias=False), Case(33, 512, 4, NB8, NB4, NB4, bias=False),
    Case(16, 272, 16, FAST, FAST, FAST, bias=False), Case(513, 64, 64, ROWS, ROWS, NB8, bias=False),
    # ---- accumulate = 1 on dx: general, fast, rows
    Case(7, 12, 20, NB4, NB4, NB4, acc=1), Case(16, 272, 16, FAST, FAST, FAST, acc=1),
    Case(513, 64, 64, ROWS, ROWS, NB8, acc=1),
]
# ---- every activation once per forward body
for _act in ("relu", "elu", "tanh", "sigmoid"):
    CASES += [Case(7, 12, 20, NB4, NB4, NB4, act=_act), Case(33, 512, 4, NB8, NB4, NB4, act=_act),
              Case(192, 256, 768, FAST, FAST, FAST, act=_act), Case(513, 64, 64, ROWS, ROWS, NB8, act=_act)]
# ---- alpha != 1 on one case of every body, all three entries (with accumulate on dx for alpha = -2: old values unscaled)
for _alpha in (0.5, -2.0):
    _acc = int(_alpha < 0)
    CASES += [Case(7, 12, 20, NB4, NB4, NB4, alpha=_alpha, acc=_acc), Case(33, 512, 4, NB8, NB4, NB4, alpha=_alpha),
              Case(7, 20, 272, NB4, NB8, NB4, alpha=_alpha), Case(16, 272, 16, FAST, FAST, FAST, alpha=_alpha, acc=_acc),
              Case(515, 192, 128, ROWS, ROWS, NB8, alpha=_alpha, acc=_acc), Case(2049, 64, 32, NB4, NB4, LONGK, alpha=_alpha)]

# (entry, body) -> [cases asserted, worst error]: filled by the cases that ran, printed by the summary test
SEEN = {}


def _pad(cols):
    """floats kept free on either side of a tensor: at least one row, a multiple of 4 (the view stays 16-byte aligned)"""
    return max(64, (cols + 3) // 4 * 4 + 4)


class Placed:
    """A (rows, cols) fp32 tensor inside a larger device buffer filled with SENTINEL.  `data` is copied in; without
    data the tensor itself holds the sentinel too, so an element the kernel never writes cannot pass."""

    def __init__(self, dev, shape, data=None, unaligned=False):
        n = 1
        for s in shape:
            n *= s
        self.head = _pad(shape[-1]) + (1 if unaligned else 0)
        self.n = n
        self.buf = torch.full((self.head + n + _pad(shape[-1]),), SENTINEL, dtype=torch.float32, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf[self.head:self.head + n].view(shape)
        if data is not None:
            self.t.copy_(data)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == (4 if unaligned else 0)
        self.before = self.buf.clone()

    def surroundings_untouched(self):
        a, b = self.buf.view(torch.int32), self.before.view(torch.int32)
        return torch.equal(a[:self.head], b[:self.head]) and torch.equal(a[self.head + self.n:], b[self.head + self.n:])

    def untouched(self):
        return torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32))


def _inputs(c):
    """fp32 inputs of a case on the CPU (weights x 0.1, as the other linear tests have them)"""
    g = syn.rng(7000 + 31 * c.R + 7 * c.I + c.O)
    return dict(x=syn.normal(g, (c.R, c.I)), w=syn.normal(g, (c.O, c.I), 0.1), b=syn.normal(g, (c.O,)),
                dy=syn.normal(g, (c.R, c.O)), dx0=syn.normal(g, (c.R, c.I)))


def _reference(c, t, shift=None):
    """fp64 results of the three entries.  shift = "w" / "x": the control's deliberately wrong reference, column 0 of the
    weight (of x, for the weight gradient) moved down by one row."""
    x, w, b, dy, dx0 = (t[k].double() for k in ("x", "w", "b", "dy", "dx0"))
    if shift == "w":
        w = w.clone()
        w[:, 0] = torch.roll(w[:, 0], 1)
    if shift == "x":
        x = x.clone()
        x[:, 0] = torch.roll(x[:, 0], 1)
    y = ACTS[c.act](c.alpha * (x @ w.t() + (b if c.bias else 0.0)))
    dx = c.alpha * (dy @ w) + (dx0 if c.acc else 0.0)
    return dict(y=y, dx=dx, dw=c.alpha * (dy.t() @ x), db=dy.sum(0))


def _run(dev, c, t):
    """The three entries on the GPU -> results (CPU, fp64), the reported body per entry, the placed tensors."""
    lib = L.lib()
    un = c.un or ""
    x = Placed(dev, (c.R, c.I), t["x"], un in ("x", "dyx"))
    w = Placed(dev, (c.O, c.I), t["w"], un == "w")
    b = Placed(dev, (c.O,), t["b"])
    dy = Placed(dev, (c.R, c.O), t["dy"], un in ("dy", "dyx"))
    y = Placed(dev, (c.R, c.O), None, un == "out")
    dx = Placed(dev, (c.R, c.I), t["dx0"] if c.acc else None, un == "out")
    dw = Placed(dev, (c.O, c.I), None, un == "out")
    db = Placed(dev, (c.O,), None, un == "out")
    stream = L.stream_of(x.t)
    routes = {}
    L.call("mpo_linear_forward", L.ptr(x.t), L.ptr(w.t), L.ptr(b.t) if c.bias else None, L.ptr(y.t), c.R, c.I, c.O,
           float(c.alpha), L.ACT[c.act], stream)
    routes["fwd"] = lib.mpo_gemm_last_route()
    L.call("mpo_linear_backward_input", L.ptr(dy.t), L.ptr(w.t), L.ptr(dx.t), c.R, c.I, c.O, float(c.alpha), int(c.acc), stream)
    routes["dx"] = lib.mpo_gemm_last_route()
    L.call("mpo_linear_backward_weight", L.ptr(dy.t), L.ptr(x.t), L.ptr(dw.t), L.ptr(db.t) if c.dbias else None, c.R, c.I, c.O,
           float(c.alpha), stream)
    routes["dw"] = lib.mpo_gemm_last_route()
    torch.cuda.synchronize(dev)
    got = {k: p.t.detach().double().cpu() for k, p in (("y", y), ("dx", dx), ("dw", dw), ("db", db))}
    return got, routes, dict(x=x, w=w, b=b, dy=dy, y=y, dx=dx, dw=dw, db=db)


def _err(got, ref):
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_linear_entries_at_dispatch_edges(dev, c):
    """One case of the table: the body each entry reports, the three results against fp64 at the bars of the module
    docstring, and no store outside the outputs (sentinels around every tensor bit-unchanged, inputs bit-unchanged)."""
    t = _inputs(c)
    got, routes, placed = _run(dev, c, t)
    ref = _reference(c, t)
    expected = {e: L.GEMM_ROUTE[getattr(c, e)] for e in ENTRIES}
    assert routes == expected, (f"bodies taken {routes}, the table expects {expected} "
                                f"({ {v: k for k, v in L.GEMM_ROUTE.items()} })")
    for k in ("x", "w", "b", "dy"):
        assert placed[k].untouched(), f"input {k} or its surroundings were written"
    for k in ("y", "dx", "dw", "db"):
        assert placed[k].surroundings_untouched(), f"a store outside {k}"
    if not c.dbias:
        assert placed["db"].untouched(), "dbias = NULL, yet the bias gradient's buffer was written"
    tol_w = TOL_LONG_K if c.R >= 2048 else TOL
    errs = dict(y=_err(got["y"], ref["y"]), dx=_err(got["dx"], ref["dx"]), dw=_err(got["dw"], ref["dw"]))
    if c.dbias:
        errs["db"] = _err(got["db"], ref["db"])
    print(f"[gemm routes] {_id(c)}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()) + f"  bodies {routes}")
    for entry, e in (("fwd", errs["y"]), ("dx", errs["dx"]), ("dw", max(errs["dw"], errs.get("db", 0.0)))):
        seen = SEEN.setdefault((entry, getattr(c, entry)), [0, 0.0])
        seen[0] += 1
        seen[1] = max(seen[1], e)
    assert errs["y"] < TOL and errs["dx"] < TOL, errs
    assert errs["dw"] < tol_w and errs.get("db", 0.0) < tol_w, errs


CONTROLS = {NB4: Case(7, 12, 20, NB4, NB4, NB4), NB8: Case(33, 512, 4, NB8, NB4, NB4), FAST: Case(16, 272, 16, FAST, FAST, FAST),
            ROWS: Case(513, 64, 64, ROWS, ROWS, NB8), LONGK: Case(2049, 64, 32, NB4, NB4, LONGK)}


@pytest.mark.parametrize("body", list(CONTROLS))
def test_route_controls_shifted_reference_column_fails_by_100x(dev, body):
    """The slack of the bars is real: against a reference whose weight has ONE column moved down by one row (for longk,
    the body of weight gradients only, one column of x) the same output misses its bar by >= 100 x."""
    c = CONTROLS[body]
    t = _inputs(c)
    got, routes, _ = _run(dev, c, t)
    if body == LONGK:
        assert routes["dw"] == L.GEMM_ROUTE[LONGK]
        err, bar = _err(got["dw"], _reference(c, t, shift="x")["dw"]), TOL_LONG_K
    else:
        assert routes["fwd"] == L.GEMM_ROUTE[body]
        err, bar = _err(got["y"], _reference(c, t, shift="w")["y"]), TOL
    print(f"  control {body}: error {err:.2e} = {err / bar:.0f} x the bar {bar:.0e}")
    assert err >= 100 * bar, (body, err)


def test_route_summary_covers_every_body_per_entry():
    """The table asserts every body at least once for each entry that can reach it (rows needs a k-contiguous A: forward
    and dx; longk needs layout 0: dW), and prints what the cases of this run measured."""
    table = {(e, getattr(c, e)) for c in CASES for e in ENTRIES}
    want = {(e, r) for e in ("fwd", "dx") for r in (NB4, NB8, FAST, ROWS)} | {("dw", r) for r in (NB4, NB8, FAST, LONGK)}
    assert table == want, sorted(table ^ want)
    for (entry, body), (n, worst) in sorted(SEEN.items()):
        print(f"[gemm routes] summary: {entry:3s} on {body:11s} (code {L.GEMM_ROUTE[body]}): {n:3d} cases asserted, worst error {worst:.1e}")
    worst = {}
    for (entry, body), (n, e) in SEEN.items():
        worst[body] = max(worst.get(body, 0.0), e)
    print("[gemm routes] worst per body: " + ", ".join(f"{b} {e:.1e}" for b, e in sorted(worst.items())))


# ------------------------------------------------------------------------------------------- grouped launches
def _bit(*bodies):
    m = 0
    for b in bodies:
        m |= 1 << L.GEMM_ROUTE[b]
    return m


# n_slides -> bodies of the backward's three pair launches (din 512, hidden 256, dout 32, 4 classes):
#   first hidden layer: dx (M = n, N = 512, K = 256) leaves for rows, dW (K = n) for longk, both with a ReLU value gate;
#   dout layer: dW (M = 32, N = 256, K = n) leaves for longk, dx (K = 32 < 64) stays and the grid is recomputed for it alone:
#               fast at n = 2048, general nb4 at n = 2049 (M % 16 != 0);
#   classifier: whole (dW has M = 4, dx has K = 4): the general body, nb8 because the pair's largest K is n.
# longk takes any K >= 2048, so the weight gradients stay on it at n = 2049 (its last slice holds one row) and rows runs a
# ragged last block there.
GROUP_BODIES = {2048: (ROWS, LONGK, FAST, NB8), 2049: (ROWS, LONGK, NB4, NB8)}


@pytest.mark.parametrize("n_slides", list(GROUP_BODIES))
def test_grouped_launch_members_leave_for_rows_and_longk(dev, n_slides):
    """ops.fusion_head_cat forward + backward against the same MLP and survival head in fp64 torch, at the fusion head's
    bars (1e-4 forward, 2e-3 of each tensor's maximum for gradients), and the bodies its grouped backward launches used."""
    din, hidden, dout, n_classes = 512, 256, 32, 4
    shapes = {"fusion_layer.0.weight": (hidden, din), "fusion_layer.0.bias": (hidden,), "fusion_layer.2.weight": (dout, hidden),
              "fusion_layer.2.bias": (dout,), "weight": (n_classes, dout), "bias": (n_classes,)}
    sd = syn.fill_state_dict(shapes, 8800 + n_slides)
    fus = ConcatFusion(dims=[din // 2, din // 2], hidden_size=hidden, output_size=dout)
    cls = nn.Linear(dout, n_classes)
    fus.load_state_dict({k: v for k, v in sd.items() if k.startswith("fusion_layer.")}, strict=True)
    cls.load_state_dict({k: v for k, v in sd.items() if not k.startswith("fusion_layer.")}, strict=True)
    fus.to(dev), cls.to(dev)
    hcat = syn.normal(syn.rng(8900 + n_slides), (n_slides, din))
    lib = L.lib()

    hd = hcat.to(dev).requires_grad_(True)
    hz, sv, y = ops.fusion_head_cat(hd, fus, cls)
    assert lib.mpo_gemm_last_route() == L.GEMM_ROUTE[NB4]                # the classifier's forward: N = 4
    params = [dict(fus.named_parameters())[k] if k.startswith("fusion_layer.") else dict(cls.named_parameters())[k] for k in sd]
    lib.mpo_gemm_last_group_routes()                                      # discard what earlier launches left
    grads = torch.autograd.grad((hz * sv).sum() + y[:, 0].sum(), [hd] + params)
    torch.cuda.synchronize(dev)
    used = lib.mpo_gemm_last_group_routes()
    assert used == _bit(*GROUP_BODIES[n_slides]), (bin(used), bin(_bit(*GROUP_BODIES[n_slides])), L.GEMM_ROUTE)
    assert lib.mpo_gemm_last_group_routes() == 0                          # reading clears the mask

    p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    ho = hcat.double().requires_grad_(True)
    z1 = torch.relu(ho @ p["fusion_layer.0.weight"].t() + p["fusion_layer.0.bias"])
    z2 = torch.relu(z1 @ p["fusion_layer.2.weight"].t() + p["fusion_layer.2.bias"])
    logits = z2 @ p["weight"].t() + p["bias"]
    hz_o = torch.sigmoid(logits)
    sv_o = torch.cumprod(1 - hz_o, dim=1)
    y_o = torch.softmax(logits, dim=1)
    grads_o = torch.autograd.grad((hz_o * sv_o).sum() + y_o[:, 0].sum(), [ho] + [p[k] for k in sd])
    e_f = {n: _err(a.detach().double().cpu(), r.detach()) for n, a, r in (("hazards", hz, hz_o), ("survs", sv, sv_o), ("Y", y, y_o))}
    e_g = {n: _err(a.double().cpu(), r) for n, a, r in zip(["hcat"] + list(sd), grads, grads_o)}
    print(f"[gemm routes] fusion head n_slides={n_slides}: forward {max(e_f.values()):.1e}, gradients "
          f"{max(e_g.values()):.1e} ({max(e_g, key=e_g.get)}), bodies {bin(used)}")
    for n, e in e_f.items():
        assert e < 1e-4, (n, e)
    for n, e in e_g.items():
        assert e < 2e-3, (n, e)
