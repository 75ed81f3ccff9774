"""The buffer contract of the bag-side C entries: the case table, the placement helper and the ledger
(tests/test_gpu_buffer_contract.py runs the table on the GPU, tests/test_buffer_contract_cpu.py holds the ledger).  Plain
module, no GPU work at import.

The contract ("Buffer contract"): an entry writes nothing outside its outputs, `saved[0, saved_floats)` and
`workspace[0, workspace_bytes)`; it reads nothing it was not given or did not write in the same call; its size queries
suffice for every plan it accepts.

How a case holds an entry to it:
  * every tensor sits in an allocation of its own between two NaN guards (`Arena`); `saved` has exactly `*_saved_floats`
    floats, `workspace` exactly `*_workspace_bytes` bytes (passed as `workspace_bytes`), outputs their documented extent;
  * the call sequence runs twice from identical inputs, outputs / saved / workspace pre-filled with NaN, then with 1.0e30
    (tests/test_gpu_gemm_routes.py's SENTINEL).  After each run every guard and every pure input is bit-unchanged, every
    output finite and within the bar of the entry's own test file against fp64 (`oracle.mpo_oracle`, or the restatement
    that file uses, on the stored values the entry was given);
  * the two runs' outputs and the contents of `saved` are bit-equal: an element the call never wrote, or one computed from
    something it never wrote, holds another value under each fill.  The exception is an entry that adds floats atomically
    on the path taken; `Case.atomic` then names the file and line, and both runs meet the bar.
A backward case consumes the `saved` (and maps) its own forward wrote into the same arena; the workspace is filled again
between the two calls.

Windows: [1, 33, 700] (under the uniform cut the one-row slide owns five empty row ranges; a partial last tile; slide
boundaries off the 4-grid of the ragged maps), [257], [1, 33, 8300], and [1, 33, 8180] under the caller plan with the most
parts `check_plan` accepts: rows_per_wg = 32 and n_wg = mpo_coattn_target_workgroups() + n_slides = 259 (1 + 2 + 256
workgroups).  At 8300 rows a 32-row plan needs 263 workgroups, which `check_plan` refuses, so that window runs under the
project's own plan builder and the largest plan runs at 8180 rows (255 full tiles and one of 20 rows).

Bars are imported by name where the entry's test file names them; a bar that file states inline is restated here beside
its source line."""
import ctypes
import hashlib
import math
import zlib
from collections import namedtuple

import torch

import nonfinite_cases as N
import test_gpu_coattn_mcat as K1
import test_gpu_coattn_nacagat as K2
import test_gpu_gemm_routes as RT
import test_gpu_patch_epilogue as PE
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import ops
from oracle import mpo_oracle as O

NAN = float("nan")
FILLS = {"nan": NAN, "finite": RT.SENTINEL}
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
GUARD_ROWS = 64            # two 32-row tiles (tests/test_gpu_plan_cuts.py's GUARD); flat tensors: 64 elements
W_EDGES, W_ONE, W_LONG, W_MAX = (1, 33, 700), (257,), (1, 33, 8300), (1, 33, 8180)

# bars the entries' own files state inline (file: the assertion)
PATCH_H_BAR = 2.0 ** -7          # test_gpu_patch_widths.py: `assert err < 2.0 ** -7` (H_bag is bf16), test_gpu_patch_coattn.py:90
FUSED_OUT_BAR = 1e-3             # test_gpu_patch_coattn.py: `relmax(out, out_k) < 1e-3`, map `rel < 1e-3`, on the kernel's own H_bag
F32_FWD_ABS, F32_DW_REL, F32_DB_REL = 3e-6, 1e-4, 1e-5      # test_gpu_patch_fc_f32.py / _f16.py: `err < 3e-6`, `e_w < 1e-4 and e_b < 1e-5`
KEY_PROJ_BAR = 2e-6              # test_gpu_coattn_nacagat.py::test_key_projection_matches_fp32_linear: `err < 2e-6`
WGRAD_BAR = 2e-6                 # test_gpu_patch_wgrad.py: `err < 2e-6`
MAP_MEAN_REL = 1e-6              # test_gpu_map_stats.py: `abs(mean - ref) <= 1e-6 * abs(ref)`
COLSUM_OF_ROWS_REL = 1e-4        # test_gpu_coattn_mcat.py: `relerr(cs8, db8.sum(0)) < 1e-4` (column sums of the rows written)


# ------------------------------------------------------------------------------------------------------------- placement
def _ints(t):
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.int8}[t.element_size()])


def guard_elements(shape, dtype):
    """Elements of NaN on either side of a tensor: 64 rows of its own pitch for a 2-D tensor, 64 elements for a flat one,
    rounded up to whole 256-byte units (a multiple of 16 bytes: the view keeps the alignment the bag kernels require)."""
    elt = torch.empty((), dtype=dtype).element_size()
    n = GUARD_ROWS * (int(shape[-1]) if len(shape) == 2 else 1)
    unit = 256 // elt
    return -(-n // unit) * unit


class Arena:
    """Every tensor of one call sequence, each inside a device allocation of its own between two NaN guards -- what
    tail_helpers.Guarded and test_gpu_gemm_routes.Placed do, for fp32, bf16 and fp16 tensors of any shape, with the guards
    and the inputs compared bit for bit (integer views) against clones taken before the call, not with isnan.

    place(name, shape, dtype, data, role): role "in" (data given: must come back bit-unchanged), "out" (pre-filled by
    fill()), "inout" (arrives holding defined data the entry updates: d_query under d_query_accumulate; checked against the
    reference's updated value by the caller).  No tensor ends where its allocation ends.

    cu_rows, work plans, labels and other integer index arrays are NOT placed here, on purpose: a guard value beside them
    could only ever be read as an index, and this helper must never steer a kernel outside an allocation.  They stay in
    ordinary torch tensors."""

    def __init__(self, dev):
        self.dev, self.items = dev, []

    def place(self, name, shape, dtype=F32, data=None, role=None):
        shape = tuple(int(s) for s in shape)
        n = math.prod(shape)
        assert n > 0 and dtype in (F32, BF16, F16), (name, shape, dtype)
        g = guard_elements(shape, dtype)
        parent = torch.full((g + n + g,), NAN, device=self.dev, dtype=dtype)
        view = parent[g:g + n].view(shape)
        assert view.data_ptr() % 16 == 0 and (g * parent.element_size()) % 16 == 0
        if data is not None:
            view.copy_(data.reshape(shape).to(dtype))
        self.items.append(dict(name=name, parent=parent, g=g, n=n, view=view, role=role or ("in" if data is not None else "out")))
        return view

    def _item(self, view):
        return next(it for it in self.items if it["view"].data_ptr() == view.data_ptr())

    def fill(self, value, only=None):
        for it in self.items:
            if it["role"] == "out" and (only is None or any(it["view"].data_ptr() == v.data_ptr() for v in only)):
                it["view"].fill_(value)

    def seal(self):
        """Clones of every guard and every input, taken before the call."""
        torch.cuda.synchronize()
        for it in self.items:
            p, g, n = _ints(it["parent"]), it["g"], it["n"]
            it["guards"] = (p[:g].clone(), p[g + n:].clone())
            it["snap"] = p[g:g + n].clone() if it["role"] == "in" else None

    def freeze(self, *views):
        """An output of the previous call becomes an input of the next (saved, maps, H_bag)."""
        torch.cuda.synchronize()
        for v in views:
            if v is not None:
                it = self._item(v)
                it["role"], it["snap"] = "in", _ints(it["parent"])[it["g"]:it["g"] + it["n"]].clone()

    def check(self, what):
        torch.cuda.synchronize()
        for it in self.items:
            p, g, n = _ints(it["parent"]), it["g"], it["n"]
            for side, now, was in (("before", p[:g], it["guards"][0]), ("behind", p[g + n:], it["guards"][1])):
                if not torch.equal(now, was):
                    at = int((now != was).nonzero()[0])
                    raise AssertionError(f"{what}: the guard {side} {it['name']} changed ({int((now != was).sum())} elements, first at {at})")
            if it["snap"] is not None and not torch.equal(p[g:g + n], it["snap"]):
                raise AssertionError(f"{what}: input {it['name']} changed ({int((p[g:g + n] != it['snap']).sum())} elements)")

    def finite(self, what, **views):
        for name, v in views.items():
            if v is not None and not bool(torch.isfinite(v.float()).all()):
                bad = int((~torch.isfinite(v.float())).sum())
                raise AssertionError(f"{what}: output {name} holds {bad} non-finite elements of {v.numel()}")


# --------------------------------------------------------------------------------------------------------------- helpers
def relmax(got, ref):
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def relelem(got, ref):
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    return float(((got - ref).abs() / ref.abs().clamp_min(1e-30)).max())


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _cpu(outs):
    return {k: v.detach().cpu().clone() for k, v in outs.items() if v is not None}


def bit_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_ints(a.contiguous()), _ints(b.contiguous()))


def _uniform(g, shape, half_width):
    return (torch.rand(*shape, generator=g) - 0.5) * (2.0 * half_width)


def _code(dtype):
    return L.MPO_F32 if dtype == F32 else L.MPO_BF16


def halves(t):
    """[T, 512] -> the split-halves layout [2][T][256] of include/mpo_hip.h; narrower bags stay row-major."""
    return t.view(t.shape[0], 2, 256).permute(1, 0, 2).contiguous() if t.shape[1] == 512 else t


def unhalves(t, T, E):
    return t.reshape(2, T, 256).permute(1, 0, 2).reshape(T, E) if E == 512 else t.reshape(T, E)


def max_plan_starts(lengths, target):
    """wg_start of the plan with rows_per_wg = 32; its n_wg must be the most check_plan accepts."""
    starts = [0]
    for m in lengths:
        starts.append(starts[-1] + -(-m // 32))
    assert starts[-1] == target + len(lengths), (starts[-1], target, lengths)
    return starts


def make_plan(mode, lengths, cu, dev, keep):
    """-> the `plan` argument: None (NULL: the uniform cut of mpo_coattn_splits), the project's plan builder
    (ops.BagBatch.plan), or the caller plan of 32-row workgroups with n_wg at check_plan's upper bound.  `keep` holds what
    the pointer refers to."""
    if mode == "uniform":
        return None
    if mode == "built":
        batch = ops.BagBatch(torch.empty(sum(lengths), 1, device=dev), cu, list(lengths))
        keep.append(batch)
        return batch.plan()
    assert mode == "max", mode
    starts = max_plan_starts(lengths, L.lib().mpo_coattn_target_workgroups())
    wg = torch.tensor(starts, dtype=torch.int32).to(dev)
    c = L.BagPlanC(L.ptr(wg), starts[-1], 32)
    keep += [wg, c]
    return ctypes.byref(c)


class Knobs:
    """The library's kernel selectors for one case, restored on the way out (also when the case fails)."""

    def __init__(self, **values):
        self.values, self.prev = values, {}

    def __enter__(self):
        lib = L.lib()
        for name, v in self.values.items():
            self.prev[name] = getattr(lib, name)(int(v))
            assert getattr(lib, name)(int(v)) == int(v), name          # the selector took the value
        return self

    def __exit__(self, *exc):
        for name, v in self.prev.items():
            getattr(L.lib(), name)(v)


Run = namedtuple("Run", "outs errs")        # outs {name: CPU tensor}; errs {name: (error, bar)}: error < bar, or == 0 at bar 0
_REFS = {}


def _cached(key, make):
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def _blocks(flat, lengths, n_q):
    out, o = [], 0
    for m in lengths:
        out.append(flat[n_q * o:n_q * (o + m)].view(n_q, m))
        o += m
    return out


# ----------------------------------------------------------------------------------------------------------- K1 (MCAT)
def k1_bwd_kernel(dtype, E, n_q, d_amap, two_wave, f32_vector):
    """Which backward bag kernel a geometry takes (mpo_coattn_bwd8_covers / mpo_coattn_bwd_f32_covers, include/mpo_hip.h)."""
    if dtype == BF16 and E == 256 and n_q <= 8 and not d_amap and two_wave:
        return "two_wave"
    if dtype == F32 and E == 256 and n_q <= 8 and f32_vector:
        return "f32_vector"
    return "general"


def _coattn_params(g, E):
    return dict(in_w=_uniform(g, (3 * E, E), 1 / 16), in_b=_uniform(g, (3 * E,), 1 / 16), out_w=_uniform(g, (E, E), 1 / 16),
                out_b=_uniform(g, (E,), 1 / 16))


def _oracle_params(i):
    return {"co_attention.in_proj_weight": i["in_w"].double().requires_grad_(True),
            "co_attention.in_proj_bias": i["in_b"].double().requires_grad_(True),
            "co_attention.out_proj.weight": i["out_w"].double().requires_grad_(True),
            "co_attention.out_proj.bias": i["out_b"].double().requires_grad_(True)}


def _mcat_problem(lengths, dtype, E, n_q, d_amap, gate, acc):
    """Inputs on the CPU and the fp64 oracle (oracle.mpo_oracle.mcat_coattention slide by slide) on the stored values."""
    g = torch.Generator().manual_seed(_seed("mcat", lengths, str(dtype), E, n_q))
    T, R = sum(lengths), len(lengths) * n_q
    i = dict(bag=torch.relu(torch.randn(T, E, generator=g)).to(dtype), query=torch.randn(R, E, generator=g), **_coattn_params(g, E),
             d_out=torch.randn(R, E, generator=g), d_map=torch.randn(n_q * T, generator=g), d_query0=torch.randn(R, E, generator=g))
    p = _oracle_params(i)
    q, bag = i["query"].double().requires_grad_(True), i["bag"].double().requires_grad_(True)
    outs, maps, loss, o = [], [], 0.0, 0
    dmaps = _blocks(i["d_map"].double(), lengths, n_q)
    for b, m in enumerate(lengths):
        out_b, a_b = O.mcat_coattention(q[b * n_q:(b + 1) * n_q], bag[o:o + m], p)
        loss = loss + (out_b * i["d_out"][b * n_q:(b + 1) * n_q].double()).sum()
        if d_amap:
            loss = loss + (a_b * dmaps[b]).sum()
        outs.append(out_b.detach())
        maps.append(a_b.detach().reshape(-1))
        o += m
    gq, gb, gw, gbias, gow, gob = torch.autograd.grad(loss, [q, bag] + list(p.values()))
    if gate:
        gb = gb * (i["bag"].double() > 0) * gate
    gbias = gbias.clone()
    gbias[E:2 * E] = 0                                              # the key bias cancels in the softmax
    ref = dict(out=torch.cat(outs), attn_map=torch.cat(maps), d_query=gq + (i["d_query0"].double() if acc else 0), d_bag=gb,
               d_bag_colsum=gb.sum(0), d_in_w=gw, d_in_b=gbias, d_out_w=gow, d_out_b=gob)
    return i, ref


def mcat_forward_call(A, t, lengths, dtype, E, n_q, plan, cu):
    T = sum(lengths)
    L.call("mpo_coattn_mcat_forward", L.ptr(t["bag"]), _code(dtype), L.ptr(cu), len(lengths), T, max(lengths), L.ptr(t["query"]),
           n_q, E, L.ptr(t["in_w"]), L.ptr(t["in_b"]), L.ptr(t["out_w"]), L.ptr(t["out_b"]), L.ptr(t["out"]), L.ptr(t.get("attn_map")),
           L.ptr(t["saved"]), plan, L.ptr(t["workspace"]), t["workspace"].numel() * 4, L.stream_of(t["bag"]))


def mcat_place(dev, fill, i, lengths, dtype, E, n_q, amap, d_amap, colsum, acc, saved_short=0):
    """The arena of one MCAT forward + backward; `saved_short` floats are taken off the END of the saved view (the control:
    the overrun then lands in the guard of the same allocation)."""
    lib = L.lib()
    n_slides, T, R = len(lengths), sum(lengths), len(lengths) * n_q
    A = Arena(dev)
    t = dict(bag=A.place("bag", (T, E), dtype, i["bag"]), query=A.place("query", (R, E), data=i["query"]))
    for k in ("in_w", "in_b", "out_w", "out_b"):
        t[k] = A.place(k, i[k].shape, data=i[k])
    t["out"] = A.place("out", (R, E))
    if amap:
        t["attn_map"] = A.place("attn_map", (n_q * T,))
    t["saved"] = A.place("saved", (lib.mpo_coattn_saved_floats(n_slides, n_q, E) - saved_short,))
    ws_bytes = lib.mpo_coattn_workspace_bytes(n_slides, n_q, E, max(lengths))
    assert ws_bytes % 4 == 0
    t["workspace"] = A.place("workspace", (ws_bytes // 4,))
    t["d_out"] = A.place("d_out", (R, E), data=i["d_out"])
    if d_amap:
        t["d_attn_map"] = A.place("d_attn_map", (n_q * T,), data=i["d_map"])
    t["d_query"] = A.place("d_query", (R, E), data=i["d_query0"] if acc else None, role="inout" if acc else "out")
    t["d_bag"] = A.place("d_bag", (T, E), dtype)
    if colsum:
        t["d_bag_colsum"] = A.place("d_bag_colsum", (E,))
    for k, src in (("d_in_w", "in_w"), ("d_in_b", "in_b"), ("d_out_w", "out_w"), ("d_out_b", "out_b")):
        t[k] = A.place(k, i[src].shape)
    A.fill(fill)
    A.seal()
    return A, t


def run_mcat(dev, fill, lengths, dtype, E, n_q, amap, d_amap, colsum, gate, acc, plan, two_wave=1, f32_vector=1, kernel=None):
    assert amap or not d_amap
    assert kernel is None or kernel == k1_bwd_kernel(dtype, E, n_q, d_amap, two_wave, f32_vector), kernel
    i, ref = _cached(("mcat", lengths, dtype, E, n_q, d_amap, gate, acc), lambda: _mcat_problem(lengths, dtype, E, n_q, d_amap, gate, acc))
    A, t = mcat_place(dev, fill, i, lengths, dtype, E, n_q, amap, d_amap, colsum, acc)
    cu, keep = ops.make_cu(lengths, dev), []
    plan_p = make_plan(plan, lengths, cu, dev, keep)
    T = sum(lengths)
    with Knobs(mpo_set_coattn_bwd_two_wave=two_wave, mpo_set_coattn_bwd_f32_vector=f32_vector):
        mcat_forward_call(A, t, lengths, dtype, E, n_q, plan_p, cu)
        A.check("mpo_coattn_mcat_forward")
        A.finite("mpo_coattn_mcat_forward", out=t["out"], attn_map=t.get("attn_map"), saved=t["saved"])
        A.freeze(t["out"], t.get("attn_map"), t["saved"])
        A.fill(fill, only=[t["workspace"]])
        L.call("mpo_coattn_mcat_backward", L.ptr(t["bag"]), _code(dtype), L.ptr(cu), len(lengths), T, max(lengths), L.ptr(t["query"]),
               n_q, E, L.ptr(t["in_w"]), L.ptr(t["out_w"]), L.ptr(t["saved"]), L.ptr(t.get("attn_map")), L.ptr(t["d_out"]),
               L.ptr(t.get("d_attn_map")), L.ptr(t["d_query"]), int(acc), L.ptr(t["d_bag"]), L.ptr(t.get("d_bag_colsum")), L.ptr(t["d_in_w"]),
               L.ptr(t["d_in_b"]), L.ptr(t["d_out_w"]), L.ptr(t["d_out_b"]), float(gate), plan_p, L.ptr(t["workspace"]),
               t["workspace"].numel() * 4, L.stream_of(t["bag"]))
        A.check("mpo_coattn_mcat_backward")
    names = ["out", "attn_map", "saved", "d_query", "d_bag", "d_bag_colsum", "d_in_w", "d_in_b", "d_out_w", "d_out_b"]
    A.finite("mpo_coattn_mcat_backward", **{k: t.get(k) for k in names})
    outs = _cpu({k: t.get(k) for k in names})
    bag_bar = K1.GRAD_TOL if dtype == F32 else K1.BAG_GRAD_TOL_BF16          # d_bag is emitted in the bag's dtype
    errs = dict(out=(relmax(outs["out"], ref["out"]), K1.OUT_TOL), d_query=(relmax(outs["d_query"], ref["d_query"]), K1.GRAD_TOL),
                d_bag=(relmax(outs["d_bag"], ref["d_bag"]), bag_bar),
                key_bias_slice=(float(outs["d_in_b"][E:2 * E].abs().max()), 0.0))
    for k in ("d_in_w", "d_in_b", "d_out_w", "d_out_b"):
        errs[k] = (relmax(outs[k], ref[k]), K1.GRAD_TOL)
    if amap:
        errs["attn_map"] = (relelem(outs["attn_map"], ref["attn_map"]), K1.MAP_REL_TOL)
    if colsum:
        errs["d_bag_colsum"] = (relmax(outs["d_bag_colsum"], ref["d_bag_colsum"]), bag_bar)
        errs["colsum_of_rows"] = (relmax(outs["d_bag_colsum"], outs["d_bag"].double().sum(0)), COLSUM_OF_ROWS_REL)
    return Run(outs, errs)


# --------------------------------------------------------------------------------------------------- patch layer + K1, one call
def _patch_problem(lengths, pd, E, seed_key):
    g = torch.Generator().manual_seed(_seed(seed_key, lengths, pd, E))
    T = sum(lengths)
    x = torch.randn(T, pd, generator=g).to(BF16)
    w = torch.randn(E, pd, generator=g) / math.sqrt(pd)
    b = torch.randn(E, generator=g) * 0.1
    pre = x.double() @ w.to(BF16).double().t() + b.double()           # the stored operands: bf16 X, W_H rounded to bf16 inside
    return g, x, w, b, pre


def _h_errors(h, pre, drop_p):
    """H_bag against fp64 at test_gpu_patch_coattn.py's measure, |diff| / max(|ref|, 1e-2) <= 2^-7.  With dropout the kept
    elements are held to ref / (1 - p) (that file's test_patch_layer_widths: `relmax(hd[kept], (ref / 0.75)[kept])`), and
    nothing may appear where the pre-activation is clearly negative."""
    h = h.double()
    ref = torch.relu(pre)
    if drop_p == 0.0:
        return {"h_bag": (float(((h - ref).abs() / ref.abs().clamp_min(1e-2)).max()), PATCH_H_BAR)}
    kept = h != 0
    ref = ref / (1.0 - drop_p)
    errs = {"h_bag_kept": (float(((h - ref).abs() / ref.abs().clamp_min(1e-2))[kept].max()) if bool(kept.any()) else 0.0, PATCH_H_BAR),
            "h_bag_where_relu_is_off": (float(h[pre < -1e-2].abs().max()) if bool((pre < -1e-2).any()) else 0.0, 0.0)}
    if h.numel() >= 4096:
        # realised rate: test_gpu_patch_widths.py::test_dropout_masks holds |rate - 0.25| < 0.005 at 1.4e6 positives; the binomial
        # sigma at this window's count of positives gives the same 4.5 sigma here
        pos = pre > 1e-2
        n = int(pos.sum())
        rate = float((pos & ~kept).sum()) / n
        errs["drop_rate"] = (abs(rate - drop_p), 4.5 * math.sqrt(drop_p * (1 - drop_p) / n) + 1.0 / n)
    return errs


def run_patch_coattn(dev, fill, lengths, n_q, drop_p, amap, plan):
    lib = L.lib()
    E, pd = 256, 1024
    n_slides, T, R = len(lengths), sum(lengths), len(lengths) * n_q

    def make():
        g, x, w, b, pre = _patch_problem(lengths, pd, E, ("f1", n_q))
        return dict(x=x, w=w, b=b, pre=pre, query=torch.randn(R, E, generator=g), **_coattn_params(g, E))
    i = _cached(("f1", lengths, n_q), make)
    A = Arena(dev)
    x = A.place("patches", (T, pd), BF16, i["x"])
    w, b = A.place("patch_weight", (E, pd), data=i["w"]), A.place("patch_bias", (E,), data=i["b"])
    query = A.place("query", (R, E), data=i["query"])
    pw = {k: A.place(k, i[k].shape, data=i[k]) for k in ("in_w", "in_b", "out_w", "out_b")}
    h = A.place("h_bag", (T, E), BF16)
    out = A.place("out", (R, E))
    am = A.place("attn_map", (n_q * T,)) if amap else None
    saved = A.place("saved", (lib.mpo_coattn_saved_floats(n_slides, n_q, E),))
    ws_bytes = lib.mpo_patch_coattn_workspace_bytes(n_slides, n_q, E, pd)
    assert ws_bytes % 4 == 0
    ws = A.place("workspace", (ws_bytes // 4,))
    A.fill(fill)
    A.seal()
    cu, keep = ops.make_cu(lengths, dev), []
    L.call("mpo_patch_coattn_mcat_forward", L.ptr(x), L.ptr(cu), n_slides, T, max(lengths), pd, L.ptr(w), L.ptr(b), float(drop_p), 1234, 99,
           None, L.ptr(query), n_q, E, L.ptr(pw["in_w"]), L.ptr(pw["in_b"]), L.ptr(pw["out_w"]), L.ptr(pw["out_b"]), L.ptr(h), L.ptr(out),
           L.ptr(am), L.ptr(saved), make_plan(plan, lengths, cu, dev, keep), L.ptr(ws), ws_bytes, L.stream_of(x))
    A.check("mpo_patch_coattn_mcat_forward")
    A.finite("mpo_patch_coattn_mcat_forward", h_bag=h, out=out, attn_map=am, saved=saved)
    outs = _cpu(dict(h_bag=h, out=out, attn_map=am, saved=saved))
    errs = _h_errors(outs["h_bag"], i["pre"], drop_p)
    # the co-attention on the kernel's own H_bag (the stored values it consumed), as test_gpu_patch_coattn.py holds it
    p = {k: v.detach() for k, v in _oracle_params(i).items()}
    o, o_ref, a_ref = 0, [], []
    for s, m in enumerate(lengths):
        out_s, a_s = O.mcat_coattention(i["query"][s * n_q:(s + 1) * n_q].double(), outs["h_bag"][o:o + m].double(), p)
        o_ref.append(out_s)
        a_ref.append(a_s.reshape(-1))
        o += m
    errs["out"] = (relmax(outs["out"], torch.cat(o_ref)), FUSED_OUT_BAR)
    if amap:
        errs["attn_map"] = (relelem(outs["attn_map"], torch.cat(a_ref)), FUSED_OUT_BAR)
    return Run(outs, errs)


def run_patch_fc(dev, fill, lengths, pd, E, drop_p, plan):
    lib = L.lib()
    T = sum(lengths)
    _, xs, wsrc, bsrc, pre = _cached(("fc", lengths, pd, E), lambda: _patch_problem(lengths, pd, E, "fc"))
    A = Arena(dev)
    x = A.place("patches", (T, pd), BF16, xs)
    w, b = A.place("patch_weight", (E, pd), data=wsrc), A.place("patch_bias", (E,), data=bsrc)
    h = A.place("h_bag", (T, E), BF16)
    ws_bytes = lib.mpo_patch_fc_workspace_bytes(E, pd)
    assert ws_bytes % 4 == 0
    ws = A.place("workspace", (ws_bytes // 4,))
    A.fill(fill)
    A.seal()
    cu, keep = ops.make_cu(lengths, dev), []
    L.call("mpo_patch_fc_forward", L.ptr(x), L.ptr(cu), len(lengths), T, max(lengths), pd, L.ptr(w), L.ptr(b), E, float(drop_p), 1234, 99,
           None, L.ptr(h), make_plan(plan, lengths, cu, dev, keep), L.ptr(ws), ws_bytes, L.stream_of(x))
    A.check("mpo_patch_fc_forward")
    A.finite("mpo_patch_fc_forward", h_bag=h)
    outs = _cpu(dict(h_bag=h))
    return Run(outs, _h_errors(outs["h_bag"], pre, drop_p))


# ----------------------------------------------------------------------------------------- fp32 and fp16 patch layers
def feature_scale(x):
    """x_scale as include/mpo_hip.h documents it: 2^(15 - e) for max |X| = m 2^e, m in [0.5, 1)."""
    m, e = math.frexp(float(x.abs().max()))
    return 2.0 ** (15 - e)


def run_patch_f32(dev, fill, rows, storage, h_given, drop_256=0, scale_on_device=False):
    """mpo_patch_fc_f32_forward (or _forward_dev) + _backward for storage fp32; mpo_patch_fc_f16_forward + _backward for fp16.
    The operands are those of tests/test_gpu_patch_fc_f32.py (the bars belong to their scale)."""
    lib = L.lib()
    E, pd = 256, 1024

    def make():
        g = torch.Generator().manual_seed(_seed("pf", rows, str(storage)))
        x = torch.randn(rows, pd, generator=g).to(storage)
        return dict(x=x, w=_uniform(g, (E, pd), 1 / 32), b=torch.randn(E, generator=g) * 0.1, d_h=torch.randn(rows, E, generator=g))
    i = _cached(("pf", rows, storage), make)
    f16 = storage == F16
    tag = "f16" if f16 else "f32"
    A = Arena(dev)
    x = A.place("patches", (rows, pd), storage, i["x"])
    w, b = A.place("patch_weight", (E, pd), data=i["w"]), A.place("patch_bias", (E,), data=i["b"])
    scale = feature_scale(i["x"].float())
    sc = A.place("x_scale", (1,), data=torch.tensor([scale])) if scale_on_device else None
    h = A.place("h_bag", (rows, E))
    fwd_bytes = getattr(lib, f"mpo_patch_fc_{tag}_workspace_bytes")(0)
    bwd_bytes = getattr(lib, f"mpo_patch_fc_{tag}_workspace_bytes")(1)
    assert fwd_bytes % 4 == 0 and bwd_bytes % 4 == 0
    ws_f, ws_b = A.place("workspace_fwd", (fwd_bytes // 4,)), A.place("workspace_bwd", (bwd_bytes // 4,))
    d_h = A.place("d_h_bag", (rows, E), data=i["d_h"])
    dw, db = A.place("d_weight", (E, pd)), A.place("d_bias", (E,))
    A.fill(fill)
    A.seal()
    s = L.stream_of(x)
    p = drop_256 / 256.0
    if f16:
        fwd = "mpo_patch_fc_f16_forward"
        L.call(fwd, L.ptr(x), rows, pd, L.ptr(w), L.ptr(b), E, drop_256, 1234, 99, None, L.ptr(h), L.ptr(ws_f), fwd_bytes, s)
    elif scale_on_device:
        fwd = "mpo_patch_fc_f32_forward_dev"
        L.call(fwd, L.ptr(x), rows, pd, L.ptr(w), L.ptr(b), E, p, 1234, 99, None, L.ptr(sc), L.ptr(h), L.ptr(ws_f), fwd_bytes, s)
    else:
        fwd = "mpo_patch_fc_f32_forward"
        L.call(fwd, L.ptr(x), rows, pd, L.ptr(w), L.ptr(b), E, p, 1234, 99, None, scale, L.ptr(h), L.ptr(ws_f), fwd_bytes, s)
    A.check(fwd)
    A.finite(fwd, h_bag=h)
    A.freeze(h)
    gate = 256.0 / (256.0 - drop_256)
    bwd = f"mpo_patch_fc_{tag}_backward"
    L.call(bwd, L.ptr(d_h), L.ptr(h) if h_given else None, L.ptr(x), rows, E, pd, drop_256 if f16 else gate, L.ptr(dw), L.ptr(db),
           L.ptr(ws_b), bwd_bytes, s)
    A.check(bwd)
    A.finite(bwd, d_weight=dw, d_bias=db)
    outs = _cpu(dict(h_bag=h, d_weight=dw, d_bias=db))
    xd = i["x"].double()
    pre = xd @ i["w"].double().t() + i["b"].double()
    hd = outs["h_bag"].double()
    errs = {}
    if drop_256 == 0:
        errs["h_bag"] = (float((hd - torch.relu(pre)).abs().max()), F32_FWD_ABS)
    else:
        kept = hd != 0
        errs["h_bag_kept"] = (float((hd - torch.relu(pre) * gate).abs()[kept].max()), F32_FWD_ABS * gate)
        errs["h_bag_where_relu_is_off"] = (float(hd[pre < -1e-4].abs().max()), 0.0)
    # dW and db against the mask the kernel itself used (as tests/test_gpu_patch_fc_f32.py does); h_bag NULL: g = d_h_bag
    # (the fp16 entry applies its gate from drop_256 either way: at drop_256 = 0 it is 1)
    gk = i["d_h"].double() * ((hd > 0) * gate if h_given else (gate if f16 else 1.0))
    errs["d_weight"] = (relmax(outs["d_weight"], gk.t() @ xd), F32_DW_REL)
    errs["d_bias"] = (relmax(outs["d_bias"], gk.sum(0)), F32_DB_REL)
    return Run(outs, errs)


# ---------------------------------------------------------------------------------------------------------- K2 (NaCAGaT)
def _nacagat_problem(lengths, dtype, E, n_q):
    g = torch.Generator().manual_seed(_seed("nacagat", lengths, str(dtype), E, n_q))
    T, R = sum(lengths), len(lengths) * n_q
    i = dict(bag=torch.relu(torch.randn(T, E, generator=g)).to(dtype), query=torch.randn(R, E, generator=g), **_coattn_params(g, E),
             d_out=torch.randn(R, E, generator=g), d_map=torch.randn(n_q * T, generator=g), d_q_proj=torch.randn(R, E, generator=g),
             d_query0=torch.randn(R, E, generator=g))
    # K = H W_k^T + b_k is the caller's GEMM: formed in fp64 from the stored bag and stored in fp32, as the entry requires
    i["kbag"] = (i["bag"].double() @ i["in_w"][E:2 * E].double().t() + i["in_b"][E:2 * E].double()).float()
    return i


def _nacagat_ref(i, lengths, E, n_q, keep, d_amap, d_qproj, acc):
    """oracle.mpo_oracle.narrow_gated_attention restated in fp64 with K taken as stored (the entry's kbag, a leaf of its own:
    d_kbag is the gradient w.r.t. it, the key slices of d_in_proj_* belong to the caller) and the value projection folded
    out, slide by slide; `keep` is the pre-scaled dropout mask the kernel drew (None: eval)."""
    p = _oracle_params(i)
    w, bias = p["co_attention.in_proj_weight"], p["co_attention.in_proj_bias"]
    q_in, k, h = (i[n].double().requires_grad_(True) for n in ("query", "kbag", "bag"))
    dmaps = _blocks(i["d_map"].double(), lengths, n_q)
    keeps = _blocks(keep.double(), lengths, n_q) if keep is not None else None
    qs, outs, maps, ctxs, loss, o = [], [], [], [], 0.0, 0
    for b, m in enumerate(lengths):
        rows = slice(b * n_q, (b + 1) * n_q)
        q = q_in[rows] @ w[:E].t() + bias[:E]
        kb = k[o:o + m]
        s = (q / math.sqrt(E)) @ kb.t() * ((torch.tanh(q) @ torch.tanh(kb).t() + 1.0) / 2.0)
        a = torch.softmax(s, dim=-1)
        if keeps is not None:
            a = a * keeps[b]
        ctx = a @ h[o:o + m]
        ctx.retain_grad()
        attn = ctx @ w[2 * E:].t() + a.sum(1, keepdim=True) * bias[2 * E:]
        out = attn @ p["co_attention.out_proj.weight"].t() + p["co_attention.out_proj.bias"]
        loss = loss + (out * i["d_out"][rows].double()).sum()
        if d_amap:
            loss = loss + (a * dmaps[b]).sum()
        if d_qproj:
            loss = loss + (q * i["d_q_proj"][rows].double()).sum()
        qs.append(q.detach())
        outs.append(out.detach())
        maps.append(a.detach().reshape(-1))
        ctxs.append(ctx)
        o += m
    gq, gk, gh, gw, gbias, gow, gob = torch.autograd.grad(loss, [q_in, k, h] + list(p.values()), retain_graph=True)
    d_ctx = torch.autograd.grad(loss, ctxs)
    return dict(q_proj=torch.cat(qs), out=torch.cat(outs), attn_map=torch.cat(maps), d_query=gq + (i["d_query0"].double() if acc else 0),
                d_kbag=gk, d_hbag=gh, d_ctx=torch.cat(d_ctx), d_kbag_colsum=gk.sum(0), d_in_w=gw, d_in_b=gbias, d_out_w=gow, d_out_b=gob)


def run_nacagat(dev, fill, lengths, dtype, E, n_q, drop_p, d_amap, d_qproj, dk_dtype, colsum, ctx_out, acc, plan, one_pass=1):
    """colsum: None | "given" | "alias" (d_kbag_colsum = d_in_proj_bias + E, the alias capi.hip special-cases at its
    `f.zero[1]` line); ctx_out: d_ctx given and d_hbag NULL, else the reverse."""
    lib = L.lib()
    n_slides, T, R = len(lengths), sum(lengths), len(lengths) * n_q
    i = _cached(("nacagat", lengths, dtype, E, n_q), lambda: _nacagat_problem(lengths, dtype, E, n_q))
    A = Arena(dev)
    bag_shape = (2 * T, 256) if E == 512 else (T, E)                # split halves: [2][T][256]
    kbag = A.place("kbag", bag_shape, F32, halves(i["kbag"]))
    hbag = A.place("hbag", bag_shape, dtype, halves(i["bag"]))
    query = A.place("query", (R, E), data=i["query"])
    pw = {k: A.place(k, i[k].shape, data=i[k]) for k in ("in_w", "in_b", "out_w", "out_b")}
    q_proj, out = A.place("q_proj", (R, E)), A.place("out", (R, E))
    amap, score_maps = A.place("attn_map", (n_q * T,)), A.place("score_maps", (2 * n_q * T,))
    saved = A.place("saved", (lib.mpo_nacagat_saved_floats(n_slides, n_q, E),))
    ws_bytes = lib.mpo_nacagat_workspace_bytes(n_slides, n_q, E, max(lengths), T)
    assert ws_bytes % 4 == 0
    ws = A.place("workspace", (ws_bytes // 4,))
    d_out = A.place("d_out", (R, E), data=i["d_out"])
    d_map = A.place("d_attn_map", (n_q * T,), data=i["d_map"]) if d_amap else None
    d_qp = A.place("d_q_proj", (R, E), data=i["d_q_proj"]) if d_qproj else None
    d_query = A.place("d_query", (R, E), data=i["d_query0"] if acc else None, role="inout" if acc else "out")
    d_kbag = A.place("d_kbag", bag_shape, dk_dtype)
    d_hbag = None if ctx_out else A.place("d_hbag", bag_shape, dtype)
    d_ctx = A.place("d_ctx", (R, E)) if ctx_out else None
    d_in_w, d_in_b = A.place("d_in_w", (3 * E, E)), A.place("d_in_b", (3 * E,))
    d_out_w, d_out_b = A.place("d_out_w", (E, E)), A.place("d_out_b", (E,))
    cs = A.place("d_kbag_colsum", (E,)) if colsum == "given" else (d_in_b[E:2 * E] if colsum == "alias" else None)
    A.fill(fill)
    A.seal()
    cu, keep_alive = ops.make_cu(lengths, dev), []
    plan_p = make_plan(plan, lengths, cu, dev, keep_alive)
    s = L.stream_of(kbag)
    seed, offset = (1234, 77) if drop_p > 0 else (0, 0)
    with Knobs(mpo_set_nacagat_one_pass_key_grad=one_pass):
        L.call("mpo_coattn_nacagat_forward", L.ptr(kbag), L.MPO_F32, L.ptr(hbag), _code(dtype), L.ptr(cu), n_slides, T, max(lengths),
               L.ptr(query), n_q, E, L.ptr(pw["in_w"]), L.ptr(pw["in_b"]), L.ptr(pw["out_w"]), L.ptr(pw["out_b"]), float(drop_p), seed, offset,
               None, L.ptr(q_proj), L.ptr(out), L.ptr(amap), L.ptr(score_maps), L.ptr(saved), plan_p, L.ptr(ws), ws_bytes, s)
        A.check("mpo_coattn_nacagat_forward")
        A.finite("mpo_coattn_nacagat_forward", q_proj=q_proj, out=out, attn_map=amap, score_maps=score_maps, saved=saved)
        A.freeze(q_proj, out, amap, score_maps, saved)
        A.fill(fill, only=[ws])
        L.call("mpo_coattn_nacagat_backward", L.ptr(kbag), L.MPO_F32, L.ptr(hbag), _code(dtype), L.ptr(cu), n_slides, T, max(lengths),
               L.ptr(query), n_q, E, L.ptr(pw["in_w"]), L.ptr(pw["in_b"]), L.ptr(pw["out_w"]), float(drop_p), seed, offset, None,
               L.ptr(saved), L.ptr(score_maps), L.ptr(amap), L.ptr(d_out), L.ptr(d_map), L.ptr(d_qp), L.ptr(d_query), int(acc),
               L.ptr(d_kbag), _code(dk_dtype), L.ptr(cs), L.ptr(d_hbag), L.ptr(d_ctx), L.ptr(d_in_w), L.ptr(d_in_b), L.ptr(d_out_w),
               L.ptr(d_out_b), plan_p, L.ptr(ws), ws_bytes, s)
        A.check("mpo_coattn_nacagat_backward")
    views = dict(q_proj=q_proj, out=out, attn_map=amap, score_maps=score_maps, saved=saved, d_query=d_query, d_kbag=d_kbag, d_hbag=d_hbag,
                 d_ctx=d_ctx, d_in_w=d_in_w, d_in_b=d_in_b, d_out_w=d_out_w, d_out_b=d_out_b,
                 d_kbag_colsum=cs if colsum == "given" else None)
    A.finite("mpo_coattn_nacagat_backward", **views)
    outs = _cpu(views)
    # the mask the kernel drew, read off the post-dropout map (A > 0 everywhere before dropout), as
    # test_nacagat_training_dropout_replays_through_oracle recovers it; the realised rate is round(256 p) / 256
    realised = int(drop_p * 256.0 + 0.5) / 256.0
    keep = (outs["attn_map"] > 0).double() / (1.0 - realised) if drop_p > 0 else None
    ref = _nacagat_ref(i, lengths, E, n_q, keep, d_amap, d_qproj, acc)
    if colsum == "alias":
        ref["d_in_b"] = ref["d_in_b"].clone()
        ref["d_in_b"][E:2 * E] = ref["d_kbag_colsum"]
    f32 = dtype == F32
    param_bar = K2.GRAD_TOL if f32 else K2.GRAD_TOL_BF16_PARAM
    bag_bar = K2.GRAD_TOL if f32 else K2.GRAD_TOL_BF16_BAG
    dk_bar = K2.GRAD_TOL_BF16_BAG if dk_dtype == BF16 else param_bar
    errs = dict(q_proj=(relmax(outs["q_proj"], ref["q_proj"]), K2.OUT_TOL), out=(relmax(outs["out"], ref["out"]), K2.OUT_TOL),
                attn_map=(relelem(outs["attn_map"], ref["attn_map"]), K2.MAP_REL_TOL),
                d_query=(relmax(outs["d_query"], ref["d_query"]), param_bar),
                d_kbag=(relmax(unhalves(outs["d_kbag"], T, E), ref["d_kbag"]), dk_bar),
                key_weight_slice=(float(outs["d_in_w"][E:2 * E].abs().max()), 0.0))
    for k in ("d_in_w", "d_in_b", "d_out_w", "d_out_b"):
        errs[k] = (relmax(outs[k], ref[k]), param_bar)
    if drop_p > 0:
        errs["drop_rate"] = (abs(float((outs["attn_map"] == 0).double().mean()) - realised),
                             4.5 * math.sqrt(realised * (1 - realised) / (n_q * T)) + 1.0 / (n_q * T))
    if colsum != "alias":
        errs["key_bias_slice"] = (float(outs["d_in_b"][E:2 * E].abs().max()), 0.0)
    if colsum == "given":
        errs["d_kbag_colsum"] = (relmax(outs["d_kbag_colsum"], ref["d_kbag_colsum"]), dk_bar)
    if ctx_out:
        errs["d_ctx"] = (relmax(outs["d_ctx"], ref["d_ctx"]), param_bar)
    else:
        errs["d_hbag"] = (relmax(unhalves(outs["d_hbag"], T, E), ref["d_hbag"]), bag_bar)
    return Run(outs, errs)


# ------------------------------------------------------------------------------- entries that had partial guards before
def run_key_projection(dev, fill, rows, E):
    def make():
        g = torch.Generator().manual_seed(_seed("kp", rows, E))
        return dict(h=torch.relu(torch.randn(rows, E, generator=g)).to(BF16), w=torch.randn(E, E, generator=g) / 16, b=torch.randn(E, generator=g))
    i = _cached(("kp", rows, E), make)
    A = Arena(dev)
    h, w, b = A.place("hbag", (rows, E), BF16, i["h"]), A.place("w_k", (E, E), data=i["w"]), A.place("b_k", (E,), data=i["b"])
    k = A.place("kbag", (rows, E))
    A.fill(fill)
    A.seal()
    L.call("mpo_key_projection", L.ptr(h), rows, E, L.ptr(w), L.ptr(b), L.ptr(k), L.stream_of(h))
    A.check("mpo_key_projection")
    A.finite("mpo_key_projection", kbag=k)
    outs = _cpu(dict(kbag=k))
    ref = i["h"].double() @ i["w"].double().t() + i["b"].double()
    return Run(outs, dict(kbag=(relmax(outs["kbag"], ref), KEY_PROJ_BAR)))


def run_nacagat_patch_grad(dev, fill, lengths, E, n_q, gate, fused, plan):
    """mpo_nacagat_patch_grad (d_bag = (A^T d_ctx + addend) (.) gate) / mpo_nacagat_patch_grad_fused (addend = d_kbag W_k inside
    the pass) at the measures of check_patch_grad_one_pass / check_fused_patch_side_gradient."""
    lib = L.lib()
    n_slides, T, R = len(lengths), sum(lengths), len(lengths) * n_q

    def make():
        g = torch.Generator().manual_seed(_seed("pg", lengths, E, n_q, fused))
        i = dict(h=torch.relu(torch.randn(T, E, generator=g)).to(BF16), d_ctx=torch.randn(R, E, generator=g))
        if fused:
            i.update(amap=torch.rand(n_q * T, generator=g) / 100, dk=(torch.randn(T, E, generator=g) * 0.1).to(BF16), w_k=_uniform(g, (E, E), 1 / 16))
            add = i["dk"].double() @ i["w_k"].to(BF16).double()      # (W_k enters the kernel's MFMA as one bf16 term)
        else:
            i.update(amap=torch.rand(n_q * T, generator=g), addend=torch.randn(T, E, generator=g).to(BF16))
            add = i["addend"].double()
        blocks = _blocks(i["amap"].double(), lengths, n_q)
        ref = torch.cat([blocks[b].t() @ i["d_ctx"][b * n_q:(b + 1) * n_q].double() for b in range(n_slides)]) + add
        i["ref"] = ref * (i["h"].double() > 0) * gate if gate else ref
        return i
    i = _cached(("pg", lengths, E, n_q, gate, fused), make)
    A = Arena(dev)
    amap, d_ctx = A.place("attn_map", (n_q * T,), data=i["amap"]), A.place("d_ctx", (R, E), data=i["d_ctx"])
    h = A.place("hbag", (T, E), BF16, i["h"])
    if fused:
        dk, w_k = A.place("d_kbag", (T, E), BF16, i["dk"]), A.place("w_k", (E, E), data=i["w_k"])
    else:
        addend = A.place("addend", (T, E), BF16, i["addend"])
    d_bag, d_bias = A.place("d_bag", (T, E), BF16), A.place("d_bias", (E,))
    ws_bytes = lib.mpo_nacagat_workspace_bytes(n_slides, n_q, E, max(lengths), T)
    assert ws_bytes % 4 == 0
    ws = A.place("workspace", (ws_bytes // 4,))
    A.fill(fill)
    A.seal()
    cu, keep = ops.make_cu(lengths, dev), []
    head = (L.ptr(cu), n_slides, T, max(lengths), n_q, E, L.ptr(amap), L.ptr(d_ctx))
    tail = (L.ptr(h), L.ptr(d_bag), float(gate), L.ptr(d_bias), make_plan(plan, lengths, cu, dev, keep), L.ptr(ws), ws_bytes, L.stream_of(h))
    name = "mpo_nacagat_patch_grad_fused" if fused else "mpo_nacagat_patch_grad"
    if fused:
        L.call(name, *head, L.ptr(dk), L.ptr(w_k), *tail)
    else:
        L.call(name, *head, L.ptr(addend), *tail)
    A.check(name)
    A.finite(name, d_bag=d_bag, d_bias=d_bias)
    outs = _cpu(dict(d_bag=d_bag, d_bias=d_bias))
    got, ref = outs["d_bag"].double(), i["ref"]
    err = (got - ref).abs()
    cs = got.sum(0)
    if fused:      # check_fused_patch_side_gradient: one bf16 ulp + 2e-3 of the largest entry; colsum assert_close(rtol 1e-4, atol 1e-3)
        errs = dict(d_bag=(float((err - 2.0 ** -7 * ref.abs()).max()), 2e-3 * float(ref.abs().max())),
                    d_bag_mean=(float(err.mean()), 2e-3 * float(ref.abs().mean())),
                    d_bias=(float(((outs["d_bias"].double() - cs).abs() - 1e-4 * cs.abs()).max()), 1e-3))
    else:          # check_patch_grad_one_pass: |diff| <= 2^-8 |ref| + 1e-4; colsum within 1e-4 max(1, max |colsum|) of the rows written
        errs = dict(d_bag=(float((err - 2.0 ** -8 * ref.abs()).max()), 1e-4),
                    d_bias=(float((outs["d_bias"].double() - cs).abs().max()), 1e-4 * max(1.0, float(cs.abs().max()))))
    if gate:
        errs["d_bag_where_h_is_zero"] = (float(got[i["h"].double() == 0].abs().max()), 0.0)
    return Run(outs, errs)


def run_patch_weight_grad(dev, fill, rows, E, pd):
    lib = L.lib()

    def make():
        g = torch.Generator().manual_seed(_seed("wg", rows, E, pd))
        return dict(g=(torch.randn(rows, E, generator=g) * (torch.rand(rows, E, generator=g) > 0.3)).to(BF16),
                    x=torch.randn(rows, pd, generator=g).to(BF16))
    i = _cached(("wg", rows, E, pd), make)
    A = Arena(dev)
    gg, x = A.place("g", (rows, E), BF16, i["g"]), A.place("patches", (rows, pd), BF16, i["x"])
    dw = A.place("d_weight", (E, pd))
    ws_bytes = lib.mpo_patch_weight_grad_workspace_bytes(E, pd)
    assert ws_bytes % 4 == 0
    ws = A.place("workspace", (ws_bytes // 4,))
    A.fill(fill)
    A.seal()
    L.call("mpo_patch_weight_grad", L.ptr(gg), L.ptr(x), rows, E, pd, L.ptr(dw), 0, L.ptr(ws), ws_bytes, L.stream_of(x))
    A.check("mpo_patch_weight_grad")
    A.finite("mpo_patch_weight_grad", d_weight=dw)
    outs = _cpu(dict(d_weight=dw))
    return Run(outs, dict(d_weight=(relmax(outs["d_weight"], i["g"].double().t() @ i["x"].double()), WGRAD_BAR)))


def run_patch_epilogue_backward(dev, fill, rows, cols, drop_p):
    lib = L.lib()

    def make():
        g = torch.Generator().manual_seed(_seed("pe", rows, cols))
        return dict(h=torch.relu(torch.randn(rows, cols, generator=g)).to(BF16), dy=torch.randn(rows, cols, generator=g).to(BF16))
    i = _cached(("pe", rows, cols), make)
    A = Arena(dev)
    h, dy = A.place("h", (rows, cols), BF16, i["h"]), A.place("dy", (rows, cols), BF16, i["dy"])
    gq, d_bias = A.place("g", (rows, cols), BF16), A.place("d_bias", (cols,))
    ws_bytes = lib.mpo_patch_epilogue_backward_workspace_bytes(rows * cols, cols)
    assert ws_bytes % 4 == 0
    ws = A.place("workspace", (ws_bytes // 4,))
    A.fill(fill)
    A.seal()
    L.call("mpo_patch_epilogue_backward", L.ptr(h), L.ptr(dy), L.ptr(gq), rows * cols, cols, float(drop_p), L.ptr(d_bias), L.ptr(ws), ws_bytes,
           L.stream_of(h))
    A.check("mpo_patch_epilogue_backward")
    A.finite("mpo_patch_epilogue_backward", g=gq, d_bias=d_bias)
    outs = _cpu(dict(g=gq, d_bias=d_bias))
    # test_epilogue_dropout_rate_scale_and_backward_mask: g bit-equal to bf16(dy * fp32(1 / (1 - p))) under the mask read off h
    scale = torch.tensor(1.0 / (1.0 - drop_p), dtype=F32)
    ref_g = torch.where(i["h"] > 0, (i["dy"].float() * scale).to(BF16), torch.zeros_like(i["dy"]))
    gd = outs["g"].double()
    return Run(outs, dict(g=(float((_ints(outs["g"]) != _ints(ref_g)).sum()), 0.0),
                          d_bias=(float(((outs["d_bias"].double() - gd.sum(0)).abs() / gd.abs().sum(0).clamp_min(1e-30)).max()), PE.COLSUM_REL)))


def run_colsum_bf16(dev, fill, rows, cols):
    i = _cached(("cs", rows, cols), lambda: (torch.randn(rows, cols, generator=torch.Generator().manual_seed(_seed("cs", rows, cols))) * 3.0).to(BF16))
    A = Arena(dev)
    x, out = A.place("x", (rows, cols), BF16, i), A.place("out", (cols,))
    A.fill(fill)
    A.seal()
    L.call("mpo_colsum_bf16", L.ptr(x), L.ptr(out), rows, cols, L.stream_of(x))
    A.check("mpo_colsum_bf16")
    A.finite("mpo_colsum_bf16", out=out)
    outs = _cpu(dict(out=out))
    err = ((outs["out"].double() - i.double().sum(0)).abs() / i.double().abs().sum(0).clamp_min(1e-30)).max()
    return Run(outs, dict(out=(float(err), PE.COLSUM_REL)))


def run_map_blocks(dev, fill, lengths, n_q):
    """mpo_map_block_dot, mpo_map_block_scale and mpo_map_block_stats over one ragged map."""
    lib = L.lib()
    n_slides, T = len(lengths), sum(lengths)

    def make():
        g = torch.Generator().manual_seed(_seed("mb", lengths, n_q))
        return dict(a=torch.randn(n_q * T, generator=g), b=torch.randn(n_q * T, generator=g), scale=torch.randn(n_slides, generator=g))
    i = _cached(("mb", lengths, n_q), make)
    A = Arena(dev)
    a, b, scale = A.place("a_map", (n_q * T,), data=i["a"]), A.place("b_map", (n_q * T,), data=i["b"]), A.place("scale", (n_slides,), data=i["scale"])
    dots, scaled, stats = A.place("dots", (n_slides * n_q,)), A.place("scaled", (n_q * T,)), A.place("stats", (n_slides, 3))
    ws_bytes = lib.mpo_map_block_stats_workspace_bytes(n_slides, n_q, max(lengths))
    assert ws_bytes % 4 == 0
    ws = A.place("workspace", (ws_bytes // 4,))
    A.fill(fill)
    A.seal()
    cu, s = ops.make_cu(lengths, dev), L.stream_of(a)
    L.call("mpo_map_block_dot", L.ptr(a), L.ptr(b), L.ptr(cu), n_slides, n_q, L.ptr(dots), s)
    L.call("mpo_map_block_scale", L.ptr(a), L.ptr(scale), L.ptr(cu), n_slides, n_q, L.ptr(scaled), s)
    L.call("mpo_map_block_stats", L.ptr(a), L.ptr(cu), n_slides, n_q, max(lengths), L.ptr(stats), L.ptr(ws), ws_bytes, s)
    A.check("mpo_map_block_dot / _scale / _stats")
    A.finite("mpo_map_block_dot / _scale / _stats", dots=dots, scaled=scaled, stats=stats)
    outs = _cpu(dict(dots=dots, scaled=scaled, stats=stats))
    ref, mags = N.map_block_fp64(i["a"], i["b"], list(lengths), n_q)
    got = outs["dots"].view(n_slides, n_q).double()
    # each error as a fraction of its own fp32 worst-case bound (test_map_block_dot_and_scale_match_fp64's measure): bar 1
    frac = max(float(((got[k] - ref[k]).abs() / N.fp32_dot_bound(m, mags[k]).clamp_min(1e-300)).max()) for k, m in enumerate(lengths))
    per_element = torch.cat([i["scale"][k].expand(n_q * m) for k, m in enumerate(lengths)])
    blocks = _blocks(i["a"], lengths, n_q)
    lo_hi = sum(int(float(outs["stats"][k, 0]) != float(blk.min())) + int(float(outs["stats"][k, 1]) != float(blk.max())) for k, blk in enumerate(blocks))
    mean = max(abs(float(outs["stats"][k, 2]) - float(blk.double().mean())) / abs(float(blk.double().mean())) for k, blk in enumerate(blocks))
    return Run(outs, dict(dots_over_bound=(frac, 1.0 + 1e-12), scaled=(float((_ints(outs["scaled"]) != _ints(per_element * i["a"])).sum()), 0.0),
                          stats_min_max=(float(lo_hi), 0.0), stats_mean=(mean, MAP_MEAN_REL + 1e-18)))


RUNNERS = dict(mcat=run_mcat, patch_coattn=run_patch_coattn, patch_fc=run_patch_fc, patch_f32=run_patch_f32, nacagat=run_nacagat,
               key_projection=run_key_projection, nacagat_patch_grad=run_nacagat_patch_grad, patch_weight_grad=run_patch_weight_grad,
               patch_epilogue_backward=run_patch_epilogue_backward, colsum_bf16=run_colsum_bf16, map_blocks=run_map_blocks)

# ------------------------------------------------------------------------------------------------------------ the table
Case = namedtuple("Case", "id runner entries kw atomic", defaults=(None,))


def _d(dtype):
    return {F32: "f32", BF16: "bf16", F16: "f16"}[dtype]


def _w(lengths):
    return "x".join(map(str, lengths))


WINDOW_PLANS = [(W_EDGES, "uniform"), (W_EDGES, "built"), (W_ONE, "uniform"), (W_LONG, "built"), (W_MAX, "max")]
K1_ENTRIES = ("mpo_coattn_mcat_forward", "mpo_coattn_mcat_backward")
K2_ENTRIES = ("mpo_coattn_nacagat_forward", "mpo_coattn_nacagat_backward")


def _pick(options, *key):
    """One of `options`, fixed by the key: spreads the case options over the window x dtype x embed grid without tying one to
    another (tests/test_buffer_contract_cpu.py asserts what the table has to cover)."""
    return options[int.from_bytes(hashlib.sha256(repr(key).encode()).digest()[:4], "big") % len(options)]


def _mcat_cases():
    cases = []
    for wi, (lengths, plan) in enumerate(WINDOW_PLANS):
        for dtype in (F32, BF16):
            for ei, E in enumerate((128, 256, 512)):
                key = (wi, E, str(dtype))
                n_q = (1, 6, 16)[(wi + ei + (dtype == BF16)) % 3]
                amap, d_amap = _pick(((False, False), (True, False), (True, True)), "map", *key)
                gate = _pick((0.0, 4.0 / 3.0), "gate", *key) if dtype == BF16 else 0.0
                kw = dict(lengths=lengths, dtype=dtype, E=E, n_q=n_q, amap=amap, d_amap=d_amap, colsum=bool(gate) or _pick((False, True), "cs", *key),
                          gate=gate, acc=_pick((0, 1), "acc", *key), plan=plan)
                kw["kernel"] = k1_bwd_kernel(dtype, E, n_q, d_amap, 1, 1)
                cases.append(kw)
    # every backward kernel once per dtype it serves, the selectors set explicitly
    base = dict(lengths=W_EDGES, E=256, n_q=6, plan="uniform", acc=0)
    cases += [dict(base, dtype=F32, amap=True, d_amap=True, colsum=True, gate=0.0, f32_vector=0, kernel="general"),
              dict(base, dtype=F32, amap=True, d_amap=True, colsum=False, gate=0.0, f32_vector=1, kernel="f32_vector"),
              dict(base, dtype=F32, amap=False, d_amap=False, colsum=True, gate=0.0, f32_vector=1, kernel="f32_vector", n_q=8),
              dict(base, dtype=BF16, amap=False, d_amap=False, colsum=True, gate=4.0 / 3.0, two_wave=0, kernel="general"),
              dict(base, dtype=BF16, amap=True, d_amap=False, colsum=True, gate=4.0 / 3.0, two_wave=1, kernel="two_wave"),
              dict(base, dtype=BF16, amap=False, d_amap=False, colsum=False, gate=0.0, two_wave=1, kernel="two_wave", n_q=1, acc=1),
              dict(base, dtype=BF16, amap=True, d_amap=True, colsum=False, gate=0.0, two_wave=1, kernel="general")]
    out = []
    for kw in cases:
        name = (f"mcat-{_w(kw['lengths'])}-{kw['plan']}-{_d(kw['dtype'])}-E{kw['E']}-q{kw['n_q']}-{kw['kernel']}"
                f"{'-map' if kw['amap'] else ''}{'-dmap' if kw['d_amap'] else ''}{'-colsum' if kw['colsum'] else ''}"
                f"{'-gate' if kw['gate'] else ''}{'-acc' if kw['acc'] else ''}")
        out.append(Case(name, "mcat", K1_ENTRIES, kw))
    return out


def _nacagat_cases():
    cases = []
    for wi, (lengths, plan) in enumerate(WINDOW_PLANS):
        for dtype in (F32, BF16):
            for ei, E in enumerate((128, 256, 512)):
                key = (wi, E, str(dtype))
                n_q = (1, 6, 7, 16)[(wi + ei + 2 * (dtype == BF16)) % 4]
                cases.append(dict(lengths=lengths, dtype=dtype, E=E, n_q=n_q, drop_p=_pick((0.0, 0.25), "drop", *key),
                                  d_amap=_pick((False, True), "dmap", *key), d_qproj=_pick((False, True), "dq", *key),
                                  dk_dtype=_pick((F32, BF16), "dk", *key) if dtype == BF16 else F32,
                                  colsum=(None, "given", "alias")[(wi + ei) % 3], ctx_out=_pick((False, True), "ctx", *key),
                                  acc=_pick((0, 1), "acc", *key), plan=plan, one_pass=1))
    # either side of the one-pass key-gradient limit with the selector on and off (n_q 6: one pass or two; n_q 7: two either way)
    base = dict(lengths=W_EDGES, E=256, drop_p=0.25, d_amap=True, d_qproj=True, plan="uniform", acc=0)
    for dtype, dk in ((F32, F32), (BF16, BF16)):
        for n_q in (6, 7):
            for one_pass in (1, 0):
                cases.append(dict(base, dtype=dtype, n_q=n_q, dk_dtype=dk, colsum="alias" if one_pass else "given",
                                  ctx_out=dtype == BF16, one_pass=one_pass))
    out = []
    for kw in cases:
        name = (f"nacagat-{_w(kw['lengths'])}-{kw['plan']}-{_d(kw['dtype'])}-E{kw['E']}-q{kw['n_q']}-dk_{_d(kw['dk_dtype'])}"
                f"-{'one_pass' if kw['one_pass'] else 'two_pass'}{'-drop' if kw['drop_p'] else ''}{'-dmap' if kw['d_amap'] else ''}"
                f"{'-dq' if kw['d_qproj'] else ''}-colsum_{kw['colsum']}-{'dctx' if kw['ctx_out'] else 'dh'}{'-acc' if kw['acc'] else ''}")
        out.append(Case(name, "nacagat", K2_ENTRIES, kw))
    return out


def _patch_cases():
    out = []
    for k, n_q in enumerate((1, 6, 8)):
        for drop_p in (0.0, 0.25):
            lengths, plan = WINDOW_PLANS[(2 * k + (drop_p > 0)) % len(WINDOW_PLANS)]
            out.append(Case(f"patch_coattn-{_w(lengths)}-{plan}-q{n_q}-p{drop_p:g}", "patch_coattn", ("mpo_patch_coattn_mcat_forward",),
                            dict(lengths=lengths, n_q=n_q, drop_p=drop_p, amap=bool((k + (drop_p > 0)) % 2), plan=plan)))
    # past the 8 queries the Python host sends through this entry: check_common admits 1..16 and the forward kernels are K1's own
    out.append(Case(f"patch_coattn-{_w(W_EDGES)}-uniform-q16-p0.25", "patch_coattn", ("mpo_patch_coattn_mcat_forward",),
                    dict(lengths=W_EDGES, n_q=16, drop_p=0.25, amap=True, plan="uniform")))
    n = 0
    for E in (128, 256, 512):
        for pd in (512, 1024, 2048):
            plan, drop_p = ("uniform", "built")[n % 2], (0.0, 0.25)[(n // 2) % 2]
            out.append(Case(f"patch_fc-{_w(W_EDGES)}-{plan}-{pd}to{E}-p{drop_p:g}", "patch_fc", ("mpo_patch_fc_forward",),
                            dict(lengths=W_EDGES, pd=pd, E=E, drop_p=drop_p, plan=plan)))
            n += 1
    out.append(Case(f"patch_fc-{_w(W_MAX)}-max-1024to256-p0", "patch_fc", ("mpo_patch_fc_forward",),
                    dict(lengths=W_MAX, pd=1024, E=256, drop_p=0.0, plan="max")))
    for rows in (1, 33, 257):
        for h_given in (True, False):
            drop = 64 if (h_given and rows == 257) else 0
            out.append(Case(f"patch_f32-{rows}-{'h' if h_given else 'no_h'}-d{drop}", "patch_f32", ("mpo_patch_fc_f32_forward", "mpo_patch_fc_f32_backward"),
                            dict(rows=rows, storage=F32, h_given=h_given, drop_256=drop)))
            out.append(Case(f"patch_f16-{rows}-{'h' if h_given else 'no_h'}-d{drop}", "patch_f32", ("mpo_patch_fc_f16_forward", "mpo_patch_fc_f16_backward"),
                            dict(rows=rows, storage=F16, h_given=h_given, drop_256=drop)))
        out.append(Case(f"patch_f32_dev-{rows}", "patch_f32", ("mpo_patch_fc_f32_forward_dev", "mpo_patch_fc_f32_backward"),
                        dict(rows=rows, storage=F32, h_given=True, scale_on_device=True)))
    return out


def _other_cases():
    return [Case("key_projection-33", "key_projection", ("mpo_key_projection",), dict(rows=33, E=256)),
            Case("key_projection-257", "key_projection", ("mpo_key_projection",), dict(rows=257, E=256)),
            Case("nacagat_patch_grad-uniform", "nacagat_patch_grad", ("mpo_nacagat_patch_grad",),
                 dict(lengths=W_EDGES, E=256, n_q=6, gate=4.0 / 3.0, fused=False, plan="uniform")),
            Case("nacagat_patch_grad-E128-max", "nacagat_patch_grad", ("mpo_nacagat_patch_grad",),
                 dict(lengths=W_MAX, E=128, n_q=16, gate=0.0, fused=False, plan="max")),
            Case("nacagat_patch_grad_fused-uniform", "nacagat_patch_grad", ("mpo_nacagat_patch_grad_fused",),
                 dict(lengths=W_EDGES, E=256, n_q=6, gate=4.0 / 3.0, fused=True, plan="uniform")),
            Case("nacagat_patch_grad_fused-max", "nacagat_patch_grad", ("mpo_nacagat_patch_grad_fused",),
                 dict(lengths=W_MAX, E=256, n_q=16, gate=0.0, fused=True, plan="max")),
            Case("patch_weight_grad-33-128x1024", "patch_weight_grad", ("mpo_patch_weight_grad",), dict(rows=33, E=128, pd=1024)),
            Case("patch_weight_grad-257-512x512", "patch_weight_grad", ("mpo_patch_weight_grad",), dict(rows=257, E=512, pd=512)),
            Case("patch_epilogue_backward-33x256", "patch_epilogue_backward", ("mpo_patch_epilogue_backward",), dict(rows=33, cols=256, drop_p=0.25)),
            # several workgroups add their partial sums into `out` with atomicAdd: the order of the additions is not fixed
            Case("colsum_bf16-257x256", "colsum_bf16", ("mpo_colsum_bf16",), dict(rows=257, cols=256),
                 atomic="multimodal_path_omic_amd/csrc/patch_epilogue.hip:94"),
            Case("map_blocks-q6", "map_blocks", ("mpo_map_block_dot", "mpo_map_block_scale", "mpo_map_block_stats"), dict(lengths=W_EDGES, n_q=6)),
            Case("map_blocks-q1", "map_blocks", ("mpo_map_block_dot", "mpo_map_block_scale", "mpo_map_block_stats"), dict(lengths=W_ONE, n_q=1))]


CASES = _mcat_cases() + _patch_cases() + _nacagat_cases() + _other_cases()
WORST = {}                 # entry group -> {quantity: (worst error, bar)} over the cases that ran (printed by the GPU file)


def run_case(dev, case):
    """Both fills; asserts every bar and the bit-equality of the two runs (or names the atomic that excuses it)."""
    runs = {}
    for tag, value in FILLS.items():
        runs[tag] = RUNNERS[case.runner](dev, value, **case.kw)
        for name, (err, bar) in runs[tag].errs.items():
            print(f"[buffer contract] {case.id} fill={tag}: {name} {err:.3e} (bar {bar:.3e})")
            w = WORST.setdefault(case.runner, {})
            if name not in w or err / max(bar, 1e-300) > w[name][0] / max(w[name][1], 1e-300):
                w[name] = (err, bar)
        for name, (err, bar) in runs[tag].errs.items():
            assert (err == 0.0) if bar == 0.0 else (err < bar), (case.id, tag, name, err, bar)
    if case.atomic is None:
        a, b = runs["nan"].outs, runs["finite"].outs
        assert a.keys() == b.keys()
        for name in a:
            if not bit_equal(a[name], b[name]):
                diff = int((_ints(a[name]) != _ints(b[name])).sum())
                raise AssertionError(f"{case.id}: {name} differs between the NaN fill and the finite fill in {diff} of {a[name].numel()} elements")
    return runs


# ----------------------------------------------------------------------------------------------------------- the ledger
# Every entry of include/*.h with a pointer-to-non-const parameter is a case above, or held by an existing test that places
# its buffers between guards, or listed here with the reason it is not held yet.
HELD_BY = {
    "mpo_linear_forward": "tests/test_gpu_gemm_routes.py::test_linear_entries_at_dispatch_edges",
    "mpo_linear_backward_input": "tests/test_gpu_gemm_routes.py::test_linear_entries_at_dispatch_edges",
    "mpo_linear_backward_weight": "tests/test_gpu_gemm_routes.py::test_linear_entries_at_dispatch_edges",
    "mpo_encoder_forward": "tests/test_gpu_tail_edges.py::test_encoder_edges",
    "mpo_encoder_backward": "tests/test_gpu_tail_edges.py::test_encoder_edges",
    "mpo_gated_pool_forward": "tests/test_gpu_tail_edges.py::test_gated_pool_edges",
    "mpo_gated_pool_backward": "tests/test_gpu_tail_edges.py::test_gated_pool_edges",
    "mpo_bag_self_attention_forward": "tests/test_gpu_bag_selfattn_edges.py::test_small_edges",
    "mpo_bag_self_attention_backward": "tests/test_gpu_bag_selfattn_edges.py::test_small_edges",
    "mpo_gated_concat_head_forward": "tests/test_gpu_fusion_next.py::test_entries_match_fp64_at_every_slide_tile_edge",
    "mpo_gated_concat_head_backward": "tests/test_gpu_fusion_next.py::test_entries_match_fp64_at_every_slide_tile_edge",
    "mpo_gated_concat_head_loss_forward": "tests/test_gpu_fusion_next.py::test_entries_match_fp64_at_every_slide_tile_edge",
    "mpo_gated_concat_head_loss_backward": "tests/test_gpu_fusion_next.py::test_entries_match_fp64_at_every_slide_tile_edge",
    "mpo_bilinear_head_forward": "tests/test_gpu_fusion_next.py::test_bilinear_entries_match_fp64_at_every_slide_tile_edge",
    "mpo_bilinear_head_backward": "tests/test_gpu_fusion_next.py::test_bilinear_entries_match_fp64_at_every_slide_tile_edge",
    "mpo_bilinear_head_loss_forward": "tests/test_gpu_fusion_next.py::test_bilinear_entries_match_fp64_at_every_slide_tile_edge",
    "mpo_bilinear_head_loss_backward": "tests/test_gpu_fusion_next.py::test_bilinear_entries_match_fp64_at_every_slide_tile_edge",
}
GUARD_WORDS = ("Guarded", "Placed", "GUARD")        # what a held_by file must use: one of the two helpers, or guards of its own

_FOLLOW_UP = "follow-up: no guarded placement yet"
NOT_HELD = {name: _FOLLOW_UP for name in (
    # the roofline legs of bench.py and the weight packer
    "mpo_patch_coattn_fwd_bagpass", "mpo_pack_patch_weight", "mpo_coattn_fwd_bagpass", "mpo_nacagat_fwd_bagpass", "mpo_coattn_bwd_bagpass",
    "mpo_patch_epilogue_forward",
    # optimisers and step counters (in-out state)
    "mpo_adam_step_flat", "mpo_optim_step_flat", "mpo_abs_sum_flat", "mpo_step_counters_bump", "mpo_grad_norm_flat", "mpo_optim_step_flat_guarded",
    # heads and losses outside the two fusion heads above
    "mpo_fusion_head_forward", "mpo_fusion_head_backward", "mpo_survival_head_forward", "mpo_survival_head_backward", "mpo_ces_loss_forward",
    "mpo_ces_loss_backward", "mpo_fusion_head_loss_forward", "mpo_fusion_head_loss_backward", "mpo_sct_loss_forward", "mpo_sct_loss_backward",
    "mpo_fusion_head_sct_loss_forward", "mpo_ge_head_loss_forward", "mpo_ge_head_loss_backward",
    # CAG and the omic SNN
    "mpo_cag_forward", "mpo_cag_backward", "mpo_omic_snn_forward", "mpo_omic_snn_backward",
    # samplers, cohorts, metrics, the feature scale
    "mpo_bag_sample_bind", "mpo_bag_sample_rows", "mpo_bag_sample_indices_host", "mpo_bag_sample_bind_slides", "mpo_bag_sample_slides",
    "mpo_class_metrics", "mpo_concordance_index", "mpo_feature_range_f32")}

_DECL_ARGS = L._DECL


def entries_with_outputs(header_text):
    """Names of the entries declared in a header that take a pointer to non-const data (what they may write through)."""
    import re
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    text = re.sub(r"//[^\n]*|^[ \t]*#.*$", " ", text, flags=re.M)
    names = []
    for m in _DECL_ARGS.finditer(text):
        _, name, args = m.groups()
        if any("*" in a and "const" not in a.split("*")[0] for a in args.split(",")):
            names.append(name)
    return names
