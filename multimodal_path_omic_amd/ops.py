"""torch.autograd.Function wrappers around the C-ABI entries of libmpo_hip.so.

One Function per kernel family of SURVEY.md section 2 (K1..K6).  Each forward/backward is ONE call
across the ABI; the sequence of kernel launches lives in csrc/capi.hip.  K2 alone makes more: one core call
each way, the key projection K = H W_k^T + b_k in front of it and that projection's gradients behind it, on a route
chosen once in the forward (_key_route).  Buffers (outputs, saved tensors, workspaces) are torch allocations; the library keeps nothing.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import List, Optional

import torch

from . import _lib as L


# Upper bound on the workgroups of a window's work plan (None: one per CU).  A measurement knob (tools/gpu_probe_overlap.py):
# persistent bag kernels on fewer CUs leave the rest to whatever another stream launches.
plan_workgroups = None
# Workgroups of the patch layer's weight-gradient kernel (None / 0: one per CU).  A data-parallel step sets 224: the kernel is
# persistent and owns its CUs outright, so the gradient all-reduce that runs beside it on another stream needs CUs of its own
# (measured with tools/gpu_probe_dp_overlap.py).
wgrad_workgroups = None


@dataclass
class BagBatch:
    """A window of slides' bags concatenated along rows ("ragged").

    data  (total_rows, E) fp32 or bf16;  cu  device int32 (n_slides+1) row offsets;
    lengths  host list of M_b (grid sizing needs max and total on the host, without a sync).
    """
    data: torch.Tensor
    cu: torch.Tensor
    lengths: List[int]
    _plan: object = None
    sampler_source = "window"       # which RowSampler reads this kind of window
    cycle = False                   # (a contiguous window is never lapped: SlideSet.cycle)

    def __post_init__(self):
        # an empty bag has no softmax (the reference's nn.MultiheadAttention returns NaN for it): refuse it here, before a
        # workgroup-less slide reaches the kernels
        if len(self.lengths) == 0 or any(int(m) <= 0 for m in self.lengths):
            raise ValueError(f"every slide of a window needs at least one patch row (lengths {list(self.lengths)[:8]}...)")
        if int(self.data.shape[0]) != sum(int(m) for m in self.lengths):
            raise ValueError(f"{int(self.data.shape[0])} rows for lengths summing to {sum(self.lengths)}")

    def plan(self):
        """Work plan of the bag passes (mpo_bag_plan): rows per workgroup uniform over the whole window, so every
        slide gets row ranges in proportion to its length.  Built once per window (one small H2D copy), kept alive
        with the batch; returns a ctypes pointer for the C ABI."""
        if self._plan is None:
            target = L.lib().mpo_coattn_target_workgroups()
            if plan_workgroups is not None:             # (fewer row ranges than CUs: leaves CUs to kernels of another stream)
                target = max(len(self.lengths), min(target, int(plan_workgroups)))
            rpw = -(-self.total_rows // target)
            rpw = max(32, -(-rpw // 32) * 32)
            # every slide rounds its workgroup count up: grow the range until the WHOLE window fits one workgroup per CU
            # (a window with more slides than CUs cannot).  A second, nearly empty round of workgroups costs a 50-us bag
            # pass little, but doubles the 0.4-ms persistent patch-layer kernel (measured on the 2k-30k windows, r02).
            while len(self.lengths) <= target and sum(-(-m // rpw) for m in self.lengths) > target:
                rpw += 32
            starts = [0]
            for m in self.lengths:
                starts.append(starts[-1] + -(-m // rpw))
            wg = torch.tensor(starts, dtype=torch.int32).to(self.data.device, non_blocking=True)
            c = L.BagPlanC(L.ptr(wg), starts[-1], rpw)
            self._plan = (wg, c)
        return ctypes.byref(self._plan[1])

    @property
    def n_slides(self):
        return len(self.lengths)

    @property
    def total_rows(self):
        return int(self.data.shape[0])

    @property
    def max_rows(self):
        return max(self.lengths)

    # what a window of either kind (this one, SlideSet) says about its rows
    @property
    def width(self):
        return int(self.data.shape[1])

    @property
    def dtype(self):
        return self.data.dtype

    @property
    def device(self):
        return self.data.device

    def row_tensors(self):
        """The tensors that hold the window's rows (what RowSampler.check looks at)."""
        return [self.data]

    @staticmethod
    def from_list(bags: "List[torch.Tensor]") -> "BagBatch":
        lengths = [int(b.shape[0]) for b in bags]
        data = bags[0] if len(bags) == 1 else torch.cat(bags, 0)
        return BagBatch(data.contiguous(), make_cu(lengths, data.device), lengths)

    @staticmethod
    def from_lengths(data: torch.Tensor, lengths: "List[int]") -> "BagBatch":
        """Rows already concatenated (e.g. a window slab shipped by ingest.WindowFeeder)."""
        lengths = [int(m) for m in lengths]
        if int(data.shape[0]) != sum(lengths):
            raise ValueError(f"{int(data.shape[0])} rows for lengths summing to {sum(lengths)}")
        return BagBatch(data, make_cu(lengths, data.device), lengths)

    def with_data(self, data: torch.Tensor) -> "BagBatch":
        assert data.shape[0] == self.total_rows
        return BagBatch(data, self.cu, self.lengths, self._plan)

    def split_map(self, flat_map: torch.Tensor, n_q: int) -> "List[torch.Tensor]":
        """Ragged attention map -> list of (n_q, M_b) views (slide b starts at n_q * cu[b]).  The list also carries the
        flat tensor (`.flat`, `.batch`, `.n_q`) for window-level consumers such as the attention-regularised loss."""
        out, off = RaggedMaps(), 0
        out.flat, out.batch, out.n_q = flat_map, self, n_q
        for m in self.lengths:
            out.append(flat_map[n_q * off:n_q * (off + m)].view(n_q, m))
            off += m
        return out


@dataclass
class SlideSet:
    """A window of SEPARATELY stored slides: what a shuffled epoch over a cohort resident on the device hands to the sampled
    step instead of a contiguous BagBatch (harness.ResidentCohort.window; csrc/bag_sample.hip gathers from it).

    slides   per-slide (M_b, width) row tensors or views into slabs, in window order (kept alive here);
    lengths  host list of M_b;
    table_ptrs / table_lens  DEVICE int64 / int32 [n_table]: address of the first row and row count of every slide the ids
             may name (a cohort's table, written once);
    ids      DEVICE int32 [n_slides]: the window, as indices into the table (in practice a slice of the epoch's order);
    cycle    a slide shorter than the sampler's k is lapped in its permuted order (row j <- pi_b(j mod M_b)) instead of
             being passed whole, so the sampled window has the static shape (n_slides * k, width) whatever the lengths.
    Only the row sampler reads a SlideSet; every bag kernel reads a contiguous window: materialize().
    `slides` / `lengths` (host) and `ids` (device) must name the same slides: the host side decides what RowSampler.check
    accepts and which lengths the output batch claims, the device side what the gather reads, and nothing compares the two (that
    would be a host synchronisation per window).  A mismatch stays in bounds -- the kernel takes lengths and pointers from the
    table alone -- but is silent: a static step would run on rows the batch's lengths do not describe.  ResidentCohort.window
    and from_batch build both sides from one list."""
    slides: List[torch.Tensor]
    lengths: List[int]
    table_ptrs: torch.Tensor
    table_lens: torch.Tensor
    ids: torch.Tensor
    cycle: bool = False
    sampler_source = "slides"

    def __post_init__(self):
        self.lengths = [int(m) for m in self.lengths]
        if len(self.lengths) == 0 or any(m <= 0 for m in self.lengths):
            raise ValueError(f"every slide of a window needs at least one patch row (lengths {self.lengths[:8]}...)")
        if len(self.slides) != len(self.lengths) or int(self.ids.numel()) != len(self.lengths):
            raise ValueError(f"SlideSet: {len(self.slides)} slides, {len(self.lengths)} lengths and {int(self.ids.numel())} ids")
        if self.ids.dtype != torch.int32 or self.table_lens.dtype != torch.int32 or self.table_ptrs.dtype != torch.int64:
            raise ValueError("SlideSet: ids and table_lens are int32, table_ptrs int64 (device addresses)")
        if self.table_ptrs.numel() != self.table_lens.numel():
            raise ValueError("SlideSet: table_ptrs and table_lens differ in length")

    @property
    def n_slides(self):
        return len(self.lengths)

    @property
    def n_table(self):
        return int(self.table_lens.numel())

    @property
    def width(self):
        return int(self.slides[0].shape[1])

    @property
    def dtype(self):
        return self.slides[0].dtype

    @property
    def device(self):
        return self.slides[0].device

    def row_tensors(self):
        return self.slides

    @staticmethod
    def slide_table(slides: "List[torch.Tensor]"):
        """(table_ptrs int64, table_lens int32) on the slides' device for row tensors that stay where they are: one small
        H2D copy each.  Every slide contiguous, (M, width), its first row 16-byte aligned."""
        for i, x in enumerate(slides):
            if x.dim() != 2 or not x.is_contiguous() or x.data_ptr() % 16:
                raise ValueError(f"SlideSet: slide {i} must be a contiguous (M, width) tensor whose first row is 16-byte aligned")
        dev = slides[0].device
        return (torch.tensor([x.data_ptr() for x in slides], dtype=torch.int64).to(dev, non_blocking=True),
                torch.tensor([int(x.shape[0]) for x in slides], dtype=torch.int32).to(dev, non_blocking=True))

    @staticmethod
    def from_batch(bags: "BagBatch", cycle: bool = False) -> "SlideSet":
        """A contiguous window presented as separately addressed slides: views of its slides, identity ids."""
        slides = list(bags.data.split(bags.lengths))
        ptrs, lens = SlideSet.slide_table(slides)
        ids = torch.arange(len(slides), dtype=torch.int32).to(bags.data.device, non_blocking=True)
        return SlideSet(slides, list(bags.lengths), ptrs, lens, ids, bool(cycle))

    def materialize(self) -> "BagBatch":
        """The contiguous window, by one torch.cat: for whatever needs every row (eval mode)."""
        return BagBatch.from_list(list(self.slides))


class RaggedMaps(list):
    """list of per-slide (n_q, M_b) views + the flat ragged tensor they alias."""
    flat: Optional[torch.Tensor] = None
    batch: Optional["BagBatch"] = None
    n_q: int = 0


def make_cu(lengths, device):
    cu = [0]
    for m in lengths:
        if m < 1:
            raise ValueError("every slide needs at least one patch")
        cu.append(cu[-1] + int(m))
    return torch.tensor(cu, dtype=torch.int32).to(device, non_blocking=True)


def grad_out(p):
    """Where a Function's backward writes the gradient of parameter `p`.

    With dp.FlatGradBucket every parameter owns a slice of ONE flat fp32 gradient buffer.  While `p.grad`
    is still unset in this window the kernels write straight into that slice and the returned view is
    adopted by autograd as `p.grad` (no accumulate kernel); otherwise a fresh tensor is returned and
    autograd adds it."""
    view = getattr(p, "_mpo_grad_view", None)
    if view is not None and p.grad is None and not getattr(p, "_mpo_slice_taken", False):
        # the slice is handed out ONCE per window (FlatGradBucket.begin() clears the flag): the kernels overwrite their
        # gradient outputs, so a second producer of the same parameter (two forwards before one backward, tied
        # weights) gets its own tensor and autograd adds the two
        p._mpo_slice_taken = True
        return view.view(p.shape)          # a FRESH alias: autograd only steals a gradient nobody else references
    return torch.empty_like(p)


_rng_epoch_tensor = None


def set_rng_epoch(t):
    """Install (or clear with None) the device uint64 scalar the kernels add (x 2^40) to their dropout offsets;
    harness.GraphedWindowStep bumps it inside the captured graph so replays draw fresh masks."""
    global _rng_epoch_tensor
    _rng_epoch_tensor = t


def _epoch():
    return L.ptr(_rng_epoch_tensor) if _rng_epoch_tensor is not None else None


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------ linear
class LinearFn(torch.autograd.Function):
    """y = act(x W^T + b) on the fp32 MFMA GEMM (stands in for torch.nn.functional.linear on the small-row tail)."""

    @staticmethod
    def forward(ctx, x, weight, bias, act: str = "none"):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        y = torch.empty(x2.shape[0], weight.shape[0], device=x.device, dtype=torch.float32)
        L.call("mpo_linear_forward", L.ptr(x2), L.ptr(weight), L.ptr(bias), L.ptr(y), x2.shape[0],
               weight.shape[1], weight.shape[0], 1.0, L.ACT[act], L.stream_of(x))
        ctx.save_for_backward(x2, weight, y)
        ctx.act = act
        ctx.has_bias = bias is not None
        ctx.xshape = x.shape
        return y.view(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, weight, y = ctx.saved_tensors
        dy = dy.reshape(-1, dy.shape[-1]).contiguous()
        if ctx.act == "relu":
            dy = dy * (y > 0)
        elif ctx.act == "tanh":
            dy = dy * (1 - y * y)
        elif ctx.act == "sigmoid":
            dy = dy * (y * (1 - y))
        elif ctx.act == "elu":
            dy = dy * torch.where(y > 0, torch.ones_like(y), y + 1)
        dy = dy.contiguous()
        R, I, O = x2.shape[0], weight.shape[1], weight.shape[0]
        dx = torch.empty_like(x2) if ctx.needs_input_grad[0] else None      # (raw patch features take no gradient)
        dw = torch.empty_like(weight)
        db = torch.empty(O, device=dy.device, dtype=torch.float32) if ctx.has_bias else None
        s = L.stream_of(dy)
        if dx is not None:
            L.call("mpo_linear_backward_input", L.ptr(dy), L.ptr(weight), L.ptr(dx), R, I, O, 1.0, 0, s)
        L.call("mpo_linear_backward_weight", L.ptr(dy), L.ptr(x2), L.ptr(dw), L.ptr(db), R, I, O, 1.0, s)
        return (dx.view(ctx.xshape) if dx is not None else None), dw, db, None


def linear(x, weight, bias=None, act="none"):
    return LinearFn.apply(x, weight, bias, act)


# ------------------------------------------------------------------------------------ K1
class CoAttnMCATFn(torch.autograd.Function):
    """MCAT co-attention over a ragged window (models/mcat/mcat.py:97)."""

    @staticmethod
    def forward(ctx, query, bag_data, in_w, in_b, out_w, out_b, batch: BagBatch, need_weights: bool,
                bag_relu_gate: float = 0.0):
        lib = L.lib()
        ctx.set_materialize_grads(False)
        ctx.bag_relu_gate = float(bag_relu_gate)
        ctx.bag_bias = getattr(bag_data, "_mpo_bias_param", None)
        n_slides = batch.n_slides
        R, E = query.shape
        n_q = R // n_slides
        dev = query.device
        query = query.contiguous()
        out = torch.empty(R, E, device=dev, dtype=torch.float32)
        amap = torch.empty(n_q * batch.total_rows, device=dev, dtype=torch.float32) if need_weights else None
        saved = torch.empty(lib.mpo_coattn_saved_floats(n_slides, n_q, E), device=dev, dtype=torch.float32)
        ws = _workspace(lib.mpo_coattn_workspace_bytes(n_slides, n_q, E, batch.max_rows), dev)
        L.call("mpo_coattn_mcat_forward",
            L.ptr(bag_data), L.bag_dtype_code(bag_data), L.ptr(batch.cu), n_slides, batch.total_rows, batch.max_rows,
            L.ptr(query), n_q, E, L.ptr(in_w), L.ptr(in_b), L.ptr(out_w), L.ptr(out_b),
            L.ptr(out), L.ptr(amap), L.ptr(saved), batch.plan(), L.ptr(ws), ws.numel(), L.stream_of(query))
        ctx.save_for_backward(query, bag_data, in_w, out_w, saved, amap)
        ctx.param_refs = (in_w, in_b, out_w, out_b)
        ctx.batch = batch
        ctx.n_q = n_q
        return out, amap          # the map (if any) is differentiable: backward accepts its gradient

    @staticmethod
    def backward(ctx, d_out, d_map):
        lib = L.lib()
        query, bag_data, in_w, out_w, saved, amap = ctx.saved_tensors
        batch, n_q = ctx.batch, ctx.n_q
        R, E = query.shape
        dev = query.device
        d_out = d_out.contiguous() if d_out is not None else torch.zeros(R, E, device=dev)
        if d_map is not None:
            d_map = d_map.contiguous()
        d_query = torch.empty_like(query)
        d_bag = torch.empty_like(bag_data)
        # with the fused gate d_bag IS the patch layer's pre-activation gradient: its column sums (that layer's bias
        # gradient) fall out of the kernel's copy-out loop and travel on the tensor to PatchFcFn.backward
        colsum = _bias_grad_slot(ctx.bag_bias, E, dev) if ctx.bag_relu_gate != 0.0 else None
        d_in_w, d_in_b, d_out_w, d_out_b = (grad_out(p) for p in ctx.param_refs)
        ws = _workspace(lib.mpo_coattn_workspace_bytes(batch.n_slides, n_q, E, batch.max_rows), dev)
        L.call("mpo_coattn_mcat_backward",
            L.ptr(bag_data), L.bag_dtype_code(bag_data), L.ptr(batch.cu), batch.n_slides, batch.total_rows,
            batch.max_rows, L.ptr(query), n_q, E, L.ptr(in_w), L.ptr(out_w), L.ptr(saved), L.ptr(amap),
            L.ptr(d_out), L.ptr(d_map), L.ptr(d_query), 0, L.ptr(d_bag), L.ptr(colsum), L.ptr(d_in_w), L.ptr(d_in_b),
            L.ptr(d_out_w), L.ptr(d_out_b), ctx.bag_relu_gate, batch.plan(), L.ptr(ws), ws.numel(), L.stream_of(query))
        if colsum is not None:
            d_bag._mpo_colsum = colsum
        return d_query, d_bag, d_in_w, d_in_b, d_out_w, d_out_b, None, None, None


def coattn_mcat(query, batch: BagBatch, in_w, in_b, out_w, out_b, need_weights: bool, bag_relu_gate: float = 0.0):
    """query (n_slides*n_q, E) -> (out (n_slides*n_q, E), ragged map or None).
    bag_relu_gate = 1/(1-p) when the bag comes from patch_fc(..., pre_gated_grad=True): d_bag then already
    carries the ReLU/dropout derivative (see include/mpo_hip.h)."""
    return CoAttnMCATFn.apply(query, batch.data, in_w, in_b, out_w, out_b, batch, need_weights, bag_relu_gate)


# counters the tests read to make sure a fused path really ran.  qpass_*: how a hand-on op's backward (the query handed on
# by patch_coattn_mcat / coattn_nacagat / contextual_gate) met the gradient of that query -- accumulated in place on a
# buffer the caller's wiring owns, or on a copy (see _query_grad_buffer)
stats = {"colsum_handoffs": 0, "qpass_in_place": 0, "qpass_copied": 0, "head_loss_ces": 0, "head_loss_sct": 0,
         "head_loss_ce": 0, "gated_concat_head": 0, "bilinear_head": 0}


def _query_grad_buffer(d_qpass, owned: bool, query):
    """-> (where a hand-on op's backward writes d_query, accumulate flag).  The kernels accumulate d_query onto the gradient
    of the handed-on query.  Autograd may share that tensor with other consumers (an add's two inputs, a tensor hook,
    the op's own other output), so the sum goes in place only when the caller's wiring owns the buffer (`owned`: the
    TokenPair slice the model's window step hands in); otherwise it goes onto a copy."""
    if d_qpass is None:
        return torch.empty_like(query), False
    if owned:
        stats["qpass_in_place"] += 1
        return d_qpass.contiguous(), True
    stats["qpass_copied"] += 1
    return d_qpass.clone(memory_format=torch.contiguous_format), True


def _bias_grad_slot(bag_param, E, dev):
    """Where a co-attention backward writes the column sums of its (pre-gated) d_bag = the bias gradient of the patch
    layer that produced the bag: straight into that bias's slice of the flat gradient bucket when patch_fc() tagged the
    bag with its bias and the slice is still unset (PatchFcFn.backward then finds the data in place and skips its copy),
    else a fresh tensor that travels on d_bag."""
    if bag_param is not None and getattr(bag_param, "_mpo_grad_view", None) is not None and bag_param.grad is None \
            and bag_param.numel() == E and not getattr(bag_param, "_mpo_slice_taken", False):
        return bag_param._mpo_grad_view.view(E)         # (PatchFcFn.backward's grad_out(bias) then claims this slice)
    return torch.empty(E, device=dev, dtype=torch.float32)

# Data-parallel steps split the backward in two: everything except the patch layer's weight gradient (dW_H = g^T X on
# csrc/patch_wgrad.hip, which nothing downstream waits for) runs first, then the all-reduce of all other gradients is
# started and dW_H is computed WHILE that collective runs (harness.GraphedWindowStep(split_patch_grad=True)).
defer_patch_weight_grad = False
_deferred_patch = []

def flush_patch_weight_grads():
    """Compute the patch-layer weight gradients PatchFcFn.backward queued (into the bucket slices it already returned)."""
    for g, x, dw in _deferred_patch:
        patch_weight_grad(g, x, dw)
    _deferred_patch.clear()

def _patch_weight_grad_now_or_deferred(g, x, dw, weight):
    """dW_H = g^T X into dw: queued for flush_patch_weight_grads() when the split exchange is on and dw IS the weight's slice
    of the flat gradient bucket (the caller has already returned it), else computed now."""
    if defer_patch_weight_grad and getattr(weight, "_mpo_grad_view", None) is not None \
            and dw.data_ptr() == weight._mpo_grad_view.data_ptr():
        _deferred_patch.append((g, x, dw))
    else:
        patch_weight_grad(g, x, dw)


# ------------------------------------------------------------------------------------ patch layer (row H2)
class PatchFcFn(torch.autograd.Function):
    """H_bag = dropout_p(relu(X W_H^T + b)) for a bf16-stored window (models/mcat/mcat.py:24-29,87).

    Forward: one pass of csrc/patch_fc_fwd.hip (patch_dim 512 / 1024 / 2048, embed 128 / 256 / 512: the same kernel, see its
    header), the dropout mask kept
    in H_bag as zeros.  Backward: the ReLU / dropout derivative (in the consumer's kernel when it can, else one element-wise
    pass) and dW_H = g^T X on csrc/patch_wgrad.hip.  X never needs a gradient (it is data).  Other geometries raise."""

    @staticmethod
    def forward(ctx, x, weight, bias, drop_p: float, pre_gated_grad: bool, batch=None):
        lib = L.lib()
        if not patch_fc_kernel_supported(x, weight):
            raise ValueError(f"patch layer: built for a contiguous bf16 window through Linear(512 | 1024 | 2048, 128 | 256 | 512) "
                             f"(patch_dim in {set(PATCH_DIMS)}; got {x.dtype} {tuple(x.shape)} through a weight {tuple(weight.shape)})")
        if batch is None:                   # a bare patch matrix: one slide
            batch = BagBatch(x, make_cu([x.shape[0]], x.device), [x.shape[0]])
        h = torch.empty(x.shape[0], weight.shape[0], device=x.device, dtype=torch.bfloat16)
        realised = _realised_drop(drop_p) if drop_p > 0 else 0.0
        seed, off = _reserve(h.numel() // 16 + 2) if drop_p > 0 else (0, 0)
        ws = _workspace(lib.mpo_patch_fc_workspace_bytes(weight.shape[0], weight.shape[1]), x.device)
        L.call("mpo_patch_fc_forward", L.ptr(x), L.ptr(batch.cu), batch.n_slides, batch.total_rows, batch.max_rows,
               x.shape[1], L.ptr(weight), L.ptr(bias), weight.shape[0], float(drop_p), seed, off,
               _epoch(), L.ptr(h), batch.plan(), L.ptr(ws), ws.numel(), L.stream_of(x))
        ctx.save_for_backward(x, h)
        ctx.param_refs = (weight, bias)
        ctx.drop_p, ctx.pre_gated = float(realised), bool(pre_gated_grad)
        return h

    @staticmethod
    def backward(ctx, dh):
        lib = L.lib()
        x, h = ctx.saved_tensors
        dh = dh.contiguous()
        if ctx.pre_gated:
            g = dh
        else:
            g = None
        dw, db = (grad_out(p) for p in ctx.param_refs)
        if g is None:                       # ReLU/dropout derivative + the bias gradient (column sums) in one pass
            g = torch.empty_like(dh)
            ws = _workspace(lib.mpo_patch_epilogue_backward_workspace_bytes(g.numel(), g.shape[1]), g.device)
            L.call("mpo_patch_epilogue_backward", L.ptr(h), L.ptr(dh), L.ptr(g), g.numel(), g.shape[1], ctx.drop_p,
                   L.ptr(db), L.ptr(ws), ws.numel(), L.stream_of(g))
        else:
            ready = getattr(dh, "_mpo_colsum", None)
            if ready is not None and ready.shape == db.shape:
                if ready.data_ptr() != db.data_ptr():       # (already in the bucket slice when patch_fc tagged the bag)
                    db.copy_(ready)         # produced by the co-attention backward kernel while it wrote dh
                stats["colsum_handoffs"] += 1
            else:
                _colsum_two_stage(g, db)
        _patch_weight_grad_now_or_deferred(g, x, dw, ctx.param_refs[0])
        return None, dw, db, None, None, None


def _colsum_two_stage(g: torch.Tensor, out: torch.Tensor, block: int = 256) -> torch.Tensor:
    """Column sums of a tall bf16 matrix in fp32: (rows/256, 256, d) -> sum(1) -> sum(0).  One flat torch.sum over
    480k rows runs at 1.7-2.4 TB/s (101-142 us); the blocked form takes 56 us (measured r01)."""
    rows, d = g.shape
    main = rows // block * block
    if main:
        torch.sum(g[:main].view(rows // block, block, d).sum(1, dtype=torch.float32), 0, out=out)
    else:
        out.zero_()
    if main < rows:
        out += g[main:].sum(0, dtype=torch.float32)
    return out


def patch_weight_grad(g: torch.Tensor, x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """dW_H = g^T x into `out` (embed, patch_dim) fp32 on csrc/patch_wgrad.hip: bf16 operands, embed 128 / 256 / 512,
    patch_dim 128, 256, 512, 1024 or 2048, any number of rows (4 GiB of patches and more go in row segments).  Anything else raises."""
    e, k = out.shape
    if not (g.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and e in (128, 256, 512) and k in (128, 256, 512, 1024, 2048)
            and g.shape == (x.shape[0], e) and x.shape[1] == k
            and g.is_contiguous() and x.is_contiguous() and out.is_contiguous() and out.dtype == torch.float32):
        raise ValueError(f"patch weight gradient: g {g.dtype} {tuple(g.shape)} x {x.dtype} {tuple(x.shape)} -> {tuple(out.shape)} is not a "
                         f"geometry the kernel is built for (contiguous bf16, embed 128/256/512, patch_dim 128/256/512/1024/2048)")
    lib = L.lib()
    ws = _workspace(lib.mpo_patch_weight_grad_workspace_bytes(e, k), g.device)
    wgs = int(wgrad_workgroups or 0)
    if wgs and k != 1024:
        wgs = 0                                        # (the setting is for the patch layer's own gradient, patch_dim 1024)
    L.call("mpo_patch_weight_grad", L.ptr(g), L.ptr(x), g.shape[0], e, k, L.ptr(out), wgs, L.ptr(ws), ws.numel(),
           L.stream_of(g))
    return out


def _patch_fc_split_forward(ctx, window, entry, x, weight, bias, drop_p, rate, *scale):
    """What PatchFcF32Fn.forward and PatchFcF16Fn.forward share (csrc/patch_fc_split.hip): H_bag, the dropout counters, the
    workspace, the call -- `rate` as the entry takes it (p, or round(256 p)), `scale` the fp32 window's feature scale -- and
    what the backward reads off ctx."""
    h = torch.empty(x.shape[0], weight.shape[0], device=x.device, dtype=torch.float32)
    seed, off = _reserve(h.numel() // 16 + 2) if drop_p > 0 else (0, 0)
    ws = _workspace(getattr(L.lib(), f"mpo_patch_fc_{window}_workspace_bytes")(0), x.device)
    L.call(entry, L.ptr(x), x.shape[0], x.shape[1], L.ptr(weight), L.ptr(bias), weight.shape[0], rate, seed, off, _epoch(), *scale,
           L.ptr(h), L.ptr(ws), ws.numel(), L.stream_of(x))
    ctx.save_for_backward(x, h)
    ctx.param_refs = (weight, bias)
    return h


def _patch_fc_split_backward(ctx, window, dh, rate):
    """The one backward pass of both windows; `rate` as the entry takes it (the fp32 window's gate, the fp16 window's drop_256)."""
    x, h = ctx.saved_tensors
    dh = dh.contiguous()
    dw, db = (grad_out(p) for p in ctx.param_refs)
    ws = _workspace(getattr(L.lib(), f"mpo_patch_fc_{window}_workspace_bytes")(1), x.device)
    L.call(f"mpo_patch_fc_{window}_backward", L.ptr(dh), L.ptr(h), L.ptr(x), x.shape[0], h.shape[1], x.shape[1], rate, L.ptr(dw),
           L.ptr(db), L.ptr(ws), ws.numel(), L.stream_of(x))
    return None, dw, db, None


class PatchFcF32Fn(torch.autograd.Function):
    """H_bag = dropout_p(relu(X W_H^T + b)) for an fp32-stored window through Linear(1024, 256) (models/mcat/mcat.py:24-29,87),
    hand-written both ways (csrc/patch_fc_split.hip): products as three bf16 MFMA terms of hi / lo operand splits (fp32
    accumulation, ~4e-6 absolute on H_bag), dropout mask kept in H_bag as zeros; backward = ONE pass that applies the
    ReLU / dropout derivative read off H_bag to the incoming gradient and forms dW_H = g^T X and db_H = colsum(g)."""

    @staticmethod
    def forward(ctx, x, weight, bias, drop_p: float):
        ctx.gate = 1.0 / (1.0 - _realised_drop(drop_p)) if drop_p > 0 else 1.0
        # a window that carries a device scale (feature_scale_device: a sampler's output, a captured step's window) is read
        # through it when the kernel starts; any other window's scale is found on the host and passed by value
        scale_dev = getattr(x, "_mpo_feature_scale_dev", None)
        entry, scale = ("mpo_patch_fc_f32_forward", feature_scale(x)) if scale_dev is None else \
                       ("mpo_patch_fc_f32_forward_dev", L.ptr(_check_scale_tensor(scale_dev, x)))
        return _patch_fc_split_forward(ctx, "f32", entry, x, weight, bias, drop_p, float(drop_p), scale)

    @staticmethod
    def backward(ctx, dh):
        return _patch_fc_split_backward(ctx, "f32", dh, ctx.gate)


def feature_scale(x) -> float:
    """The power of two that puts max |x| of an fp32 patch matrix into [2^14, 2^15): the fp16 operand splits of
    mpo_patch_fc_f32_forward then use fp16's range whatever the features' own scale (1e-4 or 1e4).  One reduction over the
    window and one host read, cached on the tensor (a resident window is scanned once; call it -- or one eager forward --
    before capturing a graph).  feature_scale_device finds the same number without the host read.

    The cache is keyed on the tensor's version counter, storage address and shape: an in-place write (mul_, copy_, a write
    through any view of the same base -- views share the counter) makes the next call scan again.  Inference tensors have
    no version counter and are scanned on every call."""
    if x.numel() == 0:
        return 1.0
    try:
        key = (x._version, x.data_ptr(), tuple(x.shape))
    except RuntimeError:                                # inference tensor: no version counter, nothing to key a cache on
        key = None
    cached = getattr(x, "_mpo_feature_scale", None) if key is not None else None
    if cached is not None and cached[:3] == key:
        return cached[3]
    if x.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("feature_scale(x) needs one host read: call ops.feature_scale(window.data) before capturing the graph")
    m = float(x.detach().abs().amax())
    s = math.ldexp(1.0, max(-100, min(100, 15 - math.frexp(m)[1]))) if (m > 0.0 and math.isfinite(m)) else 1.0
    if key is not None:
        try:
            x._mpo_feature_scale = (*key, s)
        except AttributeError:
            pass
    return s


def _check_scale_tensor(scale, x):
    if scale.shape != (1,) or scale.dtype != torch.float32 or scale.device != x.device or not scale.is_contiguous():
        raise ValueError(f"a device feature scale is one contiguous fp32 value on the window's device (got {tuple(scale.shape)} "
                         f"{scale.dtype} on {scale.device})")
    return scale


def feature_scale_device(x, out=None) -> torch.Tensor:
    """feature_scale(x) found on the device (csrc/feature_range.hip) -> a (1,) fp32 tensor on x's device (`out`, written
    in place, where given): the same bits for every x, with no full-size temporary and NO host read -- three tiny launches
    on the current stream, allowed inside a stream capture.  Nothing is cached: every call reads x as it is then.
    mpo_patch_fc_f32_forward_dev reads the result when its kernel starts; a window carries it as
    x._mpo_feature_scale_dev (PatchFcF32Fn.forward), beside the host cache _mpo_feature_scale."""
    if not x.is_cuda or x.dtype != torch.float32:
        raise ValueError(f"feature_scale_device: an fp32 tensor on the GPU (got {x.dtype} on {x.device})")
    out = torch.empty(1, dtype=torch.float32, device=x.device) if out is None else _check_scale_tensor(out, x)
    ws = _workspace(L.lib().mpo_feature_range_workspace_bytes(), x.device)
    L.call("mpo_feature_range_f32", L.ptr(x) if x.numel() else None, x.numel(), L.ptr(out), L.ptr(ws), ws.numel(), L.stream_of(x))
    return out


def patch_fc_f32_supported(x, weight) -> bool:
    """mpo_patch_fc_f32_*: an fp32 window through Linear(1024, 256)."""
    return x.dtype == torch.float32 and x.is_contiguous() and tuple(weight.shape) == (256, 1024)


def patch_fc_f32(x, weight, bias, drop_p: float):
    """H_bag = dropout(relu(x W^T + b)) in fp32 storage on the hand-written kernels (no library GEMM)."""
    return PatchFcF32Fn.apply(x, weight, bias, float(drop_p))


class PatchFcF16Fn(torch.autograd.Function):
    """H_bag = dropout_p(relu(X W_H^T + b)) for an fp16-stored window through Linear(1024, 256) (models/mcat/mcat.py:24-29,87),
    hand-written both ways (csrc/patch_fc_split.hip), H_bag in fp32: PatchFcF32Fn without a feature scale.  An fp16 feature is
    one fp16 MFMA operand as stored, so the forward takes two terms W_hi X + W_lo X (fp32 accumulation; against the fp64
    product of the stored operands only W's 2^-22 tail is lost) and the same dropout stream as the fp32 kernel: equal (seed,
    offset, epoch) give equal masks.  Backward = the fp32 window's ONE pass (ReLU / dropout derivative read off H_bag,
    dW_H = g^T X, db_H = colsum(g)) with X split exactly into bf16 hi + lo.  Like PatchFcF32Fn it computes dW_H inside
    backward whatever ops.defer_patch_weight_grad says (the split exchange defers the bf16 window's patch_weight_grad only)."""

    @staticmethod
    def forward(ctx, x, weight, bias, drop_p: float):
        if not patch_fc_f16_supported(x, weight):
            raise ValueError(f"fp16 patch layer: built for a contiguous fp16 window through Linear(1024, 256) (got {x.dtype} "
                             f"{tuple(x.shape)} through a weight {tuple(weight.shape)})")
        # the entries take the rate as the kernel realises it, in 256ths (one integer for both directions: mpo_patch_f16.h);
        # ctx.gate is the keep scale the backward entry forms from it
        ctx.drop_256 = int(round(_realised_drop(drop_p) * 256)) if drop_p > 0 else 0
        ctx.gate = 256.0 / (256.0 - ctx.drop_256)
        return _patch_fc_split_forward(ctx, "f16", "mpo_patch_fc_f16_forward", x, weight, bias, drop_p, ctx.drop_256)

    @staticmethod
    def backward(ctx, dh):
        return _patch_fc_split_backward(ctx, "f16", dh, ctx.drop_256)


def patch_fc_f16_supported(x, weight) -> bool:
    """mpo_patch_fc_f16_*: an fp16 window through Linear(1024, 256)."""
    return x.dtype == torch.float16 and x.is_contiguous() and x.dim() == 2 and x.shape[1] == 1024 and tuple(weight.shape) == (256, 1024)


def patch_fc_f16(x, weight, bias, drop_p: float):
    """H_bag (fp32) = dropout(relu(x W^T + b)) of an fp16 window on the hand-written kernels (no library GEMM, no fp32 copy
    of the window, no feature scale)."""
    return PatchFcF16Fn.apply(x, weight, bias, float(drop_p))


# ------------------------------------------------------------------------------------ row f1: patch layer + K1 in one call
class PatchCoAttnMCATFn(torch.autograd.Function):
    """H_bag = dropout_p(relu(X W_H^T + b_H)) AND MCAT's co-attention over it (models/mcat/mcat.py:24-29,87,97) in ONE
    C-ABI call, mpo_patch_coattn_mcat_forward: two bag launches, the patch-layer kernel over the raw bf16 patch matrix and K1's
    partial pass over the H_bag it wrote.  H_bag is written once (bf16) and kept for the
    backward, which is K1's backward pass (d_bag arrives already multiplied by the ReLU / dropout derivative, with its
    column sums = the patch layer's bias gradient) followed by the patch layer's weight gradient g^T X."""

    @staticmethod
    def forward(ctx, x, patch_w, patch_b, query, in_w, in_b, out_w, out_b, batch: BagBatch, need_weights: bool, drop_p: float,
                tokens: "TokenPair | None" = None, qpass_owned: bool = False):
        lib = L.lib()
        ctx.set_materialize_grads(False)
        n_slides = batch.n_slides
        R, E = query.shape
        n_q = R // n_slides
        dev, T = query.device, batch.total_rows
        query = query.contiguous()
        h_bag = torch.empty(T, E, device=dev, dtype=torch.bfloat16)
        out = tokens.slot(0, (R, E)) if tokens is not None else torch.empty(R, E, device=dev, dtype=torch.float32)
        amap = torch.empty(n_q * T, device=dev, dtype=torch.float32) if need_weights else None
        saved = torch.empty(lib.mpo_coattn_saved_floats(n_slides, n_q, E), device=dev, dtype=torch.float32)
        ws = _workspace(lib.mpo_patch_coattn_workspace_bytes(n_slides, n_q, E, x.shape[1]), dev)
        ctx.gate = 1.0 / (1.0 - _realised_drop(drop_p)) if drop_p > 0 else 1.0
        seed, off = _reserve(T * E // 16 + 2) if drop_p > 0 else (0, 0)
        L.call("mpo_patch_coattn_mcat_forward",
            L.ptr(x), L.ptr(batch.cu), n_slides, T, batch.max_rows, x.shape[1], L.ptr(patch_w), L.ptr(patch_b), float(drop_p),
            seed, off, _epoch(), L.ptr(query), n_q, E, L.ptr(in_w), L.ptr(in_b), L.ptr(out_w), L.ptr(out_b),
            L.ptr(h_bag), L.ptr(out), L.ptr(amap), L.ptr(saved), batch.plan(), L.ptr(ws), ws.numel(), L.stream_of(query))
        ctx.save_for_backward(x, h_bag, query, in_w, out_w, saved, amap)
        ctx.param_refs = (patch_w, patch_b, in_w, in_b, out_w, out_b)
        ctx.batch, ctx.n_q = batch, n_q
        ctx.qpass_owned = bool(qpass_owned)
        ctx.mark_non_differentiable(h_bag)
        # the query handed on to its second consumer (the omic branch's tokens): its gradient then arrives HERE and is
        # folded into the last GEMM of the backward (d_query += ...) instead of costing autograd an add launch
        return out, amap, h_bag, query.view_as(query)

    @staticmethod
    def backward(ctx, d_out, d_map, _d_h, d_qpass):
        lib = L.lib()
        x, h_bag, query, in_w, out_w, saved, amap = ctx.saved_tensors
        batch, n_q = ctx.batch, ctx.n_q
        R, E = query.shape
        dev = query.device
        d_out = d_out.contiguous() if d_out is not None else torch.zeros(R, E, device=dev)
        d_map = d_map.contiguous() if d_map is not None else None
        d_query, accumulate = _query_grad_buffer(d_qpass, ctx.qpass_owned, query)
        g = torch.empty_like(h_bag)               # d(pre-activation of the patch layer): ReLU/dropout derivative applied in-kernel
        patch_w, patch_b, p_in_w, p_in_b, p_out_w, p_out_b = ctx.param_refs
        d_pw, d_pb = grad_out(patch_w), grad_out(patch_b)
        d_in_w, d_in_b, d_out_w, d_out_b = (grad_out(p) for p in (p_in_w, p_in_b, p_out_w, p_out_b))
        ws = _workspace(lib.mpo_coattn_workspace_bytes(batch.n_slides, n_q, E, batch.max_rows), dev)
        L.call("mpo_coattn_mcat_backward",
            L.ptr(h_bag), L.MPO_BF16, L.ptr(batch.cu), batch.n_slides, batch.total_rows, batch.max_rows, L.ptr(query), n_q, E,
            L.ptr(in_w), L.ptr(out_w), L.ptr(saved), L.ptr(amap), L.ptr(d_out), L.ptr(d_map), L.ptr(d_query), int(accumulate),
            L.ptr(g), L.ptr(d_pb), L.ptr(d_in_w), L.ptr(d_in_b), L.ptr(d_out_w), L.ptr(d_out_b), ctx.gate, batch.plan(),
            L.ptr(ws), ws.numel(), L.stream_of(query))
        stats["colsum_handoffs"] += 1
        _patch_weight_grad_now_or_deferred(g, x, d_pw, patch_w)
        return None, d_pw, d_pb, d_query, d_in_w, d_in_b, d_out_w, d_out_b, None, None, None, None, None


class TokenPair:
    """(2, rows, d) fp32 buffer for the two token sets the branch-batched tail consumes (co-attention output | omic
    tokens).  Producers write their half in place (`slot`), `stack` hands the whole buffer to the encoder: the
    torch.stack copy and its backward disappear from the step."""

    def __init__(self, rows: int, d: int, device):
        self.buf = torch.empty(2, rows, d, device=device, dtype=torch.float32)

    def slot(self, i: int, shape):
        return self.buf[i].view(*shape)

    def stack(self, first, second):
        for i, t in enumerate((first, second)):
            if t.data_ptr() != self.buf[i].data_ptr() or t.numel() != self.buf[i].numel() or not t.is_contiguous():
                raise ValueError("TokenPair.stack: the halves must be the tensors produced into slot(0) and slot(1)")
        return _TokenPairFn.apply(first, second, self)


class _TokenPairFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, first, second, pair):
        ctx.shapes = (first.shape, second.shape)
        return pair.buf.view_as(pair.buf)

    @staticmethod
    def backward(ctx, d):
        return d[0].view(ctx.shapes[0]), d[1].view(ctx.shapes[1]), None


def _realised_drop(p: float) -> float:
    """The fused kernel draws 8 random bits per element: its drop probability is round(256 p) / 256.  A rate that rounds to
    256/256 would keep nothing (keep scale 256 / 0): refused here, in the C entries' words, before anything is reserved."""
    thr8 = int(p * 256.0 + 0.5)
    if thr8 > 255:
        raise ValueError(f"patch-layer dropout p = {p:g} is realised as round(256 p) / 256 = {thr8}/256: nothing would be kept "
                         f"(p must be below 1 - 1/512)")
    return float(thr8) / 256.0


def patch_coattn_mcat(x_bf16, batch: BagBatch, patch_w, patch_b, drop_p: float, query, in_w, in_b, out_w, out_b,
                      need_weights: bool, tokens: "TokenPair | None" = None, _qpass_owned: bool = False):
    """-> (out (n_slides*n_q, E), ragged map | None, H_bag (rows, E) bf16, not differentiable, query handed on).
    tokens: `out` is produced into tokens.slot(0).  Use the returned query (not the argument) for the query's other
    consumer: its gradient is then folded into this op's backward.  _qpass_owned (the model's TokenPair wiring only): the
    gradient arriving for the handed-on query is a buffer nobody else reads, so the backward may accumulate into it."""
    return PatchCoAttnMCATFn.apply(x_bf16, patch_w, patch_b, query, in_w, in_b, out_w, out_b, batch, need_weights,
                                   float(drop_p), tokens, bool(_qpass_owned))


def fused_patch_coattn_supported(x, embed: int, n_q: int) -> bool:
    """mpo_patch_coattn_mcat_forward is built for a bf16 window, 1024 -> 256, at most 8 omic queries."""
    return x.dtype == torch.bfloat16 and x.shape[1] == 1024 and embed == 256 and n_q <= 8


# Patch feature widths the bf16 patch layer is built for, forward (csrc/patch_fc_fwd.hip) and weight gradient
# (csrc/patch_wgrad.hip): the reference's truncated ResNet-50 (1024), CONCH / ResNet-18 / -34 (512), the full ResNet-50 (2048).
PATCH_DIMS = (512, 1024, 2048)


def patch_fc_kernel_supported(x, weight) -> bool:
    """mpo_patch_fc_forward: a bf16 window through Linear(512 | 1024 | 2048, 128 | 256 | 512)."""
    return (x.dtype == torch.bfloat16 and x.is_contiguous() and x.dim() == 2 and weight.shape[0] in (128, 256, 512)
            and weight.shape[1] in PATCH_DIMS and x.shape[1] == weight.shape[1])


def patch_fc(x_bf16, weight, bias, drop_p: float, pre_gated_grad: bool = False, batch: "BagBatch | None" = None):
    """H_bag = dropout(relu(x W^T + b)), bf16.  batch (the window's row offsets / work plan): lets the layer run as
    one hand-written pass; the tensor then carries `_mpo_keep_scale` = 1 / (1 - realised dropout rate) for consumers that
    apply the ReLU / dropout derivative themselves."""
    h = PatchFcFn.apply(x_bf16, weight, bias, drop_p, pre_gated_grad, batch)
    if pre_gated_grad:
        h._mpo_bias_param = bias          # lets the consumer's backward write this layer's bias gradient in place
    if drop_p > 0:
        h._mpo_keep_scale = 1.0 / (1.0 - _realised_drop(drop_p))
    return h


# ------------------------------------------------------------------------------------ tail (6 x d tokens per slide)
import torch.nn.functional as F  # noqa: E402


_rng_calls = 0          # counters handed out so far: the one place the dropout generator's counter space is carved


def _reserve(span: int):
    """Reserve `span` counters of the dropout generator for one C-ABI call's streams."""
    global _rng_calls
    seed = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
    off = _rng_calls
    _rng_calls += int(span) + 1
    return seed, off


def gated_scores(x, wa, ba, wb, bb, wc, bc, drop_p: float):
    """AttentionNetGated scores alone (models/blocks.py:42-47), for the module's stand-alone forward():
    HIP GEMMs (fused tanh / sigmoid) + the element-wise product.  x (..., L, D) -> (..., L, n_classes).
    The model path uses gated_pool(), which fuses scorer, pooling and rho in one C-ABI call."""
    a = linear(x, wa, ba, "tanh")
    b = linear(x, wb, bb, "sigmoid")
    if drop_p > 0.0:
        a = F.dropout(a, drop_p, True)
        b = F.dropout(b, drop_p, True)
    return linear(a * b, wc, bc)


class CagFn(torch.autograd.Function):
    """K3: ContextualAttentionGate (models/blocks.py:247-253), one C-ABI call each way.
    residual / dest: the caller's  residual + C  (models/blocks.py:110) is produced into `dest` by the forward's last launch (no
    element-wise pass).  The second output hands q on to its other consumers: their gradient then arrives HERE and the
    backward's d_q product accumulates onto it (no gradient-add launch)."""

    @staticmethod
    def forward(ctx, q, q_hat, residual, dest, qpass_owned, *params):
        lib = L.lib()
        ctx.set_materialize_grads(False)
        q, q_hat = q.contiguous(), q_hat.contiguous()
        rows, dim = q.shape
        hidden = params[0].shape[0]
        c = torch.empty(rows, hidden, device=q.device, dtype=torch.float32)
        saved = torch.empty(lib.mpo_cag_saved_floats(rows, hidden), device=q.device, dtype=torch.float32)
        pa = L.ptr_array(params)
        total = None
        if residual is not None:
            residual = residual.contiguous()
            # dest = (TokenPair, slot): a non-tensor argument -- the slot's view is created here, so autograd sees a fresh output
            total = dest[0].slot(dest[1], (rows, hidden)) if dest is not None else torch.empty_like(c)
        L.call("mpo_cag_forward", L.ptr(q), L.ptr(q_hat), rows, dim, hidden, pa, L.ptr(c), L.ptr(saved), L.ptr(residual),
               L.ptr(total), L.stream_of(q))
        ctx.save_for_backward(q, q_hat, c, saved, *params)
        ctx.param_refs = params
        ctx.has_residual = residual is not None
        ctx.qpass_owned = bool(qpass_owned)
        return (total if total is not None else c), q.view_as(q)

    @staticmethod
    def backward(ctx, dc, d_qpass):
        lib = L.lib()
        q, q_hat, c, saved, *params = ctx.saved_tensors
        rows, dim = q.shape
        hidden = params[0].shape[0]
        if dc is None:
            dc = torch.zeros_like(c)
        dc = dc.contiguous()
        dq, accumulate = _query_grad_buffer(d_qpass, ctx.qpass_owned, q)
        dqh = torch.empty_like(q_hat)
        grads = [grad_out(p) for p in ctx.param_refs]
        ws = _workspace(lib.mpo_cag_workspace_bytes(rows, hidden), q.device)
        pa, ga = L.ptr_array(params), L.ptr_array(grads)
        L.call("mpo_cag_backward", L.ptr(q), L.ptr(q_hat), rows, dim, hidden, pa, L.ptr(saved), L.ptr(c),
               L.ptr(dc), L.ptr(dq), int(accumulate), L.ptr(dqh), ga, L.ptr(ws), ws.numel(),
               L.stream_of(q))
        return (dq, dqh, dc if ctx.has_residual else None, None, None, *grads)


def contextual_gate(q, q_hat, cag, residual=None, dest=None, hand_on: bool = False, _qpass_owned: bool = False):
    """C = CAG(q, q_hat); with `residual`: residual + C (into slot dest[1] of the TokenPair dest[0] when given).  hand_on: also returns q for its other
    consumers (use THAT tensor there: their gradient is then folded into this op's backward).  _qpass_owned: see
    patch_coattn_mcat."""
    out, q_pass = CagFn.apply(q, q_hat, residual, dest, bool(_qpass_owned), cag.fc1[0].weight, cag.fc1[0].bias, cag.fc2[0].weight, cag.fc2[0].bias,
                              cag.fc3[0].weight, cag.fc3[0].bias, cag.G[1].weight, cag.G[1].bias,
                              cag.E[1].weight, cag.E[1].bias, cag.fc_c[0].weight, cag.fc_c[0].bias)
    return (out, q_pass) if hand_on else out


class EncoderFn(torch.autograd.Function):
    """K4: the whole post-norm nn.TransformerEncoder over (n_slides, T, d) tokens; `branches` encoders of identical
    geometry (x stacked branch-major, params branch-major) go through ONE launch sequence."""

    @staticmethod
    def forward(ctx, x, geom, drop_p, *params):
        lib = L.lib()
        branches, n_slides, T, d, ff, heads, layers = geom
        x = x.contiguous()
        y = torch.empty_like(x)
        saved = torch.empty(lib.mpo_encoder_saved_floats(branches * n_slides, T, d, ff, heads, layers), device=x.device,
                            dtype=torch.float32)
        seed, off = _reserve(lib.mpo_encoder_rng_span(branches * n_slides, T, d, ff, layers)) if drop_p > 0 else (0, 0)
        pa = L.ptr_array(params)
        L.call("mpo_encoder_forward", L.ptr(x), branches, n_slides, T, d, ff, heads, layers, pa, float(drop_p), seed, off,
               _epoch(), L.ptr(y), L.ptr(saved), L.stream_of(x))
        ctx.save_for_backward(x, saved, *params)
        ctx.param_refs = params
        ctx.geom, ctx.drop = geom, (float(drop_p), seed, off)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = L.lib()
        x, saved, *params = ctx.saved_tensors
        branches, n_slides, T, d, ff, heads, layers = ctx.geom
        drop_p, seed, off = ctx.drop
        dx = torch.empty_like(x)
        grads = [grad_out(p) for p in ctx.param_refs]
        ws = _workspace(lib.mpo_encoder_workspace_bytes(branches * n_slides, T, d, ff), x.device)
        pa, ga = L.ptr_array(params), L.ptr_array(grads)
        dy = dy.contiguous()
        L.call("mpo_encoder_backward",
            L.ptr(x), branches, n_slides, T, d, ff, heads, layers, pa, drop_p, seed, off, _epoch(), L.ptr(saved), L.ptr(dy),
            L.ptr(dx), ga, L.ptr(ws), ws.numel(), L.stream_of(x))
        return (dx, None, None, *grads)


def _encoder_params(layers):
    params = []
    for ly in layers:
        params += [ly.self_attn.in_proj_weight, ly.self_attn.in_proj_bias, ly.self_attn.out_proj.weight,
                   ly.self_attn.out_proj.bias, ly.linear1.weight, ly.linear1.bias, ly.linear2.weight, ly.linear2.bias,
                   ly.norm1.weight, ly.norm1.bias, ly.norm2.weight, ly.norm2.bias]
    return params


def _encoder_geom(layers):
    l0 = layers[0]
    return (l0.linear1.in_features, l0.linear1.out_features, l0.self_attn.num_heads, len(layers), l0.dropout.p)


def encoder(x, layers, training: bool):
    """x (B, T, d) through a stack of nn.TransformerEncoderLayer parameter holders."""
    return encoder_branches([x], [layers], training)[0]


def encoder_branches(xs, layer_stacks, training: bool):
    """Several encoders of identical geometry (MCAT's path_transformer and omic_transformer) on inputs of identical
    shape (B, T, d), batched into one launch sequence.  Returns one (B, T, d) tensor per branch."""
    if len(xs) == 1:
        return [encoder_stacked(xs[0].unsqueeze(0), layer_stacks, training)[0]]
    if any(x.shape != xs[0].shape for x in xs):
        raise ValueError("branch-batched encoders need identical input shapes")
    return list(encoder_stacked(torch.stack(list(xs)), layer_stacks, training).unbind(0))


def encoder_stacked(x, layer_stacks, training: bool):
    """x (branches, B, T, d) -> (branches, B, T, d): branch i goes through layer_stacks[i]."""
    nb, b, t, d = x.shape
    g0 = _encoder_geom(layer_stacks[0])
    if len(layer_stacks) != nb or any(_encoder_geom(ls) != g0 for ls in layer_stacks) or g0[0] != d:
        raise ValueError("branch-batched encoders need one layer stack per branch, all of identical geometry")
    params = [p for ls in layer_stacks for p in _encoder_params(ls)]
    geom = (nb, b, t, d, g0[1], g0[2], g0[3])
    y = EncoderFn.apply(x.reshape(nb * b * t, d), geom, g0[4] if training else 0.0, *params)
    return y.view(nb, b, t, d)


class BagSelfAttentionFn(torch.autograd.Function):
    """f3: the attention core of nn.MultiheadAttention with query = key = value = the M rows of a bag
    (models/ge_nacagat/ge_nacagat.py:27,49), one C-ABI call each way; no M x M state is kept between them."""

    @staticmethod
    def forward(ctx, qkv, heads: int, drop_p: float, need_map: bool):
        lib = L.lib()
        n_bags, m, d3 = qkv.shape
        d = d3 // 3
        qkv = qkv.contiguous()
        out = torch.empty((n_bags, m, d), device=qkv.device, dtype=torch.float32)
        saved = torch.empty(lib.mpo_bag_self_attention_saved_floats(n_bags, m, d, heads), device=qkv.device, dtype=torch.float32)
        amap = torch.empty((n_bags, m, m), device=qkv.device, dtype=torch.float32) if need_map else None
        seed, off = _reserve(1) if drop_p > 0 else (0, 0)
        L.call("mpo_bag_self_attention_forward", L.ptr(qkv), n_bags, m, d, heads, float(drop_p), seed, off, _epoch(), L.ptr(out),
               L.ptr(saved), L.ptr(amap), L.stream_of(qkv))
        ctx.save_for_backward(qkv, out, saved)
        ctx.geom, ctx.drop = (n_bags, m, d, heads), (float(drop_p), seed, off)
        if amap is not None:
            ctx.mark_non_differentiable(amap)       # the reference returns the map and never differentiates it
        return out, amap

    @staticmethod
    def backward(ctx, d_out, _d_map):
        lib = L.lib()
        qkv, out, saved = ctx.saved_tensors
        n_bags, m, d, heads = ctx.geom
        drop_p, seed, off = ctx.drop
        d_qkv = torch.empty_like(qkv)
        ws = _workspace(lib.mpo_bag_self_attention_workspace_bytes(n_bags, m, d, heads), qkv.device)
        d_out = d_out.contiguous()
        L.call("mpo_bag_self_attention_backward", L.ptr(qkv), L.ptr(out), L.ptr(saved), L.ptr(d_out), n_bags, m, d, heads, drop_p,
               seed, off, _epoch(), L.ptr(d_qkv), L.ptr(ws), ws.numel(), L.stream_of(qkv))
        return d_qkv, None, None, None


def bag_self_attention(x, mha, training: bool, need_weights: bool = True):
    """x (M, d) or (n_bags, M, d) through the parameters of an nn.MultiheadAttention `mha` as self-attention
    (query = key = value = x) -> (output, map averaged over heads | None) like mha(x, x, x).  The in / out projections are
    plain GEMMs over M rows; the attention itself is bag_selfattn.hip."""
    if mha.in_proj_weight is None or mha.bias_k is not None or mha.add_zero_attn:
        raise NotImplementedError("bag self-attention: packed in_proj, no bias_k / zero-attn (the reference's constructor)")
    if need_weights and mha.num_heads != 1:
        raise NotImplementedError("bag self-attention: the M x M map is returned for one head (models/ge_nacagat/ge_nacagat.py:27)")
    xb = x if x.dim() == 3 else x.unsqueeze(0)
    qkv = linear(xb.float(), mha.in_proj_weight, mha.in_proj_bias)          # the many-row fp32 MFMA GEMM (gemm_f32_rows.hip)
    out, amap = BagSelfAttentionFn.apply(qkv, mha.num_heads, mha.dropout if training else 0.0, bool(need_weights))
    out = linear(out, mha.out_proj.weight, mha.out_proj.bias)
    if x.dim() == 2:
        out, amap = out[0], (amap[0] if amap is not None else None)
    return out, amap


class GatedPoolFn(torch.autograd.Function):
    """K5: gated attention-MIL scorer + softmax pooling + rho, one C-ABI call each way."""

    @staticmethod
    def forward(ctx, x, geom, head_p, rho_p, interleave, *params):
        lib = L.lib()
        ctx.set_materialize_grads(False)
        branches, n_slides, Lr, d = geom
        bt = branches * n_slides
        x = x.contiguous()
        scores = torch.empty(bt * Lr, device=x.device, dtype=torch.float32)
        h = torch.empty((n_slides, branches * d) if interleave else (bt, d), device=x.device, dtype=torch.float32)
        saved = torch.empty(lib.mpo_gated_pool_saved_floats(bt, Lr, d), device=x.device, dtype=torch.float32)
        seed, off = _reserve(lib.mpo_gated_pool_rng_span(bt, Lr, d)) if (head_p > 0 or rho_p > 0) else (0, 0)
        pa = L.ptr_array(params)
        L.call("mpo_gated_pool_forward", L.ptr(x), branches, n_slides, Lr, d, pa, float(head_p), float(rho_p), seed, off,
               _epoch(), L.ptr(scores), L.ptr(h), int(interleave), L.ptr(saved), L.stream_of(x))
        ctx.save_for_backward(x, saved, h, *params)
        ctx.param_refs = params
        ctx.geom, ctx.drop, ctx.interleave = geom, (float(head_p), float(rho_p)), bool(interleave)
        return scores, h

    @staticmethod
    def backward(ctx, d_scores, dh):
        lib = L.lib()
        x, saved, h, *params = ctx.saved_tensors
        branches, n_slides, Lr, d = ctx.geom
        head_p, rho_p = ctx.drop
        dx = torch.empty_like(x)
        grads = [grad_out(p) for p in ctx.param_refs]
        if dh is None:
            dh = torch.zeros_like(h)
        ws = _workspace(lib.mpo_gated_pool_workspace_bytes(branches * n_slides, Lr, d), x.device)
        pa, ga = L.ptr_array(params), L.ptr_array(grads)
        dh = dh.contiguous()
        d_sc = d_scores.contiguous() if d_scores is not None else None
        L.call("mpo_gated_pool_backward",
            L.ptr(x), branches, n_slides, Lr, d, pa, head_p, rho_p, L.ptr(saved), L.ptr(h), L.ptr(dh), int(ctx.interleave),
            L.ptr(d_sc), L.ptr(dx), ga, L.ptr(ws), ws.numel(), L.stream_of(x))
        return (dx, None, None, None, None, *grads)


def gated_pool(tokens, head, rho, training: bool):
    """tokens (B, L, d) -> raw scores (B, 1, L), pooled embedding (B, d)   (models/mcat/mcat.py:105-109)."""
    return gated_pool_branches([tokens], [head], [rho], training)[0]


def gated_pool_branches(tokens, heads, rhos, training: bool):
    """Several pooling heads of identical geometry on token sets of identical shape (B, L, d) -- the model's
    path / omic attention heads + rho -- in one launch sequence.  Returns [(scores (B,1,L), h (B,d))] per branch."""
    if len(tokens) == 1:
        sc, h = gated_pool_stacked(tokens[0].unsqueeze(0), heads, rhos, training)
        return [(sc[0], h[0])]
    if any(t.shape != tokens[0].shape for t in tokens):
        raise ValueError("branch-batched pooling needs identical token shapes")
    sc, h = gated_pool_stacked(torch.stack(list(tokens)), heads, rhos, training)
    return list(zip(sc.unbind(0), h.unbind(0)))


def gated_pool_stacked(tokens, heads, rhos, training: bool, interleave: bool = False):
    """tokens (branches, B, L, d) -> raw scores (branches, B, 1, L), pooled embeddings (branches, B, d) -- or, with
    interleave, (B, branches * d): row b = [h_branch0 | h_branch1 | ...], the concatenation ConcatFusion reads."""
    nb, b, l, d = tokens.shape
    params = []
    for head, rho in zip(heads, rhos):
        if head.attention_c.weight.shape[0] != 1 or head.attention_a[0].weight.shape != (d, d):
            raise NotImplementedError("gated pooling kernel: n_classes=1 and hidden_dim == input_dim only")
        params += [head.attention_a[0].weight, head.attention_a[0].bias, head.attention_b[0].weight, head.attention_b[0].bias,
                   head.attention_c.weight, head.attention_c.bias, rho[0].weight, rho[0].bias]
    if len(heads) != nb or len(rhos) != nb or len({(h.drop_p, r[2].p) for h, r in zip(heads, rhos)}) != 1:
        raise ValueError("branch-batched pooling needs one head + rho per branch with identical dropout rates")
    scores, h = GatedPoolFn.apply(tokens.reshape(nb * b * l, d), (nb, b, l, d), heads[0].drop_p if training else 0.0,
                                  rhos[0][2].p if training else 0.0, bool(interleave), *params)
    return scores.view(nb, b, 1, l), (h if interleave else h.view(nb, b, d))


class OmicSnnFn(torch.autograd.Function):
    """self.G: all omic SNNs of a window in grouped launches (models/mcat/mcat.py:32-45,90-92)."""

    @staticmethod
    def forward(ctx, drop_p, n_groups, tokens, *args):
        lib = L.lib()
        xs, params = [a.contiguous() for a in args[:n_groups]], args[n_groups:]
        n_slides, d = xs[0].shape[0], params[0].shape[0]
        dev = xs[0].device
        widths = (ctypes.c_int * n_groups)(*[int(x.shape[1]) for x in xs])
        g_bag = tokens.slot(1, (n_slides, n_groups, d)) if tokens is not None else \
            torch.empty(n_slides, n_groups, d, device=dev, dtype=torch.float32)
        saved = torch.empty(lib.mpo_omic_snn_saved_floats(n_slides, n_groups, d), device=dev, dtype=torch.float32)
        seed, off = _reserve(lib.mpo_omic_snn_rng_span(n_slides, n_groups, d)) if drop_p > 0 else (0, 0)
        xa, pa = L.ptr_array(xs), L.ptr_array(params)
        L.call("mpo_omic_snn_forward", xa, widths, n_groups, n_slides, d, pa, float(drop_p), seed, off, _epoch(),
               L.ptr(g_bag), L.ptr(saved), L.stream_of(g_bag))
        ctx.save_for_backward(g_bag, saved, *xs, *params)
        ctx.param_refs, ctx.n_groups, ctx.drop = params, n_groups, (float(drop_p), seed, off)
        return g_bag

    @staticmethod
    def backward(ctx, d_g):
        lib = L.lib()
        g_bag, saved, *rest = ctx.saved_tensors
        n = ctx.n_groups
        xs, params = rest[:n], rest[n:]
        n_slides, d = xs[0].shape[0], params[0].shape[0]
        drop_p, seed, off = ctx.drop
        widths = (ctypes.c_int * n)(*[int(x.shape[1]) for x in xs])
        grads = [grad_out(p) for p in ctx.param_refs]
        ws = _workspace(lib.mpo_omic_snn_workspace_bytes(n_slides, n, d), g_bag.device)
        xa, pa, ga = L.ptr_array(xs), L.ptr_array(params), L.ptr_array(grads)
        L.call("mpo_omic_snn_backward", xa, widths, n, n_slides, d, pa, drop_p, seed, off, _epoch(), L.ptr(g_bag),
               L.ptr(saved), L.ptr(d_g.contiguous()), ga, L.ptr(ws), ws.numel(),
               L.stream_of(g_bag))
        return (None, None, None, *([None] * n), *grads)


def omic_snn(omics, g_modules, training: bool, tokens: "TokenPair | None" = None):
    """omics: per group (B, d_i) -> G_bag (B, N, d).  g_modules: the nn.ModuleList self.G (parameter holders).
    tokens: G_bag is produced into tokens.slot(1)."""
    params = []
    for g in g_modules:
        params += [g[0][0].weight, g[0][0].bias, g[1][0].weight, g[1][0].bias]
    p = g_modules[0][0][2].p if training else 0.0
    return OmicSnnFn.apply(p, len(omics), tokens, *[o.float() for o in omics], *params)


class MapBlockNormFn(torch.autograd.Function):
    """Frobenius norm of every slide's (n_q, M_b) block of a ragged attention map -> (n_slides,)."""

    @staticmethod
    def forward(ctx, flat_map, batch: BagBatch, n_q: int):
        flat_map = flat_map.contiguous()
        sq = torch.empty(batch.n_slides * n_q, device=flat_map.device, dtype=torch.float32)
        L.call("mpo_map_block_dot", L.ptr(flat_map), L.ptr(flat_map), L.ptr(batch.cu), batch.n_slides, n_q, L.ptr(sq),
               L.stream_of(flat_map))
        norm = sq.view(batch.n_slides, n_q).sum(1).sqrt()
        ctx.save_for_backward(flat_map, norm)
        ctx.batch, ctx.n_q = batch, n_q
        return norm

    @staticmethod
    def backward(ctx, d_norm):
        flat_map, norm = ctx.saved_tensors
        scale = (d_norm / norm.clamp_min(1e-30)).contiguous()
        d_map = torch.empty_like(flat_map)
        L.call("mpo_map_block_scale", L.ptr(flat_map), L.ptr(scale), L.ptr(ctx.batch.cu), ctx.batch.n_slides, ctx.n_q,
               L.ptr(d_map), L.stream_of(flat_map))
        return d_map, None, None


def map_block_norm(maps) -> torch.Tensor:
    """maps: the RaggedMaps a window forward returns -> per-slide ||A_b||_2, differentiable into the flat map."""
    return MapBlockNormFn.apply(maps.flat, maps.batch, maps.n_q)


def map_block_stats(maps) -> torch.Tensor:
    """maps: the RaggedMaps a window forward returns -> (n_slides, 3) fp32 [min, max, mean] of every slide's (n_q, M_b) block
    (what the reference's test() prints of attention_scores['coattn'], models/nacagat/main.py:169-194): two launches for
    the whole window, sums carried in fp64 in a fixed order (csrc/map_stats.hip) -- deterministic, no host sync.  Not
    differentiable."""
    flat, batch, n_q = maps.flat.detach(), maps.batch, int(maps.n_q)
    if not flat.is_cuda or flat.dtype != torch.float32:
        raise ValueError(f"map_block_stats: an fp32 map on the GPU (got {flat.dtype} on {flat.device})")
    flat = flat.contiguous()
    if flat.numel() != n_q * batch.total_rows:
        raise ValueError(f"map_block_stats: {flat.numel()} map values for {n_q} queries x {batch.total_rows} rows")
    out = torch.empty(batch.n_slides, 3, dtype=torch.float32, device=flat.device)
    ws = _workspace(L.lib().mpo_map_block_stats_workspace_bytes(batch.n_slides, n_q, batch.max_rows), flat.device)
    L.call("mpo_map_block_stats", L.ptr(flat), L.ptr(batch.cu), batch.n_slides, n_q, batch.max_rows, L.ptr(out), L.ptr(ws),
           ws.numel(), L.stream_of(flat))
    return out


def concordance_index(censorship, time, risk):
    """Harrell's C on the device (csrc/concordance.hip; harness.concordance_index_device is the checked front): censorship,
    risk fp32 (n,), time fp64 (n,), contiguous on one GPU -> (c_index (1,) fp64, counts (3,) int64 = concordant, tied,
    comparable).  Two launches, no host sync."""
    n = int(risk.numel())
    c_index = torch.empty(1, dtype=torch.float64, device=risk.device)
    counts = torch.empty(3, dtype=torch.int64, device=risk.device)
    ws = _workspace(L.lib().mpo_concordance_workspace_bytes(n), risk.device)
    L.call("mpo_concordance_index", L.ptr(time), L.ptr(censorship), L.ptr(risk), n, L.ptr(counts), L.ptr(c_index), L.ptr(ws),
           ws.numel(), L.stream_of(risk))
    return c_index, counts


def class_metrics(y, label, loss=None, want_pred: bool = True):
    """Classification metrics on the device (csrc/class_metrics.hip; harness.classification_metrics_device is the checked
    front): y fp32 (n, C), label int64 (n,), loss fp32 (n,) or None, contiguous on one GPU -> (pred (n,) int64 or None,
    confusion (C, C) int64, counts (4,) int64 = valid, correct, invalid labels, rows with a NaN, summary (3,) fp64 =
    accuracy, balanced accuracy, mean loss).  Two launches, no host sync."""
    n, c = int(y.shape[0]), int(y.shape[1])
    dev = y.device
    pred = torch.empty(n, dtype=torch.int64, device=dev) if want_pred else None
    confusion = torch.empty(c, c, dtype=torch.int64, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    summary = torch.empty(3, dtype=torch.float64, device=dev)
    ws = _workspace(L.lib().mpo_class_metrics_workspace_bytes(n, c), dev)
    L.call("mpo_class_metrics", L.ptr(y), L.ptr(label), L.ptr(loss), n, c, L.ptr(pred), L.ptr(confusion), L.ptr(counts),
           L.ptr(summary), L.ptr(ws), ws.numel(), L.stream_of(y))
    return pred, confusion, counts, summary


class SurvivalHeadFn(torch.autograd.Function):
    """logits (B, C) -> hazards, survs, Y (models/mcat/mcat.py:130-138) on the HIP head kernels."""

    @staticmethod
    def forward(ctx, logits):
        ctx.set_materialize_grads(False)
        logits = logits.contiguous()
        b, c = logits.shape
        hz, sv, y = (torch.empty_like(logits) for _ in range(3))
        L.call("mpo_survival_head_forward", L.ptr(logits), b, c, L.ptr(hz), L.ptr(sv), L.ptr(y), L.stream_of(logits))
        ctx.save_for_backward(hz, sv, y)
        return hz, sv, y

    @staticmethod
    def backward(ctx, dhz, dsv, dy):
        hz, sv, y = ctx.saved_tensors
        b, c = hz.shape
        dhz, dsv, dy = (t.contiguous() if t is not None else None for t in (dhz, dsv, dy))
        dl = torch.empty_like(hz)
        L.call("mpo_survival_head_backward", L.ptr(hz), L.ptr(sv), L.ptr(y), L.ptr(dhz), L.ptr(dsv), L.ptr(dy), b, c,
               L.ptr(dl), L.stream_of(hz))
        return dl


def survival_head(logits):
    return SurvivalHeadFn.apply(logits)


class CesLossFn(torch.autograd.Function):
    """'ces' loss (models/loss.py:5-28) for a whole window in one launch each way: per-slide losses + risks.
    The torch formulation costs ~60 tiny launches per window (cat/gather/clamp/log and their backward)."""

    @staticmethod
    def forward(ctx, hazards, survs, label, censorship, alpha, eps):
        ctx.set_materialize_grads(False)        # an unused output must not cost a zero-fill launch in backward
        hazards, survs = hazards.contiguous(), survs.contiguous()
        label = label.view(-1).to(torch.int64).contiguous()
        censorship = censorship.view(-1).to(torch.float32).contiguous()
        b, c = hazards.shape
        loss = torch.empty(b, device=hazards.device, dtype=torch.float32)
        risk = torch.empty(b, device=hazards.device, dtype=torch.float32)
        L.call("mpo_ces_loss_forward", L.ptr(hazards), L.ptr(survs), L.ptr(label), L.ptr(censorship), b, c, float(alpha),
               float(eps), L.ptr(loss), L.ptr(risk), L.stream_of(hazards))
        ctx.save_for_backward(hazards, survs, label, censorship)
        ctx.cfg = (float(alpha), float(eps))
        ctx.mark_non_differentiable(risk)
        return loss, risk

    @staticmethod
    def backward(ctx, d_loss, _d_risk):
        if d_loss is None:
            return None, None, None, None, None, None
        hazards, survs, label, censorship = ctx.saved_tensors
        alpha, eps = ctx.cfg
        b, c = hazards.shape
        # loss.sum().backward() hands an expanded (stride-0) gradient: pass its one element, no materialisation
        scalar = d_loss.stride(0) == 0 and b > 1
        d_loss = d_loss.as_strided((1,), (1,)) if scalar else d_loss.contiguous()
        d_hz, d_sv = torch.empty_like(hazards), torch.empty_like(survs)
        L.call("mpo_ces_loss_backward", L.ptr(hazards), L.ptr(survs), L.ptr(label), L.ptr(censorship), b, c, alpha, eps,
               L.ptr(d_loss), int(scalar), L.ptr(d_hz), L.ptr(d_sv), L.stream_of(hazards))
        return d_hz, d_sv, None, None, None, None


def ces_loss(hazards, survs, label, censorship, alpha: float = 0.75, eps: float = 1e-7):
    """-> (per-slide 'ces' loss (B,), risk (B,)); reduce with .sum()/.mean() as the caller needs."""
    return CesLossFn.apply(hazards, survs, label, censorship, alpha, eps)


class SctLossFn(torch.autograd.Function):
    """'sct' loss (models/loss.py:62-85) on Y = softmax(logits) for a whole window, one launch each way: per-slide losses.
    The gradient goes to Y only; the survival head's backward carries it through the softmax."""

    @staticmethod
    def forward(ctx, y, label, censorship, eps):
        ctx.set_materialize_grads(False)
        y = y.contiguous()
        label = label.view(-1).to(torch.int64).contiguous()
        censorship = censorship.view(-1).to(torch.float32).contiguous()
        b, c = y.shape
        loss = torch.empty(b, device=y.device, dtype=torch.float32)
        L.call("mpo_sct_loss_forward", L.ptr(y), L.ptr(label), L.ptr(censorship), b, c, float(eps), L.ptr(loss),
               L.stream_of(y))
        ctx.save_for_backward(y, label, censorship)
        ctx.eps = float(eps)
        return loss

    @staticmethod
    def backward(ctx, d_loss):
        if d_loss is None:
            return None, None, None, None
        y, label, censorship = ctx.saved_tensors
        b, c = y.shape
        scalar = d_loss.stride(0) == 0 and b > 1          # loss.sum().backward(): one broadcast value
        d_loss = d_loss.as_strided((1,), (1,)) if scalar else d_loss.contiguous()
        d_y = torch.empty_like(y)
        L.call("mpo_sct_loss_backward", L.ptr(y), L.ptr(label), L.ptr(censorship), b, c, ctx.eps, L.ptr(d_loss), int(scalar),
               L.ptr(d_y), L.stream_of(y))
        return d_y, None, None, None


def sct_loss(y, label, censorship, eps: float = 1e-7):
    """-> per-slide 'sct' loss (B,) of Y (B, C) (no risk: that needs survs, risk = -survs.sum(1))."""
    return SctLossFn.apply(y, label, censorship, eps)


def flat_abs_sum(x) -> torch.Tensor:
    """sum |x| over a contiguous fp32 tensor as a device scalar (1,): the L1 penalty's value (models/utils.py:33-40).
    Deterministic (two launches, fixed partial sums, no atomics); no host sync."""
    lib = L.lib()
    if x.dtype != torch.float32:
        raise ValueError("flat_abs_sum: fp32 tensors only")
    x = x.detach().contiguous().view(-1)
    out = torch.empty(1, device=x.device, dtype=torch.float32)
    ws = _workspace(lib.mpo_abs_sum_flat_workspace_bytes(x.numel()), x.device)
    L.call("mpo_abs_sum_flat", L.ptr(x), x.numel(), L.ptr(out), L.ptr(ws), ws.numel(), L.stream_of(x))
    return out


def optim_step_flat(algorithm: str, params, grads, state1, state2, lr: float, lr_dev=None, beta1: float = 0.9,
                    beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0, l1: float = 0.0, step: int = 1,
                    step_dev=None):
    """One mpo_optim_step_flat over flat fp32 buffers (include/mpo_hip.h): 'adam' | 'adamax' | 'adadelta' (rho = beta1) |
    'sgd' (state1 = state2 = None).  lr_dev (fp32 (1,)) / step_dev (int32 (1,)) override lr / step on the device."""
    if algorithm not in L.OPTIM:
        raise ValueError(f"unknown flat optimiser '{algorithm}' ({' | '.join(L.OPTIM)})")
    L.call("mpo_optim_step_flat", L.OPTIM[algorithm], L.ptr(params), L.ptr(grads), L.ptr(state1), L.ptr(state2),
           params.numel(), float(lr), L.ptr(lr_dev), float(beta1), float(beta2), float(eps),
           float(weight_decay), float(l1), int(step), L.ptr(step_dev), L.stream_of(params))


def grad_norm_flat(grads, ctl, params=None, l1: float = 0.0, max_norm: "float | None" = None, skip_nonfinite: bool = False,
                   step_dev=None):
    """One mpo_grad_norm_flat (include/mpo_grad_guard.h): measures g' = grads + l1 sign(params) into the 16-byte control block
    `ctl` (4 x 32 bits on the device: norm, coef, nonfinite, skipped).  max_norm None / 0: no clipping (coef 1).
    skip_nonfinite with a non-finite g': ctl's skipped count goes up and step_dev (int32 (1,)), if given, down by one.
    Deterministic (two launches, fixed partial sums, no atomics); no host sync."""
    lib = L.lib()
    if grads.dtype != torch.float32 or ctl.numel() * ctl.element_size() != 16:
        raise ValueError("grad_norm_flat: fp32 gradients and a 16-byte control block")
    ws = _workspace(lib.mpo_grad_norm_flat_workspace_bytes(grads.numel()), grads.device)
    L.call("mpo_grad_norm_flat", L.ptr(grads), L.ptr(params) if l1 else None, grads.numel(), float(l1), float(max_norm or 0.0),
           int(bool(skip_nonfinite)), L.ptr(step_dev), L.ptr(ctl), L.ptr(ws), ws.numel(), L.stream_of(grads))


def optim_step_flat_guarded(algorithm: str, params, grads, state1, state2, ctl, lr: float, lr_dev=None, beta1: float = 0.9,
                            beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0, l1: float = 0.0,
                            step: int = 1, step_dev=None, skip_nonfinite: bool = False):
    """One mpo_optim_step_flat_guarded (include/mpo_grad_guard.h): optim_step_flat on the clipped gradient
    ctl.coef * (grads + l1 sign(params)) + weight_decay * params; with skip_nonfinite and ctl.nonfinite set it writes
    nothing.  `ctl`: what grad_norm_flat wrote for the same grads, params and l1."""
    if algorithm not in L.OPTIM:
        raise ValueError(f"unknown flat optimiser '{algorithm}' ({' | '.join(L.OPTIM)})")
    L.call("mpo_optim_step_flat_guarded", L.OPTIM[algorithm], L.ptr(params), L.ptr(grads), L.ptr(state1), L.ptr(state2),
           params.numel(), float(lr), L.ptr(lr_dev), float(beta1), float(beta2), float(eps), float(weight_decay), float(l1),
           int(step), L.ptr(step_dev), L.ptr(ctl), int(bool(skip_nonfinite)), L.stream_of(params))


# ------------------------------------------------------------------------------------ fusion + classifier + survival head
# The three fusions (K6 concat, gated-concat, bilinear) share one head protocol -- four C entries mpo_<name>_{forward, backward,
# loss_forward, loss_backward}, csrc/tail_api.hip -- and one Python body for it: HeadFn / HeadLossFn over a _Head description.
FUSED_LOSSES = ("ces", "sct")


def _head_rows(h, interleaved: bool):
    """h: the pooled rows of the two branches as the pooling launch wrote them, (B, 2 d) rows [h_path | h_omic] when
    `interleaved`, else (2, B, d) -> (h_omic's offset in elements, row stride, B, d).  No copy either way: a tensor of
    another shape or a strided one is refused."""
    if not h.is_contiguous():
        raise ValueError("fusion head: h must be contiguous (the entries read it in place)")
    if interleaved and h.dim() == 2 and h.shape[1] % 2 == 0:
        b, d = h.shape[0], h.shape[1] // 2
        return d, 2 * d, b, d
    if not interleaved and h.dim() == 3 and h.shape[0] == 2:
        b, d = h.shape[1], h.shape[2]
        return b * d, d, b, d
    raise ValueError(f"fusion head: h {tuple(h.shape)} is not {'(B, 2 d)' if interleaved else '(2, B, d)'}")


# geometry(h, interleaved, params) -> (h as the entries read it, h_omic's offset in elements | None for one pointer,
#                                      the entries' geometry arguments, the size queries' (n_slides first, n_classes last))
def _concat_geometry(hcat, interleaved, params):
    b, din = hcat.shape
    hidden, dout, c = params[0].shape[0], params[2].shape[0], params[4].shape[0]
    return hcat.contiguous(), None, (b, din, hidden, dout, c), (b, hidden, dout, c)


def _gated_concat_geometry(h, interleaved, params):
    omic, ld, b, d = _head_rows(h, interleaved)
    c = params[8].shape[0]
    return h, omic, (ld, b, d, c), (b, d, c)


def _bilinear_geometry(h, interleaved, params):
    omic, ld, b, d = _head_rows(h, interleaved)
    c = params[16].shape[0]
    return h, omic, (ld, b, d, params[4].shape[0], params[12].shape[0], c), (b, d, c)       # (.., hidden, mm_hidden, ..)


def _concat_params(fusion_layer, classifier):
    seq = fusion_layer.fusion_layer
    return seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias, classifier.weight, classifier.bias


def _gated_concat_params(fusion_layer, classifier):
    gates = fusion_layer.gates
    return (gates[0][0].weight, gates[0][0].bias, gates[1][0].weight, gates[1][0].bias, *_concat_params(fusion_layer, classifier))


def _bilinear_params(fusion_layer, classifier):
    f = fusion_layer
    if not (f.use_bilinear and f.use_gates and f.use_skip_connection):
        raise NotImplementedError("bilinear_head: built for BilinearFusion with gates, bilinear products and the skip connection on")
    out = []
    for h, z, o in ((f.linear_h1, f.linear_z1, f.linear_o1), (f.linear_h2, f.linear_z2, f.linear_o2)):
        out += [h[0].weight, h[0].bias, z.weight, z.bias, o[0].weight, o[0].bias]
    return (*out, f.fc1[0].weight, f.fc1[0].bias, f.fc2[0].weight, f.fc2[0].bias, classifier.weight, classifier.bias)


def _bilinear_drop_p(fusion_layer, training: bool) -> float:
    f = fusion_layer
    ps = {f.linear_o1[2].p, f.linear_o2[2].p, f.post_fusion_dropout.p, f.fc1[2].p, f.fc2[2].p}
    if len(ps) != 1:
        raise NotImplementedError("bilinear_head: one dropout rate for the layer's five sites")
    return float(ps.pop()) if training else 0.0


@dataclass(frozen=True)
class _Head:
    """What one fusion's head has of its own."""
    name: str                   # mpo_<name>_* are its entries and size queries, <name>_loss names it in messages
    loss_fn: str                # the public training-step function (named when it refuses a loss)
    geometry: object            # see _concat_geometry
    params: object              # (fusion_layer, classifier) -> the parameter tensors in the entries' order
    drop_p: object = None       # (fusion_layer, training) -> the rate of the head's dropout sites; None: it has none, and its
    #                             entries no (drop_p, seed, offset, rng_epoch); mpo_<name>_rng_span is their counter span
    stat: Optional[str] = None  # the `stats` counter every forward bumps
    entry_per_loss: bool = False  # K6: mpo_fusion_head_loss_forward (alpha, eps) | _sct_loss_forward (eps), no loss_kind


_CONCAT = _Head("fusion_head", "fusion_head_loss_cat", _concat_geometry, _concat_params, entry_per_loss=True)
_GATED_CONCAT = _Head("gated_concat_head", "gated_concat_head_loss", _gated_concat_geometry, _gated_concat_params,
                      stat="gated_concat_head")
_BILINEAR = _Head("bilinear_head", "bilinear_head_loss", _bilinear_geometry, _bilinear_params, _bilinear_drop_p, "bilinear_head")


def _row_ptrs(t, omic):
    return (L.ptr(t),) if omic is None else (L.ptr(t), L.ptr(t) + 4 * omic)


def _head_begin(ctx, spec, h, interleaved, drop_p, params, slide_weight=None):
    """What the forwards of the two forms share (slide_weight: the training-step form): geometry, the counters of the dropout
    sites (reserved only when drop_p > 0, once), outputs and `saved` -> (h as the entries read it, hazards, survs, Y, saved)."""
    lib = L.lib()
    ctx.set_materialize_grads(False)
    h, omic, geom, sizes = spec.geometry(h, interleaved, params)
    b, c = sizes[0], sizes[-1]
    if slide_weight is not None and (slide_weight.shape != (b,) or slide_weight.dtype != torch.float32
                                     or not slide_weight.is_contiguous()):
        raise ValueError(f"{spec.name}_loss: slide_weight must be a contiguous fp32 tensor of one value per slide")
    rng = ()
    if spec.drop_p is not None:
        rng = (float(drop_p), *(_reserve(getattr(lib, f"mpo_{spec.name}_rng_span")(*sizes[:2])) if drop_p > 0 else (0, 0)))
    hz = torch.empty(b, c, device=h.device, dtype=torch.float32)
    sv, y = torch.empty_like(hz), torch.empty_like(hz)
    query = getattr(lib, f"mpo_{spec.name}_{'loss_' if slide_weight is not None else ''}saved_floats")
    saved = torch.empty(query(*sizes), device=h.device, dtype=torch.float32)
    ctx.head = (spec, omic, geom, sizes, rng)
    return h, hz, sv, y, saved


def _head_lead(ctx, h, params):
    """The arguments every entry starts with: row pointer(s), geometry, parameters (, dropout streams: the epoch as of now)."""
    _, omic, geom, _, rng = ctx.head
    return (*_row_ptrs(h, omic), *geom, L.ptr_array(params), *rng, *((_epoch(),) if rng else ()))


def _head_end(ctx, spec, params, *tensors):
    if spec.stat:
        stats[spec.stat] += 1
    ctx.save_for_backward(*tensors, *params)
    ctx.param_refs = params


def _head_grads(ctx, h):
    """-> (d_h, parameter gradients, the arguments every backward entry ends with)."""
    spec, omic, _, sizes, _ = ctx.head
    d_h = torch.empty_like(h)
    grads = [grad_out(p) for p in ctx.param_refs]
    ws = _workspace(getattr(L.lib(), f"mpo_{spec.name}_workspace_bytes")(*sizes), h.device)
    return d_h, grads, (*_row_ptrs(d_h, omic), L.ptr_array(grads), L.ptr(ws), ws.numel(), L.stream_of(h))


class HeadFn(torch.autograd.Function):
    """Fusion layer + classifier + survival head, one C-ABI call each way (mpo_<name>_forward / _backward).  Training-mode masks
    (bilinear) are a function of (seed, offset + epoch * 2^40): the backward regenerates them, nothing is stored."""

    @staticmethod
    def forward(ctx, h, spec, interleaved, drop_p, *params):
        h, hz, sv, y, saved = _head_begin(ctx, spec, h, interleaved, drop_p, params)
        L.call(f"mpo_{spec.name}_forward", *_head_lead(ctx, h, params), L.ptr(hz), L.ptr(sv), L.ptr(y), L.ptr(saved),
               L.stream_of(h))
        _head_end(ctx, spec, params, h, saved, hz, sv, y)
        return hz, sv, y

    @staticmethod
    def backward(ctx, dhz, dsv, dy):
        h, saved, hz, sv, y, *params = ctx.saved_tensors
        d_h, grads, tail = _head_grads(ctx, h)
        dhz, dsv, dy = (t.contiguous() if t is not None else None for t in (dhz, dsv, dy))
        L.call(f"mpo_{ctx.head[0].name}_backward", *_head_lead(ctx, h, params), L.ptr(saved), L.ptr(hz), L.ptr(sv), L.ptr(y),
               L.ptr(dhz), L.ptr(dsv), L.ptr(dy), *tail)
        return (d_h, None, None, None, *grads)


class HeadLossFn(torch.autograd.Function):
    """HeadFn for a training step: the fusion's launches, then head, `ces` / `sct` loss and the backward of both in ONE launch.
    The gradient the caller sends into the per-slide loss must be known up front: `slide_weight` (B device floats;
    1 / grad_acc_step in the reference's loop, models/mcat/main.py:69-70) -- backward() refuses any other gradient tensor.
    Returns (loss (B,), risk (B,), hazards, survs, Y); only `loss` carries gradient."""

    @staticmethod
    def forward(ctx, h, spec, interleaved, drop_p, label, censorship, slide_weight, alpha, eps, kind, *params):
        h, hz, sv, y, saved = _head_begin(ctx, spec, h, interleaved, drop_p, params, slide_weight)
        label = label.view(-1).to(torch.int64).contiguous()
        censorship = censorship.view(-1).to(torch.float32).contiguous()
        loss = torch.empty(hz.shape[0], device=h.device, dtype=torch.float32)
        risk = torch.empty_like(loss)
        entry, which = f"mpo_{spec.name}_loss_forward", (float(alpha), float(eps), FUSED_LOSSES.index(kind))
        if spec.entry_per_loss:
            entry, which = (entry, which[:2]) if kind == "ces" else (f"mpo_{spec.name}_sct_loss_forward", which[1:2])
        L.call(entry, *_head_lead(ctx, h, params), L.ptr(label), L.ptr(censorship), L.ptr(slide_weight), *which, L.ptr(hz),
               L.ptr(sv), L.ptr(y), L.ptr(loss), L.ptr(risk), L.ptr(saved), L.stream_of(h))
        stats["head_loss_" + kind] += 1
        _head_end(ctx, spec, params, h, saved, slide_weight)
        ctx.mark_non_differentiable(risk, hz, sv, y)
        return loss, risk, hz, sv, y

    @staticmethod
    def backward(ctx, d_loss, *_unused):
        h, saved, slide_weight, *params = ctx.saved_tensors
        if d_loss is None:
            return (None,) * (10 + len(params))
        name = ctx.head[0].name
        if d_loss.data_ptr() != slide_weight.data_ptr() or d_loss.shape != slide_weight.shape:
            raise RuntimeError(f"{name}_loss: backward() must be driven with the slide_weight tensor given to forward "
                               "(the loss gradient is folded into the forward launch)")
        d_h, grads, tail = _head_grads(ctx, h)
        L.call(f"mpo_{name}_loss_backward", *_head_lead(ctx, h, params), L.ptr(saved), *tail)
        return (d_h, *(None,) * 9, *grads)


def _head(spec, h, fusion_layer, classifier, training=False, targets=None, alpha=0.75, eps=1e-7, loss="ces", interleaved=True):
    if targets is not None and loss not in FUSED_LOSSES:
        raise ValueError(f"{spec.loss_fn}: loss '{loss}' has no fused head launch ({' | '.join(FUSED_LOSSES)})")
    drop_p = spec.drop_p(fusion_layer, training) if spec.drop_p else 0.0
    params = spec.params(fusion_layer, classifier)
    if targets is None:
        return HeadFn.apply(h, spec, bool(interleaved), drop_p, *params)
    return HeadLossFn.apply(h, spec, bool(interleaved), drop_p, *targets, alpha, eps, loss, *params)


def head(h, fusion_layer, classifier, training: bool = False, targets=None, alpha: float = 0.75, eps: float = 1e-7,
         loss: str = "ces", interleaved: bool = True):
    """The head of `fusion_layer` (a fusion.ConcatFusion, GatedConcatFusion or BilinearFusion) on the pooled rows h, (B, 2 d) =
    [h_path | h_omic] (`interleaved`) or (2, B, d) (the two-pointer fusions, which read h in place; concat takes a contiguous
    hcat) -> hazards, survs, Y (B, C).  training: the layer's dropout sites draw their masks (bilinear).
    targets = (label, censorship, slide_weight): the training-step form -> (per-slide loss, risk, hazards, survs, Y); drive
    backward with `slide_weight` itself.  loss: 'ces' (models/loss.py:5-28, weight `alpha`) or 'sct' (models/loss.py:62-85 on Y;
    `alpha` unused)."""
    from . import fusion
    for cls, spec in ((fusion.ConcatFusion, _CONCAT), (fusion.GatedConcatFusion, _GATED_CONCAT), (fusion.BilinearFusion, _BILINEAR)):
        if isinstance(fusion_layer, cls):
            return _head(spec, h, fusion_layer, classifier, training, targets, alpha, eps, loss, interleaved)
    raise NotImplementedError(f"ops.head: no head for a fusion layer of type {type(fusion_layer).__name__}")


def fusion_head(h_path, h_omic, fusion_layer, classifier):
    """(B,d),(B,d) -> hazards, survs, Y (B, C)   (models/fusion.py:17-19 + models/mcat/mcat.py:126-138)."""
    return _head(_CONCAT, torch.cat([h_path, h_omic], dim=-1), fusion_layer, classifier)


def fusion_head_cat(hcat, fusion_layer, classifier):
    """hcat (B, 2d) = [h_path | h_omic] already concatenated."""
    return _head(_CONCAT, hcat, fusion_layer, classifier)


def fusion_head_loss_cat(hcat, fusion_layer, classifier, label, censorship, slide_weight, alpha: float = 0.75, eps: float = 1e-7,
                         loss: str = "ces"):
    """Training-step K6: -> (per-slide loss, risk, hazards, survs, Y); drive backward with `slide_weight` itself.
    loss: 'ces' (models/loss.py:5-28, weight `alpha`) or 'sct' (models/loss.py:62-85 on Y; `alpha` unused)."""
    return _head(_CONCAT, hcat, fusion_layer, classifier, False, (label, censorship, slide_weight), alpha, eps, loss)


def gated_concat_head(h, fusion_layer, classifier, interleaved: bool = True):
    """h (B, 2 d) = [h_path | h_omic] (`interleaved`) or (2, B, d) -> hazards, survs, Y (B, C)   (models/fusion.py:22-41 +
    models/mcat/mcat.py:126-138); fusion_layer: a fusion.GatedConcatFusion."""
    return _head(_GATED_CONCAT, h, fusion_layer, classifier, interleaved=interleaved)


def gated_concat_head_loss(h, fusion_layer, classifier, label, censorship, slide_weight, alpha: float = 0.75, eps: float = 1e-7,
                           loss: str = "ces", interleaved: bool = True):
    """Training-step form of gated_concat_head: -> (per-slide loss, risk, hazards, survs, Y); drive backward with
    `slide_weight` itself.  loss: 'ces' (weight `alpha`) or 'sct' (`alpha` unused), as fusion_head_loss_cat."""
    return _head(_GATED_CONCAT, h, fusion_layer, classifier, False, (label, censorship, slide_weight), alpha, eps, loss, interleaved)


def bilinear_head(h, fusion_layer, classifier, training: bool, interleaved: bool = True):
    """h (B, 2 d) = [h_path | h_omic] (`interleaved`) or (2, B, d) -> hazards, survs, Y (B, C)   (models/fusion.py:44-113 +
    models/mcat/mcat.py:126-138); fusion_layer: a fusion.BilinearFusion as the models build it."""
    return _head(_BILINEAR, h, fusion_layer, classifier, training, interleaved=interleaved)


def bilinear_head_loss(h, fusion_layer, classifier, label, censorship, slide_weight, training: bool, alpha: float = 0.75,
                       eps: float = 1e-7, loss: str = "ces", interleaved: bool = True):
    """Training-step form of bilinear_head: -> (per-slide loss, risk, hazards, survs, Y); drive backward with `slide_weight`
    itself.  loss: 'ces' (weight `alpha`) or 'sct' (`alpha` unused), as fusion_head_loss_cat."""
    return _head(_BILINEAR, h, fusion_layer, classifier, training, (label, censorship, slide_weight), alpha, eps, loss, interleaved)


class GeHeadLossFn(torch.autograd.Function):
    """Training-step head of the gene-expression model: classifier + softmax (models/ge_nacagat/ge_nacagat.py:63-67) and the
    reference's `ce` loss on the already soft-maxed Y (models/ge_nacagat/main.py:33), one launch each way
    (mpo_ge_head_loss_*).  Returns (loss (B,), Y (B, C)); only `loss` carries gradient.  Drive it as
    loss.backward(slide_weight) with one weight per bag (1 / grad_acc_step in the reference's loop, main.py:51)."""

    @staticmethod
    def forward(ctx, h, label, weight, bias):
        ctx.set_materialize_grads(False)
        h = h.contiguous()
        b, d = h.shape
        c = weight.shape[0]
        label = label.view(-1).to(torch.int64).contiguous()
        if label.numel() != b:
            raise ValueError(f"ge_head_loss: {label.numel()} labels for {b} bags")
        y = torch.empty(b, c, device=h.device, dtype=torch.float32)
        loss = torch.empty(b, device=h.device, dtype=torch.float32)
        L.call("mpo_ge_head_loss_forward", L.ptr(h), b, d, c, L.ptr_array((weight, bias)), L.ptr(label), L.ptr(y), L.ptr(loss),
               L.stream_of(h))
        stats["head_loss_ce"] += 1
        ctx.save_for_backward(h, label, weight, bias)
        ctx.param_refs = (weight, bias)
        ctx.mark_non_differentiable(y)
        return loss, y

    @staticmethod
    def backward(ctx, d_loss, _d_y):
        h, label, weight, bias = ctx.saved_tensors
        if d_loss is None:
            return None, None, None, None
        b, d = h.shape
        d_loss = d_loss.to(torch.float32).contiguous()          # (loss.sum().backward() hands a stride-0 expansion)
        d_h = torch.empty_like(h)
        grads = [grad_out(p) for p in ctx.param_refs]
        L.call("mpo_ge_head_loss_backward", L.ptr(h), b, d, weight.shape[0], L.ptr_array((weight, bias)), L.ptr(label),
               L.ptr(d_loss), L.ptr(d_h), L.ptr_array(grads), L.stream_of(h))
        return (d_h, None, *grads)


def ge_head_loss(h, classifier, label):
    """h (B, d) pooled rows, classifier nn.Linear(d, C), label (B,) -> (per-bag `ce` loss (B,), Y (B, C)).  d in 128 / 256 /
    512 and C in 2..8, anything else raises; a label outside [0, C) gives that bag a NaN loss and no gradient."""
    return GeHeadLossFn.apply(h, label, classifier.weight, classifier.bias)


def bump_step_counters(rng_epoch=None, adam_step=None):
    """rng_epoch (int64[1]) += 1 and adam_step (int32[1]) += 1 in one launch (either may be None)."""
    t = rng_epoch if rng_epoch is not None else adam_step
    L.call("mpo_step_counters_bump", L.ptr(rng_epoch), L.ptr(adam_step), L.stream_of(t))


# ------------------------------------------------------------------------------------ K2
def next_dropout_stream(n_elements: int):
    """(seed, offset) for one dropout mask of n_elements: the generator's counter space is carved sequentially per
    process, the seed follows torch.initial_seed() (so torch.manual_seed(rank-dependent) de-correlates ranks)."""
    return _reserve((n_elements + 3) // 4)          # (one counter per four elements)


def rng_state() -> dict:
    """The dropout generator's three values: {'seed': torch.initial_seed(), 'calls': the host counter the stream offsets
    are carved from, 'epoch': the device epoch scalar's value, None while none is installed}.  One host sync when an
    epoch tensor is installed."""
    epoch = None if _rng_epoch_tensor is None else int(_rng_epoch_tensor)
    return {"seed": int(torch.initial_seed()), "calls": int(_rng_calls), "epoch": epoch}


def set_rng_state(state: dict, device=None):
    """Put rng_state() back.  The epoch tensor is written IN PLACE (a captured step holds its address); with none
    installed and a stored epoch, one is created on `device` and installed.  A stored epoch of None zeroes an installed
    tensor (no tensor and epoch 0 draw the same masks).  The seed is re-seeded only where it differs."""
    global _rng_calls
    if int(state["seed"]) != torch.initial_seed():
        torch.manual_seed(int(state["seed"]))
    _rng_calls = int(state["calls"])
    epoch = state.get("epoch")
    if _rng_epoch_tensor is not None:
        _rng_epoch_tensor.fill_(0 if epoch is None else int(epoch))
    elif epoch is not None:
        if device is None:
            raise ValueError("set_rng_state: no epoch tensor is installed; name the device to create one on")
        set_rng_epoch(torch.full((1,), int(epoch), dtype=torch.int64, device=device))


# ------------------------------------------------------------------------------------ fixed-budget patch sampling
class RowSampler:
    """k randomly chosen rows of every slide of a window, without replacement, gathered on the device into one buffer
    (csrc/bag_sample.hip; beyond the reference, off unless asked for).  Owns the output buffer (n_slides * k, width), the
    output BagBatch and the device-resident descriptor (base pointer + row offsets of the bound window) the gather reads at
    run time.

    static=True (what a captured step needs): every bound window must have at least k rows per slide; the output batch
    -- lengths [k] * n_slides, its cu and its work plan -- is built HERE (both do an H2D copy, which must not happen
    inside a capture) and is the same object for every window, so everything behind the sampler sees static shapes.
    static=False (eager): a slide shorter than k is passed whole (k_b = min(k, M_b), in permuted order) and the output
    batch is built per bind().

    bind(bags) writes the descriptor with one tiny launch on the current stream (no host sync, no staging memory) and
    keeps `bags` alive; the rows must stay valid until the last gather that reads the binding has finished (for a ring
    slot of ingest.WindowFeeder: bind and run the step before requesting `depth` further windows).
    __call__() launches the gather on the current stream and returns the output batch.  The draw is keyed by
    (torch.initial_seed(), one offset taken with _reserve(RNG_SPAN), the device epoch): every eager call draws anew; in a
    capture the offset is baked and the epoch (bumped inside the graph) advances the draw.  The sampler takes exactly ONE
    value of the generator's host counter per call -- the offset is a key, not a range of counters -- so
    GraphedWindowStep.rng_base and checkpoint.save / load see it like any other stream.  `last_stream` = (seed, offset) of
    the most recent call, for tests/row_sampling_replay.py.

    source="slides": the sampler binds SlideSet windows (separately stored slides of a cohort resident on the device) and
    gathers through their descriptor layout (same file, same kernel); same draw, keyed by the slide's position in the window.
    Every window type names its source (`sampler_source`); for_window builds the sampler a given window needs.  A SlideSet with
    `cycle` laps a slide shorter than k in its permuted order, so the output keeps lengths [k] * n_slides: static mode
    accepts such a window, and refuses a short slide without `cycle` as it does for a BagBatch.  A sampler binds the
    kind of window it was built for and refuses the other.

    device_feature_scale=True on an fp32 sampler: it owns `scale`, a (1,) fp32 tensor, runs feature_scale_device over the
    rows it wrote after EVERY gather, eager or captured, and tags the output batch's data with it
    (_mpo_feature_scale_dev), so that the fp32 patch layer reads the sample's scale on the device -- no host read, nothing
    baked into a graph.  On a bf16 or fp16 sampler, and without the flag, `scale` is None and nothing is added (an fp16
    window's patch layer, patch_fc_f16, takes no feature scale)."""

    RNG_SPAN = 0            # _reserve(0): one counter value
    SOURCES = {"window": (BagBatch, "mpo_bag_sample_desc_bytes", "mpo_bag_sample_rows"),
               "slides": (SlideSet, "mpo_bag_sample_slides_desc_bytes", "mpo_bag_sample_slides")}

    def __init__(self, n_slides: int, k: int, width: int, dtype, device, static: bool = True,
                 device_feature_scale: bool = False, source: str = "window"):
        if source not in self.SOURCES:
            raise ValueError(f"RowSampler: source '{source}' ({' | '.join(self.SOURCES)})")
        self.source = source
        self.window_type, desc_bytes, self.gather = self.SOURCES[source]
        n_slides, k, width = int(n_slides), int(k), int(width)
        if n_slides < 1 or k < 1:
            raise ValueError(f"RowSampler: n_slides {n_slides} and k {k} must be at least 1")
        if dtype not in (torch.bfloat16, torch.float16, torch.float32):
            raise ValueError(f"RowSampler: bag dtype must be float32, float16 or bfloat16, got {dtype}")
        self.elem_bytes = torch.empty(0, dtype=dtype).element_size()     # (the gather copies bytes: 2 or 4 per element)
        if (width * self.elem_bytes) % 16:
            raise ValueError(f"RowSampler: a row of {width} x {self.elem_bytes} bytes is not a multiple of 16 bytes")
        self.n_slides, self.k, self.width, self.dtype, self.static = n_slides, k, width, dtype, bool(static)
        self.device = torch.device(device)
        self.out = torch.empty(n_slides * k, width, dtype=dtype, device=self.device)
        self.desc = torch.zeros(getattr(L.lib(), desc_bytes)(n_slides) // 8, dtype=torch.int64, device=self.device)
        self.bound = None
        self.last_stream = None
        self.batch = None
        # fp32 with device_feature_scale: the (1,) scale of the rows the last gather wrote; None: no range pass
        self.scale = (torch.ones(1, dtype=torch.float32, device=self.device)
                      if device_feature_scale and dtype == torch.float32 else None)
        if self.static:
            self._set_batch(BagBatch(self.out, make_cu([k] * n_slides, self.device), [k] * n_slides))
            self.batch.plan()

    @classmethod
    def for_window(cls, bags, k: int, **kw) -> "RowSampler":
        """The sampler for windows like `bags` (a BagBatch or a SlideSet): its slide count, row width, dtype, device and source."""
        return cls(bags.n_slides, int(k), bags.width, bags.dtype, bags.device, source=bags.sampler_source, **kw)

    def _set_batch(self, batch):
        self.batch = batch
        if self.scale is not None:
            batch.data._mpo_feature_scale_dev = self.scale

    def check(self, bags):
        """Raise ValueError with the reason when `bags` cannot be bound."""
        if not isinstance(bags, self.window_type):
            raise ValueError(f"RowSampler: the sampler was built for {self.window_type.__name__} windows (source='{self.source}': its "
                             f"descriptor and gather address the rows that way), not for a {type(bags).__name__}")
        if bags.n_slides != self.n_slides:
            raise ValueError(f"RowSampler: the window has {bags.n_slides} slides, the sampler was built for {self.n_slides}")
        for x in bags.row_tensors():
            if x.dim() != 2 or int(x.shape[1]) != self.width:
                raise ValueError(f"RowSampler: the window's rows are {tuple(x.shape)[1:]} wide, the sampler was built for width "
                                 f"{self.width}")
            if x.dtype != self.dtype:
                raise ValueError(f"RowSampler: the window is stored as {x.dtype}, the sampler was built for {self.dtype}")
        if self.static and not bags.cycle:
            for b, m in enumerate(bags.lengths):
                if m < self.k:
                    raise ValueError(f"RowSampler: slide {b} has {m} rows, fewer than k = {self.k} (static mode neither pads "
                                     "nor samples with replacement)")

    def bind(self, bags):
        self.check(bags)
        if self.source == "slides":
            L.call("mpo_bag_sample_bind_slides", L.ptr(self.desc), L.ptr(bags.table_ptrs), L.ptr(bags.table_lens), bags.n_table,
                   L.ptr(bags.ids), self.n_slides, self.k, int(bags.cycle), L.stream_of(self.desc))
        else:
            L.call("mpo_bag_sample_bind", L.ptr(self.desc), L.ptr(bags.data), L.ptr(bags.cu), self.n_slides, self.k,
                   L.stream_of(self.desc))
        self.bound = bags
        if not self.static:
            lengths = [self.k if bags.cycle else min(self.k, int(m)) for m in bags.lengths]
            self._set_batch(BagBatch(self.out[:sum(lengths)], make_cu(lengths, self.device), lengths))
        return self

    def __call__(self) -> BagBatch:
        if self.bound is None:
            raise RuntimeError("RowSampler: bind(bags) a window first")
        seed, off = _reserve(self.RNG_SPAN)
        self.last_stream = (seed, off)
        self.batch.data.__dict__.pop("_mpo_feature_scale", None)        # (fp32: the rows are about to change under the cache)
        L.call(self.gather, L.ptr(self.desc), self.n_slides, self.k, self.width, self.elem_bytes, seed, off,
               _epoch(), L.ptr(self.out), L.stream_of(self.out))
        if self.scale is not None:            # over the rows the gather just wrote (ocu[n_slides] of them: the batch's)
            feature_scale_device(self.batch.data, out=self.scale)
        return self.batch


# ------------------------------------------------------------------------------------ K2 (NaCAGaT co-attention)
# K = H W_k^T + b_k is formed on this side of the ABI, in front of the one core call each way, and differentiated behind it:
#   route        taken for                     _project_key                          _finish_key
#   'kernel'     bf16 bag, E = 256 (medium)    mpo_key_projection                    'fused': one hand-written pass, dW_k kernel
#   'gemm_bf16'  bf16 bag, E = 128 (small)     fp32 GEMM over a float copy           'one_pass': fp32 GEMM, one pass, dW_k kernel
#   'gemm_f32'   fp32 bag, E <= 256            fp32 GEMM                             'gemm': two fp32 GEMMs
#   'halves'     E = 512 (big), either dtype   two half GEMMs + the permuted bag     'gemm' after un-permuting, cast on the way out
# False: the patch-side gradient of K2 as library GEMM + mpo_nacagat_patch_grad (the r02 path; kept for the small model and as
# the cross-check of csrc/k2_patchgrad.hip in tools/gpu_diag_nacagat.py)
k2_fused_patch_grad = True


def _key_route(bag_dtype, E: int, bag_relu_gate: float) -> str:
    """The one place that looks at (bag dtype, E, gate)."""
    bf16 = bag_dtype == torch.bfloat16
    if bag_relu_gate != 0.0 and not bf16:
        raise ValueError("bag_relu_gate (fused ReLU/dropout derivative of the patch layer) needs a bf16-stored bag")
    if E == 512 and bag_relu_gate != 0.0:
        raise ValueError("embed_dim 512: the fused ReLU/dropout gate of the patch layer is built for embed_dim <= 256")
    if E == 512:
        return "halves"
    return ("kernel" if E == 256 else "gemm_bf16") if bf16 else "gemm_f32"


def _key_finish(route: str) -> str:
    """How a backward of `route` finishes, read when it runs: k2_fused_patch_grad = False sends 'kernel' the 'gemm_bf16' way."""
    if route in ("gemm_f32", "halves"):
        return "gemm"
    return "fused" if route == "kernel" and k2_fused_patch_grad else "one_pass"


def _project_key(route, bag, w_k, b_k, stream):
    """-> (K in fp32, the bag as the core call reads it: itself, or its split-halves copy)."""
    T, E = bag.shape
    if route == "halves":
        # 'big' (models/nacagat/nacagat.py:17-18): both bags in the split-halves layout [2][T][256] of include/mpo_hip.h --
        # K half h straight out of its own GEMM (rows 256 h .. of W_k), the bag as one strided copy
        xf = bag.float().contiguous()
        kbag = torch.empty(2, T, 256, device=bag.device, dtype=torch.float32)
        for h in range(2):
            L.call("mpo_linear_forward", L.ptr(xf), L.ptr(w_k[256 * h:]), L.ptr(b_k[256 * h:]), L.ptr(kbag[h]), T, E, 256, 1.0, L.ACT["none"], stream)
        return kbag, bag.view(T, 2, 256).permute(1, 0, 2).contiguous()
    kbag = torch.empty(T, E, device=bag.device, dtype=torch.float32)
    if route == "kernel":
        # HIP key projection: bf16 bag (exact) x fp32 weights split into three bf16 terms, fp32 accumulate and output
        L.call("mpo_key_projection", L.ptr(bag), T, E, L.ptr(w_k), L.ptr(b_k), L.ptr(kbag), stream)
    else:
        # fp32 bag (or the small model's bf16 bag): the exact-fp32 MFMA GEMM of the token tail in its many-row form
        L.call("mpo_linear_forward", L.ptr(bag.float().contiguous()), L.ptr(w_k), L.ptr(b_k), L.ptr(kbag), T, E, E, 1.0, L.ACT["none"], stream)
    return kbag, bag


def _finish_key(finish, ctx, bag, amap, w_k, d_k, d_h, d_ctx, d_wk, ws):
    """-> d_h: back through K = H W_k^T + b_k.  The forward K stays fp32 (the gate amplifies its rounding); its GRADIENT goes
    through bf16 operands with fp32 accumulation for a bf16 bag of E <= 256: dW_k as a batched split-K product (one 480 000-deep
    fp32 contraction took 1.19 ms in rocBLAS), dH += dK W_k as a bf16 GEMM (0.59 ms in fp32).  (d_in_b[E:2E], the key bias
    gradient = column sums of d_k, came out of the kernel that wrote d_k.)"""
    (T, E), batch, gate, s = bag.shape, ctx.batch, ctx.bag_relu_gate, L.stream_of(bag)
    if finish == "gemm":
        # d_h += d_k W_k and dW_k = d_k^T H on the fp32 MFMA GEMMs (many-row / long-K forms); split-halves results go back to
        # [T, 512] first (a bf16 bag: in fp32, rounded once on the way out)
        if d_k.dim() == 3:
            d_k, d_h = (t.permute(1, 0, 2).reshape(T, E).float().contiguous() for t in (d_k, d_h))
        L.call("mpo_linear_backward_input", L.ptr(d_k), L.ptr(w_k), L.ptr(d_h), T, E, E, 1.0, 1, s)
        L.call("mpo_linear_backward_weight", L.ptr(d_k), L.ptr(bag.float().contiguous()), L.ptr(d_wk), None, T, E, E, 1.0, s)
        return d_h.to(bag.dtype)
    # bf16 bag: dH = (dK W_k + A_drop^T dctx) (.) gate is finished by ONE pass over the bag instead of outer-product kernel ->
    # addmm_ read-modify-write -> element-wise derivative pass
    colsum = _bias_grad_slot(ctx.bag_bias, E, bag.device) if gate != 0.0 else None
    head = (L.ptr(batch.cu), batch.n_slides, T, batch.max_rows, ctx.n_q, E, L.ptr(amap), L.ptr(d_ctx))
    tail = (gate, L.ptr(colsum), batch.plan(), L.ptr(ws), ws.numel(), s)
    if finish == "fused":                      # the product with W_k inside the pass (no library GEMM): csrc/k2_patchgrad.hip
        d_h = torch.empty_like(d_k)
        L.call("mpo_nacagat_patch_grad_fused", *head, L.ptr(d_k), L.ptr(w_k), L.ptr(bag), L.ptr(d_h), *tail)
    else:                                      # the small model (E = 128): dK W_k on the fp32 MFMA GEMM (many-row form) first
        dhf = torch.empty(T, E, device=bag.device, dtype=torch.float32)
        L.call("mpo_linear_backward_input", L.ptr(d_k.float()), L.ptr(w_k), L.ptr(dhf), T, E, E, 1.0, 0, s)
        d_h = dhf.to(torch.bfloat16)
        L.call("mpo_nacagat_patch_grad", *head, L.ptr(d_h), L.ptr(bag), L.ptr(d_h), *tail)
    if colsum is not None:
        d_h._mpo_colsum = colsum              # the producing layer's bias gradient (PatchFcFn.backward picks it up)
    patch_weight_grad(d_k, bag, d_wk)         # dW_k = d_k^T H_bag (hand-written for 256 x 256, bf16)
    return d_h


class CoAttnNaCAGaTFn(torch.autograd.Function):
    """NaCAGaT narrow-gated attention core over a ragged window (models/blocks.py:114-206).
    Returns (q_proj, attn_out, post-dropout map).  K = H W_k^T + b_k is formed here first, by the bag's key route.  K is
    always fp32, also for a bf16-stored bag: the gate multiplies k's rounding error (hard part 4)."""

    @staticmethod
    def forward(ctx, query, bag_data, in_w, in_b, out_w, out_b, batch: BagBatch, drop_p: float, bag_relu_gate: float = 0.0,
                qpass_owned: bool = False):
        lib = L.lib()
        n_slides = batch.n_slides
        R, E = query.shape
        n_q = R // n_slides
        dev, T = query.device, batch.total_rows
        query = query.contiguous()
        ctx.set_materialize_grads(False)
        ctx.bag_relu_gate = float(bag_relu_gate)
        ctx.bag_bias = getattr(bag_data, "_mpo_bias_param", None)
        ctx.route = _key_route(bag_data.dtype, E, ctx.bag_relu_gate)
        kbag, hb = _project_key(ctx.route, bag_data, in_w[E:2 * E], in_b[E:2 * E], L.stream_of(query))
        q_proj = torch.empty(R, E, device=dev, dtype=torch.float32)
        out = torch.empty(R, E, device=dev, dtype=torch.float32)
        amap = torch.empty(n_q * T, device=dev, dtype=torch.float32)
        score_maps = torch.empty(2 * n_q * T, device=dev, dtype=torch.float32)
        saved = torch.empty(lib.mpo_nacagat_saved_floats(n_slides, n_q, E), device=dev, dtype=torch.float32)
        ws = _workspace(lib.mpo_nacagat_workspace_bytes(n_slides, n_q, E, batch.max_rows, T), dev)
        seed, offset = next_dropout_stream(n_q * T) if drop_p > 0 else (0, 0)
        L.call("mpo_coattn_nacagat_forward",
            L.ptr(kbag), L.MPO_F32, L.ptr(hb), L.bag_dtype_code(bag_data), L.ptr(batch.cu), n_slides, T, batch.max_rows,
            L.ptr(query), n_q, E, L.ptr(in_w), L.ptr(in_b), L.ptr(out_w), L.ptr(out_b), float(drop_p), seed, offset,
            _epoch(), L.ptr(q_proj), L.ptr(out), L.ptr(amap), L.ptr(score_maps), L.ptr(saved),
            batch.plan(), L.ptr(ws), ws.numel(), L.stream_of(query))
        ctx.save_for_backward(query, bag_data, hb, kbag, in_w, in_b, out_w, saved, score_maps, amap)   # (hb: bag_data itself, or its split-halves copy)
        ctx.param_refs = (in_w, in_b, out_w, out_b)
        ctx.batch, ctx.n_q, ctx.drop = batch, n_q, (float(drop_p), seed, offset)
        ctx.qpass_owned = bool(qpass_owned)
        # (4th output: the query handed on to its other consumers -- NaCAGaT's CAG and the omic branch's tokens; their gradient
        #  arrives here and the backward's d_query product accumulates onto it)
        return q_proj, out, amap, query.view_as(query)

    @staticmethod
    def backward(ctx, d_qproj, d_out, d_map, d_qpass=None):
        lib = L.lib()
        query, bag_data, hb, kbag, in_w, in_b, out_w, saved, score_maps, amap = ctx.saved_tensors
        batch, n_q, finish = ctx.batch, ctx.n_q, _key_finish(ctx.route)
        drop_p, seed, offset = ctx.drop
        R, E = query.shape
        dev, T = query.device, batch.total_rows
        d_out = d_out.contiguous() if d_out is not None else torch.zeros(R, E, device=dev)
        d_qproj = d_qproj.contiguous() if d_qproj is not None else None
        d_map = d_map.contiguous() if d_map is not None else None
        d_query, accumulate = _query_grad_buffer(d_qpass, ctx.qpass_owned, query)
        d_k = torch.empty_like(kbag, dtype=bag_data.dtype)       # a bf16 bag takes its key gradient in bf16 (see _finish_key)
        # 'gemm': the core call writes d_h and _finish_key adds to it; else it hands out d_ctx and _finish_key builds d_h
        d_h = torch.empty_like(hb) if finish == "gemm" else None
        d_ctx = None if finish == "gemm" else torch.empty(R, E, device=dev, dtype=torch.float32)
        d_in_w, d_in_b, d_out_w, d_out_b = (grad_out(p) for p in ctx.param_refs)
        ws = _workspace(lib.mpo_nacagat_workspace_bytes(batch.n_slides, n_q, E, batch.max_rows, T), dev)   # (also the finish's)
        L.call("mpo_coattn_nacagat_backward",
            L.ptr(kbag), L.MPO_F32, L.ptr(hb), L.bag_dtype_code(bag_data), L.ptr(batch.cu), batch.n_slides, T,
            batch.max_rows, L.ptr(query), n_q, E, L.ptr(in_w), L.ptr(in_b), L.ptr(out_w), drop_p, seed, offset,
            _epoch(), L.ptr(saved), L.ptr(score_maps), L.ptr(amap), L.ptr(d_out), L.ptr(d_map), L.ptr(d_qproj),
            L.ptr(d_query), int(accumulate), L.ptr(d_k), L.bag_dtype_code(d_k), L.ptr(d_in_b[E:2 * E]), L.ptr(d_h), L.ptr(d_ctx), L.ptr(d_in_w), L.ptr(d_in_b), L.ptr(d_out_w),
            L.ptr(d_out_b), batch.plan(), L.ptr(ws), ws.numel(), L.stream_of(query))
        d_h = _finish_key(finish, ctx, bag_data, amap, in_w[E:2 * E], d_k, d_h, d_ctx, d_in_w[E:2 * E], ws)
        return d_query, d_h, d_in_w, d_in_b, d_out_w, d_out_b, None, None, None, None


def coattn_nacagat(query, batch: BagBatch, in_w, in_b, out_w, out_b, drop_p: float, bag_relu_gate: float = 0.0,
                   hand_on: bool = False, _qpass_owned: bool = False):
    """query (n_slides*n_q, E) -> (q_proj, attn_out (n_slides*n_q, E), ragged post-dropout map[, query handed on]).
    bag_relu_gate = 1/(1-p) when the bag comes from patch_fc(..., pre_gated_grad=True): d_bag then already carries
    that layer's ReLU/dropout derivative (bf16 bags only).  hand_on: a 4th result, the query for its other consumers.
    _qpass_owned: see patch_coattn_mcat."""
    res = CoAttnNaCAGaTFn.apply(query, batch.data, in_w, in_b, out_w, out_b, batch, drop_p, bag_relu_gate, bool(_qpass_owned))
    return res if hand_on else res[:3]
