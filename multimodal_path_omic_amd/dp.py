"""Process-per-GPU data parallelism for slide windows.

Slides are independent units, so the only exchange step is ONE all-reduce of the flat fp32 gradient
buffer per optimiser step (RCCL over xGMI via torch.distributed backend 'nccl'; 'gloo' on CPU for
tests).  Parameter .grad tensors are views into one contiguous buffer, so backward accumulates
straight into the bucket and the collective needs no packing.  The reference's nn.DataParallel
(models/mcat/main.py:267-268) is not reproduced: with batch_size=1 it never used more than one GPU.

Whole epochs over a cohort sharded across the ranks: shard_slides, epoch_orders, global_order and gather_ragged below are
the plan (pure host functions) and the one ragged collective; harness.train_epoch_dp / validate_dp are the loops.
"""
from __future__ import annotations

from typing import List, Sequence

import torch
import torch.distributed as dist


SLICE_ALIGN = 64        # elements: every parameter's slice starts on a 256-byte boundary of the flat buffers


def _aligned_offsets(params):
    """Start offset of every parameter in the flat buffers and their total length.  Slices are 256-byte aligned: the
    GEMM kernels read weights with 16-byte loads, and one 1-element bias (attention_c.bias) packed tight would leave
    every parameter behind it 4-byte aligned, i.e. on the general (guarded) GEMM body."""
    offs, off = [], 0
    for p in params:
        offs.append(off)
        off += (p.numel() + SLICE_ALIGN - 1) // SLICE_ALIGN * SLICE_ALIGN
    return offs, off


class FlatGradBucket:
    """One contiguous fp32 gradient buffer; every parameter owns a slice (`p._mpo_grad_view`, 256-byte aligned,
    `offsets[i]`; the padding between slices stays zero).

    Per window:  begin() -> forward/backward -> finish().  begin() unsets every `p.grad`, so the HIP
    backward entries write their parameter gradients straight into the slices (ops.grad_out) and autograd
    adopts those views as `.grad` without an accumulate kernel; finish() copies in the few gradients that
    came from stock torch ops and zero-fills slices of unused parameters.  A second backward before the
    optimiser step accumulates in place into the same slices."""

    def __init__(self, params: Sequence[torch.nn.Parameter]):
        self.params = [p for p in params if p.requires_grad]
        self.offsets, n = _aligned_offsets(self.params)
        dev = self.params[0].device
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        for p, off in zip(self.params, self.offsets):
            p._mpo_grad_view = self.flat[off:off + p.numel()].view_as(p)
            p.grad = p._mpo_grad_view.view(p.shape)

    def begin(self):
        for p in self.params:
            p.grad = None
            p._mpo_slice_taken = False

    def finish(self):
        for p in self.params:
            view = p._mpo_grad_view
            if p.grad is None:
                view.zero_()
            elif p.grad.data_ptr() != view.data_ptr():
                view.copy_(p.grad)
            else:
                continue
            p.grad = view.view(p.shape)

    def head_numel(self, param) -> int:
        """Number of leading bucket elements owned by `param`, which must be the FIRST parameter of the bucket (the
        split exchange reduces flat[head:] while the patch layer's weight gradient, flat[:head], is still being
        computed).  Raises if the layout assumption does not hold."""
        if param._mpo_grad_view.data_ptr() != self.flat.data_ptr():
            raise RuntimeError("split exchange: the patch layer's weight (H.0.weight) must lead the gradient bucket")
        return param.numel()

    def zero(self):
        self.flat.zero_()
        for p in self.params:
            p.grad = p._mpo_grad_view.view(p.shape)

    def all_reduce_mean(self, group=None):
        """Sum over ranks, divide by world size: with per-rank 1/grad_acc_step loss scaling the update
        equals the reference's accumulation over world_size * grad_acc_step slides."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            if dist.get_backend(group) == "nccl":            # RCCL averages inside the collective: no extra 16 MB pass
                dist.all_reduce(self.flat, op=dist.ReduceOp.AVG, group=group)
            else:
                dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)
                self.flat.div_(dist.get_world_size(group))

    def all_reduce_mean_async(self, lo: int = 0, hi: int = None, group=None):
        """Start the mean all-reduce of flat[lo:hi] and return a handle whose wait() orders the current stream behind it
        (None when there is nothing to reduce): lets the caller keep computing into OTHER slices of the bucket meanwhile."""
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
            return None
        view = self.flat[lo:hi]
        if dist.get_backend(group) == "nccl":
            return dist.all_reduce(view, op=dist.ReduceOp.AVG, group=group, async_op=True)
        work = dist.all_reduce(view, op=dist.ReduceOp.SUM, group=group, async_op=True)
        world = dist.get_world_size(group)

        class _Then:
            def wait(self_inner):
                work.wait()
                view.div_(world)
        return _Then()


# torch.optim class and the names of the two per-parameter moments (state1, state2 of the flat pass) per algorithm
_TORCH_OPTIM = {"adam": ("Adam", ("exp_avg", "exp_avg_sq")), "adamax": ("Adamax", ("exp_avg", "exp_inf")),
                "adadelta": ("Adadelta", ("square_avg", "acc_delta")), "sgd": ("SGD", ())}
# param-group flags of torch.optim whose non-default setting selects arithmetic the flat pass does not have
_UNBUILT_FLAGS = ("amsgrad", "maximize", "decoupled_weight_decay", "momentum", "dampening", "nesterov")


def package_only_parameter_names(model) -> "List[str]":
    """Names of the parameters of `model` that the reference model does not register (modules declare them in
    `package_only_parameters`; today fusion.GatedConcatFusion's gates): they appear in neither dict a reference program
    reads from a checkpoint."""
    out = []
    for prefix, module in model.named_modules():
        for sub in getattr(module, "package_only_parameters", ()):
            head = f"{prefix}.{sub}." if prefix else f"{sub}."
            out += [n for n, _ in model.named_parameters() if n.startswith(head)]
    return out


def _host_clone(t: torch.Tensor) -> torch.Tensor:
    """A compact copy on the CPU (never a view: torch.save pickles a view's whole storage)."""
    t = t.detach()
    return t.cpu() if t.device.type != "cpu" else t.clone()


class _TorchStateDict:
    """state_dict() / load_state_dict() of the flat optimisers in the format of the torch.optim class they restate, so that
    either side continues a run of the other.  Expects lr, betas, eps, wd and what _FlatState holds."""

    def _param_group(self, n_params: int) -> dict:
        """The one param group as the installed torch.optim class writes it: its own key set and flag defaults."""
        cls_name, _ = _TORCH_OPTIM[self.algorithm]
        kw = dict(lr=self.lr, weight_decay=self.wd)
        if self.algorithm in ("adam", "adamax"):
            kw.update(betas=tuple(self.betas), eps=self.eps)
        elif self.algorithm == "adadelta":
            kw.update(rho=self.betas[0], eps=self.eps)
        group = getattr(torch.optim, cls_name)([torch.zeros(1)], **kw).state_dict()["param_groups"][0]
        group["params"] = list(range(n_params))
        return group

    def _split_by_name(self, model):
        """(bucket indices of the parameters the reference has, in its order; {name: bucket index} of the others)."""
        if model is None:
            return list(range(len(self.bucket.params))), {}
        by_id = {id(p): n for n, p in model.named_parameters()}
        names = [by_id.get(id(p)) for p in self.bucket.params]
        if None in names:
            raise ValueError("state_dict: the bucket holds a parameter that is not one of the model's")
        only = set(package_only_parameter_names(model))
        return ([i for i, n in enumerate(names) if n not in only], {n: i for i, n in enumerate(names) if n in only})

    def state_dict(self, model=None):
        """torch.optim.{Adam, Adamax, Adadelta, SGD}.state_dict() of the same run: one param group, `params` 0 .. n-1 in
        bucket order, per parameter `step` (0-dim fp32) and the two moments in the parameter's shape (SGD: no state).  Every
        tensor is a clone on the CPU.  One host sync (the step count).

        With `model`: returns (dict, package_only).  The dict covers the parameters the reference model has, in its
        filter(requires_grad, model.parameters()) order; `package_only` maps the names of the others
        (package_only_parameter_names) to their state entries."""
        shared, only = self._split_by_name(model)
        _, keys = _TORCH_OPTIM[self.algorithm]
        host = [m.detach().cpu() for m in self._moments()]
        t = float(int(self.t_dev))

        def entry(i):
            p, off = self.bucket.params[i], self.bucket.offsets[i]
            e = {"step": torch.tensor(t, dtype=torch.float32)}
            for k, m in zip(keys, host):
                e[k] = m[off:off + p.numel()].view(p.shape).clone()
            return e

        state = {j: entry(i) for j, i in enumerate(shared)} if keys else {}
        sd = {"state": state, "param_groups": [self._param_group(len(shared))]}
        if model is None:
            return sd
        return sd, ({n: entry(i) for n, i in only.items()} if keys else {})

    def load_state_dict(self, state_dict, model=None, package_only=None):
        """Continue from a state_dict() of this class or of the torch.optim class it restates (`step` a tensor or an int,
        moments of any float dtype).  Everything is checked first and then copied IN PLACE into the flat buffers, t_dev and
        lr_dev: every data_ptr() is kept (a captured step stays valid) and the padding stays zero.  Hyper-parameters come
        from the dict, as with torch.  Parameters without an entry (torch keeps none for a parameter that never had a
        gradient) get zero moments.  `model` / `package_only`: as returned by state_dict(model); package-only parameters
        without an entry (a file written by the reference) get zero moments too.  Raises ValueError on moments of another
        algorithm, a wrong shape or parameter count, or per-parameter steps that differ (there is one step count)."""
        shared, only = self._split_by_name(model)
        _, keys = _TORCH_OPTIM[self.algorithm]
        groups = state_dict["param_groups"]
        if len(groups) != 1:
            raise ValueError(f"load_state_dict: {len(groups)} param groups; the flat optimiser has one")
        group = groups[0]
        if len(group["params"]) != len(shared):
            raise ValueError(f"load_state_dict: parameter count differs: the state_dict lists {len(group['params'])} "
                             f"parameters, the optimiser holds {len(shared)}")
        for flag in _UNBUILT_FLAGS:
            if group.get(flag):
                raise ValueError(f"load_state_dict: {flag}={group[flag]!r} is not built in the flat {self.algorithm} pass")
        entries = {}                                        # bucket index -> (label, state entry)
        for j, pid in enumerate(group["params"]):
            e = state_dict["state"].get(pid)
            if e:
                entries[shared[j]] = (f"parameter {pid}", e)
        unknown = [k for k in state_dict["state"] if k not in group["params"]]
        if unknown:
            raise ValueError(f"load_state_dict: state for parameters {unknown[:5]} that the param group does not list")
        for name, e in (package_only or {}).items():
            if name not in only:
                raise ValueError(f"load_state_dict: package-only state for '{name}', which this model does not have")
            if e:
                entries[only[name]] = (f"parameter '{name}'", e)
        steps = set()
        for i, (label, e) in entries.items():
            got = sorted(k for k, v in e.items() if k != "step" and v is not None)
            if got != sorted(keys):
                raise ValueError(f"load_state_dict: {label} holds {got}: not the moments of '{self.algorithm}' "
                                 f"({', '.join(keys) if keys else 'none'})")
            for k in keys:
                if tuple(e[k].shape) != tuple(self.bucket.params[i].shape):
                    raise ValueError(f"load_state_dict: shape of {k} of {label} differs: the state_dict has "
                                     f"{tuple(e[k].shape)}, the parameter {tuple(self.bucket.params[i].shape)}")
            if "step" in e:
                steps.add(int(float(e["step"])))
        if len(steps) > 1:
            raise ValueError(f"load_state_dict: per-parameter steps differ ({sorted(steps)[:4]} ...): the flat optimiser "
                             f"keeps one step count")
        with torch.no_grad():
            for j, (k, flat) in enumerate(zip(keys, self._moments())):
                for i, (p, off) in enumerate(zip(self.bucket.params, self.bucket.offsets)):
                    sl = flat[off:off + p.numel()]
                    if i in entries:
                        sl.copy_(entries[i][1][k].reshape(-1))
                    else:
                        sl.zero_()
            if keys:
                self.t_dev.fill_(steps.pop() if steps else 0)
        self._set_hyper(group)

    def _set_hyper(self, group: dict):
        self.lr = float(group["lr"])
        if getattr(self, "lr_dev", None) is not None:
            self.lr_dev.fill_(self.lr)
        self.wd = float(group.get("weight_decay", 0.0))
        if self.algorithm in ("adam", "adamax"):
            self.betas, self.eps = tuple(float(b) for b in group["betas"]), float(group["eps"])
        elif self.algorithm == "adadelta":
            self.betas, self.eps = (float(group["rho"]), 0.0), float(group["eps"])


def _repoint_params(bucket: FlatGradBucket, tag: bool) -> torch.Tensor:
    """Flat fp32 parameter buffer laid out like the gradient bucket; every parameter is re-pointed at its slice (the padding
    between slices stays zero, and every update below keeps it zero).  tag: mark each parameter with its buffer
    (`_mpo_flat_param_base`): harness.weights_abs_sum then reduces the buffer once instead of every parameter."""
    flat_p = torch.zeros_like(bucket.flat)
    for p, off in zip(bucket.params, bucket.offsets):
        sl = flat_p[off:off + p.numel()].view_as(p)
        sl.copy_(p.data)
        p.data = sl
        if tag:
            p._mpo_flat_param_base = flat_p
    return flat_p


class _FlatState(_TorchStateDict):
    """What the flat optimisers share: parameters re-pointed into `flat_p`, the two flat moments of `algorithm` (`state1`,
    `state2`; None for sgd) and the step count `t_dev`.  The count is incremented and read on the device, so a step can sit
    inside a captured HIP graph and still apply the right bias correction on every replay."""

    def _allocate(self, bucket: FlatGradBucket, tag_params: bool):
        self.bucket = bucket
        self.flat_p = _repoint_params(bucket, tag_params)
        stateful = self.algorithm != "sgd"
        self.state1 = torch.zeros_like(self.flat_p) if stateful else None
        self.state2 = torch.zeros_like(self.flat_p) if stateful else None
        self.t_dev = torch.zeros(1, dtype=torch.int32, device=self.flat_p.device)

    def _advance(self, bump: bool):
        """bump=False: the caller has advanced t_dev already (ops.bump_step_counters: one launch for it and the epoch)."""
        if bump:
            self.t_dev += 1

    def _moments(self):
        return [] if self.state1 is None else [self.state1, self.state2]

    def state_tensors(self):
        """Every tensor a step writes (what a warm-up that must not train puts back)."""
        return [self.flat_p, *self._moments(), self.t_dev]


class FlatAdam(_FlatState):
    """torch.optim.Adam(lr, betas, eps, weight_decay) (the reference's default optimiser,
    models/mcat/main.py:284-300) as ONE HIP kernel over flat buffers (mpo_adam_step_flat): parameters are re-pointed at
    slices of a flat fp32 buffer laid out like the gradient bucket; exp_avg / exp_avg_sq are flat too.  Its parameters
    carry no `_mpo_flat_param_base`: an L1 penalty on a FlatAdam run is summed parameter by parameter, as it always was."""

    algorithm = "adam"

    def __init__(self, bucket: FlatGradBucket, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self._allocate(bucket, tag_params=False)
        self.exp_avg, self.exp_avg_sq = self.state1, self.state2

    def step(self, bump: bool = True):
        """One update (bump: see _advance)."""
        from . import _lib as L
        self._advance(bump)
        L.call("mpo_adam_step_flat", L.ptr(self.flat_p), L.ptr(self.bucket.flat), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq),
               self.flat_p.numel(), self.lr, self.betas[0], self.betas[1], self.eps, self.wd,
               0, L.ptr(self.t_dev), L.stream_of(self.flat_p))


class FlatOptimizer(_FlatState):
    """The reference's training.optimizer choices (models/mcat/main.py:284-300) as ONE HIP pass over flat buffers
    (mpo_optim_step_flat): 'adam' | 'adamax' | 'adadelta' | 'sgd', torch.optim 2.x single-tensor arithmetic in fp32.
    Parameters are re-pointed at slices of a flat buffer as in FlatAdam.

    The learning rate lives in a device scalar (`lr_dev`) and the step count in `t_dev`, so a captured step follows a
    schedule (FlatExponentialLR) and the bias correction.  `l1_lambda` > 0 folds the L1 penalty's gradient
    (training.lambda: lambda * l1_reg(model) added to every slide's loss, models/mcat/main.py:61,69, not divided by
    grad_acc_step) into the pass: g' = g + lambda * S * sign(p) + weight_decay * p, S = the window's slides over ALL ranks
    (step(l1_slides=S)); after the data-parallel AVG all-reduce this is the reference's update.

    `max_grad_norm` / `skip_nonfinite` (both off by default: step() is then the one call it always was) guard the step on
    the device, inside a captured graph as well: step() first measures g + lambda * S * sign(p) (ops.grad_norm_flat, two
    launches) and then runs the guarded pass, which scales that sum -- not the weight decay, which torch adds after the clip --
    by torch.nn.utils.clip_grad_norm_'s coefficient and, with skip_nonfinite, writes nothing when an element of it is an
    infinity or a NaN; a skipped step does not count in `t_dev`.  `grad_ctl` (16 bytes on the device) holds the outcome;
    `last_grad_norm`, `clip_coef` (fp32 (1,)) and `skipped_steps` (int32 (1,)) are views of it, read without a sync by
    whoever wants one.  Data-parallel runs step after the all-reduce: every rank measures the same bucket."""

    DEFAULTS = {"adam": dict(betas=(0.9, 0.999), eps=1e-8), "adamax": dict(betas=(0.9, 0.999), eps=1e-8),
                "adadelta": dict(betas=(0.9, 0.0), eps=1e-6), "sgd": dict(betas=(0.0, 0.0), eps=0.0)}

    def __init__(self, bucket: FlatGradBucket, algorithm: str = "adam", lr: float = 2e-4, weight_decay: float = 0.0,
                 betas=None, eps=None, rho=None, l1_lambda: float = 0.0, max_grad_norm: "float | None" = None,
                 skip_nonfinite: bool = False):
        """betas / eps default to torch.optim's for the algorithm; adadelta takes rho (default 0.9) instead of betas.
        max_grad_norm (None / 0: no clipping) and skip_nonfinite: the class docstring."""
        if algorithm not in self.DEFAULTS:
            raise ValueError(f"unknown flat optimiser '{algorithm}' ({' | '.join(self.DEFAULTS)})")
        d = self.DEFAULTS[algorithm]
        self.algorithm = algorithm
        self.betas = tuple(betas) if betas is not None else d["betas"]
        if algorithm == "adadelta":
            self.betas = (0.9 if rho is None else float(rho), 0.0)
        self.eps = d["eps"] if eps is None else float(eps)
        self.wd = float(weight_decay)
        self.l1_lambda = float(l1_lambda or 0.0)
        self._allocate(bucket, tag_params=True)
        self.lr = float(lr)
        self.lr_dev = torch.full((1,), self.lr, dtype=torch.float32, device=self.flat_p.device)
        self.max_grad_norm = float(max_grad_norm) if max_grad_norm else None
        if self.max_grad_norm is not None and not self.max_grad_norm > 0.0:
            raise ValueError(f"FlatOptimizer: max_grad_norm = {max_grad_norm} (a positive norm, or None for no clipping)")
        self.skip_nonfinite = bool(skip_nonfinite)
        self.grad_ctl = None
        if self.max_grad_norm is not None or self.skip_nonfinite:
            # the control block of include/mpo_grad_guard.h: norm, coef (fp32), nonfinite, skipped (int32)
            self.grad_ctl = torch.zeros(4, dtype=torch.int32, device=self.flat_p.device)
            self.last_grad_norm, self.clip_coef = self.grad_ctl[0:1].view(torch.float32), self.grad_ctl[1:2].view(torch.float32)
            self.skipped_steps = self.grad_ctl[3:4]

    def state_tensors(self):
        """_FlatState's, and the control block of a guarded optimiser (its count of skipped steps)."""
        return super().state_tensors() + ([] if self.grad_ctl is None else [self.grad_ctl])

    def set_lr(self, lr: float):
        """New learning rate (host value and the device scalar a captured step reads).  Call outside graph capture."""
        self.lr = float(lr)
        self.lr_dev.fill_(self.lr)

    def l1_value(self) -> torch.Tensor:
        """sum |p| over the flat parameters as a device scalar (deterministic; ops.flat_abs_sum)."""
        from . import ops
        return ops.flat_abs_sum(self.flat_p)

    def step(self, bump: bool = True, l1_slides: "int | None" = None):
        """One update (bump: see _advance).  l1_slides: the number of slides whose losses carried the L1 penalty since the
        last step (all ranks); required when l1_lambda > 0."""
        from . import ops
        if self.l1_lambda and l1_slides is None:
            raise ValueError("FlatOptimizer.step: l1_lambda > 0 needs l1_slides (slides of the window over all ranks)")
        self._advance(bump)
        l1 = self.l1_lambda * l1_slides if self.l1_lambda else 0.0
        if self.grad_ctl is None:
            ops.optim_step_flat(self.algorithm, self.flat_p, self.bucket.flat, self.state1, self.state2, self.lr, self.lr_dev,
                                self.betas[0], self.betas[1], self.eps, self.wd, l1, 1, self.t_dev)
            return
        ops.grad_norm_flat(self.bucket.flat, self.grad_ctl, self.flat_p, l1, self.max_grad_norm, self.skip_nonfinite, self.t_dev)
        ops.optim_step_flat_guarded(self.algorithm, self.flat_p, self.bucket.flat, self.state1, self.state2, self.grad_ctl,
                                    self.lr, self.lr_dev, self.betas[0], self.betas[1], self.eps, self.wd, l1, 1, self.t_dev,
                                    self.skip_nonfinite)


class FlatExponentialLR:
    """torch.optim.lr_scheduler.ExponentialLR (the reference's training.scheduler 'exp', models/mcat/main.py:302-307; one
    step per epoch, main.py:82-84) for a FlatOptimizer: the chainable form lr <- lr * gamma on a Python float, written to
    the optimiser's device scalar outside any graph."""

    def __init__(self, opt: FlatOptimizer, gamma: float):
        self.opt, self.gamma = opt, float(gamma)
        self.last_epoch = 0

    def step(self):
        self.last_epoch += 1
        self.opt.set_lr(self.opt.lr * self.gamma)

    def get_last_lr(self):
        return [self.opt.lr]


def assign_slides(lengths: Sequence[int], world_size: int) -> "List[List[int]]":
    """Length-aware split of one accumulation window across ranks: greedy longest-first bin packing
    on the patch count (step time = slowest rank; SURVEY.md section 7, hard part 7).  Deterministic;
    every rank computes the same assignment.  Returns slide indices per rank."""
    order = sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))
    loads = [0] * world_size
    out: "List[List[int]]" = [[] for _ in range(world_size)]
    for i in order:
        r = min(range(world_size), key=lambda k: (loads[k], k))
        out[r].append(i)
        loads[r] += lengths[i]
    for r in range(world_size):
        out[r].sort()
    return out


# ------------------------------------------------------------------------------------ epochs over a sharded resident cohort
# Every rank keeps its own slides resident for the whole run (harness.ResidentCohort([slides[i] for i in shards[rank]])) and
# runs the same number of windows per epoch: the one rule that keeps the collectives matched.  Everything below is a pure
# function of host lists, so every rank computes the whole plan and no size is ever exchanged.
def shard_slides(lengths: Sequence[int], world_size: int) -> "List[List[int]]":
    """The cohort's slides dealt to `world_size` ranks for a whole run: global slide ids per rank, each list sorted.  The
    slides are sorted by (-length, id) and dealt in boustrophedon order (rank 0 .. W-1, then W-1 .. 0, and so on), so the
    shards are disjoint, cover every slide, differ in SIZE by at most 1 and in ROWS by at most the longest slide (round j
    moves the difference of two ranks by at most that round's range of lengths, with alternating sign, and the rounds'
    ranges do not overlap).  Deterministic: every rank computes the same plan.
    Not assign_slides: that one balances the rows of one window and lets the counts fall where they may.  A sampled step
    costs k rows per slide whatever the slide's length, so equal counts balance compute; the rows balance memory."""
    world_size = int(world_size)
    if world_size < 1:
        raise ValueError(f"shard_slides: world_size {world_size} below 1")
    order = sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i))
    out: "List[List[int]]" = [[] for _ in range(world_size)]
    for j, i in enumerate(order):
        rnd, pos = divmod(j, world_size)
        out[pos if rnd % 2 == 0 else world_size - 1 - pos].append(i)
    for shard in out:
        shard.sort()
    return out


_MASK64 = (1 << 64) - 1


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK64
    return x ^ (x >> 31)


def _permutation(n: int, seed: int, epoch: int, rank: int) -> "List[int]":
    """Fisher-Yates over range(n) on a splitmix64 stream keyed by (seed, epoch, rank): integer arithmetic alone, so the
    order is the same on every host and under every library version."""
    state = _splitmix64(int(seed) & _MASK64)
    state = _splitmix64(state ^ (int(epoch) & _MASK64))
    state = _splitmix64(state ^ (int(rank) & _MASK64))
    perm = list(range(n))
    for i in range(n - 1, 0, -1):
        state = _splitmix64(state)
        j = state % (i + 1)             # (modulo bias below 2^-40 for any cohort that fits a machine)
        perm[i], perm[j] = perm[j], perm[i]
    return perm


def epoch_orders(shard_sizes: Sequence[int], n_per_window: int, seed: int, epoch: int):
    """The shuffled epoch of every rank and the number of windows all of them run: -> (orders, n_windows).  orders[r] is a
    permutation of range(shard_sizes[r]) -- ids LOCAL to rank r's cohort -- and a pure function of (seed, epoch, r,
    shard_sizes[r]): every rank can compute every rank's order, and one process can replay the global schedule
    (global_order).  n_windows = min over r of shard_sizes[r] // n_per_window: what harness.train_epoch_dp runs on EVERY
    rank, whatever its own shard would allow; the ids behind n_windows * n_per_window are that epoch's leftover.
    A world whose smallest shard holds fewer than n_per_window slides raises ValueError: it has no window to run."""
    sizes = [int(s) for s in shard_sizes]
    n = int(n_per_window)
    if not sizes or n < 1:
        raise ValueError(f"epoch_orders: {len(sizes)} shards and {n} slides per window (at least one of each)")
    if min(sizes) < n:
        r = sizes.index(min(sizes))
        raise ValueError(f"epoch_orders: rank {r}'s shard holds {sizes[r]} slides, fewer than one window of {n}: every rank "
                         "must run the same number of windows, and this world has none to run")
    return [_permutation(s, seed, epoch, r) for r, s in enumerate(sizes)], min(sizes) // n


def global_order(orders, shards, n_per_window: int, n_windows: int) -> "List[int]":
    """The GLOBAL slide ids one process would run to form the windows the ranks form together under (orders, n_windows) of
    epoch_orders over shards of shard_slides: global window w is rank 0's window w, then rank 1's, and so on -- n_windows
    windows of n_per_window * world slides."""
    n = int(n_per_window)
    out = []
    for w in range(int(n_windows)):
        for order, shard in zip(orders, shards):
            if len(order) < (w + 1) * n:
                raise ValueError(f"global_order: an order of {len(order)} ids has no window {w} of {n}")
            out += [shard[i] for i in order[w * n:(w + 1) * n]]
    return out


def _world(group=None) -> int:
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


def _rank(group=None) -> int:
    return dist.get_rank(group) if dist.is_available() and dist.is_initialized() else 0


def gather_ragged(t: torch.Tensor, sizes: Sequence[int], group=None) -> torch.Tensor:
    """Per-slide results of every rank, concatenated rank-major: `t` is (sizes[rank], ...) on this rank and `sizes` is the
    shard plan every rank holds already, so no size is exchanged -- pad to max(sizes), ONE all-gather, keep the valid
    prefixes.  The result is the same tensor, bit for bit, on every rank.  Without an initialised process group, or at world
    size 1, `t` itself comes back.  Raises ValueError, before the collective, where `sizes` does not name the world or
    this rank's rows.  (nccl: enqueued on the device, no host synchronisation; gloo stages through the host.)"""
    world = _world(group)
    if world == 1:
        return t
    sizes = [int(s) for s in sizes]
    rank = dist.get_rank(group)
    if len(sizes) != world or min(sizes) < 0 or int(t.shape[0]) != sizes[rank]:
        raise ValueError(f"gather_ragged: sizes {sizes} for a world of {world}, and {int(t.shape[0])} rows on rank {rank}")
    most = max(sizes)
    mine = t.contiguous()
    if sizes[rank] < most:
        mine = torch.cat([mine, mine.new_zeros((most - sizes[rank], *t.shape[1:]))])
    parts = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(parts, mine, group=group)
    return torch.cat([p[:s] for p, s in zip(parts, sizes)])
