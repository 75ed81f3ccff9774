"""Checkpoint and resume of a training run, in the reference's own file format.

The reference writes {'epoch', 'model_state_dict', 'optimizer_state_dict', 'loss'} every `checkpoint_epoch` epochs
(models/mcat/main.py:88-100, models/ge_nacagat/main.py:67-79) and reads the file back through `load_from_checkpoint`
(main.py:261-266, 309-312).  save() writes exactly those four keys -- the model's state_dict with the reference's names in
its order, the optimiser's in the format of the torch.optim class the flat optimiser restates -- so a reference program
continues a run of this package and load() continues a run of the reference.  One extra key, `mpo`, which the reference
never looks at, holds what exists only here:

    version          MPO_FORMAT
    algorithm        'adam' | 'adamax' | 'adadelta' | 'sgd'
    step             the optimiser's step count (torch keeps none for SGD)
    rng              ops.rng_state(): {'seed', 'calls', 'epoch'}, the dropout generator's three values
    scheduler        {'gamma', 'last_epoch'} of dp.FlatExponentialLR, or None
    graph_rng_base   harness.GraphedWindowStep.rng_base of the captured step (a list for a list of steps), or None:
                     pass it to the re-capture
    model_state      parameters the reference model does not register (dp.package_only_parameter_names: the gates of
    optimizer_state  fusion.GatedConcatFusion) and their optimiser state, by name

Every tensor in the file is a compact clone on the CPU: the parameters and moments are slices of padded flat buffers,
and torch.save of a view pickles the view's whole storage.  The file is read with torch.load(weights_only=True): nothing
in it is executed.

Data parallel: nothing in the file is rank-specific (every rank holds the same parameters, moments, step count and,
with the same seed, generator values).  Rank 0 saves, every rank loads the same file; no collective is involved.

Works alike for the fusion models and the gene-expression model (a model, a bucket, an optimiser; no omics).
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import NamedTuple

import torch

from . import ops
from .dp import _host_clone, package_only_parameter_names

MPO_FORMAT = 1


class Resume(NamedTuple):
    """What load() hands back: `epoch` and `loss` as stored (the reference stores the index of the epoch just FINISHED),
    the capture base for harness.GraphedWindowStep(rng_base=...) (None: none stored), and whether the file lacks the
    `mpo` block, i.e. was written by the reference."""
    epoch: object
    loss: object
    graph_rng_base: "int | list | None"
    from_reference: bool


def _split_model_state(model):
    only = set(package_only_parameter_names(model))
    shared, extra = OrderedDict(), OrderedDict()
    for k, v in model.state_dict().items():
        (extra if k in only else shared)[k] = _host_clone(v)
    return shared, extra


def _capture_base(graphed_step):
    if graphed_step is None:
        return None
    if isinstance(graphed_step, (list, tuple)):                  # one captured step per resident window
        return [int(g.rng_base) for g in graphed_step]
    return int(graphed_step.rng_base)


def save(path, model, opt, epoch, loss, scheduler=None, graphed_step=None):
    """Write the checkpoint of the module docstring to `path`.  opt: dp.FlatOptimizer or dp.FlatAdam over the model's
    parameters; loss: a number or a tensor, stored as given (a tensor as a CPU clone); scheduler: dp.FlatExponentialLR
    or None; graphed_step: the harness.GraphedWindowStep in use (or the list of them, one per resident window) or None.
    The file is written under a temporary name in the same directory and moved over `path` with os.replace: a job killed
    mid-write leaves the previous checkpoint whole.
    A few dozen device-to-host copies and one host sync; call it between steps, outside graph capture."""
    model_state, extra_model = _split_model_state(model)
    opt_state, extra_opt = opt.state_dict(model)
    mpo = {
        "version": MPO_FORMAT,
        "algorithm": opt.algorithm,
        "step": int(opt.t_dev),
        "rng": ops.rng_state(),
        "scheduler": None if scheduler is None else {"gamma": float(scheduler.gamma), "last_epoch": int(scheduler.last_epoch)},
        "graph_rng_base": _capture_base(graphed_step),
        "model_state": extra_model,
        "optimizer_state": extra_opt,
    }
    ck = {"epoch": epoch, "model_state_dict": model_state, "optimizer_state_dict": opt_state,
          "loss": _host_clone(loss) if torch.is_tensor(loss) else loss, "mpo": mpo}
    path = os.fspath(path)
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        # torch's sequential container, not the zip one: a checkpoint is 400-odd tensors, most of them tiny (biases, one
        # `step` per parameter), and a zip record with its 64-byte alignment costs ~250 bytes a tensor (98 KB for MCAT,
        # measured) against ~110 here.  torch.load reads both alike, weights_only included.
        torch.save(ck, tmp, _use_new_zipfile_serialization=False)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def peek(path) -> dict:
    """The file's contents on the CPU (weights_only: nothing is executed), nothing restored -- e.g. to read
    peek(path)['mpo']['graph_rng_base'] for a capture that comes before load()."""
    return torch.load(os.fspath(path), map_location="cpu", weights_only=True)


def load(path, model, opt=None, scheduler=None) -> Resume:
    """Restore `model` (and `opt`, `scheduler`, the dropout generator) from a file written by save() or by the reference's
    main.py.  Everything is copied IN PLACE: parameters re-pointed into an optimiser's flat buffer stay there, every
    data_ptr() is kept, and a step captured before the load stays valid (load-then-capture and capture-then-load give the
    same run; re-capture with rng_base=Resume.graph_rng_base).

    A file of the reference has no `mpo` block: the dropout generator is left alone, parameters only this package has keep
    their values and get zero moments, and the scheduler continues from the param group's `lr` as the reference's own
    resume does (its ExponentialLR is the chainable form lr <- lr * gamma, which dp.FlatExponentialLR is too)."""
    ck = peek(path)
    mpo = ck.get("mpo")
    if mpo is not None and mpo.get("version") != MPO_FORMAT:
        raise ValueError(f"checkpoint '{path}': mpo format {mpo.get('version')!r}, this package reads {MPO_FORMAT}")
    state = OrderedDict(ck["model_state_dict"])
    if mpo is not None:
        state.update(mpo["model_state"])
    only = set(package_only_parameter_names(model))
    res = model.load_state_dict(state, strict=False)
    missing = [k for k in res.missing_keys if k not in only]
    if missing or res.unexpected_keys:
        raise ValueError(f"checkpoint '{path}' does not fit the model: missing {missing[:5]}, "
                         f"unexpected {list(res.unexpected_keys)[:5]}")
    if opt is not None:
        if mpo is not None and mpo["algorithm"] != opt.algorithm:
            raise ValueError(f"checkpoint '{path}' holds the state of '{mpo['algorithm']}', the optimiser is "
                             f"'{opt.algorithm}'")
        opt.load_state_dict(ck["optimizer_state_dict"], model, None if mpo is None else mpo["optimizer_state"])
        if mpo is not None and not ck["optimizer_state_dict"]["state"]:
            opt.t_dev.fill_(int(mpo["step"]))                   # SGD: torch keeps no step count
    if mpo is not None:
        if scheduler is not None and mpo["scheduler"] is not None:
            scheduler.gamma = float(mpo["scheduler"]["gamma"])
            scheduler.last_epoch = int(mpo["scheduler"]["last_epoch"])
        ops.set_rng_state(mpo["rng"], device=next(model.parameters()).device)
    return Resume(ck["epoch"], ck["loss"], None if mpo is None else mpo["graph_rng_base"], mpo is None)
