"""CPU-only checks of the flat optimisers' gradient guard (include/mpo_grad_guard.h, csrc/grad_guard.hip, dp.FlatOptimizer's
max_grad_norm / skip_nonfinite, harness.TrainOptions): the header and its exports, the entries' refusals, and the options'
way from a training config to the optimiser's constructor.  Nothing here launches a kernel."""
import ctypes
import dataclasses
import inspect
import os

import pytest
import torch

from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import dp, harness, ops

HEADER = "mpo_grad_guard.h"
NAMES = ["mpo_grad_norm_flat_workspace_bytes", "mpo_grad_norm_flat", "mpo_optim_step_flat_guarded"]
TRAINING = {"loss": "ces", "alpha": 0.5, "grad_acc_step": 8, "optimizer": "adamax", "lr": 2e-3, "weight_decay": 1e-4,
            "lambda": 1e-5, "scheduler": "exp", "gamma": 0.9}


def test_header_parses_and_its_entries_are_exported_and_bound():
    with open(L.HEADER_PATH) as f:
        assert f'#include "{HEADER}"' in f.read()
    path = [p for p in L.MORE_HEADER_PATHS if os.path.basename(p) == HEADER]
    assert len(path) == 1 and os.path.dirname(path[0]) == os.path.dirname(L.HEADER_PATH)
    with open(path[0]) as f:
        signatures, constants, version = L.parse_header(f.read())
    assert list(signatures) == NAMES and not constants and version is None
    assert L.header_symbols(HEADER) == NAMES
    handle = ctypes.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert hasattr(handle, name), f"{name} declared in include/{HEADER} but not exported"
        assert name not in L.exported_symbols() + L.all_companion_symbols() + L.later_symbols()
    p, i, i64, f, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
    lib = L.lib()
    assert lib.mpo_grad_norm_flat_workspace_bytes.argtypes == [i64] and lib.mpo_grad_norm_flat_workspace_bytes.restype == z
    assert lib.mpo_grad_norm_flat.argtypes == [p, p, i64, f, f, i, p, p, p, z, p]
    # the guarded step: mpo_optim_step_flat's arguments, then ctl and skip_nonfinite in front of the stream
    plain = lib.mpo_optim_step_flat.argtypes
    assert lib.mpo_optim_step_flat_guarded.argtypes == plain[:-1] + [p, i] + plain[-1:]
    assert lib.mpo_abi_version() == 14 and L.ABI_VERSION == 14
    # one fp64 partial and one flag per workgroup of a grid that is a function of n alone, at most 1024 workgroups
    sizes = [lib.mpo_grad_norm_flat_workspace_bytes(n) for n in (0, 1, 1024, 1025, 1024 * 1024, 1024 * 1024 + 1, 1 << 40)]
    assert sizes == [12, 12, 12, 24, 12 * 1024, 12 * 1024, 12 * 1024]


def _rc(name, *args):
    rc = getattr(L.lib(), name)(*args)
    msg = L.lib().mpo_last_error()
    return rc, (msg.decode() if msg else "")


def test_refusals_come_before_any_launch():
    fake = 0x1000                 # never dereferenced: every call below is refused while its arguments are checked
    need = L.lib().mpo_grad_norm_flat_workspace_bytes(5000)
    # grads, params, n, l1, max_norm, skip_nonfinite, step_dev, ctl, workspace, workspace_bytes, stream
    for args, text in (((fake, None, 5000, 0.0, 1.0, 1, None, None, fake, need, None), "ctl"),
                       ((fake, None, 5000, 0.0, 1.0, 1, None, fake, fake, need - 1, None), "workspace"),
                       ((fake, None, 5000, 0.0, 1.0, 1, None, fake, None, need, None), "workspace"),
                       ((fake, None, 5000, 0.0, 1.0, 1, None, fake, fake + 4, need, None), "workspace"),
                       ((None, None, 5000, 0.0, 1.0, 1, None, fake, fake, need, None), "grads"),
                       ((fake, None, 5000, 1e-3, 1.0, 1, None, fake, fake, need, None), "params"),
                       ((fake, None, -1, 0.0, 1.0, 1, None, fake, fake, need, None), "n = -1"),
                       ((fake + 2, None, 5000, 0.0, 1.0, 1, None, fake, fake, need, None), "4-byte aligned")):
        rc, msg = _rc("mpo_grad_norm_flat", *args)
        assert rc == 1 and text in msg, (args, rc, msg)
    # algorithm, params, grads, state1, state2, n, lr, lr_dev, b1, b2, eps, wd, l1, step, step_dev, ctl, skip_nonfinite, stream
    tail = (64, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 0.0, 1, None)
    for args, text in (((7, fake, fake, fake, fake) + tail + (fake, 1, None), "algorithm"),
                       ((0, fake, fake, fake, fake) + tail + (None, 1, None), "ctl"),
                       ((1, fake, fake, None, None) + tail + (fake, 1, None), "state buffers"),
                       ((3, fake + 2, fake, None, None) + tail + (fake, 1, None), "4-byte aligned"),
                       ((0, fake, fake, fake, fake) + tail[:8] + (0, None, fake, 1, None), "step counts from 1")):
        rc, msg = _rc("mpo_optim_step_flat_guarded", *args)
        assert rc == 1 and text in msg, (args, rc, msg)


def test_training_options_without_the_keys_map_as_before():
    o = harness.training_options(dict(TRAINING))
    assert o.max_grad_norm is None and o.skip_nonfinite is False
    assert dataclasses.astuple(o)[:9] == ("ces", 0.5, 0.01, 8, "adamax", 2e-3, 1e-4, 1e-5, 0.9)
    assert [f.name for f in dataclasses.fields(o)] == ["loss", "alpha", "lambda_reg", "grad_acc_step", "optimizer", "lr",
                                                       "weight_decay", "l1", "gamma", "max_grad_norm", "skip_nonfinite"]
    with_keys = harness.training_options(dict(TRAINING, max_grad_norm=2.5, skip_nonfinite=True))
    assert with_keys.max_grad_norm == 2.5 and with_keys.skip_nonfinite is True
    assert dataclasses.astuple(with_keys)[:9] == dataclasses.astuple(o)[:9]
    assert harness.training_options(dict(TRAINING, max_grad_norm=None, skip_nonfinite=False)) == o


def test_train_options_takes_its_nine_fields_positionally():
    o = harness.TrainOptions("sct", 0.75, 0.01, 4, "sgd", 1e-2, 0.0, 0.0, None)
    assert (o.loss, o.grad_acc_step, o.optimizer, o.gamma) == ("sct", 4, "sgd", None)
    assert o.max_grad_norm is None and o.skip_nonfinite is False


def test_the_new_arguments_are_last_and_off_by_default():
    sig = inspect.signature(dp.FlatOptimizer.__init__).parameters
    assert list(sig)[-2:] == ["max_grad_norm", "skip_nonfinite"]
    assert sig["max_grad_norm"].default is None and sig["skip_nonfinite"].default is False
    assert callable(ops.grad_norm_flat) and callable(ops.optim_step_flat_guarded)
    # make_optimizer hands both on; with both off nothing is allocated and state_tensors() is what it was
    params = lambda: [torch.nn.Parameter(torch.ones(8))]
    plain = harness.training_options(dict(TRAINING)).make_optimizer(dp.FlatGradBucket(params()))
    assert plain.grad_ctl is None and plain.max_grad_norm is None and plain.skip_nonfinite is False
    assert [t.data_ptr() for t in plain.state_tensors()] == [t.data_ptr() for t in
                                                             (plain.flat_p, plain.state1, plain.state2, plain.t_dev)]
    opt = harness.training_options(dict(TRAINING, max_grad_norm=2.5, skip_nonfinite=True)).make_optimizer(
        dp.FlatGradBucket(params()))
    assert opt.max_grad_norm == 2.5 and opt.skip_nonfinite is True
    ctl = opt.grad_ctl
    assert ctl.numel() * ctl.element_size() == 16 and opt.state_tensors()[-1] is ctl and len(opt.state_tensors()) == 5
    assert (opt.last_grad_norm.dtype, opt.clip_coef.dtype, opt.skipped_steps.dtype) == (torch.float32, torch.float32, torch.int32)
    assert [t.data_ptr() - ctl.data_ptr() for t in (opt.last_grad_norm, opt.clip_coef, opt.skipped_steps)] == [0, 4, 12]
    assert dp.FlatOptimizer(dp.FlatGradBucket(params()), "sgd", skip_nonfinite=True).grad_ctl is not None
    with pytest.raises(ValueError, match="max_grad_norm"):
        dp.FlatOptimizer(dp.FlatGradBucket(params()), "sgd", max_grad_norm=-1.0)
