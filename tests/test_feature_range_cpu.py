"""CPU-only checks of the device feature scale's entries (include/mpo_feature_range.h, csrc/feature_range.hip, the _dev
forward of csrc/patch_fc_split.hip): the header and its exports, the entry points' refusals, the new Python arguments, and
ops.feature_scale itself, which the device pass must equal bit for bit, pinned on CPU tensors.  Nothing here launches a
kernel."""
import ctypes
import inspect
import math
import os

import pytest
import torch

from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import harness, ops

HEADER = "mpo_feature_range.h"
NAMES = ["mpo_feature_range_workspace_bytes", "mpo_feature_range_f32", "mpo_patch_fc_f32_forward_dev"]


def test_header_is_included_and_its_entries_are_exported_and_bound():
    with open(L.HEADER_PATH) as f:
        assert f'#include "{HEADER}"' in f.read()
    assert HEADER in [os.path.basename(p) for p in L.MORE_HEADER_PATHS]
    assert all(os.path.dirname(p) == os.path.dirname(L.HEADER_PATH) for p in L.MORE_HEADER_PATHS)
    assert L.header_symbols(HEADER) == NAMES
    handle = ctypes.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert hasattr(handle, name), f"{name} declared in include/{HEADER} but not exported"
        assert name not in L.exported_symbols() + L.all_companion_symbols() + L.later_symbols()
    p, i, i64, f, u, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64, ctypes.c_size_t
    lib = L.lib()
    assert lib.mpo_feature_range_workspace_bytes.argtypes == [] and lib.mpo_feature_range_workspace_bytes.restype == z
    assert lib.mpo_feature_range_f32.argtypes == [p, i64, p, p, z, p]
    # the by-value entry keeps its signature; the _dev entry differs in the one argument
    by_value = [p, i64, i, p, p, i, f, u, u, p, f, p, p, z, p]
    assert lib.mpo_patch_fc_f32_forward.argtypes == by_value
    assert lib.mpo_patch_fc_f32_forward_dev.argtypes == by_value[:10] + [p] + by_value[11:]
    assert lib.mpo_abi_version() == 14 and L.ABI_VERSION == 14
    assert 4 <= lib.mpo_feature_range_workspace_bytes() <= 256


def _rc(name, *args):
    rc = getattr(L.lib(), name)(*args)
    msg = L.lib().mpo_last_error()
    return rc, (msg.decode() if msg else "")


def test_refusals_come_before_any_launch():
    fake = 0x1000                 # never dereferenced: every call below is refused while its arguments are checked
    for args, text in (((fake, 8, None, fake, 16, None), "null scale_out"),
                       ((fake, -1, fake, fake, 16, None), "n -1 < 0"),
                       ((None, 8, fake, fake, 16, None), "null x"),
                       ((fake + 4, 8, fake, fake, 16, None), "16-byte aligned"),
                       ((fake, 8, fake, None, 16, None), "workspace"),
                       ((fake, 8, fake, fake + 2, 16, None), "workspace"),
                       ((fake, 8, fake, fake, 2, None), "workspace")):
        rc, msg = _rc("mpo_feature_range_f32", *args)
        assert rc == 1 and text in msg, (args, rc, msg)
    # patches, rows, patch_dim, weight, bias, embed, p, seed, offset, epoch, x_scale (DEVICE), h_bag, workspace, bytes, stream
    for args, text in (((fake, 4, 1024, fake, fake, 256, 0.0, 0, 0, None, None, fake, fake, 1 << 30, None), "null device scale"),
                       ((None, 4, 1024, fake, fake, 256, 0.0, 0, 0, None, fake, fake, fake, 1 << 30, None), "null operand"),
                       ((fake, 0, 1024, fake, fake, 256, 0.0, 0, 0, None, fake, fake, fake, 1 << 30, None), "total_rows 0"),
                       ((fake, 4, 1024, fake, fake, 256, 0.0, 0, 0, None, fake, fake, fake, 64, None), "workspace too small"),
                       ((fake, 4, 512, fake, fake, 256, 0.0, 0, 0, None, fake, fake, fake, 1 << 30, None), "built for 1024 -> 256"),
                       ((fake, 4, 1024, fake, fake, 256, 1.0, 0, 0, None, fake, fake, fake, 1 << 30, None), "dropout p")):
        rc, msg = _rc("mpo_patch_fc_f32_forward_dev", *args)
        assert rc == 1 and text in msg, (args, rc, msg)
    # the by-value entry still looks at its scale
    rc, msg = _rc("mpo_patch_fc_f32_forward", fake, 4, 1024, fake, fake, 256, 0.0, 0, 0, None, 3.0, fake, fake, 1 << 30, None)
    assert rc == 1 and "power of two" in msg


def test_feature_scale_on_cpu_tensors_is_unchanged():
    """What the device pass is held to, on the host: 2^(15 - e) for max |x| = m 2^e, the exponent clamped to +-100; 1.0 for an
    all-zero, empty or non-finite matrix."""
    assert ops.feature_scale(torch.zeros(3, 8)) == 1.0
    assert ops.feature_scale(torch.empty(0, 1024)) == 1.0
    for top, want in ((1.0, 2.0 ** 14), (0.75, 2.0 ** 15), (-3.0, 2.0 ** 13), (32767.0, 1.0), (32768.0, 0.5), (3e-4, 2.0 ** 26),
                      (1e4, 2.0), (1e37, 2.0 ** -100), (3e38, 2.0 ** -100), (1e-30, 2.0 ** 100), (1e-45, 2.0 ** 100)):
        x = torch.full((2, 4), 0.25 * top)
        x[1, 2] = top
        assert ops.feature_scale(x) == want, (top, ops.feature_scale(x), want)
        m = float(x.abs().max())
        if 2.0 ** -85 < m < 2.0 ** 100:
            assert 2.0 ** 14 <= m * ops.feature_scale(x) < 2.0 ** 15
    for bad in (float("inf"), float("-inf"), float("nan")):
        x = torch.randn(5, 8)
        x[3, 1] = bad
        assert ops.feature_scale(x) == 1.0
    x = torch.randn(4, 4)
    first = ops.feature_scale(x)
    x.mul_(1024)
    assert ops.feature_scale(x) == first / 1024 and math.frexp(first)[0] == 0.5        # the host cache follows an in-place write


def test_the_new_arguments_are_public_and_off_by_default():
    sig = inspect.signature(ops.RowSampler.__init__).parameters
    assert sig["device_feature_scale"].default is False and list(sig)[-1] == "source"
    sig = inspect.signature(harness.GraphedWindowStep.__init__).parameters
    assert sig["device_feature_scale"].default is False
    assert list(inspect.signature(ops.feature_scale_device).parameters) == ["x", "out"]
    with pytest.raises(ValueError, match="fp32 tensor on the GPU"):
        ops.feature_scale_device(torch.zeros(2, 4))
