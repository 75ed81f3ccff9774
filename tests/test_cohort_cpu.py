"""CPU-only checks of the resident-cohort sampler's entries (include/mpo_cohort.h, csrc/bag_sample.hip): the header and
its exports, the descriptor size, the entry points' refusals, and the lapped indices restated on the host.  Nothing here
launches a kernel."""
import ctypes
import os

import numpy as np

import row_sampling_replay as R
from multimodal_path_omic_amd import _lib as L

NAMES = ["mpo_bag_sample_slides_desc_bytes", "mpo_bag_sample_bind_slides", "mpo_bag_sample_slides"]


def lapped_indices(seed, offset, epoch, slide, m, k):
    """Source rows of a slide of m rows under `cycle`: pi(j mod m), i.e. the prefix pi(0 .. min(k, m) - 1) tiled to k."""
    prefix = R.permutation_prefix(seed, offset, epoch, slide, m, k)
    return np.resize(prefix, k)


def test_header_is_included_and_its_entries_are_exported_and_bound():
    with open(L.HEADER_PATH) as f:
        assert '#include "mpo_cohort.h"' in f.read()
    assert [os.path.basename(p) for p in L.LATER_HEADER_PATHS] == ["mpo_cohort.h"]
    assert os.path.dirname(L.LATER_HEADER_PATHS[0]) == os.path.dirname(L.HEADER_PATH)
    assert L.later_symbols() == NAMES and L.later_symbols("mpo_cohort.h") == NAMES
    handle = ctypes.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert hasattr(handle, name), name
        assert name not in L.exported_symbols() and name not in L.companion_symbols() and name not in L.all_companion_symbols()
        assert getattr(L.lib(), name).argtypes is not None
    p, i, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    assert L.lib().mpo_bag_sample_slides_desc_bytes.argtypes == [i] and L.lib().mpo_bag_sample_slides_desc_bytes.restype == ctypes.c_size_t
    assert L.lib().mpo_bag_sample_bind_slides.argtypes == [p, p, p, i, p, i, i, i, p]
    assert L.lib().mpo_bag_sample_slides.argtypes == L.lib().mpo_bag_sample_rows.argtypes == [p, i, i, i, i, u, u, p, p, p]
    assert L.lib().mpo_abi_version() == 14 and L.ABI_VERSION == 14


def test_a_name_declared_twice_is_rejected_across_the_header_lists(tmp_path):
    dup = tmp_path / "dup.h"
    dup.write_text("int mpo_bag_sample_rows(int n);\n")
    taken = {name: None for name in L.exported_symbols() + L.all_companion_symbols()}
    try:
        L._read_companions([str(dup)], taken)
    except RuntimeError as e:
        assert "mpo_bag_sample_rows is declared twice" in str(e)
    else:
        raise AssertionError("a duplicate declaration was accepted")


def test_descriptor_size():
    f = L.lib().mpo_bag_sample_slides_desc_bytes
    assert f(0) == 0 and f(-3) == 0
    for n in (1, 4, 32, 33):
        assert f(n) % 16 == 0 and f(n) >= 16 * n + 4, (n, f(n))
        assert f(n) < 16 * n + 4 + 16


def _rc(name, *args):
    rc = getattr(L.lib(), name)(*args)
    msg = L.lib().mpo_last_error()
    return rc, (msg.decode() if msg else "")


def test_refusals_come_before_any_launch():
    fake = 0x1000                 # never dereferenced: every call below is refused while its arguments are checked
    for args, text in (((fake, 2, 0, 1024, 2, 1, 0, None, fake, None), "k 0 < 1"),
                       ((fake, 0, 4, 1024, 2, 1, 0, None, fake, None), "n_slides 0 < 1"),
                       ((fake, 2, 4, 1020, 2, 1, 0, None, fake, None), "not a multiple of 16 bytes"),
                       ((fake, 2, 4, 6, 4, 1, 0, None, fake, None), "not a multiple of 16 bytes"),
                       ((fake, 2, 4, 1024, 3, 1, 0, None, fake, None), "element size 3"),
                       ((None, 2, 4, 1024, 2, 1, 0, None, fake, None), "null argument"),
                       ((fake, 2, 4, 1024, 2, 1, 0, None, None, None), "null argument"),
                       ((fake, 2, 4, 1024, 2, 1, 0, None, fake + 8, None), "16-byte aligned"),
                       ((fake, 1 << 20, 1 << 20, 1024, 2, 1, 0, None, fake, None), "32-bit row indices")):
        rc, msg = _rc("mpo_bag_sample_slides", *args)
        assert rc == 1 and text in msg, (args, rc, msg)
    # desc, table_ptrs, table_lens, n_table, ids, n_slides, k, cycle, stream
    for args, text in (((fake, fake, fake, 7, fake, 2, 0, 0, None), "k 0 < 1"),
                       ((fake, fake, fake, 7, fake, 0, 4, 0, None), "n_slides 0 < 1"),
                       ((fake, fake, fake, 0, fake, 2, 4, 1, None), "n_table 0 < 1"),
                       ((None, fake, fake, 7, fake, 2, 4, 0, None), "null argument"),
                       ((fake, None, fake, 7, fake, 2, 4, 0, None), "null argument"),
                       ((fake, fake, None, 7, fake, 2, 4, 0, None), "null argument"),
                       ((fake, fake, fake, 7, None, 2, 4, 1, None), "null argument"),
                       ((fake + 4, fake, fake, 7, fake, 2, 4, 0, None), "8-byte aligned"),
                       ((fake, fake, fake, 7, fake, 1 << 20, 1 << 20, 1, None), "32-bit row indices")):
        rc, msg = _rc("mpo_bag_sample_bind_slides", *args)
        assert rc == 1 and text in msg, (args, rc, msg)


def test_lapped_indices_restated_on_the_host():
    """Under `cycle` output row j of a slide of M < k rows is pi(j mod M): the prefix the host entry gives, tiled."""
    for seed, offset, epoch, slide in ((7, 3, 0, 0), (0xDEADBEEFCAFEF00D, (1 << 33) + 5, 2, 3)):
        idx = lapped_indices(seed, offset, epoch, slide, 16, 64)
        assert idx.shape == (64,)
        np.testing.assert_array_equal(np.bincount(idx, minlength=16), np.full(16, 4))     # every row exactly 4 times
        np.testing.assert_array_equal(idx[:16], idx[16:32])                               # lap after lap, the same order
        idx = lapped_indices(seed, offset, epoch, slide, 33, 64)
        counts = np.bincount(idx, minlength=33)
        assert set(counts.tolist()) == {1, 2} and counts.sum() == 64
        np.testing.assert_array_equal(np.sort(idx[:33]), np.arange(33))                   # a whole lap before any row repeats
        np.testing.assert_array_equal(idx[33:], idx[:31])
        np.testing.assert_array_equal(lapped_indices(seed, offset, epoch, slide, 1, 5), np.zeros(5, dtype=np.int64))
        # a slide of at least k rows is not lapped: the sample without replacement
        np.testing.assert_array_equal(lapped_indices(seed, offset, epoch, slide, 700, 64),
                                      R.permutation_prefix(seed, offset, epoch, slide, 700, 64))


def test_window_types_and_the_epoch_loop_are_public():
    import inspect

    from multimodal_path_omic_amd import harness, ops
    assert [f.name for f in ops.SlideSet.__dataclass_fields__.values()] == ["slides", "lengths", "table_ptrs", "table_lens", "ids", "cycle"]
    assert callable(ops.SlideSet.from_batch) and callable(ops.SlideSet.materialize)
    assert list(inspect.signature(ops.RowSampler.__init__).parameters)[-1] == "source"
    assert inspect.signature(ops.RowSampler.__init__).parameters["source"].default == "window"
    sig = inspect.signature(harness.ResidentCohort.__init__).parameters
    assert list(sig)[1:5] == ["slides", "device", "bag_dtype", "cycle"] and sig["cycle"].default is False
    assert list(inspect.signature(harness.train_epoch).parameters) == ["step", "cohort", "order"]
