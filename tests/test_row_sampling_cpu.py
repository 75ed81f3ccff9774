"""CPU-only checks of the row sampler's draw (csrc/bag_sample.h): the library's host entry mpo_bag_sample_indices_host against
the numpy restatement tests/row_sampling_replay.py, the properties a sample without replacement must have, and the entry
points' refusals.  Nothing here launches a kernel."""
import ctypes

import numpy as np
import pytest

import row_sampling_replay as R
from multimodal_path_omic_amd import _lib as L

LENGTHS = [1, 2, 3, 17, 64, 65, 257, 4097, 15000]
SEEDS = [0, 1234567, 0xDEADBEEFCAFEF00D]
OFFSETS = [0, (1 << 33) + 12345]


def host_indices(lengths, k, seed, offset, epoch):
    """(n_slides, k) int32 from the library: row b = pi_b(0 .. k-1), -1 past min(k, M_b)."""
    n = len(lengths)
    ln = (ctypes.c_int32 * n)(*lengths)
    out = (ctypes.c_int32 * (n * k))()
    L.call("mpo_bag_sample_indices_host", ctypes.addressof(ln), n, k, seed, offset, epoch, ctypes.addressof(out))
    return np.ctypeslib.as_array(out).reshape(n, k).copy()


def ks_of(m):
    return sorted({k for k in (1, m - 1, m, m + 5) if k >= 1})


@pytest.mark.parametrize("m", LENGTHS)
def test_host_entry_equals_the_numpy_restatement(m):
    for k in ks_of(m):
        for seed in SEEDS:
            for offset in OFFSETS:
                for epoch in (0, 1):
                    got = host_indices([m] * 6, k, seed, offset, epoch)
                    for slide in (0, 5):
                        want = R.permutation_prefix(seed, offset, epoch, slide, m, k)
                        kb = min(k, m)
                        assert want.shape == (kb,)
                        np.testing.assert_array_equal(got[slide, :kb], want, err_msg=str((m, k, seed, offset, epoch, slide)))
                        assert (got[slide, kb:] == -1).all()
                        # without replacement: distinct rows of the slide; the whole slide when k >= M
                        assert want.min() >= 0 and want.max() < m and len(np.unique(want)) == kb
                        if k >= m:
                            np.testing.assert_array_equal(np.sort(want), np.arange(m))


def test_ragged_window_uses_each_slides_own_length_and_index():
    lengths = [1, 33, 700, 4097, 33]
    got = host_indices(lengths, 32, 7, 3, 2)
    per, flat = R.window_indices(7, 3, 2, lengths, 32)
    for b, m in enumerate(lengths):
        np.testing.assert_array_equal(got[b, :min(32, m)], per[b])
    assert [len(p) for p in per] == [1, 32, 32, 32, 32] and len(flat) == 129
    assert not np.array_equal(per[1], per[4])                  # equal lengths, different slides


def test_slide_epoch_offset_and_seed_all_move_the_draw():
    m, k = 4097, 64
    base = R.permutation_prefix(11, 5, 0, 0, m, k)
    assert not np.array_equal(base, R.permutation_prefix(11, 5, 0, 1, m, k))       # slide
    assert not np.array_equal(base, R.permutation_prefix(11, 5, 1, 0, m, k))       # epoch
    assert not np.array_equal(base, R.permutation_prefix(11, 6, 0, 0, m, k))       # offset
    assert not np.array_equal(base, R.permutation_prefix(11, 5 + (1 << 32), 0, 0, m, k))   # the offset's upper word
    assert not np.array_equal(base, R.permutation_prefix(12, 5, 0, 0, m, k))       # seed
    assert not np.array_equal(base, R.permutation_prefix(11 + (1 << 32), 5, 0, 0, m, k))
    got = host_indices([m, m], k, 11, 5, 0)
    np.testing.assert_array_equal(got[0], base)
    assert not np.array_equal(got[0], got[1])
    # an epoch is 2^40 counters of offset (csrc/mpo_common.h kEpochStride)
    np.testing.assert_array_equal(R.permutation_prefix(11, 5, 3, 0, m, k), R.permutation_prefix(11, 5 + 3 * (1 << 40), 0, 0, m, k))


def test_whole_permutation_and_walk_length():
    """k = M: a bijection at every length tried, and the cycle walk stays short (the Feistel domain is < 4 M)."""
    for m in LENGTHS + [63, 255, 256, 4096, 100000, 1 << 20]:
        perm, walks = R.permutation_prefix(5, 9, 0, 2, m, m, return_walks=True)
        np.testing.assert_array_equal(np.sort(perm), np.arange(m))
        if m > 1:         # no element of the domain is visited twice over the walks of one permutation, and the domain is < 4 M
            assert walks.sum() <= 4 ** ((int(m - 1).bit_length() + 1) // 2) < 4 * m, (m, walks.sum())
    perm = host_indices([100000], 100000, 5, 9, 0)[0]
    np.testing.assert_array_equal(np.sort(perm), np.arange(100000))


def test_inclusion_frequency_is_uniform():
    """M = 64, k = 8 over 4 000 seeds: every row is drawn 500 times in expectation; the count of a row is binomial with
    sigma = sqrt(4000 * 1/8 * 7/8) = 20.9, and every count must lie within 5 sigma (500 +- 105).  A cap, not a measurement:
    numpy's own permutation stays inside it."""
    counts = np.zeros(64, dtype=np.int64)
    got = np.stack([host_indices([64], 8, seed, 0, 0)[0] for seed in range(4000)])
    np.testing.assert_array_equal(got[:50], np.stack([R.permutation_prefix(s, 0, 0, 0, 64, 8) for s in range(50)]))
    np.add.at(counts, got.reshape(-1), 1)
    assert counts.sum() == 32000
    sigma = (4000 * (1 / 8) * (7 / 8)) ** 0.5
    assert np.abs(counts - 500).max() <= 5 * sigma, (counts.min(), counts.max())
    ref = np.zeros(64, dtype=np.int64)
    g = np.random.Generator(np.random.PCG64(1))
    for _ in range(4000):
        np.add.at(ref, g.permutation(64)[:8], 1)
    assert np.abs(ref - 500).max() <= 5 * sigma


def test_sampling_is_the_last_keyword_and_off_by_default():
    import inspect

    from multimodal_path_omic_amd import harness
    for fn in (harness.train_window, harness.train_ge_window, harness.GraphedWindowStep.__init__):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "sample_rows" and last.default is None, fn
    o = harness.training_options(dict(loss="ces", grad_acc_step=4, lr=1e-3), "mcat")
    assert o.train_kwargs() == dict(loss="ces", alpha=0.75, lambda_reg=0.01, l1=0.0)


def _rc(name, *args):
    rc = getattr(L.lib(), name)(*args)
    msg = L.lib().mpo_last_error()
    return rc, (msg.decode() if msg else "")


def test_refusals_come_before_any_launch():
    ln = (ctypes.c_int32 * 2)(5, 5)
    out = (ctypes.c_int32 * 16)()
    a_ln, a_out = ctypes.addressof(ln), ctypes.addressof(out)
    fake = 0x1000                 # never dereferenced: every call below is refused while its arguments are checked
    for args, text in (((a_ln, 2, 0, 1, 0, 0, a_out), "k 0 < 1"),
                       ((a_ln, 0, 4, 1, 0, 0, a_out), "n_slides 0 < 1"),
                       ((None, 2, 4, 1, 0, 0, a_out), "null argument"),
                       ((a_ln, 2, 4, 1, 0, 0, None), "null argument")):
        rc, msg = _rc("mpo_bag_sample_indices_host", *args)
        assert rc == 1 and text in msg, (args, rc, msg)
    bad = (ctypes.c_int32 * 2)(5, 0)
    rc, msg = _rc("mpo_bag_sample_indices_host", ctypes.addressof(bad), 2, 4, 1, 0, 0, a_out)
    assert rc == 1 and "slide 1 has 0 rows" in msg
    for args, text in (((fake, 2, 0, 1024, 2, 1, 0, None, fake, None), "k 0 < 1"),
                       ((fake, 0, 4, 1024, 2, 1, 0, None, fake, None), "n_slides 0 < 1"),
                       ((fake, 2, 4, 1020, 2, 1, 0, None, fake, None), "not a multiple of 16 bytes"),
                       ((fake, 2, 4, 6, 4, 1, 0, None, fake, None), "not a multiple of 16 bytes"),
                       ((fake, 2, 4, 1024, 3, 1, 0, None, fake, None), "element size 3"),
                       ((None, 2, 4, 1024, 2, 1, 0, None, fake, None), "null argument"),
                       ((fake, 2, 4, 1024, 2, 1, 0, None, None, None), "null argument"),
                       ((fake, 2, 4, 1024, 2, 1, 0, None, fake + 8, None), "16-byte aligned"),
                       ((fake, 1 << 20, 1 << 20, 1024, 2, 1, 0, None, fake, None), "32-bit row indices")):
        rc, msg = _rc("mpo_bag_sample_rows", *args)
        assert rc == 1 and text in msg, (args, rc, msg)
    for args, text in (((fake, fake, fake, 2, 0, None), "k 0 < 1"),
                       ((fake, fake, fake, 0, 4, None), "n_slides 0 < 1"),
                       ((None, fake, fake, 2, 4, None), "null argument"),
                       ((fake, None, fake, 2, 4, None), "null argument"),
                       ((fake, fake, None, 2, 4, None), "null argument"),
                       ((fake, fake + 8, fake, 2, 4, None), "16-byte aligned")):
        rc, msg = _rc("mpo_bag_sample_bind", *args)
        assert rc == 1 and text in msg, (args, rc, msg)


def test_new_symbols_are_exported_and_the_abi_version_stays():
    """The four entries are declared in include/mpo_bag_sample.h, which mpo_hip.h includes; the binding reads both."""
    import os
    handle = ctypes.CDLL(L.LIB_PATH)
    names = ["mpo_bag_sample_desc_bytes", "mpo_bag_sample_bind", "mpo_bag_sample_rows", "mpo_bag_sample_indices_host"]
    assert L.companion_symbols() == names
    for name in names:
        assert hasattr(handle, name) and name not in L.exported_symbols(), name
        assert getattr(L.lib(), name).argtypes is not None
    assert L.lib().mpo_bag_sample_rows.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                    ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p]
    with open(L.HEADER_PATH) as f:
        assert '#include "mpo_bag_sample.h"' in f.read()
    assert os.path.dirname(L.COMPANION_HEADER_PATHS[0]) == os.path.dirname(L.HEADER_PATH)
    assert L.lib().mpo_abi_version() == 14 and L.ABI_VERSION == 14
    assert L.lib().mpo_bag_sample_desc_bytes(0) == 0
    for n in (1, 4, 32, 33):
        b = L.lib().mpo_bag_sample_desc_bytes(n)
        assert b >= 8 + 8 * (n + 1) and b % 16 == 0
