"""CPU-only checks of the device-side validation / test epoch (include/mpo_eval.h, harness.cut_eval_windows,
harness.CohortEvaluator's refusals): the header and its exports, the entries' refusals, the window cutter as a pure function
and on a CPU ResidentCohort, and the loss refusals.  Nothing here launches a kernel."""
import ctypes
import os

import pytest
import torch

from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import harness
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.models import (GeneExprNarrowContextualAttentionGateTransformer,
                                             MultimodalCoAttentionTransformer, NarrowContextualAttentionGateTransformer)

HEADER = "mpo_eval.h"
NAMES = ["mpo_concordance_workspace_bytes", "mpo_concordance_tile", "mpo_concordance_index",
         "mpo_map_block_stats_workspace_bytes", "mpo_map_block_stats"]


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
    p, i, i64, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    lib = L.lib()
    assert lib.mpo_concordance_workspace_bytes.argtypes == [i64] and lib.mpo_concordance_workspace_bytes.restype == z
    assert lib.mpo_concordance_tile.argtypes == [] and lib.mpo_concordance_tile.restype == i
    # time, censorship, risk, n, counts, c_index, workspace, workspace_bytes, stream: no tolerance argument
    assert lib.mpo_concordance_index.argtypes == [p, p, p, i64, p, p, p, z, p]
    assert lib.mpo_map_block_stats_workspace_bytes.argtypes == [i, i, i] and lib.mpo_map_block_stats_workspace_bytes.restype == z
    assert lib.mpo_map_block_stats.argtypes == [p, p, i, i, i, p, p, z, p]
    assert lib.mpo_abi_version() == 14 and L.ABI_VERSION == 14


def test_concordance_workspace_is_three_words_per_workgroup_of_a_grid_that_follows_n_alone():
    lib = L.lib()
    t = lib.mpo_concordance_tile()
    assert t >= 64 and t % 64 == 0
    slots = lambda n: lib.mpo_concordance_workspace_bytes(n) // 24
    assert all(lib.mpo_concordance_workspace_bytes(n) % 24 == 0 for n in (1, t, t + 1, 65536))
    # tiles of i x chunks of j (at most 16 chunks): one tile, then tiles^2 up to 16 tiles, then 16 per tile or fewer
    assert [slots(n) for n in (1, t, t + 1, 2 * t + 1, 16 * t)] == [1, 1, 4, 9, 256]
    tiles = -(-65536 // t)
    assert tiles <= slots(65536) <= 16 * tiles
    assert lib.mpo_concordance_workspace_bytes(0) == 0 and lib.mpo_concordance_workspace_bytes(-3) == 0
    assert lib.mpo_concordance_workspace_bytes((1 << 24) + 1) == 0
    # one 16-byte slot per 4096-value chunk of the longest slide, per slide
    assert lib.mpo_map_block_stats_workspace_bytes(3, 6, 1) == 3 * 16
    assert lib.mpo_map_block_stats_workspace_bytes(3, 16, 257) == 3 * 2 * 16
    assert lib.mpo_map_block_stats_workspace_bytes(0, 6, 10) == 0


def _rc(name, *args):
    rc = getattr(L.lib(), name)(*args)
    msg = L.lib().mpo_last_error()
    return rc, (msg.decode() if msg else "")


def test_refusals_come_before_any_launch():
    fake = 0x1000                 # never dereferenced: every call below is refused while its arguments are checked
    need = L.lib().mpo_concordance_workspace_bytes(1000)
    # time, censorship, risk, n, counts, c_index, workspace, workspace_bytes, stream
    for args, text in (((fake, fake, fake, 0, fake, fake, fake, need, None), "n = 0"),
                       ((fake, fake, fake, (1 << 24) + 1, fake, fake, fake, 1 << 30, None), "outside"),
                       ((None, fake, fake, 1000, fake, fake, fake, need, None), "null"),
                       ((fake, fake, fake, 1000, None, fake, fake, need, None), "null"),
                       ((fake + 4, fake, fake, 1000, fake, fake, fake, need, None), "8-byte aligned"),
                       ((fake, fake, fake + 2, 1000, fake, fake, fake, need, None), "4-byte aligned"),
                       ((fake, fake, fake, 1000, fake, fake, None, need, None), "workspace"),
                       ((fake, fake, fake, 1000, fake, fake, fake + 4, need, None), "workspace"),
                       ((fake, fake, fake, 1000, fake, fake, fake, need - 1, None), "workspace")):
        rc, msg = _rc("mpo_concordance_index", *args)
        assert rc == 1 and text in msg, (args, rc, msg)
    need = L.lib().mpo_map_block_stats_workspace_bytes(4, 6, 300)
    # a_map, cu_rows, n_slides, n_q, max_rows, out, workspace, workspace_bytes, stream
    for args, text in (((None, fake, 4, 6, 300, fake, fake, need, None), "bad argument"),
                       ((fake, fake, 0, 6, 300, fake, fake, need, None), "bad argument"),
                       ((fake, fake, 4, 6, 0, fake, fake, need, None), "bad argument"),
                       ((fake, fake, 70000, 6, 300, fake, fake, 1 << 30, None), "out of range"),
                       ((fake, fake, 4, 6, 300, fake, None, need, None), "workspace"),
                       ((fake, fake, 4, 6, 300, fake, fake, need - 1, None), "workspace")):
        rc, msg = _rc("mpo_map_block_stats", *args)
        assert rc == 1 and text in msg, (args, rc, msg)


# ---------------------------------------------------------------------------------------------------- the window cutter
LENGTHS = [10, 20, 30, 40, 50, 60, 70, 80, 90, 100]
SLABS = [0, 0, 0, 0, 1, 1, 1, 2, 2, 2]


def cut(ids, rows=1 << 19, slides=32):
    return harness.cut_eval_windows(ids, LENGTHS, SLABS, rows, slides)


def test_adjacent_runs_merge_and_a_slab_boundary_cuts():
    assert cut(range(10)) == ([[0, 1, 2, 3], [4, 5, 6], [7, 8, 9]], list(range(10)))
    assert cut([2, 3, 4, 5])[0] == [[2, 3], [4, 5]]                      # adjacent ids, two slabs
    assert cut([1, 2, 8, 9, 5])[0] == [[1, 2], [5], [8, 9]]


def test_the_caps_cut_a_run():
    assert cut(range(10), slides=2)[0] == [[0, 1], [2, 3], [4, 5], [6], [7, 8], [9]]
    assert cut(range(10), rows=60)[0] == [[0, 1, 2], [3], [4], [5], [6], [7], [8], [9]]      # 10 + 20 + 30 = 60 fits exactly
    assert cut(range(10), rows=59)[0] == [[0, 1], [2], [3], [4], [5], [6], [7], [8], [9]]
    assert cut([9], rows=1)[0] == [[9]]                                   # a slide longer than the cap is a window of its own
    assert cut(range(10), slides=1)[0] == [[i] for i in range(10)]


def test_scattered_and_reversed_ids_give_runs_of_one_and_the_permutation_restores_the_order():
    ids = [8, 6, 4, 2, 0]
    windows, perm = cut(ids)
    assert windows == [[0], [2], [4], [6], [8]] and perm == [4, 3, 2, 1, 0]
    for ids in ([9, 8, 7, 3, 2, 1], [5, 0, 6, 9, 4, 1], list(range(10))[::-1], [3]):
        windows, perm = cut(ids, slides=2)
        run = [i for w in windows for i in w]
        assert run == sorted(ids) and [run[k] for k in perm] == ids
        assert all(SLABS[w[0]] == SLABS[w[-1]] and w == list(range(w[0], w[-1] + 1)) for w in windows)


@pytest.mark.parametrize("ids, text", [([1, 2, 1], "twice"), ([0, 10], "outside"), ([-1], "outside"), ([], "no slide ids")])
def test_a_duplicate_or_out_of_range_id_raises(ids, text):
    with pytest.raises(ValueError, match=text):
        cut(ids)
    with pytest.raises(ValueError, match="below 1"):
        cut([0], rows=0)


OMIC_SIZES = [8, 12, 16]


def cpu_cohort():
    slides = syn.make_cohort(7, 40, 40, OMIC_SIZES, seed=5)
    for s, m in zip(slides, [40, 17, 33, 40, 9, 25, 40]):
        s["wsi"] = s["wsi"][:m].contiguous()
    return harness.ResidentCohort(slides, "cpu", bag_dtype=torch.float32, slab_bytes=100 * 4096)


def test_resident_cohort_says_where_a_slide_lies():
    cohort = cpu_cohort()                                       # 100-row slabs: [40, 17, 33] [40, 9, 25] [40]
    assert cohort.slab_index == [0, 0, 0, 1, 1, 1, 2] and cohort.row_offset == [0, 40, 57, 0, 40, 49, 0]
    for i in range(cohort.n_slides):
        lo = cohort.row_offset[i]
        view = cohort.slabs[cohort.slab_index[i]][lo:lo + cohort.lengths[i]]
        assert view.data_ptr() == cohort.rows[i].data_ptr() and torch.equal(view, cohort.rows[i])


def test_evaluator_windows_are_views_of_the_slabs():
    cohort = cpu_cohort()
    model = MultimodalCoAttentionTransformer(omic_sizes=OMIC_SIZES)
    ids = [5, 1, 2, 4, 6]
    ev = harness.CohortEvaluator(model, cohort, ids, max_window_slides=2)
    assert [w.ids for w in ev.windows] == [[1, 2], [4, 5], [6]] and ev.perm.tolist() == [3, 0, 1, 2, 4]
    assert [(w.lo, w.hi) for w in ev.windows] == [(0, 2), (2, 4), (4, 5)]
    for w in ev.windows:
        assert w.bags.lengths == [cohort.lengths[i] for i in w.ids]
        assert w.bags.data.data_ptr() == cohort.rows[w.ids[0]].data_ptr()                 # a view: no row was copied
        assert w.bags.data.untyped_storage().data_ptr() == cohort.slabs[cohort.slab_index[w.ids[0]]].untyped_storage().data_ptr()
        assert w.bags.cu.tolist() == [0] + list(torch.tensor(w.bags.lengths).cumsum(0))
        assert torch.equal(w.labels, cohort.labels[w.ids]) and torch.equal(w.cens, cohort.censorship[w.ids])
        assert all(torch.equal(o, x[w.ids]) for o, x in zip(w.omics, cohort.omics))
    assert torch.equal(ev.censorship, cohort.censorship[ids]) and torch.equal(ev.survival_months, cohort.survival_months[ids])
    with pytest.raises(ValueError, match="twice"):
        harness.CohortEvaluator(model, cohort, [1, 2, 1])
    with pytest.raises(ValueError, match="outside"):
        harness.CohortEvaluator(model, cohort, [7])


def test_loss_refusals():
    cohort = cpu_cohort()
    mcat = MultimodalCoAttentionTransformer(omic_sizes=OMIC_SIZES)
    nacagat = NarrowContextualAttentionGateTransformer(omic_sizes=OMIC_SIZES)
    for model in (mcat, nacagat):
        with pytest.raises(ValueError) as e:
            harness.CohortEvaluator(model, cohort, [0, 1], loss="ce")
        assert str(e.value) == harness.CE_REFUSAL
        with pytest.raises(ValueError, match='Loss "nll" not implemented'):
            harness.CohortEvaluator(model, cohort, [0, 1], loss="nll")
    with pytest.raises(ValueError, match='Loss "cesar" not implemented for mcat'):
        harness.CohortEvaluator(mcat, cohort, [0, 1], loss="cesar")                         # LOSSES lists it for NaCAGaT only
    with pytest.raises(ValueError, match="capture=True.*cesar.*map"):
        harness.CohortEvaluator(nacagat, cohort, [0, 1], loss="cesar", capture=True)
    with pytest.raises(ValueError, match="capture=True.*need_maps"):
        harness.CohortEvaluator(nacagat, cohort, [0, 1], capture=True, need_maps=True)
    with pytest.raises(ValueError, match="not a survival model"):
        harness.CohortEvaluator(GeneExprNarrowContextualAttentionGateTransformer(), cohort, [0, 1])
    with pytest.raises(ValueError, match="nothing to replay"):
        harness.validate(mcat, cohort, [0, 1], capture=True)
    harness.CohortEvaluator(nacagat, cohort, [0, 1], loss="cesar")                           # eager: built
    # the host form is what it was
    assert harness.concordance_index_censored([True, True, False], [1.0, 2.0, 3.0], [3.0, 2.0, 1.0]) == 1.0
    with pytest.raises(ValueError, match="GPU"):
        harness.concordance_index_device(torch.zeros(3), torch.ones(3, dtype=torch.float64), torch.zeros(3))


def test_eval_result_reads_the_host_in_one_method_only():
    z = torch.zeros(2)
    r = harness.EvalResult(z, z, z, z, z, z[:1], torch.tensor([0.75], dtype=torch.float64), torch.tensor([3, 0, 4]))
    assert r.c_index_value() == 0.75 and r.maps is None and r.map_stats is None
    empty = harness.EvalResult(z, z, z, z, z, z[:1], torch.tensor([float("nan")], dtype=torch.float64), torch.tensor([0, 0, 0]))
    with pytest.raises(ValueError, match="no comparable pairs"):
        empty.c_index_value()
