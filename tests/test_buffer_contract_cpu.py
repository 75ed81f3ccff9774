"""The ledger of the buffer contract (tests/buffer_contract.py), without a GPU: every C entry that takes a pointer to
non-const data is a case of the table, or held by an existing test that places its buffers between guards, or on the
`not_held` list -- which is compared with the literal list below, so it cannot grow silently.  A new entry in a header
without a line in the table fails here.  Also: the table covers the values the contract names, per storage type."""
import glob
import os
import re

import torch

import buffer_contract as B
from multimodal_path_omic_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NOT_HELD = [
    "mpo_abs_sum_flat", "mpo_adam_step_flat", "mpo_bag_sample_bind", "mpo_bag_sample_bind_slides", "mpo_bag_sample_indices_host",
    "mpo_bag_sample_rows", "mpo_bag_sample_slides", "mpo_cag_backward", "mpo_cag_forward", "mpo_ces_loss_backward", "mpo_ces_loss_forward",
    "mpo_class_metrics", "mpo_coattn_bwd_bagpass", "mpo_coattn_fwd_bagpass", "mpo_concordance_index", "mpo_feature_range_f32",
    "mpo_fusion_head_backward", "mpo_fusion_head_forward", "mpo_fusion_head_loss_backward", "mpo_fusion_head_loss_forward",
    "mpo_fusion_head_sct_loss_forward", "mpo_ge_head_loss_backward", "mpo_ge_head_loss_forward", "mpo_grad_norm_flat", "mpo_nacagat_fwd_bagpass",
    "mpo_omic_snn_backward", "mpo_omic_snn_forward", "mpo_optim_step_flat", "mpo_optim_step_flat_guarded", "mpo_pack_patch_weight",
    "mpo_patch_coattn_fwd_bagpass", "mpo_patch_epilogue_forward", "mpo_sct_loss_backward", "mpo_sct_loss_forward", "mpo_step_counters_bump",
    "mpo_survival_head_backward", "mpo_survival_head_forward",
]


def _headers():
    return sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))


def _entries():
    names = []
    for path in _headers():
        with open(path) as f:
            text = f.read()
        declared, _, _ = L.parse_header(text)
        found = B.entries_with_outputs(text)
        assert set(found) <= set(declared), path
        names += found
    return names


def test_every_header_is_one_the_package_binds():
    bound = {L.HEADER_PATH, *L.COMPANION_HEADER_PATHS, *L.LATER_HEADER_PATHS, *L.MORE_HEADER_PATHS}
    assert {os.path.realpath(p) for p in _headers()} == {os.path.realpath(p) for p in bound}


def test_pointer_constness_is_read_as_the_header_spells_it():
    text = """int mpo_a(const float* x, float* y, int n);
              int mpo_b(const float* x, const void* w, const float* const* params, int n);
              int mpo_c(const float* x, float* const* grads);
              size_t mpo_d(int n);  /* float* in a comment */
              int mpo_e(void* workspace, size_t bytes);"""
    assert B.entries_with_outputs(text) == ["mpo_a", "mpo_c", "mpo_e"]


def test_every_entry_with_an_output_pointer_is_in_the_ledger():
    entries = _entries()
    assert len(entries) == len(set(entries)) and len(entries) >= 72
    cased = {e for c in B.CASES for e in c.entries}
    for group, other in ((cased, set(B.HELD_BY)), (cased, set(B.NOT_HELD)), (set(B.HELD_BY), set(B.NOT_HELD))):
        assert not group & other, sorted(group & other)
    ledger = cased | set(B.HELD_BY) | set(B.NOT_HELD)
    assert not set(entries) - ledger, f"entries without a line in tests/buffer_contract.py: {sorted(set(entries) - ledger)}"
    assert not ledger - set(entries), f"ledger lines for entries no header declares: {sorted(ledger - set(entries))}"


def test_held_by_names_an_existing_test_in_a_file_that_guards_its_buffers():
    for entry, where in B.HELD_BY.items():
        path, _, test = where.partition("::")
        assert path.startswith("tests/") and test.startswith("test_"), (entry, where)
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        assert re.search(rf"^def {re.escape(test)}\(", text, re.M), (entry, where)
        assert any(word in text for word in B.GUARD_WORDS), (entry, path)


def test_not_held_is_the_list_this_file_states():
    print("not held by the buffer contract yet:")
    for name in sorted(B.NOT_HELD):
        print(f"  {name}: {B.NOT_HELD[name]}")
    assert sorted(B.NOT_HELD) == NOT_HELD
    assert all(reason.strip() for reason in B.NOT_HELD.values())


def test_case_ids_are_unique_and_runners_exist():
    ids = [c.id for c in B.CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    for c in B.CASES:
        assert c.runner in B.RUNNERS and c.entries, c.id
        if c.atomic is not None:                      # the exception names a line that holds an atomicAdd
            path, _, line = c.atomic.partition(":")
            with open(os.path.join(ROOT, path)) as f:
                assert "atomicAdd" in f.read().splitlines()[int(line) - 1], c.atomic


def test_atomic_adds_are_where_the_table_assumes():
    """Bit-equality is asserted for every case but the ones that name an atomic: atomicAdd occurs in three files only, and of
    those only patch_epilogue.hip's column sum is reached by a case (the co-attention entries' GEMMs have R = n_slides * n_q
    <= 48 rows, far below the long-K body's 2048; tail.hip serves the token tail)."""
    found = set()
    for path in glob.glob(os.path.join(ROOT, "multimodal_path_omic_amd", "csrc", "*.h*")):
        with open(path) as f:
            if "atomicAdd" in f.read():
                found.add(os.path.basename(path))
    assert found == {"gemm_f32_longk.hip", "patch_epilogue.hip", "tail.hip"}
    assert max(len(c.kw["lengths"]) * c.kw["n_q"] for c in B.CASES if c.runner in ("mcat", "nacagat", "patch_coattn")) <= 48


def _values(runner, key, **where):
    return {c.kw.get(key) for c in B.CASES if c.runner == runner and all(c.kw.get(k) == v for k, v in where.items())}


def test_the_table_covers_what_the_contract_names():
    windows = {B.W_EDGES, B.W_ONE, B.W_LONG, B.W_MAX}
    for dtype in (B.F32, B.BF16):
        for runner, n_qs in (("mcat", {1, 6, 16}), ("nacagat", {1, 6, 7, 16})):
            assert _values(runner, "lengths", dtype=dtype) == windows
            assert _values(runner, "E", dtype=dtype) == {128, 256, 512}
            assert _values(runner, "n_q", dtype=dtype) >= n_qs
            assert _values(runner, "plan", dtype=dtype) == {"uniform", "built", "max"}
            assert _values(runner, "acc", dtype=dtype) >= {0, 1}
            assert _values(runner, "d_amap", dtype=dtype) == {False, True}
            for E in (128, 256, 512):
                assert len(_values(runner, "lengths", dtype=dtype, E=E)) == 4
        assert _values("mcat", "amap", dtype=dtype) == {False, True}
        assert _values("mcat", "colsum", dtype=dtype) == {False, True}
        assert _values("nacagat", "drop_p", dtype=dtype) == {0.0, 0.25}
        assert _values("nacagat", "colsum", dtype=dtype) == {None, "given", "alias"}
        assert _values("nacagat", "ctx_out", dtype=dtype) == {False, True}
        assert _values("nacagat", "d_qproj", dtype=dtype) == {False, True}
        assert _values("nacagat", "one_pass", dtype=dtype, n_q=6) == {0, 1} and _values("nacagat", "one_pass", dtype=dtype, n_q=7) == {0, 1}
    assert _values("mcat", "gate", dtype=B.BF16) == {0.0, 4.0 / 3.0} and _values("mcat", "gate", dtype=B.F32) == {0.0}
    assert _values("mcat", "kernel", dtype=B.F32) == {"general", "f32_vector"}
    assert _values("mcat", "kernel", dtype=B.BF16) == {"general", "two_wave"}
    assert _values("nacagat", "dk_dtype", dtype=B.BF16) == {B.F32, B.BF16} and _values("nacagat", "dk_dtype", dtype=B.F32) == {B.F32}
    assert _values("nacagat", "colsum", E=512) >= {"given", "alias"}                 # the column halves write side by side
    assert _values("patch_coattn", "n_q") >= {1, 6, 8} and _values("patch_coattn", "drop_p") == {0.0, 0.25}
    assert {(c.kw["E"], c.kw["pd"]) for c in B.CASES if c.runner == "patch_fc"} == {(e, p) for e in (128, 256, 512) for p in (512, 1024, 2048)}
    for storage in (B.F32, B.F16):
        assert _values("patch_f32", "rows", storage=storage) == {1, 33, 257}
        assert _values("patch_f32", "h_given", storage=storage) == {False, True}
    assert _values("patch_f32", "scale_on_device", storage=B.F32) == {None, True}


def test_the_largest_plan_is_the_most_check_plan_accepts():
    """rows_per_wg = 32 over [1, 33, 8180]: 1 + 2 + 256 workgroups = target + n_slides, the bound in csrc/capi.hip's check_plan
    and the `parts` every *_workspace_bytes query sizes for; [1, 33, 8300] would need 263."""
    target = 256
    assert B.max_plan_starts(B.W_MAX, target) == [0, 1, 3, 259]
    assert sum(-(-m // 32) for m in B.W_LONG) == 263 > target + len(B.W_LONG)
    assert sum(-(-m // 32) for m in B.W_LONG) >= target + len(B.W_LONG)          # "at least target + n_slides tiles of 32 rows"


def test_guards_keep_the_alignment_and_the_two_tiles():
    for dtype in (B.F32, B.BF16, B.F16):
        elt = torch.empty((), dtype=dtype).element_size()
        for shape in ((700, 128), (734, 512), (18, 256), (2 * 734, 256), (33, 2048)):
            g = B.guard_elements(shape, dtype)
            assert g >= 64 * shape[1] and (g * elt) % 16 == 0
        for n in (1, 3, 18, 4404):
            g = B.guard_elements((n,), dtype)
            assert g >= 64 and (g * elt) % 16 == 0
