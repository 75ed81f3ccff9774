"""The bag-side C entries held to their buffers (tests/buffer_contract.py has the contract, the case table and the
placement helper): exact `saved` / `workspace` / output sizes between NaN guards, two runs under a NaN and a finite
pre-fill, every guard and input bit-unchanged, every output finite, within the entry's own bar against fp64 and bit-equal
between the two runs.

Measured on an MI355X: the file's 122 tests take 6.4 s, the slowest case 0.36 s (the 8300-row window at embed 512); the worst
error over the cases of an entry next to its bar is in NOTES.md ("Bag-side C entries held to their buffers")."""
import pytest
import torch

import buffer_contract as B
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", B.CASES, ids=[c.id for c in B.CASES])
def test_entry_keeps_to_its_buffers(dev, case):
    B.run_case(dev, case)


def test_selectors_are_back_at_their_defaults(dev):
    """Knobs restores every selector, also after a failing case: each still reports its default (1)."""
    lib = L.lib()
    for name in ("mpo_set_coattn_bwd_two_wave", "mpo_set_coattn_bwd_f32_vector", "mpo_set_nacagat_one_pass_key_grad"):
        prev = getattr(lib, name)(1)
        assert prev == 1, name


def _control(dev, saved_short):
    lengths, E, n_q = B.W_EDGES, 256, 6
    i, _ = B._mcat_problem(lengths, B.F32, E, n_q, False, 0.0, 0)
    A, t = B.mcat_place(dev, B.NAN, i, lengths, B.F32, E, n_q, amap=False, d_amap=False, colsum=False, acc=0, saved_short=saved_short)
    cu = ops.make_cu(lengths, dev)
    B.mcat_forward_call(A, t, lengths, B.F32, E, n_q, None, cu)
    return A


def test_control_a_saved_view_one_block_short_trips_the_guard(dev):
    """The instrument, without touching a kernel: the MCAT forward on a `saved` view that ends one block (lse2, R = 18 floats)
    before the size the query states, inside the same guarded allocation.  The entry has no length for `saved`, so it writes
    its last block into the 64-float guard behind the view -- never outside the allocation -- and the checker must say so.
    With the full view the same call passes."""
    R = len(B.W_EDGES) * 6
    assert R <= B.guard_elements((1,), torch.float32)
    _control(dev, 0).check("control, full view")
    A = _control(dev, R)
    with pytest.raises(AssertionError, match="guard behind saved"):
        A.check("control, short view")


def test_worst_errors_per_entry(dev):
    """Prints the worst error per quantity next to its bar over the cases that ran (pytest -rA; quoted in NOTES.md)."""
    for runner, worst in B.WORST.items():
        for name, (err, bar) in worst.items():
            print(f"[buffer contract] worst {runner}: {name} {err:.3e} (bar {bar:.3e})")
