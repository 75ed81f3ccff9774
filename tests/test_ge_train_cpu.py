"""The gene-expression model's training options (harness.training_options(cfg, "ge_nacagat");
models/ge_nacagat/main.py:223-263), the binding of its head + `ce` loss entries, and the refusals that need no GPU."""
import ctypes
import inspect

import pytest
import torch

from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import harness, ops
from multimodal_path_omic_amd.models import GeneExprNarrowContextualAttentionGateTransformer

BASE = dict(loss="ce", optimizer="adam", lr=2e-4, weight_decay=1e-5, grad_acc_step=32, scheduler=None, gamma=1.0,
            **{"lambda": 0.0})


def opts(model="ge_nacagat", **kw):
    return harness.training_options({**BASE, **kw}, model)


def test_ce_is_the_one_loss_of_the_gene_expression_model():
    o = opts()
    assert (o.loss, o.optimizer, o.lr, o.weight_decay, o.l1, o.gamma, o.grad_acc_step) == ("ce", "adam", 2e-4, 1e-5, 0.0, None, 32)
    assert harness.LOSSES["ge_nacagat"] == ("ce",)
    for loss in ("ces", "sct", "cesar", "nll", "mse"):
        with pytest.raises(ValueError, match="not implemented"):
            opts(loss=loss)


def test_ce_stays_refused_for_the_fusion_models():
    for model in ("mcat", "nacagat"):
        with pytest.raises(ValueError, match="0D or 1D target tensor expected"):
            opts(model, loss="ce")
    with pytest.raises(ValueError, match="0D or 1D target tensor expected"):
        harness.train_window(None, None, None, None, None, 1, loss="ce")
    with pytest.raises(ValueError, match="no training loop"):
        opts("resnet")


def test_optimiser_penalty_and_schedule_map_like_the_other_mains():
    for name in ("adam", "adamax", "adadelta", "sgd"):
        assert opts(optimizer=name).optimizer == name
    for name in ("rms", None, "Adam"):
        assert opts(optimizer=name).optimizer == "adam"
    assert opts(**{"lambda": None}).l1 == 0.0 and opts(**{"lambda": 0}).l1 == 0.0 and opts(**{"lambda": 1e-4}).l1 == 1e-4
    assert opts(scheduler="exp", gamma=0.8).gamma == 0.8
    for s in (None, "step", "cos"):
        assert opts(scheduler=s, gamma=0.8).gamma is None


def test_head_entries_are_bound_exported_and_additive():
    names = set(L.exported_symbols())
    assert {"mpo_ge_head_loss_forward", "mpo_ge_head_loss_backward"} <= names
    handle = ctypes.CDLL(L.LIB_PATH)
    for n in ("mpo_ge_head_loss_forward", "mpo_ge_head_loss_backward"):
        assert hasattr(handle, n)
    assert L.lib().mpo_abi_version() == 14                    # additive: nothing that existed changed
    assert callable(ops.ge_head_loss) and issubclass(ops.GeHeadLossFn, torch.autograd.Function)
    assert callable(harness.make_ge_window) and callable(harness.train_ge_window)
    sig = inspect.signature(GeneExprNarrowContextualAttentionGateTransformer.forward_window)
    assert list(sig.parameters)[1:] == ["bags", "need_maps", "ce_targets"]
    assert sig.parameters["need_maps"].default is False and sig.parameters["ce_targets"].default is None


@pytest.mark.parametrize("d,c,what", [(192, 3, "d = 192"), (1024, 3, "d = 1024"), (256, 1, "1 classes"), (256, 9, "9 classes")])
def test_head_entries_refuse_a_geometry_they_are_not_built_for(d, c, what):
    """The geometry check sits in front of the launch: on a machine without a GPU the refusal is the message (rc 1)."""
    lib = L.lib()
    one = ctypes.c_void_p(1)                                  # non-null placeholders: the refusal comes before any use
    arr = (ctypes.c_void_p * 2)(1, 1)
    assert lib.mpo_ge_head_loss_forward(one, 4, d, c, arr, one, one, one, None) == 1
    assert what.encode() in lib.mpo_last_error()
    assert lib.mpo_ge_head_loss_backward(one, 4, d, c, arr, one, one, one, arr, None) == 1
    assert what.encode() in lib.mpo_last_error()
    assert lib.mpo_ge_head_loss_forward(None, 4, 256, 3, arr, one, one, one, None) == 1
    assert b"null argument" in lib.mpo_last_error()


def test_forward_window_refuses_bags_of_the_short_token_axis():
    model = GeneExprNarrowContextualAttentionGateTransformer()
    bags = ops.BagBatch(torch.zeros(316, 1024), torch.tensor([0, 300, 316], dtype=torch.int32), [300, 16])
    with pytest.raises(ValueError, match="at least 17 rows"):
        model.forward_window(bags)


def test_graphed_step_refuses_the_split_exchange_for_the_gene_expression_model():
    with pytest.raises(ValueError, match="not for the gene-expression model"):
        harness.GraphedWindowStep(None, None, (None, None), 4, split_patch_grad=True)
