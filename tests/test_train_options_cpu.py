"""The reference's `training:` config -> this package's loss, optimiser, schedule and penalty (harness.training_options;
models/mcat/main.py:272-318, models/nacagat/main.py:283-296), and the new C entries in the binding.  No GPU."""
import pytest

from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import harness

BASE = dict(loss="ces", optimizer="adam", lr=2e-4, weight_decay=1e-5, grad_acc_step=32, scheduler=None, alpha=0.75,
            gamma=1.0, **{"lambda": 0.0})


def opts(model="mcat", **kw):
    return harness.training_options({**BASE, **kw}, model)


def test_default_config_is_todays_step():
    o = opts()
    assert (o.loss, o.alpha, o.optimizer, o.lr, o.weight_decay, o.l1, o.gamma, o.grad_acc_step) == \
        ("ces", 0.75, "adam", 2e-4, 1e-5, 0.0, None, 32)
    assert o.train_kwargs() == dict(loss="ces", alpha=0.75, lambda_reg=0.01, l1=0.0)


def test_losses_and_refusals():
    assert opts(loss="sct").loss == "sct"
    assert opts(loss="ces", alpha=0.5).alpha == 0.5
    o = opts("nacagat", loss="cesar", alpha=0.3)
    assert (o.loss, o.alpha, o.lambda_reg) == ("cesar", 0.75, 0.01)         # the reference ignores the config for cesar
    with pytest.raises(ValueError, match="not implemented"):
        opts(loss="cesar")                                                  # MCAT's main has no cesar branch
    with pytest.raises(ValueError, match="not implemented"):
        opts(loss="nll")
    for model in ("mcat", "nacagat"):
        with pytest.raises(ValueError, match="0D or 1D target tensor expected"):
            opts(model, loss="ce")
    with pytest.raises(ValueError):
        opts("ge_nacagat")


def test_optimisers_penalty_and_schedule():
    for name in ("adam", "adamax", "adadelta", "sgd"):
        assert opts(optimizer=name).optimizer == name
    for name in ("rms", "rmsprop", None, "Adam"):
        assert opts(optimizer=name).optimizer == "adam"
    assert opts(**{"lambda": None}).l1 == 0.0
    assert opts(**{"lambda": 0}).l1 == 0.0
    assert opts(**{"lambda": 1e-4}).l1 == 1e-4
    assert opts(scheduler="exp", gamma=0.8).gamma == 0.8
    for s in (None, "~", "step", "cos"):
        assert opts(scheduler=s, gamma=0.8).gamma is None


def test_train_window_refuses_ce_with_the_reason():
    with pytest.raises(ValueError, match="0D or 1D target tensor expected"):
        harness.train_window(None, None, None, None, None, 1, loss="ce")
    with pytest.raises(ValueError, match="not built"):
        harness.train_window(None, None, None, None, None, 1, loss="nll")


def test_new_entries_are_bound_and_the_abi_is_additive():
    names = set(L.exported_symbols())
    for n in ("mpo_sct_loss_forward", "mpo_sct_loss_backward", "mpo_fusion_head_sct_loss_forward", "mpo_optim_step_flat",
              "mpo_abs_sum_flat", "mpo_abs_sum_flat_workspace_bytes", "mpo_adam_step_flat", "mpo_fusion_head_loss_forward"):
        assert n in names
    assert L.OPTIM == {"adam": 0, "adamax": 1, "adadelta": 2, "sgd": 3}
    from multimodal_path_omic_amd.dp import FlatExponentialLR, FlatOptimizer    # noqa: F401
    from multimodal_path_omic_amd.ops import flat_abs_sum, sct_loss            # noqa: F401
