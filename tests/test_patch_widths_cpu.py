"""The constructor argument `patch_dim` (patch feature width 512 / 1024 / 2048) on the host side: the default leaves every
state_dict as it was, the two other widths change the patch layer's weight alone, anything else is refused at construction,
and the synthetic cohort follows the argument.  No GPU, no library call."""
import pytest
import torch

from multimodal_path_omic_amd import ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.models import (MODEL_SIZES, GeneExprNarrowContextualAttentionGateTransformer,
                                             MultimodalCoAttentionTransformer, NarrowContextualAttentionGateTransformer)

SIZES = [64, 100, 31]
MODELS = {
    "mcat": lambda **kw: MultimodalCoAttentionTransformer(omic_sizes=SIZES, **kw),
    "nacagat": lambda **kw: NarrowContextualAttentionGateTransformer(omic_sizes=SIZES, **kw),
    "ge": lambda **kw: GeneExprNarrowContextualAttentionGateTransformer(**kw),
}


def _shapes(model):
    return [(k, tuple(v.shape)) for k, v in model.state_dict().items()]


@pytest.mark.parametrize("kind", sorted(MODELS))
def test_default_width_leaves_the_state_dict_as_it_was(kind):
    plain, named = MODELS[kind](), MODELS[kind](patch_dim=1024)
    assert _shapes(plain) == _shapes(named)                      # same keys, same order, same shapes
    assert dict(_shapes(plain))["H.0.weight"] == (256, 1024)
    assert plain.patch_dim == named.patch_dim == 1024


def test_patch_dim_is_the_last_positional_argument():
    """It follows bag_dtype: every positional call written for the reference's signature means what it meant."""
    m = MultimodalCoAttentionTransformer(SIZES, "medium", 4, 0.25, "concat", "cpu", torch.bfloat16, 512)
    assert m.bag_dtype == torch.bfloat16 and m.H[0].in_features == 512
    m = NarrowContextualAttentionGateTransformer(SIZES, "medium", 4, 0.25, "concat", "cpu", torch.bfloat16, 2048)
    assert m.bag_dtype == torch.bfloat16 and m.H[0].in_features == 2048
    m = GeneExprNarrowContextualAttentionGateTransformer("medium", 3, 0.25, torch.bfloat16, 512)
    assert m.bag_dtype == torch.bfloat16 and m.H[0].in_features == 512


@pytest.mark.parametrize("size", sorted(MODEL_SIZES))
@pytest.mark.parametrize("width", [512, 2048])
@pytest.mark.parametrize("kind", sorted(MODELS))
def test_other_widths_change_the_patch_weight_alone(kind, width, size):
    d0 = MODEL_SIZES[size][0]
    ref, got = dict(_shapes(MODELS[kind](model_size=size))), dict(_shapes(MODELS[kind](model_size=size, patch_dim=width)))
    assert got["H.0.weight"] == (d0, width)
    assert list(got) == list(ref)
    assert {k for k in ref if ref[k] != got[k]} == {"H.0.weight"}


@pytest.mark.parametrize("width", [768, 1280, 1536, 0, 1000])
@pytest.mark.parametrize("kind", sorted(MODELS))
def test_construction_refuses_widths_outside_the_set(kind, width):
    with pytest.raises(ValueError, match=r"patch_dim.*512.*1024.*2048"):
        MODELS[kind](patch_dim=width)


def test_the_kernel_gate_follows_the_set():
    assert ops.PATCH_DIMS == (512, 1024, 2048)
    for k in (512, 1024, 2048):
        for e in (128, 256, 512):
            assert ops.patch_fc_kernel_supported(torch.empty(4, k, dtype=torch.bfloat16), torch.empty(e, k))
    x = torch.empty(4, 1024, dtype=torch.bfloat16)
    assert not ops.patch_fc_kernel_supported(x, torch.empty(256, 512))                # the window is not the weight's width
    assert not ops.patch_fc_kernel_supported(torch.empty(4, 768, dtype=torch.bfloat16), torch.empty(256, 768))
    assert not ops.patch_fc_kernel_supported(torch.empty(4, 512), torch.empty(256, 512))                 # fp32 window
    assert not ops.fused_patch_coattn_supported(torch.empty(4, 512, dtype=torch.bfloat16), 256, 6)      # one-call form: 1024 only


def test_cohort_follows_patch_dim():
    slides = syn.make_cohort(3, 20, 40, SIZES, 7, patch_dim=512)
    assert all(s["wsi"].shape == (s["wsi"].shape[0], 512) and 20 <= s["wsi"].shape[0] <= 40 for s in slides)
    assert all([o.shape for o in s["omics"]] == [(n,) for n in SIZES] for s in slides)
    assert all(s["survival_class"] in range(4) for s in slides)
    # the default is the reference's width, and the draw of the default has not moved
    a, b = syn.make_cohort(2, 20, 40, SIZES, 7), syn.make_cohort(2, 20, 40, SIZES, 7, patch_dim=1024)
    assert a[0]["wsi"].shape[1] == 1024 and all(torch.equal(x["wsi"], y["wsi"]) for x, y in zip(a, b))
