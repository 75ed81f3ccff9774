"""K2's key routes (ops._key_route, ops._key_finish): which of the four ways K = H W_k^T + b_k is formed and differentiated
for every (bag dtype, embed_dim, bag_relu_gate), the two refusals, and what ops.k2_fused_patch_grad changes.  No GPU."""
import pytest
import torch

from multimodal_path_omic_amd import ops

F32, BF16 = torch.float32, torch.bfloat16
GATE = 4.0 / 3.0
NEEDS_BF16 = "bag_relu_gate (fused ReLU/dropout derivative of the patch layer) needs a bf16-stored bag"
NO_GATE_AT_512 = "embed_dim 512: the fused ReLU/dropout gate of the patch layer is built for embed_dim <= 256"
# (bag dtype, E, gate) -> (route, its finish) | the ValueError's text
TABLE = {
    (F32, 128, 0.0): ("gemm_f32", "gemm"), (F32, 128, GATE): NEEDS_BF16,
    (F32, 256, 0.0): ("gemm_f32", "gemm"), (F32, 256, GATE): NEEDS_BF16,
    (F32, 512, 0.0): ("halves", "gemm"), (F32, 512, GATE): NEEDS_BF16,
    (BF16, 128, 0.0): ("gemm_bf16", "one_pass"), (BF16, 128, GATE): ("gemm_bf16", "one_pass"),
    (BF16, 256, 0.0): ("kernel", "fused"), (BF16, 256, GATE): ("kernel", "fused"),
    (BF16, 512, 0.0): ("halves", "gemm"), (BF16, 512, GATE): NO_GATE_AT_512,
}


@pytest.mark.parametrize("dtype,E,gate", list(TABLE), ids=lambda v: str(v).replace("torch.", ""))
def test_route_table(dtype, E, gate):
    want = TABLE[(dtype, E, gate)]
    assert ops.k2_fused_patch_grad is True
    if isinstance(want, str):
        with pytest.raises(ValueError) as e:
            ops._key_route(dtype, E, gate)
        assert str(e.value) == want
    else:
        route = ops._key_route(dtype, E, gate)
        assert (route, ops._key_finish(route)) == want


def test_unfused_patch_grad_changes_only_the_finish_of_the_bf16_256_route(monkeypatch):
    monkeypatch.setattr(ops, "k2_fused_patch_grad", False)
    for key, want in TABLE.items():
        if isinstance(want, str):
            with pytest.raises(ValueError) as e:
                ops._key_route(*key)
            assert str(e.value) == want
            continue
        route = ops._key_route(*key)
        assert route == want[0]                                      # the route, and with it the projection, is the same
        if route == "kernel":
            assert ops._key_finish(route) == "one_pass" == ops._key_finish("gemm_bf16")
        else:
            assert ops._key_finish(route) == want[1]
