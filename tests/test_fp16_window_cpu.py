"""CPU-only checks of the fp16 window (include/mpo_patch_f16.h, csrc/patch_fc_split.hip): the header and its exports, the
entries' refusals before any launch, the compiler's resource rows of the two new kernels and of the fp32 window's kernels
beside them (those must not have moved), and what fp16 storage of the patch matrix costs by the oracle at the benchmarked
bag length -- the reason the storage mode exists.  Nothing here launches a kernel."""
import ctypes
import importlib
import os

import pytest
import torch

import cases as C
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import ops
from multimodal_path_omic_amd import synthetic as syn
from oracle import mpo_oracle as O

HEADER = "mpo_patch_f16.h"
NAMES = ["mpo_patch_fc_f16_workspace_bytes", "mpo_patch_fc_f16_forward", "mpo_patch_fc_f16_backward"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    p, i, i64, u64, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_size_t
    lib = L.lib()
    assert lib.mpo_patch_fc_f16_workspace_bytes.argtypes == [i] and lib.mpo_patch_fc_f16_workspace_bytes.restype == z
    # the fp32 entries' parameters without the feature scale; the rate as round(256 p), one integer both ways
    f32_fwd, f32_bwd = lib.mpo_patch_fc_f32_forward.argtypes, lib.mpo_patch_fc_f32_backward.argtypes
    assert lib.mpo_patch_fc_f16_forward.argtypes == [p, i64, i, p, p, i, i, u64, u64, p, p, p, z, p]
    assert lib.mpo_patch_fc_f16_forward.argtypes == f32_fwd[:6] + [i] + f32_fwd[7:10] + f32_fwd[11:]
    assert lib.mpo_patch_fc_f16_backward.argtypes == f32_bwd[:6] + [i] + f32_bwd[7:]
    assert lib.mpo_abi_version() == 14 and L.ABI_VERSION == 14
    for b in (0, 1):
        assert lib.mpo_patch_fc_f16_workspace_bytes(b) == lib.mpo_patch_fc_f32_workspace_bytes(b)


def _rc(name, *args):
    rc = getattr(L.lib(), name)(*args)
    msg = L.lib().mpo_last_error()
    return rc, (msg.decode() if msg else "")


def test_refusals_come_before_any_launch():
    """In the fp32 entries' words, on pointers that are never dereferenced."""
    fake, big = 0x1000, 1 << 30
    # patches, total_rows, patch_dim, weight, bias, embed, drop_256, seed, offset, epoch, h_bag, workspace, bytes, stream
    for args, text in (((fake, 4, 768, fake, fake, 256, 0, 0, 0, None, fake, fake, big, None), "built for 1024 -> 256 (got 768 -> 256)"),
                       ((fake, 4, 1024, fake, fake, 128, 0, 0, 0, None, fake, fake, big, None), "built for 1024 -> 256 (got 1024 -> 128)"),
                       ((fake, 4, 1024, fake, fake, 256, 256, 0, 0, None, fake, fake, big, None),
                        "realised as round(256 p) / 256 = 256/256: nothing would be kept (p must be below 1 - 1/512)"),
                       ((fake, 4, 1024, fake, fake, 256, -1, 0, 0, None, fake, fake, big, None), "patch-layer dropout p must be in [0,1)"),
                       ((fake, 0, 1024, fake, fake, 256, 0, 0, 0, None, fake, fake, big, None), "total_rows 0"),
                       ((None, 4, 1024, fake, fake, 256, 0, 0, 0, None, fake, fake, big, None), "null operand"),
                       ((fake, 4, 1024, fake, fake, 256, 0, 0, 0, None, fake, fake, 64, None), "workspace too small")):
        rc, msg = _rc("mpo_patch_fc_f16_forward", *args)
        assert rc != 0 and text in msg, (args, rc, msg)
    # d_h_bag, h_bag, patches, total_rows, embed, patch_dim, drop_256, d_weight, d_bias, workspace, bytes, stream
    for args, text in (((fake, fake, fake, 4, 256, 768, 0, fake, fake, fake, big, None), "built for 256 x 1024 (got 256 x 768)"),
                       ((fake, fake, fake, 4, 128, 1024, 0, fake, fake, fake, big, None), "built for 256 x 1024 (got 128 x 1024)"),
                       ((fake, fake, fake, 4, 256, 1024, 256, fake, fake, fake, big, None), "realised as round(256 p) / 256 = 256/256"),
                       ((fake, fake, fake, 0, 256, 1024, 0, fake, fake, fake, big, None), "total_rows 0"),
                       ((fake, fake, fake, 4, 256, 1024, 0, fake, fake, fake, 64, None), "workspace too small")):
        rc, msg = _rc("mpo_patch_fc_f16_backward", *args)
        assert rc != 0 and text in msg, (args, rc, msg)
    # the same words as the fp32 entries give for the same mistakes
    rc, msg32 = _rc("mpo_patch_fc_f32_forward", fake, 4, 768, fake, fake, 256, 0.0, 0, 0, None, 1.0, fake, fake, big, None)
    rc, msg16 = _rc("mpo_patch_fc_f16_forward", fake, 4, 768, fake, fake, 256, 0, 0, 0, None, fake, fake, big, None)
    assert msg16 == msg32.replace("fp32", "fp16")
    # (the fp32 entry prints the p it was given, 0.999; this one the p its integer stands for, 256 / 256 = 1)
    rc, msg32 = _rc("mpo_patch_fc_f32_forward", fake, 4, 1024, fake, fake, 256, 0.999, 0, 0, None, 1.0, fake, fake, big, None)
    rc, msg16 = _rc("mpo_patch_fc_f16_forward", fake, 4, 1024, fake, fake, 256, 256, 0, 0, None, fake, fake, big, None)
    assert msg32.startswith("patch-layer dropout p = 0.999 is realised") and msg16.startswith("patch-layer dropout p = 1 is realised")
    assert msg16.split("is realised")[1] == msg32.split("is realised")[1]


def test_python_surface():
    x16, w = torch.empty(4, 1024, dtype=torch.float16), torch.empty(256, 1024)
    assert ops.patch_fc_f16_supported(x16, w) and not ops.patch_fc_f32_supported(x16, w)
    assert not ops.patch_fc_f16_supported(x16.float(), w) and not ops.patch_fc_f16_supported(x16.bfloat16(), w)
    assert not ops.patch_fc_f16_supported(x16, torch.empty(128, 1024))
    assert not ops.patch_fc_f16_supported(torch.empty(4, 512, dtype=torch.float16), torch.empty(256, 512))
    with pytest.raises(ValueError, match=r"realised as round\(256 p\) / 256 = 256/256"):
        ops._realised_drop(0.999)


def test_the_new_kernels_use_no_scratch_and_the_fp32_windows_kernels_have_not_moved():
    """Both windows' kernels are instances of one body per direction in csrc/patch_fc_split.hip: the compiler's resource rows
    of the fp32 window's kernels, recorded when they had a file of their own, are held here (NOTES.md: what the ISA text of
    each kernel differs in)."""
    _build = importlib.import_module("multimodal_path_omic_amd._build")
    _build.build(verbose=False)
    usage = _build.resource_usage()
    for kernel in ("patch_fc_f16_kernel", "patch_wgrad_f16x_kernel"):
        rows = [v for k, v in usage.items() if kernel in k]
        assert len(rows) == 1, kernel
        assert rows[0]["scratch_bytes"] == 0 and rows[0]["vgpr_spill"] == 0, (kernel, rows[0])
    row = [v for k, v in usage.items() if "patch_fc_f16_kernel" in k][0]
    assert row["lds_bytes"] == 16384                              # one 8 KiB fp16 image per stage: half the fp32 kernel's
    recorded = {"patch_fc_f32_kernelILi4E": dict(agprs=252, lds_bytes=32768, scratch_bytes=0, vgpr_spill=0, vgprs=256, waves_per_simd=1),
                "patch_wgrad_f32_kernel": dict(agprs=0, lds_bytes=131072, scratch_bytes=0, vgpr_spill=0, vgprs=256, waves_per_simd=2),
                "patch_wgrad_f32_reduce_kernel": dict(agprs=0, lds_bytes=0, scratch_bytes=0, vgpr_spill=0, vgprs=45, waves_per_simd=8),
                "pack_patch_weight_f32_kernel": dict(agprs=0, lds_bytes=0, scratch_bytes=0, vgpr_spill=0, vgprs=28, waves_per_simd=8),
                "weight_range_kernel": dict(agprs=0, lds_bytes=64, scratch_bytes=0, vgpr_spill=0, vgprs=12, waves_per_simd=8)}
    for kernel, want in recorded.items():
        rows = [v for k, v in usage.items() if kernel in k]
        assert rows and all(v == want for v in rows), (kernel, rows)


def test_models_take_the_dtype():
    from multimodal_path_omic_amd.models import (GeneExprNarrowContextualAttentionGateTransformer,
                                                 MultimodalCoAttentionTransformer, NarrowContextualAttentionGateTransformer)
    for m in (MultimodalCoAttentionTransformer(omic_sizes=[8] * 6, bag_dtype=torch.float16),
              NarrowContextualAttentionGateTransformer(omic_sizes=[8] * 6, bag_dtype=torch.float16),
              GeneExprNarrowContextualAttentionGateTransformer(bag_dtype=torch.float16)):
        assert m.bag_dtype == torch.float16


@pytest.fixture(scope="module")
def floors():
    """{case: {dtype: (co-attention map rel. error, hazards abs. error)}} with X ALONE stored in that dtype, by the oracle
    against the reference's fixtures at M = 15 000 -- the measure of tools/cpu_storage_floor.py.  Computed once."""
    import numpy as np
    with np.load(os.path.join(ROOT, "tests", "golden", "models.npz"), allow_pickle=False) as z:
        g = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.split("/")[0] in ("mcat_m15000", "nacagat_m15000")}
    out = {}
    for case in ("mcat_m15000", "nacagat_m15000"):
        kind, m, omic_sizes, seed = C.MODEL_CASES[case]
        sd = syn.fill_state_dict(C.model_shapes(omic_sizes, kind == "nacagat"), seed)
        wsi, omics, _, _ = C.model_inputs(m, omic_sizes, seed + 1)
        fwd = O.mcat_forward if kind == "mcat" else O.nacagat_forward
        kw = dict(inference=True) if kind == "mcat" else {}
        ga = g[f"{case}/A_coattn_sub"]
        out[case] = {}
        with torch.no_grad():
            for dt in (torch.float16, torch.bfloat16):
                hz, _, _, att = fwd(sd, wsi, omics, bag_storage=dt, storage_points=("x",), **kw)
                out[case][dt] = (float(((syn.subsample(att["coattn"]) - ga).abs() / ga.clamp_min(1e-30)).max()),
                                 float((hz - g[f"{case}/hazards"]).abs().max()))
    print("[fp16 / bf16 at X only, M = 15 000] " + "  ".join(
        f"{c}: fp16 map {v[torch.float16][0]:.2e} hazards {v[torch.float16][1]:.1e}, bf16 map {v[torch.bfloat16][0]:.2e}" for c, v in out.items()))
    return out


def test_fp16_storage_of_x_puts_mcats_map_inside_parity(floors):
    assert floors["mcat_m15000"][torch.float16][0] < 1e-3          # (4.5e-4; bf16 at X alone: 3.1e-3)
    assert all(v[torch.float16][1] < 1e-4 for v in floors.values())


@pytest.mark.parametrize("case", ["mcat_m15000", "nacagat_m15000"])
def test_fp16_storage_of_x_costs_a_fifth_of_bf16s_or_less(floors, case):
    """A ratio (three more significand bits: 2^-3 per element in expectation), so a host BLAS that sums in another order
    cannot flip it."""
    f16, b16 = floors[case][torch.float16][0], floors[case][torch.bfloat16][0]
    assert f16 <= b16 / 5, (f16, b16)
