"""The launch arithmetic of csrc/bag_selfattn.hip, restated in plain Python, and the tile / batch / map classes it gives.

The file holds two kernel families -- fp32 (head widths 16 .. 512) and three-term bf16, "b3" (8 x 32 and 1 x 256 heads) -- each
with forward, map, dQ and dK/dV kernels.  A workgroup owns 64 queries (or keys) and streams the other axis in tiles of BN rows;
the map kernels cut the key blocks over grid.y so that one launch has ~2048 workgroups, which below ~2050 rows means ONE block
per workgroup.  This file shows on the CPU that the case table of tests/test_gpu_bag_selfattn_edges.py reaches, for every
instantiated kernel, every class of the list in `classes()` that the kernel can reach; the GPU file imports the table from here.

`csrc/` is multimodal_path_omic_amd/csrc/; line numbers are bag_selfattn.hip's.
"""
import pytest
import torch

from multimodal_path_omic_amd import synthetic as syn

F32_HD = (16, 32, 64, 128, 256, 512)         # :1191 mpo_bag_sa_supported_head_dim, :1224-1231 the fp32 dispatch
B3_HD = (32, 256)                            # :1221-1222
KERNELS = [("f32", hd) for hd in F32_HD] + [("b3", hd) for hd in B3_HD]


def b3_geometry(d, heads):
    """:1120  (H > 1 && d == 32 H) || (H == 1 && d == 256)"""
    return (heads > 1 and d == 32 * heads) or (heads == 1 and d == 256)


def kernel_of(d, heads, hook=1):
    """:1220 b3_applies = the hook (mpo_set_bag_self_attention_bf16x3, default on) && b3_geometry -> (family, head width)"""
    return ("b3" if hook and b3_geometry(d, heads) else "f32", d // heads)


def bn(family, hd):
    """Rows of the streamed tile.  :31 SaCfg::BN = HD >= 128 ? 32 : 64;  :453 B3Cfg::BN = HD == 32 ? 64 : 32"""
    if family == "b3":
        return 64 if hd == 32 else 32
    return 32 if hd >= 128 else 64


def mp(m):
    """:1118 b3_mp: rows of the b3 operand forms, M rounded up to 64 (padding rows zero)"""
    return (m + 63) // 64 * 64


def qb(family, m):
    """Query (key) blocks of 64 = grid.x.  :412 / :416 (M + 63) / 64;  b3 :1149, :1154, :1172  Mp / 64"""
    return mp(m) // 64 if family == "b3" else (m + 63) // 64


def n_steps(family, hd, m):
    """Trips of the streamed loop `for (n0 = 0; n0 < M; n0 += BN)`: :177, :306, :366 (fp32), :760, :939, :1040 (b3)"""
    return -(-m // bn(family, hd))


def np_passes(hd):
    """:433 column passes of the fp32 dK/dV kernel: NP = HD > 256 ? 2 : 1 (grid.y = H * NP)"""
    return 2 if hd > 256 else 1


def map_capable(family, hd):
    """The map is returned for one head only (:1217), so d = HD; on the b3 path one head means HD = 256 (:1120)."""
    return family == "f32" or hd == 256


def vec(m):
    """:244, :849 the float4 store of the map kernels: vec = (M & 3) == 0 (taken where key + 3 < M, :256, :877)"""
    return m % 4 == 0


def map_cut(family, hd, m):
    """The map launch.  :416-419 and :1154-1156: split = min(ceil(2048 / qb), nblk) = grid.y;  :242-243 and :847-848:
    per = ceil(nblk / grid.y), b0 = blockIdx.y * per, b1 = min(nblk, b0 + per).  -> (nblk, split, per, [(b0, b1)])"""
    nblk = -(-m // bn(family, hd))
    split = min(-(-2048 // qb(family, m)), nblk)
    per = -(-nblk // split)
    return nblk, split, per, [(y * per, min(nblk, y * per + per)) for y in range(split)]


def thr(p):
    """:57-58 sa_drop: thr = p > 0 ? min((unsigned)(256 p + 0.5), 255) : 0; a byte below thr is dropped, kept entries are
    scaled by 256 / (256 - thr) (:59).  thr == 0 is the no-dropout instantiation (:205 `if (dr.thr)`, :1148, :1173)."""
    return min(int(p * 256.0 + 0.5), 255) if p > 0 else 0


def smallest_multi_block_m(family, hd, want_vec):
    """Smallest M at which a map workgroup handles more than one key block AND one workgroup is short AND one is empty."""
    for m in range(1, 1 << 14):
        if vec(m) == want_vec and {"per>=2 with a short and an empty workgroup"} <= map_classes(family, hd, m):
            return m
    raise AssertionError((family, hd))


def map_classes(family, hd, m):
    nblk, split, per, cut = map_cut(family, hd, m)
    got = {"vec" if vec(m) else "scalar"}
    if per == 1:
        got.add("per==1")
    elif any(0 < b1 - b0 < per for b0, b1 in cut) and any(b0 >= nblk for b0, _ in cut):
        got.add("per>=2 with a short and an empty workgroup")
    return got


def classes(family, hd, n, m, need_map):
    """The classes of the issue that one call reaches on one kernel."""
    got = {f"n_seq={n}"} if n in (1, 3) else set()
    if m % 64 in (0, 1, 63):
        got.add(f"M%64=={m % 64}")
    if m < 16:
        got.add("M<16")
    if 16 < m < 64:
        got.add("16<M<64")
    got.add("last tile full" if m % bn(family, hd) == 0 else "last tile partial")
    if need_map:
        got |= {"map " + c for c in map_classes(family, hd, m)}
    if hd == 512 and n == 3:
        got.add("NP=2 at n_seq=3")
    return got


def wanted(family, hd):
    want = {"n_seq=1", "n_seq=3", "M%64==0", "M%64==1", "M%64==63", "M<16", "16<M<64", "last tile full", "last tile partial"}
    if map_capable(family, hd):
        want |= {"map vec", "map scalar", "map per==1", "map per>=2 with a short and an empty workgroup"}
    if hd == 512:
        assert np_passes(hd) == 2
        want.add("NP=2 at n_seq=3")
    return want


# ---------------------------------------------------------------------------------------------------------------- the case table
# geometry (d, heads): 256/1 = b3-256 | fp32-256 under the hook, 256/8 = b3-32 | fp32-32, 128/1 = fp32-128, 128/8 = fp32-16,
# 512/8 = fp32-64, 512/1 = fp32-512, and single heads of 16, 32, 64: the narrow fp32 kernels WITH a map
GEOMETRIES = [(256, 1), (256, 8), (128, 1), (128, 8), (512, 8), (512, 1), (16, 1), (32, 1), (64, 1)]
SMALL_M = {1: (1, 15, 16, 64, 127, 191), 3: (3, 63, 65, 128, 132)}      # n_seq -> lengths (half of the product)
SMALL_CASES = [(n, m, d, h) for d, h in GEOMETRIES for n in (1, 3) for m in SMALL_M[n]]          # n_seq, M, d, heads

M32_SCALAR, M32_VEC = 2049, 2052             # BN = 32: 65 blocks over 63 workgroups of 2 -> 32 full, one short, 30 empty
M64_SCALAR, M64_VEC = 2945, 2948             # BN = 64: 47 blocks over 44 workgroups of 2 -> 23 full, one short, 20 empty
# n_seq, M, d, heads, hook, with backward
MAP_CASES = [(1, M32_SCALAR, 256, 1, 1, True), (2, M32_VEC, 256, 1, 1, False), (1, M32_VEC, 256, 1, 0, True),
             (1, M32_SCALAR, 512, 1, 1, False), (1, M32_VEC, 128, 1, 1, False), (1, M64_SCALAR, 64, 1, 1, False),
             (1, M64_VEC, 32, 1, 1, False), (1, M64_SCALAR, 16, 1, 1, False)]


# ---------------------------------------------------------------------------------------------------------------- large logits
LARGE_LOGIT_SHAPE = (200, 256)               # M, d of the one-head case; Q is scaled until the largest |score| * scale is 80
# Yardstick: torch_fp32_map_error() on large_logit_input(), plain torch fp32 on the CPU against fp64, measured 5.82e-5 (the same
# with 1, 4 and 8 threads).  Margin: 4 x -- the b3 operands carry ~16 mantissa bits and the exponent's argument error scales
# with |s|.  4 x 5.82e-5 = 2.3e-4 is below the file's map bar, so the bar of the large-logit case stays 1e-3.
FP32_LARGE_LOGIT_MAP_ERR = 5.82e-5
LARGE_LOGIT_MAP_BAR = max(1e-3, 4 * FP32_LARGE_LOGIT_MAP_ERR)


def large_logit_input():
    m, d = LARGE_LOGIT_SHAPE
    g = syn.rng(8800)
    qkv, probe = syn.normal(g, (1, m, 3 * d)), syn.normal(g, (1, m, d))
    peak = float((qkv[0, :, :d].double() @ qkv[0, :, d:2 * d].double().t()).abs().max()) / d ** 0.5
    qkv[..., :d] *= 80.0 / peak
    return qkv, probe


def torch_fp32_map_error(qkv, d):
    """Largest elementwise relative error (where fp64 exceeds 1e-30) of softmax(q k^T / sqrt(d)) in plain torch fp32."""
    q, k = qkv[0, :, :d], qkv[0, :, d:2 * d]
    ref = torch.softmax(q.double() @ k.double().t() / d ** 0.5, -1)
    got = torch.softmax(q @ k.t() / d ** 0.5, -1).double()
    big = ref > 1e-30
    return float(((got - ref).abs() / ref.clamp_min(1e-30))[big].max())


def table():
    """Every (kernel, n_seq, M, with map) the two tables run."""
    out = []
    for n, m, d, h in SMALL_CASES:
        for hook in ((1, 0) if b3_geometry(d, h) else (1,)):
            out.append((kernel_of(d, h, hook), n, m, h == 1))
    for n, m, d, h, hook, _ in MAP_CASES:
        out.append((kernel_of(d, h, hook), n, m, True))
    return out


def test_restated_arithmetic_on_known_shapes():
    assert [kernel_of(d, h) for d, h in GEOMETRIES] == [("b3", 256), ("b3", 32), ("f32", 128), ("f32", 16), ("f32", 64),
                                                         ("f32", 512), ("f32", 16), ("f32", 32), ("f32", 64)]
    assert kernel_of(256, 1, 0) == ("f32", 256) and kernel_of(256, 8, 0) == ("f32", 32)
    assert not b3_geometry(32, 1) and not b3_geometry(512, 8) and b3_geometry(64, 2)
    assert [bn("f32", hd) for hd in F32_HD] == [64, 64, 64, 32, 32, 32] and [bn("b3", hd) for hd in B3_HD] == [64, 32]
    assert (mp(1), mp(64), mp(65), mp(15000)) == (64, 64, 128, 15040)
    # the long-bag shape itself: 235 query blocks, 9 workgroups per block, 469 key blocks in 9 runs of 53 (the last 45)
    nblk, split, per, cut = map_cut("b3", 256, 15000)
    assert (qb("b3", 15000), nblk, split, per) == (235, 469, 9, 53) and cut[-1] == (424, 469)
    # ge_m3000, until now the one case with several blocks per workgroup: 94 blocks in 44 workgroups of 3 -> 31 full, one of 1
    nblk, split, per, cut = map_cut("b3", 256, 3000)
    assert (nblk, split, per) == (94, 44, 3) and cut[31] == (93, 94) and cut[32] == (96, 94)
    # every key block is in exactly one workgroup, whatever the cut
    for fam, hd in KERNELS:
        for m in (1, 63, 64, 65, 2048, M32_SCALAR, M64_VEC, 3000, 15000):
            nblk, split, per, cut = map_cut(fam, hd, m)
            assert [b for b0, b1 in cut for b in range(b0, b1)] == list(range(nblk)), (fam, hd, m)
    assert [thr(p) for p in (0.0, 0.001, 0.0019, 0.002, 0.1, 0.25, 0.5, 0.999, 1.0)] == [0, 0, 0, 1, 26, 64, 128, 255, 255]


def test_smallest_lengths_with_several_blocks_per_map_workgroup():
    """Up to 2048 rows qb <= 32 and ceil(2048 / qb) >= nblk: one block per workgroup.  At 2049 rows and BN = 32, 33 query blocks
    give 63 workgroups for 65 key blocks; at BN = 64 the count of key blocks equals qb, so it takes qb (qb - 1) > 2048 --
    46 blocks, 2881 rows -- for per = 2, and an odd count, 47 blocks, for a short workgroup."""
    for fam, hd in KERNELS:
        if not map_capable(fam, hd):
            continue
        want = (M32_SCALAR, M32_VEC) if bn(fam, hd) == 32 else (M64_SCALAR, M64_VEC)
        assert (smallest_multi_block_m(fam, hd, False), smallest_multi_block_m(fam, hd, True)) == want, (fam, hd)
        assert all(map_cut(fam, hd, m)[2] == 1 for m in range(1, 2049)), (fam, hd)
    assert map_cut("f32", 64, 2881)[2] == 2 and "map per==1" not in classes("f32", 64, 1, 2881, True)
    nblk, split, per, cut = map_cut("b3", 256, M32_SCALAR)
    assert (nblk, split, per) == (65, 63, 2) and cut[31] == (62, 64) and cut[32] == (64, 65) and cut[33] == (66, 65)
    nblk, split, per, cut = map_cut("f32", 64, M64_VEC)
    assert (nblk, split, per) == (47, 44, 2) and cut[23] == (46, 47) and cut[24] == (48, 47)


@pytest.mark.parametrize("family,hd", KERNELS, ids=lambda v: str(v))
def test_case_table_reaches_every_class(family, hd):
    got = set()
    for kernel, n, m, need_map in table():
        if kernel == (family, hd):
            assert not need_map or map_capable(family, hd)
            got |= classes(family, hd, n, m, need_map)
    print(f"{family} HD {hd}: {sorted(got)}")
    assert got >= wanted(family, hd), sorted(wanted(family, hd) - got)


def test_a_class_removed_from_the_table_is_noticed():
    """The check above is not vacuous: without the lengths that carry a class, that class is reported missing."""
    def got_without(drop):
        got = set()
        for kernel, n, m, need_map in table():
            if kernel == ("b3", 256) and not drop(n, m):
                got |= classes("b3", 256, n, m, need_map)
        return wanted("b3", 256) - got
    assert got_without(lambda n, m: False) == set()
    assert got_without(lambda n, m: m > 2048) == {"map per>=2 with a short and an empty workgroup"}
    assert got_without(lambda n, m: m % 64 == 63) == {"M%64==63", "16<M<64"}
    assert got_without(lambda n, m: n == 3) == {"n_seq=3", "16<M<64"}             # (63 rows run at n_seq = 3)
    assert got_without(lambda n, m: m % 4 == 0) == {"map vec", "M%64==0", "last tile full"}


def test_what_the_kernel_level_cases_reached_before():
    """The gap.  (n_seq, M, d, heads) of test_attention_core_equals_torch: no map workgroup with two blocks, the b3 kernels on a
    second sequence at M = 64 without a map only, fp32-256 never, one length per narrow head width, no map at a length that takes the float4 store."""
    old = [(1, 333, 256, 1), (1, 1000, 256, 8), (2, 64, 256, 8), (1, 70, 128, 1), (1, 130, 128, 8), (1, 200, 512, 8),
           (1, 257, 256, 1), (1, 515, 256, 8), (1, 1, 256, 8), (1, 17, 256, 1), (1, 150, 512, 1), (2, 333, 512, 1)]
    assert all(map_cut(*kernel_of(d, h), m)[2] == 1 for n, m, d, h in old if h == 1)
    assert [(m, d, h) for n, m, d, h in old if n > 1 and b3_geometry(d, h)] == [(64, 256, 8)]
    assert [(m, d) for n, m, d, h in old if h == 1 and vec(m)] == []            # (200 rows ran with eight heads: no map)
    for hd, lengths in ((16, [130]), (64, [200]), (128, [70])):
        assert [m for n, m, d, h in old if d // h == hd] == lengths


def test_large_logit_yardstick():
    """The input peaks at 80, and the constant beside LARGE_LOGIT_MAP_BAR is what plain torch fp32 does on it (within the
    spread of another summation order)."""
    qkv, _ = large_logit_input()
    m, d = LARGE_LOGIT_SHAPE
    peak = float((qkv[0, :, :d].double() @ qkv[0, :, d:2 * d].double().t()).abs().max()) / d ** 0.5
    assert abs(peak - 80.0) < 1e-3
    err = torch_fp32_map_error(qkv, d)
    print(f"torch fp32 map error at peak 80: {err:.3e}; bar {LARGE_LOGIT_MAP_BAR:.1e}")
    assert FP32_LARGE_LOGIT_MAP_ERR / 3 < err < FP32_LARGE_LOGIT_MAP_ERR * 3
    assert LARGE_LOGIT_MAP_BAR == 1e-3
