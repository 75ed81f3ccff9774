"""The work plan of the bag passes, restated in plain Python, and the tile depth per wave it gives.

Every plan-driven bag kernel hands a workgroup one row range of one slide (csrc/coattn_tile.h, wg_geom) and deals the
range's 32-row tiles (16-row steps in the two vector-ALU kernels) to its waves one by one:
n_my = ceil((ntiles - wave) / WAVES).  At the benchmark's 32 x 15 000 rows a workgroup owns 59 tiles, 15 per wave on four
waves and 8 on eight; a window of a few thousand rows is cut into one or two tiles per workgroup, so the loops that carry
state from trip to trip (double-buffered images, load-ahead / write-late stages, the online softmax, accumulators kept
over tiles, a ragged last tile after full ones, idle waves beside busy ones in the LDS merge) would not run the way they
run in the benchmark.  `ops.plan_workgroups` caps the number of workgroups; this file shows on the CPU that the case table
of tests/test_gpu_plan_cuts.py reaches every depth class for every divisor the kernels use, and records that the largest
bf16 and window cases of the suite before it stayed at n_my <= 2 (two 100 000-row fp32 tests reach 4).

The restatement is compared with the real BagBatch.plan() in tests/test_gpu_plan_cuts.py (the plan needs a device tensor).
"""
import math

import pytest
import torch

import cases as C
from multimodal_path_omic_amd import synthetic as syn

TARGET_WORKGROUPS = 256          # mpo_coattn_target_workgroups(), csrc/capi.hip:83-85
TILE_ROWS = 32                   # kTileRows, csrc/coattn_tile.h:27

# kernel / instantiation -> (divisor of the n_my formula, rows per unit).  Copied from the sources; `csrc/` and `ops.py` are
# multimodal_path_omic_amd/csrc/ and multimodal_path_omic_amd/ops.py.
WAVES = {
    # csrc/coattn_fwd.hip:25   FwdCfg::WAVES = (F32BAG && E_ == 512) ? 2 : 4;  n_my at :100
    "coattn_fwd bf16 E128/256/512": (4, 32),
    "coattn_fwd f32 E128/256": (4, 32),
    "coattn_fwd f32 E512": (2, 32),
    # csrc/bagops.hip:27       BagCfg::WAVES = (F32BAG && E_ == 512) ? 2 : 4;  split_geom at :41
    "bag_rowdot / bag_colacc / gated colacc bf16": (4, 32),
    "bag_rowdot / bag_colacc / gated colacc f32 E128/256": (4, 32),
    "bag_rowdot / bag_colacc / gated colacc f32 E512": (2, 32),
    # csrc/bagops.hip:168, :261, :656   split_geom<4>: bag_outer and its gated forms
    "bag_outer": (4, 32),
    # csrc/coattn_bwd.hip:28   BwdCfg::WAVES = E_ == 512 ? (F32BAG ? 1 : 2) : 4;  n_my at :87
    "coattn_bwd E128/256": (4, 32),
    "coattn_bwd bf16 E512": (2, 32),
    "coattn_bwd f32 E512": (1, 32),
    # csrc/coattn_bwd8.hip:39  W8 = 8;  n_my at :104
    "coattn_bwd8": (8, 32),
    # csrc/coattn_bwd_f32.hip:27-28  F_WAVES = 8, F_HR = 16: 16-row steps, n_steps at :119
    "coattn_bwd_f32": (8, 16),
    # csrc/k2_patchgrad.hip:27  PG_WAVES = 8.  (Its eight waves share every tile -- each owns 32 output columns -- so the
    # kernel's own loop makes `ntiles` trips, two per round, :193; the entry is here for the row ranges it is given.)
    "k2_patchgrad": (8, 32),
    # csrc/bagops.hip:410-411  GateCfg::WAVES = NG <= 2 ? 8 : 4, PAIRS = WAVES / 2: a wave PAIR shares a tile,
    # split_geom<PAIRS> at :471
    "bag_rowdot_gated_exact NG2 (<= 8 queries)": (4, 32),
    "bag_rowdot_gated_exact NG4 (9..16 queries)": (2, 32),
    # csrc/bagops.hip:844-845  WAVES = 8, HR = 16: 16-row steps, n_steps at :880
    "bag_key_grad": (8, 16),
}
DIVISORS = sorted(set(WAVES.values()))

# (lengths, plan_workgroups) of tests/test_gpu_plan_cuts.py
RAGGED = [1, 31, 33, 700, 2999, 129]
CASES = [([2000], 1), ([2000], 3), ([2000], 7), ([777], 1), (RAGGED, 1), (RAGGED, 9)]


def rows_per_wg(lengths, plan_workgroups=None, target=TARGET_WORKGROUPS):
    """BagBatch.plan (multimodal_path_omic_amd/ops.py:52-62)."""
    if plan_workgroups is not None:
        target = max(len(lengths), min(target, int(plan_workgroups)))
    rpw = -(-sum(lengths) // target)
    rpw = max(32, -(-rpw // 32) * 32)
    while len(lengths) <= target and sum(-(-m // rpw) for m in lengths) > target:
        rpw += 32
    return rpw


def plan(lengths, plan_workgroups=None):
    """-> (wg_start, n_wg, rows_per_wg) as BagBatch.plan hands them to the C ABI."""
    rpw = rows_per_wg(lengths, plan_workgroups)
    starts = [0]
    for m in lengths:
        starts.append(starts[-1] + -(-m // rpw))
    return starts, starts[-1], rpw


def workgroups(lengths, plan_workgroups=None):
    """wg_geom (csrc/coattn_tile.h:51-78), planned branch: (slide, r0, r1) of every workgroup."""
    starts, n_wg, rpw = plan(lengths, plan_workgroups)
    out = []
    for b, m in enumerate(lengths):
        for split in range(starts[b + 1] - starts[b]):
            r0 = split * rpw
            out.append((b, r0, min(m, r0 + rpw)))
    assert len(out) == n_wg
    return out


def n_units(r0, r1, unit=TILE_ROWS):
    return -(-(r1 - r0) // unit) if r1 > r0 else 0


def n_my(ntiles, wave, waves):
    return (ntiles - wave + waves - 1) // waves if wave < ntiles else 0


def depths(lengths, plan_workgroups, waves, unit=TILE_ROWS):
    """Per workgroup: [n_my of wave 0 .. waves - 1]."""
    return [[n_my(n_units(r0, r1, unit), w, waves) for w in range(waves)] for _, r0, r1 in workgroups(lengths, plan_workgroups)]


def classes(lengths, plan_workgroups, waves, unit=TILE_ROWS):
    """The depth classes of the issue that this case reaches for this divisor."""
    got = set()
    rpw = rows_per_wg(lengths, plan_workgroups)
    for (b, r0, r1), per_wave in zip(workgroups(lengths, plan_workgroups), depths(lengths, plan_workgroups, waves, unit)):
        for n in per_wave:
            if n == 1:
                got.add("one")
            if n == 2:
                got.add("two")
            if n >= 3 and n % 2 == 1:
                got.add("odd>=3")
            if n >= 4 and n % 2 == 0:
                got.add("even>=4")
            if n >= 8:
                got.add(">=8")
        if max(per_wave) > 0 and min(per_wave) == 0:
            got.add("idle wave beside busy ones")
        units = n_units(r0, r1, unit)
        if (r1 - r0) % unit != 0 and (units - 1) // waves >= 1:      # the last unit is trip (units - 1) // waves of its wave
            got.add("partial last tile after full ones")
        if r1 - r0 < rpw and r0 > 0:
            got.add("short last workgroup of a slide")
    return got


ALL_CLASSES = {"one", "two", "odd>=3", "even>=4", ">=8", "idle wave beside busy ones", "partial last tile after full ones",
               "short last workgroup of a slide"}


def test_restated_plan_on_known_windows():
    """The figures quoted in the sources and in NOTES.md: the benchmark's 32 x 15 000 window gets 1888-row ranges (59 tiles),
    a 15 000-row slide 64-row ranges, [15000] * 6 384-row ranges (352 = ceil(90 000 / 256) rounded up would need 258
    workgroups, so the loop grows it once: 12 tiles)."""
    assert rows_per_wg([15000] * 32) == 1888 and n_units(0, 1888) == 59
    assert max(depths([15000] * 32, None, 4)[0]) == 15 and max(depths([15000] * 32, None, 8)[0]) == 8
    assert rows_per_wg([15000]) == 64
    assert rows_per_wg([15000] * 6) == 384 and n_units(0, 384) == 12
    assert rows_per_wg([30000] + [40] * 15 + [7] * 16) == 160
    assert plan([1000]) == ([0, 32], 32, 32)                       # smoke(): one tile per workgroup, only wave 0 works
    # every row of every slide is in exactly one workgroup
    for lengths, wgs in CASES + [([15000] * 6, None)]:
        seen = [0] * len(lengths)
        for b, r0, r1 in workgroups(lengths, wgs):
            assert r0 == seen[b] and r1 > r0
            seen[b] = r1
        assert seen == list(lengths)


def test_case_table_matches_its_description():
    assert depths([2000], 1, 4) == [[16, 16, 16, 15]]                          # 63 tiles
    assert depths([2000], 1, 8) == [[8] * 7 + [7]]
    assert depths([2000], 3, 8)[0] == [3, 3, 3, 3, 3, 2, 2, 2] and plan([2000], 3)[2] == 672     # 21 tiles per workgroup
    assert depths([2000], 7, 4)[0] == [3, 2, 2, 2] and depths([2000], 7, 8)[0] == [2] + [1] * 7   # 9 tiles
    assert plan([777], 1) == ([0, 1], 1, 800)
    assert n_units(0, 777) == 25 and 777 - 24 * 32 == 9 and 24 // 8 == 3 and 24 // 4 == 6        # wave 0's fourth / seventh trip
    assert n_units(0, 777, 16) == 49 and 48 // 8 == 6                                            # 16-row steps: the seventh
    starts, n_wg, rpw = plan(RAGGED, 1)                                         # clamped to one workgroup per slide
    assert n_wg == len(RAGGED) and rpw >= 2999 and n_units(0, 2999) == 94
    assert plan(RAGGED, 9)[1] <= 9


@pytest.mark.parametrize("waves,unit", DIVISORS, ids=lambda v: str(v))
def test_case_table_reaches_every_depth_class(waves, unit):
    got = set()
    for lengths, wgs in CASES:
        c = classes(lengths, wgs, waves, unit)
        print(f"WAVES {waves} unit {unit} {lengths} cut {wgs}: rows_per_wg {rows_per_wg(lengths, wgs)}, "
              f"n_my {sorted({tuple(d) for d in depths(lengths, wgs, waves, unit)})}; {sorted(c)}")
        got |= c
    want = set(ALL_CLASSES)
    if waves == 1:
        want.discard("idle wave beside busy ones")                 # a one-wave workgroup with work has no idle wave
    assert got >= want, sorted(want - got)


def test_largest_cases_before_this_file_stayed_at_two_tiles_per_wave():
    """What the gap was.  The three largest plan-driven cases of the suite, with the divisors of the kernels they reach:
    every one of them runs at E = 256 with six queries (4-wave kernels, the 8-wave ones, wave pairs of the gated row
    product = 4); [15000] * 6 is the fused K2 patch gradient's alone (eight waves)."""
    at_256 = [(4, 32), (8, 32), (8, 16)]
    for lengths, divisors in (([15000], at_256), ([30000] + [40] * 15 + [7] * 16, at_256), ([15000] * 6, [(8, 32)])):
        for waves, unit in divisors:
            worst = max(max(d) for d in depths(lengths, None, waves, unit))
            assert worst <= 2, (lengths, waves, unit, worst)
    # (the two 100 000-row fp32 tests go further -- 416-row ranges, 13 tiles -- on the fp32-bag kernels only)
    assert rows_per_wg([100000]) == 416 and depths([100000], None, 4)[0] == [4, 3, 3, 3]
    # and the case table goes to the benchmark's depth
    assert max(max(d) for d in depths([2000], 1, 4)) >= 15 and max(max(d) for d in depths([2000], 1, 8)) >= 8


def test_k1_online_softmax_rescale_is_exercised():
    """With the m2000_peaky weights the running maximum of a wave moves between its tiles in both directions, whichever end
    the wave starts from: for some query the per-tile maxima of the oracle's logits, in one wave's tile order under
    plan_workgroups = 1 (tiles wave, wave + 4, ...), are neither non-decreasing nor non-increasing -- so alpha != 1 occurs."""
    m, gain, seed = C.COATTN_CASES["m2000_peaky"]
    sd = syn.fill_state_dict(C.MCAT_COATTN_SHAPES, seed, gain)
    q, bag, _, _ = C.coattn_inputs(m, seed + 1)
    w, b = sd["co_attention.in_proj_weight"].double(), sd["co_attention.in_proj_bias"].double()
    e = C.E
    logits = (q.double() @ w[:e].t() + b[:e]) @ (bag.double() @ w[e:2 * e].t() + b[e:2 * e]).t() / math.sqrt(e)
    pad = torch.full((C.N_OMIC, 63 * 32 - m), -math.inf, dtype=torch.float64)
    tile_max = torch.cat([logits, pad], 1).view(C.N_OMIC, 63, 32).max(2).values
    assert depths([m], 1, 4) == [[16, 16, 16, 15]]
    moving = 0
    for wave in range(4):
        d = tile_max[:, wave::4].diff(dim=1)
        moving += int(((d > 0).any(1) & (d < 0).any(1)).sum())
    assert moving > 0
    assert float(logits.max(1).values.min() - logits.min(1).values.max()) > 8.0        # peaky: the rescale factors are far from 1
