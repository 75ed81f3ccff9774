"""Dropout rates other than 0.25, the part that needs no GPU: the table of every dropout site of the C ABI against the public
headers, the rounding of the four rates the GPU file runs, the count of elements on which the 8-bit and the 24-bit keep rule
differ at every replayed site and shape of tests/test_gpu_dropout_rates.py (a comparison there can tell the two rules apart
only through those elements and the two scales), the host restatement of the K2 map's mask, and the refusal of a rate that
rounds to 256 / 256."""
import glob
import os
import re

import numpy as np
import pytest

import dropout_replay as R
import rate_cases as T
import step_replay as S
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import ops
from tail_helpers import FF, HEADS, LAYERS, OFF, SEED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 256


# ------------------------------------------------------------------------------------------- the site table
def _float_parameters():
    """{entry: [names of its scalar float parameters]} over include/*.h; every header passes _lib.parse_header first (whole
    declarations, known types), the names are then read off the same declarations."""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        with open(path) as f:
            text = f.read()
        signatures, _, _ = L.parse_header(text)
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*|^[ \t]*#.*$", " ", text, flags=re.M)
        seen = set()
        for m in L._DECL.finditer(text):
            _, name, args = m.groups()
            seen.add(name)
            words = [[w for w in a.split() if w != "const"] for a in args.split(",") if "*" not in a]
            floats = [w[1] for w in words if len(w) == 2 and w[0] == "float"]
            assert len(floats) == sum(t is L.c_float for t in signatures[name][1]), (name, "an unnamed float parameter")
            if floats:
                out[name] = floats
        assert seen == set(signatures), path
    return out


def test_every_entry_with_a_rate_or_a_keep_scale_is_in_the_site_table():
    floats = _float_parameters()
    assert len(floats) > 30                                                   # (the headers were found and read)
    unknown = {(e, n) for e, names in floats.items() for n in names} - \
        {(e, n) for e, names in floats.items() for n in names if n in T.RATE_NAMES | T.SCALE_NAMES | T.OTHER_FLOATS}
    assert not unknown, f"float parameters nobody has classified as rate, keep scale or neither: {sorted(unknown)}"
    carrying = {e: tuple(n for n in names if n in T.RATE_NAMES | T.SCALE_NAMES) for e, names in floats.items()}
    carrying = {e: names for e, names in carrying.items() if names}
    missing = sorted(set(carrying) - set(T.SITES))
    assert not missing, f"entries with a dropout rate or keep scale that the site table does not list: {missing}"
    stale = sorted(set(T.SITES) - set(carrying))
    assert not stale, f"site table rows whose entry has no such parameter any more: {stale}"
    for entry, (params, width, scale, test) in T.SITES.items():
        assert tuple(params) == carrying[entry], (entry, params, carrying[entry])
        assert width in ("8", "16", "24", "8+24", "scale") and scale, entry
        assert (width == "scale") == all(n in T.SCALE_NAMES for n in params) or entry == "mpo_patch_epilogue_backward", entry


def test_every_row_names_a_gpu_test_that_exists():
    for entry, (_, _, _, test) in T.SITES.items():
        fname, _, name = test.rpartition("::")
        with open(os.path.join(ROOT, "tests", fname or T.GPU_FILE)) as f:
            assert re.search(rf"^def {name}\(", f.read(), re.M), (entry, test)


def test_design_document_carries_the_site_table():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    for entry in T.SITES:
        assert f"`{entry}`" in text, f"DESIGN.md's dropout-site table does not list {entry}"


# ------------------------------------------------------------------------------------------- rounding
def test_rounding_directions_of_the_four_rates():
    assert [T.thr8(p) for p in T.RATES] == [26, 51, 128, 64]
    assert T.realised(0.1) > 0.1 and T.realised(0.2) < 0.2 and T.realised(0.5) == 0.5 and T.realised(0.25) == 0.25
    assert T.thr8(T.SMALL) == 0 and T.thr8(1 / 512) == 1 and T.thr8(0.99) == 253 and T.thr8(0.999) == 256
    for p in (0.25, 0.5):
        assert T.scale8(p) == T.scale24(p)
    assert abs(T.scale8(0.1) / T.scale24(0.1) - 1) == pytest.approx(1.74e-3, rel=0.01)      # 1.11304 against 1.11111
    assert abs(T.scale8(0.2) / T.scale24(0.2) - 1) == pytest.approx(9.76e-4, rel=0.01)      # 1.24878 against 1.25
    for p in T.RATES + (T.SMALL, 0.99):
        assert ops._realised_drop(p) == T.realised(p) and R.sa_threshold(p) == T.thr8(p)
    # step_replay.patch_keep scales by the 8-bit site's own scale
    import torch
    h = torch.tensor([[0.0, 1.0], [2.0, 0.0]])
    assert S.patch_keep(h, 0.1).tolist() == [[0.0, 256 / 230], [256 / 230, 0.0]]
    assert S.patch_keep(h).tolist() == [[0.0, 4 / 3], [4 / 3, 0.0]]
    assert S.map_keep(h, 0.1).tolist() == [[0.0, 1 / 0.9], [1 / 0.9, 0.0]]


# ------------------------------------------------------------------------------------------- band population
def _encoder_bands(p, nb, ns, T_, d):
    """{(layer, site): elements of that site's streams in the band}; site 0 only where it is on the 24-bit stream."""
    bt, rows = nb * ns, ns * T_
    stride = R.enc_stream_stride(bt, T_, d, FF)
    out = {}
    for layer in range(LAYERS):
        base = OFF + 4 * stride * layer
        if T_ <= R.SMALL_ATTN_MAX_T:
            out[layer, 0] = T.band(SEED, base, bt * HEADS * T_ * T_, p)
        for site, width in ((1, d), (2, FF), (3, d)):
            out[layer, site] = sum(T.band(SEED, base + stride * site + br * R._ceil4(rows * width), rows * width, p) for br in range(nb))
    return out


def _pool_bands(p_head, p_rho, ns, L_, interleave, nb=2, d=D):
    stride = R.pool_stride(nb * ns, L_, d)
    n = ns * L_ * d
    a, b = (sum(T.band(SEED, OFF + stride * site + br * R._ceil4(n), n, p_head) for br in range(nb)) for site in (0, 1))
    right = R.pool_keeps(SEED, OFF, nb, ns, L_, d, p_head, p_rho, interleave)[2]
    other = R.pool_keeps(SEED, OFF, nb, ns, L_, d, p_head, T.realised(p_rho), interleave)[2]
    return a, b, int(((right != 0) != (other != 0)).sum())


def _snn_bands(p, ns, n_groups=6, d=D):
    right, other = (R.snn_keeps(SEED, OFF, ns, n_groups, d, q) for q in (p, T.realised(p)))
    return [sum(int((r[i] != o[i]).sum()) for r, o in zip(right, other)) for i in (0, 1)]


@pytest.mark.parametrize("p", T.INEXACT + (T.SMALL,))
def test_band_is_populated_at_every_replayed_site(p):
    """Every comparison of the GPU file that replays a 24-bit site must contain at least one element the 8-bit rule would treat
    differently; a later change of shape or stream must not empty the band unnoticed.  (0.001: the 8-bit rule keeps everything,
    the band is the elements the 24-bit rule drops.)"""
    counts = {}
    enc = T.ENCODER if p != T.SMALL else T.ENCODER            # (the small-rate encoder case is the same shape)
    for key, c in _encoder_bands(p, enc["nb"], enc["ns"], enc["T"], enc["d"]).items():
        counts["encoder", key] = c
    if p != T.SMALL:
        e = T.ENCODER_LONG
        for key, c in _encoder_bands(p, e["nb"], e["ns"], e["T"], e["d"]).items():
            counts["encoder T=17", key] = c
        for i, c in enumerate(_snn_bands(p, T.SNN_NS)):
            counts["snn layer", i] = c
    for lengths in T.MAP_LENGTHS if p != T.SMALL else T.MAP_LENGTHS[1:]:
        counts["map", tuple(lengths)] = T.band(SEED, T.MAP_OFF, T.MAP_N_Q * sum(lengths), p)
    print(f"p = {p}: {counts}")
    empty = [k for k, c in counts.items() if c < 1]
    assert not empty, empty


@pytest.mark.parametrize("p_head,p_rho", T.POOL_PAIRS)
def test_band_is_populated_at_the_pooling_sites(p_head, p_rho):
    """(L 6, ns 32): the two scorer sites and rho each have elements in the band.  (L 65, ns 1): the scorer sites have; rho's 512
    elements have none at either rate (512 x 1.6e-3 = 0.8 expected), so rho's rule shows at this shape through its scale alone
    -- its mask is pinned element by element at ns = 32."""
    for interleave in (False, True):
        a, b, r = _pool_bands(p_head, p_rho, 32, 6, interleave)
        assert a >= 1 and b >= 1 and r >= 1, (interleave, a, b, r)
        a, b, r = _pool_bands(p_head, p_rho, 1, 65, interleave)
        assert a >= 1 and b >= 1, (interleave, a, b, r)
        print(f"pool ({p_head}, {p_rho}) interleave={interleave}: (6, 32) and (65, 1) checked; rho band at (65, 1): {r}")


def test_band_is_empty_where_256_p_is_an_integer():
    for p in (0.25, 0.5):
        assert sum(_encoder_bands(p, **{k: v for k, v in (("nb", 2), ("ns", 5), ("T_", 6), ("d", D))}).values()) == 0
        assert _snn_bands(p, T.SNN_NS) == [0, 0]
        assert T.band(SEED, T.MAP_OFF, T.MAP_N_Q * 777, p) == 0


# ------------------------------------------------------------------------------------------- K2 map restatement
def test_map_keeps_is_one_stream_over_the_absolute_element_index():
    """csrc/bag_maps.hip: MapRow.base = n_q * cu[b] + q * M_b, one draw per aligned group of four absolute indices."""
    n_q, lengths, p, off = 6, [33, 5], 0.1, T.MAP_OFF
    keeps = R.map_keeps(SEED, off, n_q, lengths, p)
    assert [k.shape for k in keeps] == [(6, 33), (6, 5)]
    words = R.stream_words(SEED, off, n_q * sum(lengths))
    cu = np.concatenate([[0], np.cumsum(lengths)])
    for b, m in enumerate(lengths):
        for q in range(n_q):
            for j in (0, m - 1):
                idx = n_q * int(cu[b]) + q * m + j
                u = np.float32(int(words[idx]) >> 8) * np.float32(1.0 / 16777216.0)
                assert (keeps[b][q, j] != 0) == bool(u >= np.float32(p))
    assert set(np.unique(np.concatenate([k.reshape(-1) for k in keeps]))) == {0.0, 1.0 / 0.9}
    assert R.map_span(n_q, sum(lengths)) == (n_q * sum(lengths) + 3) // 4
    # the epoch moves the stream by 2^40 counters; p = 0 keeps everything
    assert not np.array_equal(R.map_keeps(SEED, off, n_q, [777], p, 1)[0], R.map_keeps(SEED, off, n_q, [777], p)[0])
    assert float(R.map_keeps(SEED, off, n_q, [777], 0.0)[0].min()) == 1.0


def test_host_keeps_hands_every_site_its_own_rate():
    sites = {"snn": 100, "encoder": 50000, "pool": 900000, "map": 2000000}
    lengths = [33, 5]
    k = S.host_keeps(sites, SEED, 2, 2, 6, D, p=0.1, p_head=0.2, p_map=0.5, lengths=lengths)

    def scales(a):
        return set(np.unique(a)) - {0.0}
    assert scales(k["encoder"][0][1]) == {1 / 0.9} and scales(k["pool"][0]) == {1 / 0.8} == scales(k["pool"][1])
    assert scales(k["pool"][2]) == {1 / 0.9} and scales(k["map"][0]) == {2.0}
    assert 0.05 < 1 - float(np.mean(k["snn"][0][0])) < 0.15
    default = S.host_keeps(sites, SEED, 2, 2, 6, D)
    assert "map" not in default and scales(default["pool"][2]) == {1 / 0.75} == scales(default["encoder"][1][3])


# ------------------------------------------------------------------------------------------- the upper end
def test_a_rate_that_rounds_to_256_is_refused_before_anything_is_reserved():
    calls = ops._rng_calls
    with pytest.raises(ValueError, match=r"realised as round\(256 p\) / 256 = 256/256"):
        ops._realised_drop(0.999)
    assert ops._realised_drop(0.99) == 253 / 256 and ops._rng_calls == calls
    # the C entries word it the same way (csrc/patch_fc_fwd.hip, csrc/patch_fc_split.hip)
    for name in ("patch_fc_fwd.hip", "patch_fc_split.hip"):
        with open(os.path.join(ROOT, "multimodal_path_omic_amd", "csrc", name)) as f:
            assert "is realised as round(256 p) / 256 = %u/256" in f.read(), name
