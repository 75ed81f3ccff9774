"""Host restatement of every training-mode dropout mask the tail kernels draw, so a test can replay a GPU run's masks
exactly in the fp64 oracle.  Plain module (not a conftest): numpy only, no GPU.

Two generators, both pure functions of (seed, counter):
  * csrc/mpo_common.h draw4x32 / dropout_keep: element idx of the stream starting at counter `off` takes word idx % 4 of
    the 128-bit draw at counter off + idx // 4; keep when its top 24 bits, as u in [0, 1), are >= p; scale 1 / (1 - p).
  * csrc/bag_selfattn.hip sa_drop / sa_block (attention probabilities over long token axes): one 16-byte block per
    4 x 4 (query, key) tile under a key hashed from (seed, off + epoch * 2^40, sequence * H + head); keep when the
    element's byte >= round(256 p); scale 256 / (256 - thr).

Where each site's stream starts is restated from csrc/tail_api.hip (enc_stream_stride, stream_of, drop_br, the pooling
head's stride and interleaved d / 4 shift, the SNN's offset + stride * (2 i | 2 i + 1)).  The *_sites functions return
the counter range [lo, hi) each site touches, so a CPU test can check spans and disjointness without a GPU.

Every keep returned here is a float64 numpy array already scaled (0 or 1 / (1 - p)), except the AlphaDropout masks,
which are booleans (True = kept): the oracle forms a * (keep ? x : alpha') + b from them.
"""
from __future__ import annotations

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
EPOCH_STRIDE = 1 << 40
MAX_BRANCHES = 4                  # kMaxBranches, csrc/mpo_kernels.h
SMALL_ATTN_MAX_T = 16             # kSmallAttnMaxT: T <= 16 -> mha_small (counter stream), else bag self-attention hash
ALPHA_PRIME = -1.7580993408473766


# ------------------------------------------------------------------------------------------- the two hashes
def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def fmix32(h):
    """murmur3 finaliser on uint32 values held in uint64 (every multiply masked back to 32 bits)."""
    h = _u64(h) & M32
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & M32
    return h ^ (h >> np.uint64(16))


def hash4x32(key, ctr):
    """(n, 4) words of counters ctr (uint64 array) under 32-bit stream key `key`."""
    ctr = _u64(ctr)
    key = np.uint64(int(key))
    x = (fmix32(key ^ (ctr & M32)) + ((ctr >> np.uint64(32)) * np.uint64(0x85EBCA77) & M32)) & M32
    inc = fmix32(key ^ np.uint64(0x9E3779B9)) | np.uint64(1)
    return np.stack([fmix32((x + np.uint64(j) * inc) & M32) for j in (1, 2, 3, 4)], axis=-1)


def seed_key(seed: int) -> int:
    s_lo, s_hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    return int(fmix32(np.uint64(s_lo) ^ fmix32(np.uint64(s_hi ^ 0x5A17))))


def draw4x32(seed: int, ctr):
    return hash4x32(seed_key(seed), ctr)


def stream_words(seed: int, off: int, n: int):
    """The 32-bit words of elements 0 .. n-1 of the stream starting at counter `off`."""
    n_ctr = (n + 3) // 4
    ctr = np.uint64(off) + np.arange(n_ctr, dtype=np.uint64)
    return draw4x32(seed, ctr).reshape(-1)[:n]


def kept(seed: int, off: int, n: int, p: float):
    """dropout_keep != 0 for elements 0 .. n-1: u = (w >> 8) / 2^24 compared with p in float32."""
    w = stream_words(seed, off, n)
    u = (w >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u >= np.float32(p)


def keep_scale(seed: int, off: int, n: int, p: float):
    return kept(seed, off, n, p).astype(np.float64) / (1.0 - p)


def epoch_off(off: int, epoch: int) -> int:
    return off + epoch * EPOCH_STRIDE


def alpha_dropout(x, keep, p: float):
    """nn.AlphaDropout with a given boolean keep mask: a * (keep ? x : alpha') + b (mpo_common.h alpha_drop_a / _b)."""
    a = 1.0 / ((1.0 - p) * (1.0 + p * ALPHA_PRIME * ALPHA_PRIME)) ** 0.5
    b = -a * ALPHA_PRIME * p
    return a * np.where(keep, x, ALPHA_PRIME) + b


# ------------------------------------------------------------------------------------------- bag self-attention hash
def sa_threshold(p: float) -> int:
    t = int(p * 256.0 + 0.5) if p > 0 else 0
    return min(t, 255)


def sa_keys(seed: int, off: int, heads):
    """(key, inc) per entry of `heads` (= sequence * H + head) for the stream offset `off` (epoch already added)."""
    k = fmix32(np.uint64((seed & 0xFFFFFFFF) ^ 0x5A17))
    k = fmix32(k ^ np.uint64((seed >> 32) & 0xFFFFFFFF))
    k = fmix32(k ^ np.uint64(off & 0xFFFFFFFF))
    k = fmix32(k ^ np.uint64((off >> 32) & 0xFFFFFFFF))
    key = fmix32(k ^ (_u64(heads) & M32))
    inc = fmix32(key ^ np.uint64(0x9E3779B9)) | np.uint64(1)
    return key, inc


def sa_keep(seed: int, off: int, head_key: int, M: int, p: float):
    """(M, M) keep scale of one (sequence, head): element (q, k) is byte k % 4 of word q % 4 of block (q / 4, k / 4)."""
    thr = sa_threshold(p)
    if thr == 0:
        return np.ones((M, M))
    key, inc = sa_keys(seed, off, head_key)
    qb = np.arange((M + 3) // 4, dtype=np.uint64)
    kb = np.arange((M + 3) // 4, dtype=np.uint64)
    x = ((key ^ ((qb * np.uint64(0x9E3779B1)) & M32))[:, None] + (kb * np.uint64(0x85EBCA77) & M32)[None, :]) & M32
    nb = x.shape[0]
    out = np.empty((nb, 4, nb, 4), dtype=bool)
    for i in range(4):
        w = fmix32((x + np.uint64(i) * inc) & M32)                                   # (qb, kb): word i = query row qb*4+i
        for byte in range(4):
            out[:, i, :, byte] = ((w >> np.uint64(8 * byte)) & np.uint64(255)) >= np.uint64(thr)
    return out.reshape(4 * nb, 4 * nb)[:M, :M].astype(np.float64) * (256.0 / (256.0 - thr))


# ------------------------------------------------------------------------------------------- encoder (mpo_encoder_forward)
def enc_stream_stride(bt: int, T: int, d: int, ff: int) -> int:
    return bt * T * max(ff, 3 * d) // 4 + 2


def _ceil4(n: int) -> int:
    return (n + 3) // 4


def encoder_sites(n_branches, n_slides, T, d, ff, heads, layers, off=0):
    """[(layer, site, branch, lo, hi)]: the counters each site of mpo_encoder_forward draws.  Site 0 on the long-T path
    is the bag self-attention hash, whose only counter-space input is its stream offset (one counter)."""
    bt = n_branches * n_slides
    R = n_slides * T
    stride = enc_stream_stride(bt, T, d, ff)
    out = []
    for l in range(layers):
        base = off + 4 * stride * l
        s0 = base
        n0 = bt * heads * T * T if T <= SMALL_ATTN_MAX_T else 1
        out.append((l, 0, None, s0, s0 + (_ceil4(n0) if T <= SMALL_ATTN_MAX_T else 1)))
        for site, width in ((1, d), (2, ff), (3, d)):
            so = base + stride * site
            for br in range(n_branches):
                lo = so + br * _ceil4(R * width)
                out.append((l, site, br, lo, lo + _ceil4(R * width)))
    return out


def encoder_span(n_slides_total, T, d, ff, layers) -> int:
    """mpo_encoder_rng_span restated (n_slides_total = branches * slides, as ops passes it)."""
    return enc_stream_stride(n_slides_total, T, d, ff) * 4 * layers


def encoder_keeps(seed, off, n_branches, n_slides, T, d, ff, heads, layers, p, epoch=0):
    """Per layer a tuple (attn (nb, B, H, T, T), out (nb, B, T, d), ff (nb, B, T, ff), ff_out (nb, B, T, d)) of keep
    scales, in the positions of nn.TransformerEncoderLayer (norm_first=False)."""
    bt = n_branches * n_slides
    R = n_slides * T
    stride = enc_stream_stride(bt, T, d, ff)
    res = []
    for l in range(layers):
        base = epoch_off(off + 4 * stride * l, epoch)
        s0, s1, s2, s3 = (base + stride * k for k in range(4))
        if T <= SMALL_ATTN_MAX_T:
            attn = keep_scale(seed, s0, bt * heads * T * T, p).reshape(n_branches, n_slides, heads, T, T)
        else:
            attn = np.empty((n_branches, n_slides, heads, T, T))
            for seq in range(bt):
                for h in range(heads):
                    attn[seq // n_slides, seq % n_slides, h] = sa_keep(seed, s0, seq * heads + h, T, p)

        def site(so, width):
            return np.stack([keep_scale(seed, so + br * _ceil4(R * width), R * width, p).reshape(n_slides, T, width)
                             for br in range(n_branches)])
        res.append((attn, site(s1, d), site(s2, ff), site(s3, d)))
    return res


# ------------------------------------------------------------------------------------------- gated pool
def pool_stride(bt: int, L: int, d: int) -> int:
    return bt * L * d // 4 + 2 + MAX_BRANCHES


def pool_sites(n_branches, n_slides, L, d, interleave, off=0):
    """[(site, branch, lo, hi)] of mpo_gated_pool_forward: 0 attention_a, 1 attention_b, 2 rho."""
    bt = n_branches * n_slides
    R = n_slides * L
    stride = pool_stride(bt, L, d)
    out = []
    for site in (0, 1):
        for br in range(n_branches):
            lo = off + stride * site + br * _ceil4(R * d)
            out.append((site, br, lo, lo + _ceil4(R * d)))
    s2 = off + 2 * stride
    if interleave:
        # one stream over the interleaved [slide][branch][d] rows: element (s, j) of branch br is element
        # s * nb * d + br * d + j (branch br's pointer starts d / 4 counters in), every element drawn once
        out.append((2, None, s2, s2 + _ceil4(n_slides * n_branches * d)))
        return out
    for br in range(n_branches):
        lo = s2 + br * _ceil4(n_slides * d)
        out.append((2, br, lo, lo + _ceil4(n_slides * d)))
    return out


def pool_span(n_slides_total, L, d) -> int:
    """mpo_gated_pool_rng_span restated."""
    return 3 * (n_slides_total * L * d // 4 + 2 + MAX_BRANCHES)


def pool_keeps(seed, off, n_branches, n_slides, L, d, p_head, p_rho, interleave, epoch=0):
    """(keep_a (nb, B, L, d), keep_b (nb, B, L, d), keep_rho (nb, B, d)) keep scales."""
    bt = n_branches * n_slides
    R = n_slides * L
    stride = pool_stride(bt, L, d)
    base = epoch_off(off, epoch)
    ka = np.stack([keep_scale(seed, base + br * _ceil4(R * d), R * d, p_head).reshape(n_slides, L, d)
                   for br in range(n_branches)])
    kb = np.stack([keep_scale(seed, base + stride + br * _ceil4(R * d), R * d, p_head).reshape(n_slides, L, d)
                   for br in range(n_branches)])
    s2 = base + 2 * stride
    if interleave:
        krho = np.stack([keep_scale(seed, s2 + br * (d // 4), n_slides * n_branches * d, p_rho)
                         .reshape(n_slides, n_branches * d)[:, :d] for br in range(n_branches)])
    else:
        krho = np.stack([keep_scale(seed, s2 + br * _ceil4(n_slides * d), n_slides * d, p_rho).reshape(n_slides, d)
                         for br in range(n_branches)])
    return ka, kb, krho


# ------------------------------------------------------------------------------------------- omic SNN
def snn_stride(n_slides, n_groups, d) -> int:
    return n_slides * n_groups * d // 4 + 2


def snn_sites(n_slides, n_groups, d, off=0):
    """[(group, layer, lo, hi)] of mpo_omic_snn_forward."""
    stride = snn_stride(n_slides, n_groups, d)
    out = []
    for i in range(n_groups):
        lo = off + stride * 2 * i
        out.append((i, 0, lo, lo + _ceil4(n_slides * d)))
        lo = off + stride * (2 * i + 1)                 # layer 2 writes G_bag rows of stride n_groups * d
        out.append((i, 1, lo, lo + _ceil4((n_slides - 1) * n_groups * d + d)))
    return out


def snn_span(n_slides, n_groups, d) -> int:
    """mpo_omic_snn_rng_span restated."""
    return 2 * n_groups * snn_stride(n_slides, n_groups, d)


def snn_keeps(seed, off, n_slides, n_groups, d, p, epoch=0):
    """Per group (keep1 (B, d), keep2 (B, d)) booleans (True = kept) of the two AlphaDropouts."""
    stride = snn_stride(n_slides, n_groups, d)
    base = epoch_off(off, epoch)
    res = []
    for i in range(n_groups):
        k1 = kept(seed, base + stride * 2 * i, n_slides * d, p).reshape(n_slides, d)
        k2 = kept(seed, base + stride * (2 * i + 1), n_slides * n_groups * d, p).reshape(n_slides, n_groups * d)[:, :d]
        res.append((k1, k2))
    return res


# ------------------------------------------------------------------------------------------- K2 map (NaCAGaT)
def map_span(n_q: int, rows: int) -> int:
    """ops.next_dropout_stream(n_q * rows) restated: one counter per four elements of the ragged map."""
    return _ceil4(n_q * rows)


def map_keeps(seed, off, n_q, lengths, p, epoch=0):
    """Per slide the (n_q, M_b) keep scale of the co-attention map's dropout.  csrc/bag_maps.hip map_keep4 is dropout_keep
    over the ABSOLUTE element index of the ragged map -- slide b's block starts at n_q * (rows before b), query q's row at
    q * M_b inside it -- so the whole window is ONE stream of n_q * rows elements: kept(seed, off, n_q * rows, p), scale
    1 / (1 - p)."""
    rows = int(sum(lengths))
    flat = keep_scale(seed, epoch_off(off, epoch), n_q * rows, p)
    out, at = [], 0
    for m in lengths:
        out.append(flat[n_q * at:n_q * (at + m)].reshape(n_q, m))
        at += m
    return out
