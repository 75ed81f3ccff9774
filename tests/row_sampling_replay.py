"""Host restatement of the row sampler's draw (csrc/bag_sample.h), so a test can say which source rows a GPU run gathered.
Plain module (not a conftest): numpy only, no GPU.

Output row j < min(k, M) of slide b is source row pi_b(j) of that slide.  pi_b is a four-round balanced Feistel network over
2 h bits, h = ceil(bits(M - 1) / 2), with round function fmix32(R ^ round_key) & (2^h - 1), cycle-walked until the value is
< M.  Round keys: key = fmix32(hash_stream_key(seed, offset + epoch * 2^40) ^ fmix32(b + 0x9E3779B9)),
rk[r] = fmix32(key + (r + 1) * 0x85EBCA77).  hash_stream_key is csrc/mpo_common.h's.
"""
from __future__ import annotations

import numpy as np

from dropout_replay import EPOCH_STRIDE, fmix32

M64 = (1 << 64) - 1


def hash_stream_key(seed: int, offset: int) -> int:
    seed, offset = seed & M64, offset & M64
    k = fmix32(np.uint64((seed & 0xFFFFFFFF) ^ 0x5A17))
    k = fmix32(k ^ np.uint64(seed >> 32))
    k = fmix32(k ^ np.uint64(offset & 0xFFFFFFFF))
    return int(fmix32(k ^ np.uint64(offset >> 32)))


def round_keys(seed: int, offset: int, epoch: int, slide: int):
    key = hash_stream_key(seed, offset + epoch * EPOCH_STRIDE) ^ int(fmix32(np.uint64((slide + 0x9E3779B9) & 0xFFFFFFFF)))
    key = int(fmix32(np.uint64(key)))
    return [fmix32(np.uint64((key + (r + 1) * 0x85EBCA77) & 0xFFFFFFFF)) for r in range(4)]


def permutation_prefix(seed: int, offset: int, epoch: int, slide: int, m: int, k: int, return_walks: bool = False):
    """pi_slide(0 .. min(k, m) - 1) as an int64 array; with return_walks also the Feistel applications each element took."""
    n = min(int(k), int(m))
    if m == 1:
        out, walks = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        return (out, walks) if return_walks else out
    h = (int(m - 1).bit_length() + 1) // 2
    mask, sh = np.uint64((1 << h) - 1), np.uint64(h)
    rk = round_keys(seed, offset, epoch, slide)
    x = np.arange(n, dtype=np.uint64)
    walks = np.zeros(n, dtype=np.int64)
    todo = np.ones(n, dtype=bool)
    while todo.any():                        # ends by construction: an element's cycle returns to its start, which is < m
        v = x[todo]
        left, right = v >> sh, v & mask
        for r in range(4):
            left, right = right, left ^ (fmix32(right ^ rk[r]) & mask)
        x[todo] = (left << sh) | right
        walks[todo] += 1
        todo = x >= np.uint64(m)
    out = x.astype(np.int64)
    return (out, walks) if return_walks else out


def window_indices(seed: int, offset: int, epoch: int, lengths, k: int):
    """Per slide the slide-local source rows, and the window-level row indices into the concatenated rows (int64):
    x[window] is what the sampler writes for a window x with these lengths."""
    per, flat, start = [], [], 0
    for b, m in enumerate(lengths):
        idx = permutation_prefix(seed, offset, epoch, b, int(m), k)
        per.append(idx)
        flat.append(idx + start)
        start += int(m)
    return per, np.concatenate(flat)
