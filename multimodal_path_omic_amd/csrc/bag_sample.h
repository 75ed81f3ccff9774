// The draw of the fixed-budget row sampler (csrc/bag_sample.hip): which source row of slide b becomes output row j.
//
//   pi_b = a permutation of [0, M_b), a pure function of (seed, offset + epoch * 2^40, b, M_b); output row j < min(k, M_b) of
//   slide b is source row pi_b(j): sampling WITHOUT replacement, every pi_b(j) computed on its own (no sort, no scratch).
//
// Construction: a balanced Feistel network over 2 h bits, h = ceil(bits(M - 1) / 2), four rounds with the round function
// fmix32(R ^ round_key) masked to h bits -- a bijection of [0, 2^(2h)) whatever the round function is -- and cycle-walking:
// apply it again until the value is < M.  The walk starts at j < M and follows j's cycle of that bijection, which returns
// to j itself at the latest, so it ends by construction (no iteration cap), and distinct j stay distinct.  2^(2h) < 4 M, so
// a step lands inside with probability > 1/4: under 4 steps per element expected.
// The four round keys hang off hash_stream_key(seed, offset) (mpo_common.h: the dropout generator's stream key, so the
// device epoch moves them through the offset) and the slide index.
// tests/row_sampling_replay.py restates this file in numpy.
#pragma once
#include "mpo_common.h"

struct RowDraw {
    uint32_t rk[4];         // round keys
    uint32_t m;             // rows of the slide
    uint32_t h;             // bits per Feistel half; 0 for a slide of one row
};

__host__ __device__ __forceinline__ RowDraw row_draw_make(unsigned long long seed, unsigned long long offset, uint32_t slide,
                                                          uint32_t m) {
    RowDraw d;
    const uint32_t key = fmix32(hash_stream_key(seed, offset) ^ fmix32(slide + 0x9E3779B9u));
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) d.rk[r] = fmix32(key + (r + 1u) * 0x85EBCA77u);
    const uint32_t bits = m > 1u ? 32u - (uint32_t)__builtin_clz(m - 1u) : 0u;      // bits(m - 1); m >= 1
    d.m = m;
    d.h = (bits + 1u) >> 1;
    return d;
}

// pi(j) for j < d.m
__host__ __device__ __forceinline__ uint32_t row_draw_index(const RowDraw& d, uint32_t j) {
    if (d.h == 0u) return 0u;
    const uint32_t mask = (1u << d.h) - 1u;         // h <= 16
    uint32_t x = j;
    do {
        uint32_t l = x >> d.h, r = x & mask;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t t = l ^ (fmix32(r ^ d.rk[i]) & mask);
            l = r;
            r = t;
        }
        x = (l << d.h) | r;
    } while (x >= d.m);
    return x;
}
