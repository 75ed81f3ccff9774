// Fixed-budget patch sampling from SEPARATELY STORED slides: the gather of csrc/bag_sample.hip for a window that is a list
// of slide ids into a cohort resident on the device, instead of one contiguous slab.  A shuffled epoch groups the slides into
// other windows every time; with this gather the window is never assembled -- no copy, no per-window H2D transfer, no host
// synchronisation.  Same draw (csrc/bag_sample.h, unchanged), same rows-per-wave rule, same five instantiations, same
// nontemporal loads and stores as the contiguous gather; the one difference in the address is ptr[b] + pi_b(j) * row_bytes
// instead of base + (cu[b] + pi_b(j)) * row_bytes.  Per-slide pointers: the cohort's total row count has no 32-bit limit,
// only a slide's own rows (int32) and the window's output rows (2^31 - 1) do.
//
// The source is reached through a DEVICE-resident descriptor the kernel reads at run time:
//     uint64 ptr[n_slides]           address of each slide's first row
//     int32  len[n_slides]           its rows M_b (0: nothing is gathered for this slide)
//     int32  ocu[n_slides + 1]       output row offsets
// mpo_bag_sample_bind_slides writes it with one tiny launch from the cohort's DEVICE table (ptr / len of every slide, written
// once when the cohort is built) and a DEVICE array of slide ids (a slice of the epoch's order, uploaded once per epoch): an
// id outside the table, or a table pointer that is not 16-byte aligned, gets length 0 -- the gather writes nothing for it and
// never reads outside the table.  Ordered on the stream like any kernel.
//
// Lapping (`cycle`): ocu[b + 1] - ocu[b] = k for every slide; where that exceeds M_b, output row j comes from pi_b(j mod M_b):
// the slide is lapped in its permuted order, every source row appears floor(k / M_b) or ceil(k / M_b) times, and a lap is
// complete before any row repeats.  The walk of row_draw_index still starts at j mod M_b < M_b, so the termination argument
// of bag_sample.h (the walk follows the cycle of its start, which returns to a value < M_b) holds unchanged.
#include "../../include/mpo_hip.h"
#include "bag_sample.h"

namespace {

constexpr int kRowsPerWave = 4;
constexpr int kWavesPerBlock = 4;
// (csrc/bag_sample.hip's rule, restated: four loads in flight, eight for an 8 KiB row)
__host__ __device__ constexpr int rows_per_wave(int vpl) { return vpl >= 4 ? 1 : vpl == 2 ? 2 : kRowsPerWave; }
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;                  // 16 bytes per lane
typedef __attribute__((address_space(1))) u32x4 GlobalVec;

__host__ __device__ inline size_t slides_desc_bytes(int n_slides) {
    return (sizeof(uint64_t) * (size_t)n_slides + sizeof(int32_t) * (size_t)n_slides + sizeof(int32_t) * (size_t)(n_slides + 1) + 15) /
           16 * 16;
}

// length of the slide `id` names as the gather may use it: 0 for an id outside the table, a negative length or a pointer
// the 16-byte accesses cannot take
__device__ __forceinline__ int32_t table_len(const unsigned long long* __restrict__ table_ptrs, const int32_t* __restrict__ table_lens,
                                             int n_table, int32_t id) {
    if (id < 0 || id >= n_table) return 0;
    const int32_t m = table_lens[id];
    return (m > 0 && (table_ptrs[id] & 15ull) == 0) ? m : 0;
}

__global__ void bag_sample_bind_slides_kernel(unsigned long long* __restrict__ desc, const unsigned long long* __restrict__ table_ptrs,
                                              const int32_t* __restrict__ table_lens, int n_table, const int32_t* __restrict__ ids,
                                              int n_slides, int k, int cycle) {
    int32_t* len = reinterpret_cast<int32_t*>(desc + n_slides);
    int32_t* ocu = len + n_slides;
    // one wave, 64 slides per trip: a lane looks its slide up (two dependent loads, all lanes' in flight together) and the
    // output offsets are a prefix sum across the wave, so the launch costs two memory latencies, not two per slide
    const int lane = threadIdx.x;
    int32_t carry = 0;
    for (int b0 = 0; b0 < n_slides; b0 += 64) {
        const int b = b0 + lane;
        int32_t take = 0;
        if (b < n_slides) {
            const int32_t id = ids[b];
            const int32_t m = table_len(table_ptrs, table_lens, n_table, id);
            desc[b] = m > 0 ? table_ptrs[id] : 0ull;
            len[b] = m;
            take = (cycle || m >= k) ? k : m;
        }
        int32_t incl = take;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (b < n_slides) ocu[b] = carry + incl - take;
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) ocu[n_slides] = carry;
}

// Virtual row v = b * k + j of the output comes from row pi_b(j mod M_b) of slide b and goes to output row ocu[b] + j; rows
// j >= ocu[b + 1] - ocu[b] do not exist, nor does any row of a slide of length 0.  Everything below is wave-uniform: scalar
// loads of the descriptor, the draw on the scalar ALU.
struct SlideWindow {
    const unsigned long long* ptr;
    GlobalVec* out;
    const int32_t* len;
    const int32_t* ocu;
    unsigned long long seed, off;
    uint32_t total, k;
    int vecs;
};
struct SlideDraw {
    RowDraw d;
    const GlobalVec* rows;
    int32_t o0;
    uint32_t kb;            // output rows of the slide
    uint32_t m;             // M_b (1 where the slide has none: kb is 0 then)
};
__device__ __forceinline__ SlideDraw slide_draw(const SlideWindow& w, uint32_t b) {
    SlideDraw s;
    s.rows = reinterpret_cast<const GlobalVec*>(w.ptr[b]);          // (global, not flat, accesses)
    s.o0 = w.ocu[b];
    const int32_t m = w.len[b], kb = w.ocu[b + 1] - s.o0;
    s.kb = (m > 0 && kb > 0) ? (uint32_t)kb : 0u;
    s.m = m > 0 ? (uint32_t)m : 1u;
    s.d = row_draw_make(w.seed, w.off, b, s.m);
    return s;
}

// VPL as in csrc/bag_sample.hip: 16-byte vectors per lane and row (1, 2, 4, 8), 0 = any other width in a loop.  jm = j mod M_b
// is kept beside j: one division per wave, only where the slide is lapped at all, then a compare per row.
template <int VPL>
__global__ void __launch_bounds__(64 * kWavesPerBlock)
bag_sample_slides_kernel(const unsigned long long* __restrict__ desc, int n_slides, int k, int vecs, unsigned long long seed,
                         unsigned long long offset, const unsigned long long* __restrict__ epoch, u32x4* __restrict__ out) {
    constexpr int R = rows_per_wave(VPL);
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));
    SlideWindow w;
    w.ptr = desc;
    w.out = (GlobalVec*)out;
    w.len = reinterpret_cast<const int32_t*>(desc + n_slides);
    w.ocu = w.len + n_slides;
    w.seed = seed;
    w.off = epoch_offset(offset, epoch);
    w.total = (uint32_t)n_slides * (uint32_t)k;                 // (the launcher refuses more than 2^31 - 1 rows)
    w.k = (uint32_t)k;
    w.vecs = vecs;
    const unsigned long long v0 = (unsigned long long)wave * R;
    if (v0 >= w.total) return;

    const GlobalVec* src[R];
    GlobalVec* dst[R];
    uint32_t b = (uint32_t)v0 / w.k, j = (uint32_t)v0 - b * w.k;
    SlideDraw s = slide_draw(w, b);
    uint32_t jm = j < s.m ? j : j % s.m;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        src[i] = nullptr;
        dst[i] = nullptr;
        if ((uint32_t)v0 + i < w.total) {
            if (j == w.k) {                 // the next slide begins inside this wave's rows
                j = 0;
                jm = 0;
                ++b;
                s = slide_draw(w, b);
            }
            if (j < s.kb) {
                const uint32_t p = row_draw_index(s.d, jm);     // jm < M_b
                src[i] = s.rows + (size_t)p * w.vecs;
                dst[i] = w.out + (size_t)((long long)s.o0 + j) * w.vecs;
            }
            ++j;
            if (++jm == s.m) jm = 0;
        }
    }
    if constexpr (VPL > 0) {
        u32x4 x[R][VPL];
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
            for (int c = 0; c < VPL; ++c) {
                x[i][c] = u32x4{0u, 0u, 0u, 0u};
                if (src[i]) x[i][c] = __builtin_nontemporal_load(src[i] + lane + 64 * c);
            }
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
            for (int c = 0; c < VPL; ++c)
                if (src[i]) __builtin_nontemporal_store(x[i][c], dst[i] + lane + 64 * c);
    } else {
        for (int c = lane; c < vecs; c += 64) {
            u32x4 x[R];
#pragma unroll
            for (int i = 0; i < R; ++i) {
                x[i] = u32x4{0u, 0u, 0u, 0u};
                if (src[i]) x[i] = __builtin_nontemporal_load(src[i] + c);
            }
#pragma unroll
            for (int i = 0; i < R; ++i)
                if (src[i]) __builtin_nontemporal_store(x[i], dst[i] + c);
        }
    }
}

}  // namespace

extern "C" {

size_t mpo_bag_sample_slides_desc_bytes(int n_slides) { return n_slides < 1 ? 0 : slides_desc_bytes(n_slides); }

int mpo_bag_sample_bind_slides(void* desc, const uint64_t* table_ptrs, const int32_t* table_lens, int n_table, const int32_t* ids,
                               int n_slides, int k, int cycle, mpo_stream_t stream) {
    MPO_CHECK(desc && table_ptrs && table_lens && ids, "bag sample bind: null argument");
    MPO_CHECK(n_slides >= 1, "bag sample: n_slides %d < 1", n_slides);
    MPO_CHECK(k >= 1, "bag sample: k %d < 1", k);
    MPO_CHECK(n_table >= 1, "bag sample: n_table %d < 1", n_table);
    MPO_CHECK((reinterpret_cast<uintptr_t>(desc) & 7) == 0, "bag sample bind: the descriptor must be 8-byte aligned");
    MPO_CHECK((long long)n_slides * k <= 0x7FFFFFFFll, "bag sample: %lld output rows do not fit 32-bit row indices",
              (long long)n_slides * k);
    bag_sample_bind_slides_kernel<<<1, 64, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<unsigned long long*>(desc), reinterpret_cast<const unsigned long long*>(table_ptrs), table_lens, n_table, ids,
        n_slides, k, cycle != 0);
    MPO_LAUNCH_CHECK();
    return 0;
}

int mpo_bag_sample_slides(const void* desc, int n_slides, int k, int width, int elem_bytes, uint64_t seed, uint64_t offset,
                          const uint64_t* rng_epoch, void* out, mpo_stream_t stream) {
    MPO_CHECK(desc && out, "bag sample: null argument");
    MPO_CHECK(n_slides >= 1, "bag sample: n_slides %d < 1", n_slides);
    MPO_CHECK(k >= 1, "bag sample: k %d < 1", k);
    MPO_CHECK(elem_bytes == 2 || elem_bytes == 4, "bag sample: element size %d (bf16 = 2 or fp32 = 4)", elem_bytes);
    MPO_CHECK(width >= 1 && ((long long)width * elem_bytes) % 16 == 0,
              "bag sample: a row of %d x %d bytes is not a multiple of 16 bytes", width, elem_bytes);
    MPO_CHECK((reinterpret_cast<uintptr_t>(out) & 15) == 0, "bag sample: the output must be 16-byte aligned");
    const long long rows = (long long)n_slides * k;
    MPO_CHECK(rows <= 0x7FFFFFFFll, "bag sample: %lld output rows do not fit 32-bit row indices", rows);
    const int vecs = (int)((long long)width * elem_bytes / 16);
    const int vpl = (vecs == 64 || vecs == 128 || vecs == 256 || vecs == 512) ? vecs / 64 : 0;
    const int rows_per_chunk = rows_per_wave(vpl);
    const long long blocks = ((rows + rows_per_chunk - 1) / rows_per_chunk + kWavesPerBlock - 1) / kWavesPerBlock;
    auto kernel = vpl == 1 ? bag_sample_slides_kernel<1> : vpl == 2 ? bag_sample_slides_kernel<2>
                  : vpl == 4 ? bag_sample_slides_kernel<4> : vpl == 8 ? bag_sample_slides_kernel<8> : bag_sample_slides_kernel<0>;
    kernel<<<(unsigned)blocks, 64 * kWavesPerBlock, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const unsigned long long*>(desc), n_slides, k, vecs, seed, offset,
        reinterpret_cast<const unsigned long long*>(rng_epoch), static_cast<u32x4*>(out));
    MPO_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
