// Fixed-budget patch sampling: gather k randomly chosen rows of every slide of a ragged window into a buffer of static shape
// (n_slides * k, width), so that everything behind it sees the same lengths, plan and grids for every window.  Beyond the
// reference (its loops feed every patch of a slide); off unless asked for.
//
// A memory-bound row gather.  A wave moves a few output rows at a time: their source rows pi_b(j) (csrc/bag_sample.h) are
// computed once per row on the scalar unit (the wave index goes through readfirstlane, so everything derived from it is
// wave-uniform), then every lane moves 16 bytes per instruction, four loads in flight before the stores.
// No LDS, no scratch, no atomics; vector loads and stores with the nontemporal hint: a source row is read once and the
// output (268 MB at 32 x 4 096 x 1024 bf16) is far larger than the L2, so neither should displace what is resident --
// measured 87 us against 102 us with plain accesses, bit-identical.
//
// ONE gather, two kinds of window.  The source is reached through a small DEVICE-resident descriptor the kernel reads at run
// time, so a launch captured into a HIP graph follows whatever window was last bound there; a source type (below) per layout:
//
//     WindowSource: a contiguous window              SlidesSource: separately stored slides (include/mpo_cohort.h)
//     bytes 0..7        base pointer of its rows     uint64 ptr[n_slides]      address of each slide's first row
//     int32 cu[n + 1]   the window's row offsets     int32  len[n_slides]      its rows M_b (0: nothing is gathered for it)
//     int32 ocu[n + 1]  output row offsets           int32  ocu[n_slides + 1]  output row offsets
//     row pi_b(j) at base + (cu[b] + pi_b(j)) * row_bytes                      at ptr[b] + pi_b(j) * row_bytes
//
// and that address is the one difference: same draw, same rows-per-wave rule, same five instantiations.  A SlideSet window is a
// list of slide ids into a cohort resident on the device; a shuffled epoch groups the slides into other windows every time and
// the window is never assembled -- no copy, no per-window H2D transfer, no host synchronisation.  Per-slide pointers: the
// cohort's total row count has no 32-bit limit, only a slide's own rows (int32) and the window's output rows (2^31 - 1) do.
//
// A bind is one tiny single-wave launch, ordered on the stream like any kernel: no host synchronisation, no staging memory
// that a later window could overwrite while an earlier one is still in flight.
//   mpo_bag_sample_bind: the base pointer travels as a kernel argument (copied when the launch is enqueued), cu is copied
//     device to device from the window's own array; ocu[b + 1] - ocu[b] = min(k, M_b).
//   mpo_bag_sample_bind_slides: from the cohort's DEVICE table (ptr / len of every slide, written once when the cohort is
//     built) and a DEVICE array of slide ids (a slice of the epoch's order, uploaded once per epoch): an id outside the table,
//     or a table pointer that is not 16-byte aligned, gets length 0 -- the gather writes nothing for it and never reads
//     outside the table.
//
// Lapping (`cycle`, slides only): ocu[b + 1] - ocu[b] = k for every slide; where that exceeds M_b, output row j comes from
// pi_b(j mod M_b): the slide is lapped in its permuted order, every source row appears floor(k / M_b) or ceil(k / M_b) times,
// and a lap is complete before any row repeats.  The walk of row_draw_index still starts at j mod M_b < M_b, so the
// termination argument of bag_sample.h (the walk follows the cycle of its start, which returns to a value < M_b) holds unchanged.
#include "../../include/mpo_hip.h"
#include "bag_sample.h"

namespace {

constexpr int kRowsPerWave = 4;
constexpr int kWavesPerBlock = 4;
// rows a wave moves, by 16-byte vectors per lane and row (0: the loop form): four loads in flight (eight for an 8 KiB row).
// Measured at 2 KiB rows: 2 rows per wave beat 4 by 2-5 %; more than 4 spill their addresses out of the scalar registers.
__host__ __device__ constexpr int rows_per_wave(int vpl) { return vpl >= 4 ? 1 : vpl == 2 ? 2 : kRowsPerWave; }
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;                  // 16 bytes per lane
typedef __attribute__((address_space(1))) u32x4 GlobalVec;

// One slide as the gather sees it: virtual row v = b * k + j of the output comes from row pi_b(j) of slide b (pi_b(j mod M_b)
// where the source laps) and goes to output row o0 + j; rows j >= kb do not exist.
struct SlideDraw {
    RowDraw d;
    const GlobalVec* rows;  // the slide's first row (global, not flat, accesses)
    int32_t o0;
    uint32_t kb;            // output rows of the slide (0 for a slide without rows)
    uint32_t m;             // M_b (1 where the slide has none: kb is 0 then)
};
__device__ __forceinline__ SlideDraw slide_draw(const GlobalVec* rows, int32_t m, int32_t o0, int32_t kb, unsigned long long seed,
                                                unsigned long long off, uint32_t b) {
    SlideDraw s;
    s.rows = rows;
    s.o0 = o0;
    s.kb = (m > 0 && kb > 0) ? (uint32_t)kb : 0u;
    s.m = m > 0 ? (uint32_t)m : 1u;
    s.d = row_draw_make(seed, off, b, s.m);
    return s;
}

// The two descriptor layouts.  Everything here is wave-uniform: scalar loads of the descriptor, the draw on the scalar ALU.
struct WindowSource {           // base | cu[n + 1] | ocu[n + 1]
    static constexpr bool kLaps = false;
    const GlobalVec* base;
    const int32_t *cu, *ocu;
    int vecs;
    __host__ __device__ static size_t desc_bytes(int n) { return (8 + 2 * sizeof(int32_t) * (size_t)(n + 1) + 15) / 16 * 16; }
    __device__ __forceinline__ WindowSource(const unsigned long long* desc, int n, int vecs_)
        : base(reinterpret_cast<const GlobalVec*>(desc[0])), cu(reinterpret_cast<const int32_t*>(desc + 1)), ocu(cu + n + 1),
          vecs(vecs_) {}
    __device__ __forceinline__ SlideDraw draw(unsigned long long seed, unsigned long long off, uint32_t b) const {
        const int32_t r0 = cu[b], m = cu[b + 1] - r0, o0 = ocu[b], kb = ocu[b + 1] - o0;
        return slide_draw(base + (size_t)(long long)r0 * vecs, m, o0, kb < m ? kb : m, seed, off, b);
    }
};
struct SlidesSource {           // ptr[n] | len[n] | ocu[n + 1]
    static constexpr bool kLaps = true;
    const unsigned long long* ptr;
    const int32_t *len, *ocu;
    __host__ __device__ static size_t desc_bytes(int n) {
        return (sizeof(uint64_t) * (size_t)n + sizeof(int32_t) * (size_t)n + sizeof(int32_t) * (size_t)(n + 1) + 15) / 16 * 16;
    }
    __device__ __forceinline__ SlidesSource(const unsigned long long* desc, int n, int)
        : ptr(desc), len(reinterpret_cast<const int32_t*>(desc + n)), ocu(len + n) {}
    __device__ __forceinline__ SlideDraw draw(unsigned long long seed, unsigned long long off, uint32_t b) const {
        const int32_t o0 = ocu[b];
        return slide_draw(reinterpret_cast<const GlobalVec*>(ptr[b]), len[b], o0, ocu[b + 1] - o0, seed, off, b);
    }
};

// ocu of a binding, by the one wave of a bind kernel: 64 slides per trip, take(b) = output rows of slide b (all lanes' loads
// in flight together), the offsets a prefix sum across the wave with a carry from trip to trip -- two memory latencies per
// trip, not two per slide.
template <class Take>
__device__ __forceinline__ void bind_output_offsets(int32_t* __restrict__ ocu, int n_slides, Take take) {
    const int lane = threadIdx.x;
    int32_t carry = 0;
    for (int b0 = 0; b0 < n_slides; b0 += 64) {
        const int b = b0 + lane;
        const int32_t t = b < n_slides ? take(b) : 0;
        int32_t incl = t;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (b < n_slides) ocu[b] = carry + incl - t;
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) ocu[n_slides] = carry;
}

__global__ void bag_sample_bind_kernel(unsigned long long* __restrict__ desc, unsigned long long base,
                                       const int32_t* __restrict__ cu_rows, int n_slides, int k) {
    int32_t* cu = reinterpret_cast<int32_t*>(desc + 1);
    if (threadIdx.x == 0) desc[0] = base;
    for (int b = threadIdx.x; b <= n_slides; b += 64) cu[b] = cu_rows[b];
    bind_output_offsets(cu + n_slides + 1, n_slides, [&](int b) {
        const int32_t m = cu_rows[b + 1] - cu_rows[b];
        return m < k ? (m > 0 ? m : 0) : k;
    });
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
    bind_output_offsets(len + n_slides, n_slides, [&](int b) {      // a lane looks its slide up: two dependent loads
        const int32_t id = ids[b];
        const int32_t m = table_len(table_ptrs, table_lens, n_table, id);
        desc[b] = m > 0 ? table_ptrs[id] : 0ull;
        len[b] = m;
        return (cycle || m >= k) ? k : m;
    });
}

// VPL = 16-byte vectors per lane and row when a row is exactly 64 * VPL of them (1, 2, 4, 8: rows of 1 .. 8 KiB, i.e. the three
// patch widths in bf16 and fp32); 0 = any other width, copied in a loop.  A wave takes R consecutive virtual rows: one
// division and (unless they straddle two slides) one set of round keys for all of them, then their loads in flight
// before the stores.  A source that laps keeps jm = j mod M_b beside j: one division per wave, only where the slide is
// lapped at all, then a compare per row; the other source's j < kb <= M_b needs none of it.
template <class Source, int VPL>
__global__ void __launch_bounds__(64 * kWavesPerBlock)
bag_gather_kernel(const unsigned long long* __restrict__ desc, int n_slides, int k, int vecs, unsigned long long seed,
                  unsigned long long offset, const unsigned long long* __restrict__ epoch, u32x4* __restrict__ out_) {
    constexpr int R = rows_per_wave(VPL);
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));
    const Source w(desc, n_slides, vecs);
    GlobalVec* const out = (GlobalVec*)out_;
    const unsigned long long off = epoch_offset(offset, epoch);
    const uint32_t total = (uint32_t)n_slides * (uint32_t)k, uk = (uint32_t)k;      // (the launcher refuses more than 2^31 - 1 rows)
    const unsigned long long v0 = (unsigned long long)wave * R;
    if (v0 >= total) return;

    const GlobalVec* src[R];
    GlobalVec* dst[R];
    uint32_t b = (uint32_t)v0 / uk, j = (uint32_t)v0 - b * uk;
    SlideDraw s = w.draw(seed, off, b);
    uint32_t jm = j;
    if constexpr (Source::kLaps) jm = j < s.m ? j : j % s.m;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        src[i] = nullptr;
        dst[i] = nullptr;
        if ((uint32_t)v0 + i < total) {
            if (j == uk) {                  // the next slide begins inside this wave's rows
                j = 0;
                jm = 0;
                ++b;
                s = w.draw(seed, off, b);
            }
            if (j < s.kb) {
                const uint32_t p = row_draw_index(s.d, Source::kLaps ? jm : j);     // its argument < M_b
                src[i] = s.rows + (size_t)p * vecs;
                dst[i] = out + (size_t)((long long)s.o0 + j) * vecs;
            }
            ++j;
            if constexpr (Source::kLaps)
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

template <class Source>
int launch_gather(const void* desc, int n_slides, int k, int width, int elem_bytes, uint64_t seed, uint64_t offset,
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
    auto kernel = vpl == 1 ? bag_gather_kernel<Source, 1> : vpl == 2 ? bag_gather_kernel<Source, 2>
                  : vpl == 4 ? bag_gather_kernel<Source, 4> : vpl == 8 ? bag_gather_kernel<Source, 8> : bag_gather_kernel<Source, 0>;
    kernel<<<(unsigned)blocks, 64 * kWavesPerBlock, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const unsigned long long*>(desc), n_slides, k, vecs, seed, offset,
        reinterpret_cast<const unsigned long long*>(rng_epoch), static_cast<u32x4*>(out));
    MPO_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

size_t mpo_bag_sample_desc_bytes(int n_slides) { return n_slides < 1 ? 0 : WindowSource::desc_bytes(n_slides); }
size_t mpo_bag_sample_slides_desc_bytes(int n_slides) { return n_slides < 1 ? 0 : SlidesSource::desc_bytes(n_slides); }

int mpo_bag_sample_bind(void* desc, const void* rows, const int32_t* cu_rows, int n_slides, int k, mpo_stream_t stream) {
    MPO_CHECK(desc && rows && cu_rows, "bag sample bind: null argument");
    MPO_CHECK(n_slides >= 1, "bag sample: n_slides %d < 1", n_slides);
    MPO_CHECK(k >= 1, "bag sample: k %d < 1", k);
    MPO_CHECK((reinterpret_cast<uintptr_t>(desc) & 7) == 0, "bag sample bind: the descriptor must be 8-byte aligned");
    MPO_CHECK((reinterpret_cast<uintptr_t>(rows) & 15) == 0, "bag sample bind: the window's rows must be 16-byte aligned");
    bag_sample_bind_kernel<<<1, 64, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<unsigned long long*>(desc), (unsigned long long)reinterpret_cast<uintptr_t>(rows), cu_rows, n_slides, k);
    MPO_LAUNCH_CHECK();
    return 0;
}

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

int mpo_bag_sample_rows(const void* desc, int n_slides, int k, int width, int elem_bytes, uint64_t seed, uint64_t offset,
                        const uint64_t* rng_epoch, void* out, mpo_stream_t stream) {
    return launch_gather<WindowSource>(desc, n_slides, k, width, elem_bytes, seed, offset, rng_epoch, out, stream);
}

int mpo_bag_sample_slides(const void* desc, int n_slides, int k, int width, int elem_bytes, uint64_t seed, uint64_t offset,
                          const uint64_t* rng_epoch, void* out, mpo_stream_t stream) {
    return launch_gather<SlidesSource>(desc, n_slides, k, width, elem_bytes, seed, offset, rng_epoch, out, stream);
}

int mpo_bag_sample_indices_host(const int32_t* lengths, int n_slides, int k, uint64_t seed, uint64_t offset, uint64_t epoch,
                                int32_t* indices) {
    MPO_CHECK(lengths && indices, "bag sample: null argument");
    MPO_CHECK(n_slides >= 1, "bag sample: n_slides %d < 1", n_slides);
    MPO_CHECK(k >= 1, "bag sample: k %d < 1", k);
    for (int b = 0; b < n_slides; ++b) MPO_CHECK(lengths[b] >= 1, "bag sample: slide %d has %d rows", b, (int)lengths[b]);
    const unsigned long long off = offset + epoch * kEpochStride;
    for (int b = 0; b < n_slides; ++b) {
        const RowDraw d = row_draw_make(seed, off, (uint32_t)b, (uint32_t)lengths[b]);
        for (int j = 0; j < k; ++j)
            indices[(size_t)b * k + j] = j < lengths[b] ? (int32_t)row_draw_index(d, (uint32_t)j) : -1;
    }
    return 0;
}

}  // extern "C"
