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
// The source is reached through a small DEVICE-resident descriptor the kernel reads at run time:
//     bytes 0..7                     base pointer of the window's rows
//     int32 cu[n_slides + 1]         the window's row offsets
//     int32 ocu[n_slides + 1]        output row offsets: ocu[b + 1] - ocu[b] = min(k, M_b)
// so a launch captured into a HIP graph follows whatever window mpo_bag_sample_bind last wrote there.  bind is one tiny
// launch: the base pointer travels as a kernel argument (copied when the launch is enqueued), cu is copied device to device
// from the window's own array, ocu is formed from it.  Ordered on the stream like any kernel: no host synchronisation, no
// staging memory that a later window could overwrite while an earlier one is still in flight.
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

__host__ __device__ inline size_t sample_desc_bytes(int n_slides) {
    return (8 + 2 * sizeof(int32_t) * (size_t)(n_slides + 1) + 15) / 16 * 16;
}

__global__ void bag_sample_bind_kernel(unsigned long long* __restrict__ desc, unsigned long long base,
                                       const int32_t* __restrict__ cu_rows, int n_slides, int k) {
    int32_t* cu = reinterpret_cast<int32_t*>(desc + 1);
    int32_t* ocu = cu + n_slides + 1;
    for (int b = threadIdx.x; b <= n_slides; b += blockDim.x) cu[b] = cu_rows[b];
    if (threadIdx.x == 0) {
        desc[0] = base;
        int32_t o = 0;
        for (int b = 0; b < n_slides; ++b) {        // (a window has tens of slides)
            ocu[b] = o;
            const int32_t m = cu_rows[b + 1] - cu_rows[b];
            o += m < k ? (m > 0 ? m : 0) : k;
        }
        ocu[n_slides] = o;
    }
}

// Virtual row v = b * k + j of the output comes from row pi_b(j) of slide b and goes to output row ocu[b] + j; rows
// j >= min(k, M_b) do not exist.  Everything below is wave-uniform: scalar loads of the descriptor, the draw on the scalar ALU.
struct RowWindow {
    const GlobalVec* base;
    GlobalVec* out;
    const int32_t* cu;
    const int32_t* ocu;
    unsigned long long seed, off;
    uint32_t total, k;
    int vecs;
};
struct SlideDraw {
    RowDraw d;
    int32_t r0, o0;
    uint32_t kb;            // min(k, M_b)
};
__device__ __forceinline__ SlideDraw slide_draw(const RowWindow& w, uint32_t b) {
    SlideDraw s;
    s.r0 = w.cu[b];
    s.o0 = w.ocu[b];
    const int32_t m = w.cu[b + 1] - s.r0, kb = w.ocu[b + 1] - s.o0;
    s.kb = (m > 0 && kb > 0) ? (uint32_t)(kb < m ? kb : m) : 0u;
    s.d = row_draw_make(w.seed, w.off, b, m > 0 ? (uint32_t)m : 1u);
    return s;
}

// VPL = 16-byte vectors per lane and row when a row is exactly 64 * VPL of them (1, 2, 4, 8: rows of 1 .. 8 KiB, i.e. the three
// patch widths in bf16 and fp32); 0 = any other width, copied in a loop.  A wave takes R consecutive virtual rows: one
// division and (unless they straddle two slides) one set of round keys for all of them, then their loads in flight
// before the stores.
template <int VPL>
__global__ void __launch_bounds__(64 * kWavesPerBlock)
bag_sample_rows_kernel(const unsigned long long* __restrict__ desc, int n_slides, int k, int vecs, unsigned long long seed,
                       unsigned long long offset, const unsigned long long* __restrict__ epoch, u32x4* __restrict__ out) {
    constexpr int R = rows_per_wave(VPL);
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));
    RowWindow w;
    w.base = reinterpret_cast<const GlobalVec*>(desc[0]);        // (global, not flat, accesses)
    w.out = (GlobalVec*)out;
    w.cu = reinterpret_cast<const int32_t*>(desc + 1);
    w.ocu = w.cu + n_slides + 1;
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
#pragma unroll
    for (int i = 0; i < R; ++i) {
        src[i] = nullptr;
        dst[i] = nullptr;
        if ((uint32_t)v0 + i < w.total) {
            if (j == w.k) {                 // the next slide begins inside this wave's rows
                j = 0;
                ++b;
                s = slide_draw(w, b);
            }
            if (j < s.kb) {
                const uint32_t p = row_draw_index(s.d, j);      // < M_b
                src[i] = w.base + (size_t)((long long)s.r0 + p) * w.vecs;
                dst[i] = w.out + (size_t)((long long)s.o0 + j) * w.vecs;
            }
            ++j;
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

size_t mpo_bag_sample_desc_bytes(int n_slides) { return n_slides < 1 ? 0 : sample_desc_bytes(n_slides); }

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

int mpo_bag_sample_rows(const void* desc, int n_slides, int k, int width, int elem_bytes, uint64_t seed, uint64_t offset,
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
    auto kernel = vpl == 1 ? bag_sample_rows_kernel<1> : vpl == 2 ? bag_sample_rows_kernel<2> : vpl == 4 ? bag_sample_rows_kernel<4>
                  : vpl == 8 ? bag_sample_rows_kernel<8> : bag_sample_rows_kernel<0>;
    kernel<<<(unsigned)blocks, 64 * kWavesPerBlock, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const unsigned long long*>(desc), n_slides, k, vecs, seed, offset,
        reinterpret_cast<const unsigned long long*>(rng_epoch), static_cast<u32x4*>(out));
    MPO_LAUNCH_CHECK();
    return 0;
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
