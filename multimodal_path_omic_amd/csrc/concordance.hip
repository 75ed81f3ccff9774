// Harrell's concordance index of a cohort on the device (include/mpo_eval.h): the metric an epoch ends with, without the
// copy to the host, the synchronisation and the n x n numpy temporaries of harness.concordance_index_censored (a
// gigabyte at 10 000 subjects).  The definition is that function's, pair by pair -- scikit-survival's conventions, which
// the reference calls (models/mcat/main.py:81):
//     event_i     = (1 - censorship_i) != 0
//     comparable  = i != j and event_i and (time_j > time_i or (time_j == time_i and not event_j))
//     diff        = (double)risk_i - (double)risk_j,   tie = |diff| <= 1e-8
//     concordant  = comparable and diff > 0 and not tie,      tied = comparable and tie
// (a NaN risk fails every comparison, as in numpy: its pairs stay comparable and are neither concordant nor tied).
//
// Counting is integer work throughout, so the result depends neither on the launch geometry nor on the order the workgroups
// finish in.  Launch 1: workgroup (x, y) owns the subjects i of tile x, one per thread, and walks the subjects j of chunk y
// through LDS a tile at a time (every lane reads the same LDS word: a broadcast); a thread's three counts are at most n
// each (32 bits), a workgroup's sum goes, as 64-bit words, to its own slot of the workspace -- nothing is zeroed and
// nothing is atomic.  Launch 2: one workgroup adds the slots and divides.  O(n^2) pair tests: 4.3e9 at n = 65 536, a few
// milliseconds; the grid (a function of n alone) cuts j into at most kMaxChunks chunks so that a cohort of a few thousand
// still fills the device.
#include "../../include/mpo_hip.h"
#include "mpo_common.h"

namespace {

constexpr int kTile = 256;                      // subjects per tile = threads per workgroup (the tests pin their sizes to it)
constexpr int kMaxChunks = 16;                  // at most this many workgroups share one tile of i
constexpr long long kMaxSubjects = 1ll << 24;   // 65 536 tiles x 16 chunks of slots; far beyond what O(n^2) is used for
constexpr double kTiedTol = 1e-8;               // scikit-survival's default tied_tol, the only one the reference uses

struct Geometry {
    int tiles;                  // ceil(n / kTile): gridDim.x
    int chunks;                 // gridDim.y
    int tiles_per_chunk;        // tiles of j a workgroup walks
};

Geometry geometry(long long n) {
    Geometry g;
    g.tiles = (int)((n + kTile - 1) / kTile);
    g.tiles_per_chunk = (g.tiles + kMaxChunks - 1) / kMaxChunks;
    g.chunks = (g.tiles + g.tiles_per_chunk - 1) / g.tiles_per_chunk;
    return g;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o);
    return v;
}

// the sum of `v` over the workgroup in thread 0 (integers: the order is immaterial)
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long* red) {
    v = wave_sum_u64(v);
    __syncthreads();                                            // (red may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long s = 0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < kTile / 64; ++w) s += red[w];
    }
    return s;
}

__global__ void __launch_bounds__(kTile)
concordance_pairs_kernel(const double* __restrict__ time, const float* __restrict__ censorship, const float* __restrict__ risk,
                         int n, int tiles_per_chunk, unsigned long long* __restrict__ part) {
    __shared__ double t_tile[kTile];
    __shared__ double r_tile[kTile];
    __shared__ int e_tile[kTile];
    __shared__ unsigned long long red[kTile / 64];
    const int i = blockIdx.x * kTile + threadIdx.x;
    const bool live = i < n;
    const double t_i = live ? time[i] : 0.0;
    const double r_i = live ? (double)risk[i] : 0.0;
    const bool e_i = live && (1.0f - censorship[i]) != 0.0f;      // (no event: no comparable pair starts at i)
    uint32_t concordant = 0, tied = 0, comparable = 0;
    const int j_begin = blockIdx.y * tiles_per_chunk * kTile;
    const int j_end = min(n, j_begin + tiles_per_chunk * kTile);
    for (int j0 = j_begin; j0 < j_end; j0 += kTile) {
        const int j = j0 + threadIdx.x;
        __syncthreads();
        if (j < j_end) {
            t_tile[threadIdx.x] = time[j];
            r_tile[threadIdx.x] = (double)risk[j];
            e_tile[threadIdx.x] = (1.0f - censorship[j]) != 0.0f;
        }
        __syncthreads();
        const int count = min(kTile, j_end - j0);
        if (e_i) {
            for (int k = 0; k < count; ++k) {
                const double t_j = t_tile[k];
                const bool comp = (j0 + k != i) && (t_j > t_i || (t_j == t_i && !e_tile[k]));
                const double diff = r_i - r_tile[k];
                const bool tie = fabs(diff) <= kTiedTol;
                comparable += comp;
                tied += comp && tie;
                concordant += comp && diff > 0.0 && !tie;
            }
        }
    }
    unsigned long long* slot = part + 3ull * ((unsigned long long)blockIdx.y * gridDim.x + blockIdx.x);
    const unsigned long long c = block_sum_u64(concordant, red);
    const unsigned long long t = block_sum_u64(tied, red);
    const unsigned long long p = block_sum_u64(comparable, red);
    if (threadIdx.x == 0) {
        slot[0] = c;
        slot[1] = t;
        slot[2] = p;
    }
}

__global__ void __launch_bounds__(kTile)
concordance_finish_kernel(const unsigned long long* __restrict__ part, int slots, long long* __restrict__ counts,
                          double* __restrict__ c_index) {
    __shared__ unsigned long long red[kTile / 64];
    unsigned long long c = 0, t = 0, p = 0;
    for (int s = threadIdx.x; s < slots; s += kTile) {
        c += part[3ull * s];
        t += part[3ull * s + 1];
        p += part[3ull * s + 2];
    }
    c = block_sum_u64(c, red);
    t = block_sum_u64(t, red);
    p = block_sum_u64(p, red);
    if (threadIdx.x == 0) {
        counts[0] = (long long)c;
        counts[1] = (long long)t;
        counts[2] = (long long)p;
        // (concordant + 0.5 tied) / comparable as the host form rounds it: both terms exact in fp64, one division
        *c_index = p != 0 ? ((double)c + 0.5 * (double)t) / (double)p : __longlong_as_double(0x7ff8000000000000ll);
    }
}

}  // namespace

extern "C" {

int mpo_concordance_tile(void) { return kTile; }

size_t mpo_concordance_workspace_bytes(int64_t n) {
    if (n < 1 || n > kMaxSubjects) return 0;
    const Geometry g = geometry(n);
    return (size_t)g.tiles * g.chunks * 3 * sizeof(unsigned long long);
}

int mpo_concordance_index(const double* time, const float* censorship, const float* risk, int64_t n, int64_t* counts,
                          double* c_index, void* workspace, size_t workspace_bytes, mpo_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPO_CHECK(n >= 1 && n <= kMaxSubjects, "concordance index: n = %lld outside 1 .. %lld", (long long)n, kMaxSubjects);
    MPO_CHECK(time && censorship && risk && counts && c_index, "concordance index: null time, censorship, risk, counts or c_index");
    MPO_CHECK(((reinterpret_cast<uintptr_t>(time) | reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(c_index)) & 7) == 0 &&
              ((reinterpret_cast<uintptr_t>(censorship) | reinterpret_cast<uintptr_t>(risk)) & 3) == 0,
              "concordance index: time, counts and c_index must be 8-byte aligned, censorship and risk 4-byte aligned");
    MPO_CHECK(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && workspace_bytes >= mpo_concordance_workspace_bytes(n),
              "concordance index: workspace null, misaligned or too small (%zu bytes)", workspace_bytes);
    const Geometry g = geometry(n);
    unsigned long long* part = static_cast<unsigned long long*>(workspace);
    concordance_pairs_kernel<<<dim3(g.tiles, g.chunks), kTile, 0, stream>>>(time, censorship, risk, (int)n, g.tiles_per_chunk, part);
    MPO_LAUNCH_CHECK();
    concordance_finish_kernel<<<1, kTile, 0, stream>>>(part, g.tiles * g.chunks, reinterpret_cast<long long*>(counts), c_index);
    MPO_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
