// min / max / mean of every slide's block of a ragged attention map (include/mpo_eval.h), beside mpo_map_block_dot / _scale:
// what the reference's test() prints per slide of attention_scores['coattn'] (models/nacagat/main.py:169-194), for a whole
// window in one launch chain.  Slide b's block is the n_q * M_b contiguous values from n_q * cu[b] on (BagBatch.split_map).
//
// Launch 1: workgroup (c, b) reduces chunk c (kChunk values) of slide b's block -- a chunk past the block's end leaves at
// once -- to one (sum, min, max) in its own slot of the workspace.  Launch 2: one workgroup per slide folds that slide's
// slots and writes [min, max, mean].  Every sum is carried in fp64 from the first addition (lane, wave tree, workgroup,
// slots) and rounded to fp32 once, after the division: a 100 000-row slide's mean is the correctly rounded one to within
// an ulp, whatever the signs.  The order of every addition is a function of the shape alone: no atomics, the same bits
// every time.  min and max propagate a NaN, as torch's do.
#include "../../include/mpo_hip.h"
#include "mpo_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 16;
constexpr int kChunk = kThreads * kPerThread;           // values per workgroup of launch 1

struct Stat {
    double sum;
    float lo, hi;
};
static_assert(sizeof(Stat) == 16, "one 16-byte slot per chunk");

__device__ __forceinline__ float nan_min(float a, float b) { return (b < a || b != b) ? b : a; }     // a NaN once in stays
__device__ __forceinline__ float nan_max(float a, float b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the workgroup's fold of (s, lo, hi) in thread 0: wave trees, then the waves in index order
__device__ __forceinline__ void block_fold(double& s, float& lo, float& hi) {
    __shared__ Stat red[kThreads / 64];
    s = wave_sum_f64(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = nan_min(lo, __shfl_xor(lo, o));
        hi = nan_max(hi, __shfl_xor(hi, o));
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = Stat{s, lo, hi};
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) {
            s += red[w].sum;
            lo = nan_min(lo, red[w].lo);
            hi = nan_max(hi, red[w].hi);
        }
    }
}

__global__ void __launch_bounds__(kThreads)
map_block_stats_partial_kernel(const float* __restrict__ a_map, const int* __restrict__ cu, int n_q, int max_chunks,
                               Stat* __restrict__ part) {
    const int b = blockIdx.y;
    const long long row_begin = cu[b];
    const long long len = (long long)n_q * (cu[b + 1] - row_begin);
    const long long begin = (long long)blockIdx.x * kChunk;
    if (begin >= len) return;                                   // (uniform over the workgroup)
    const float* a = a_map + n_q * row_begin + begin;
    const int count = (int)min((long long)kChunk, len - begin);
    double s = 0.0;
    float lo = INFINITY, hi = -INFINITY;
#pragma unroll 4
    for (int k = threadIdx.x; k < count; k += kThreads) {
        const float v = a[k];
        s += (double)v;
        lo = nan_min(lo, v);
        hi = nan_max(hi, v);
    }
    block_fold(s, lo, hi);
    if (threadIdx.x == 0) part[(long long)b * max_chunks + blockIdx.x] = Stat{s, lo, hi};
}

// out[b] = [min, max, mean]
__global__ void __launch_bounds__(kThreads)
map_block_stats_finish_kernel(const Stat* __restrict__ part, const int* __restrict__ cu, int n_q, int max_chunks,
                              float* __restrict__ out) {
    const int b = blockIdx.x;
    const long long len = (long long)n_q * (cu[b + 1] - cu[b]);
    const int chunks = (int)((len + kChunk - 1) / kChunk);      // (<= max_chunks: the entry sized the grid by the longest slide)
    double s = 0.0;
    float lo = INFINITY, hi = -INFINITY;
    for (int c = threadIdx.x; c < chunks && c < max_chunks; c += kThreads) {
        const Stat p = part[(long long)b * max_chunks + c];
        s += p.sum;
        lo = nan_min(lo, p.lo);
        hi = nan_max(hi, p.hi);
    }
    block_fold(s, lo, hi);
    if (threadIdx.x == 0) {
        out[3 * b] = lo;
        out[3 * b + 1] = hi;
        out[3 * b + 2] = (float)(s / (double)len);
    }
}

long long chunks_of(int n_q, int max_rows) { return ((long long)n_q * max_rows + kChunk - 1) / kChunk; }

}  // namespace

extern "C" {

size_t mpo_map_block_stats_workspace_bytes(int n_slides, int n_q, int max_rows) {
    if (n_slides < 1 || n_q < 1 || max_rows < 1) return 0;
    return (size_t)n_slides * (size_t)chunks_of(n_q, max_rows) * sizeof(Stat);
}

int mpo_map_block_stats(const float* a_map, const int32_t* cu_rows, int n_slides, int n_q, int max_rows, float* out,
                        void* workspace, size_t workspace_bytes, mpo_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPO_CHECK(a_map && cu_rows && out && n_slides >= 1 && n_q >= 1 && max_rows >= 1, "map block stats: bad argument");
    const long long chunks = chunks_of(n_q, max_rows);
    MPO_CHECK(n_slides <= 65535 && chunks <= 0x7fffffff, "map block stats: %d slides / %lld chunks per slide out of range",
              n_slides, chunks);
    MPO_CHECK(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 &&
              workspace_bytes >= mpo_map_block_stats_workspace_bytes(n_slides, n_q, max_rows),
              "map block stats: workspace null, misaligned or too small (%zu bytes)", workspace_bytes);
    Stat* part = static_cast<Stat*>(workspace);
    map_block_stats_partial_kernel<<<dim3((unsigned)chunks, n_slides), kThreads, 0, stream>>>(a_map, cu_rows, n_q, (int)chunks, part);
    MPO_LAUNCH_CHECK();
    map_block_stats_finish_kernel<<<n_slides, kThreads, 0, stream>>>(part, cu_rows, n_q, (int)chunks, out);
    MPO_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
