// Classification metrics of a set of slides on the device (include/mpo_classify.h): what the gene-expression model's
// validation ends with -- predictions, the confusion matrix, accuracy, balanced accuracy and the mean loss -- without the copy
// of Y to the host and the per-slide .item() of the reference's loop (models/ge_nacagat/main.py:85-142).  The definition is
// harness.classification_metrics', row by row:
//     pred_b      = torch.argmax(y[b]): the first index of a NaN if the row holds one, otherwise the first index of the maximum
//     valid_b     = 0 <= label_b < C
//     confusion[label_b][pred_b] += 1 over valid rows
//     counts      = valid, correct (the trace), invalid labels, rows that hold a NaN (valid or not)
//
// Counting is integer work throughout, so counts and confusion depend neither on the launch geometry nor on the order the
// workgroups finish in.  Launch 1: a workgroup walks its tiles of kTile rows, one row per thread.  A wave counts a tile's
// rows per confusion cell with one ballot per cell; lane c of every wave keeps the count of cell c in a register -- no
// atomics, not even in LDS.  The loss is added per thread in fp64 from the first addition, then over the wave and the
// workgroup in a fixed tree.  A workgroup's C*C + 2 words go to its own column of the workspace (word-major, so that the
// second launch reads along lanes); nothing is zeroed.  Launch 2: one workgroup adds the columns -- a wave per word, lanes
// over workgroups, the same tree -- and thread 0 forms the three fp64 figures.  The grid is a function of n alone, and so
// is the order of every floating-point addition.
#include "../../include/mpo_hip.h"
#include "mpo_common.h"

namespace {

constexpr int kTile = 256;                      // rows per tile = threads per workgroup (the tests pin their sizes to it)
constexpr int kWaves = kTile / 64;
constexpr int kMaxGroups = 256;                 // workgroups of the first launch at most: one per CU, a few tiles each beyond
constexpr long long kMaxRows = 1ll << 24;
constexpr int kMinClasses = 2, kMaxClasses = 8; // the head's range (csrc/ge_head.hip)
constexpr int kMaxCells = kMaxClasses * kMaxClasses;            // <= 64: one lane per confusion cell

struct Geometry {
    int tiles;                  // ceil(n / kTile)
    int tiles_per_group;        // tiles a workgroup walks
    int groups;                 // gridDim.x of the first launch = columns of the workspace
};

Geometry geometry(long long n) {
    Geometry g;
    g.tiles = (int)((n + kTile - 1) / kTile);
    g.tiles_per_group = (g.tiles + kMaxGroups - 1) / kMaxGroups;
    g.groups = (g.tiles + g.tiles_per_group - 1) / g.tiles_per_group;
    return g;
}

// words of one workgroup's column: the C*C cells, the rows with a NaN, the loss sum (a double in the same 8 bytes)
__host__ __device__ __forceinline__ int words_of(int n_classes) { return n_classes * n_classes + 2; }

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o);
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

__global__ void __launch_bounds__(kTile)
class_metrics_rows_kernel(const float* __restrict__ y, const long long* __restrict__ label, const float* __restrict__ loss,
                          int n, int n_classes, int tiles_per_group, long long* __restrict__ pred,
                          unsigned long long* __restrict__ part) {
    __shared__ unsigned long long cell_red[kWaves][kMaxCells];
    __shared__ unsigned long long nan_red[kWaves];
    __shared__ double loss_red[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cells = n_classes * n_classes;
    uint32_t cell_count = 0;            // lane c: this wave's rows in cell c (a workgroup walks at most 2^16 rows)
    uint32_t nan_rows = 0;
    double loss_sum = 0.0;
    const int first = blockIdx.x * tiles_per_group * kTile;
    const int last = min(n, first + tiles_per_group * kTile);
    for (int i0 = first; i0 < last; i0 += kTile) {
        const int i = i0 + threadIdx.x;
        int cell = -1;
        if (i < last) {
            const float* row = y + (size_t)i * n_classes;
            float best = row[0];
            int arg = 0;
            bool has_nan = best != best;
            for (int c = 1; c < n_classes; ++c) {
                const float v = row[c];
                const bool v_nan = v != v;
                // a NaN already found stays; otherwise a NaN wins, then a strictly larger value (ties: the first index)
                if (!(best != best) && (v_nan || v > best)) {
                    best = v;
                    arg = c;
                }
                has_nan |= v_nan;
            }
            nan_rows += has_nan;
            if (pred) pred[i] = arg;
            const long long l = label[i];
            if (l >= 0 && l < n_classes) cell = (int)l * n_classes + arg;
            if (loss) loss_sum += (double)loss[i];
        }
        for (int c = 0; c < cells; ++c) {
            const unsigned long long rows = __ballot(cell == c);
            if (lane == c) cell_count += (uint32_t)__popcll(rows);
        }
    }
    cell_red[wave][lane] = cell_count;
    const unsigned long long nan_wave = wave_sum_u64(nan_rows);
    const double loss_wave = wave_sum_f64(loss_sum);
    if (lane == 0) {
        nan_red[wave] = nan_wave;
        loss_red[wave] = loss_wave;
    }
    __syncthreads();
    const size_t groups = gridDim.x;
    if ((int)threadIdx.x < cells) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += cell_red[w][threadIdx.x];
        part[(size_t)threadIdx.x * groups + blockIdx.x] = s;
    }
    if (threadIdx.x == 64) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += nan_red[w];
        part[(size_t)cells * groups + blockIdx.x] = s;
    }
    if (threadIdx.x == 128) {
        double s = loss_red[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) s += loss_red[w];
        part[(size_t)(cells + 1) * groups + blockIdx.x] = (unsigned long long)__double_as_longlong(s);
    }
}

__global__ void __launch_bounds__(kTile)
class_metrics_finish_kernel(const unsigned long long* __restrict__ part, int groups, int n, int n_classes, int has_loss,
                            long long* __restrict__ confusion, long long* __restrict__ counts, double* __restrict__ summary) {
    __shared__ unsigned long long total[kMaxCells + 1];
    __shared__ double loss_total;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cells = n_classes * n_classes;
    for (int w = wave; w < cells + 2; w += kWaves) {                   // (wave-uniform)
        const unsigned long long* word = part + (size_t)w * groups;
        if (w <= cells) {
            unsigned long long s = 0;
            for (int g = lane; g < groups; g += 64) s += word[g];
            s = wave_sum_u64(s);
            if (lane == 0) total[w] = s;
        } else {
            double s = 0.0;
            for (int g = lane; g < groups; g += 64) s += __longlong_as_double((long long)word[g]);
            s = wave_sum_f64(s);
            if (lane == 0) loss_total = s;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < cells) confusion[threadIdx.x] = (long long)total[threadIdx.x];
    if (threadIdx.x == 0) {
        unsigned long long valid = 0, correct = 0;
        double recall_sum = 0.0;
        int with_support = 0;
        for (int c = 0; c < n_classes; ++c) {                          // class order: the host form's
            unsigned long long support = 0;
            for (int p = 0; p < n_classes; ++p) support += total[c * n_classes + p];
            const unsigned long long hit = total[c * n_classes + c];
            valid += support;
            correct += hit;
            if (support != 0) {
                recall_sum += (double)hit / (double)support;
                ++with_support;
            }
        }
        counts[0] = (long long)valid;
        counts[1] = (long long)correct;
        counts[2] = (long long)n - (long long)valid;
        counts[3] = (long long)total[cells];
        summary[0] = valid != 0 ? (double)correct / (double)valid : quiet_nan();
        summary[1] = with_support != 0 ? recall_sum / (double)with_support : quiet_nan();
        summary[2] = has_loss ? loss_total / (double)n : quiet_nan();
    }
}

}  // namespace

extern "C" {

int mpo_class_metrics_tile(void) { return kTile; }

size_t mpo_class_metrics_workspace_bytes(int64_t n, int n_classes) {
    if (n < 1 || n > kMaxRows || n_classes < kMinClasses || n_classes > kMaxClasses) return 0;
    return (size_t)geometry(n).groups * words_of(n_classes) * sizeof(unsigned long long);
}

int mpo_class_metrics(const float* y, const int64_t* label, const float* loss, int64_t n, int n_classes, int64_t* pred,
                      int64_t* confusion, int64_t* counts, double* summary, void* workspace, size_t workspace_bytes,
                      mpo_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPO_CHECK(n >= 1 && n <= kMaxRows, "class metrics: n = %lld outside 1 .. %lld", (long long)n, kMaxRows);
    MPO_CHECK(n_classes >= kMinClasses && n_classes <= kMaxClasses, "class metrics: n_classes = %d outside %d .. %d", n_classes,
              kMinClasses, kMaxClasses);
    MPO_CHECK(y && label && confusion && counts && summary, "class metrics: null y, label, confusion, counts or summary");
    MPO_CHECK(((reinterpret_cast<uintptr_t>(label) | reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(confusion) |
                reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(summary)) & 7) == 0 &&
              ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(loss)) & 3) == 0,
              "class metrics: label, pred, confusion, counts and summary must be 8-byte aligned, y and loss 4-byte aligned");
    MPO_CHECK(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 &&
              workspace_bytes >= mpo_class_metrics_workspace_bytes(n, n_classes),
              "class metrics: workspace null, misaligned or too small (%zu bytes)", workspace_bytes);
    const Geometry g = geometry(n);
    unsigned long long* part = static_cast<unsigned long long*>(workspace);
    class_metrics_rows_kernel<<<g.groups, kTile, 0, stream>>>(y, reinterpret_cast<const long long*>(label), loss, (int)n, n_classes,
                                                             g.tiles_per_group, reinterpret_cast<long long*>(pred), part);
    MPO_LAUNCH_CHECK();
    class_metrics_finish_kernel<<<1, kTile, 0, stream>>>(part, g.groups, (int)n, n_classes, loss != nullptr,
                                                        reinterpret_cast<long long*>(confusion), reinterpret_cast<long long*>(counts),
                                                        summary);
    MPO_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
