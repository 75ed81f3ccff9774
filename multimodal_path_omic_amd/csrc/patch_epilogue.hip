// The bf16 patch layer's element-wise epilogue, h = drop(relu(h + bias)) in place, its derivative with the layer's bias
// gradient (column sums) from the same pass, and the stand-alone bf16 column sum.
#include "mpo_common.h"
#include "mpo_kernels.h"

namespace {

// patch-layer epilogue: h = drop(relu(h + bias)), bf16 in place, 8 elements (16 bytes) per lane.
// The launch guarantees (total threads) % (cols / 8) == 0, so a thread meets the same 8 columns on every
// grid-stride iteration and keeps their biases in registers (8 scalar, poorly coalesced bias loads per
// iteration made the first version 3x slower than a plain element-wise pass).
__global__ void bias_relu_dropout_bf16_kernel(bf16x8* __restrict__ h, const float* __restrict__ bias, size_t n8, int cols,
                                              float drop_p, unsigned long long seed, unsigned long long offset_,
                                              const unsigned long long* epoch) {
    const float inv_keep = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
    const unsigned long long offset = epoch_offset(offset_, epoch);
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c0 = (int)((tid * 8) % (size_t)cols);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(bias + c0), b1 = *reinterpret_cast<const f32x4*>(bias + c0 + 4);
    const float bv[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
    const uint32_t thr = (uint32_t)(drop_p * 65536.0f);
    for (size_t i = tid; i < n8; i += (size_t)gridDim.x * blockDim.x) {
        bf16x8 v = h[i];
        // one Philox call per 8 elements: 16 random bits each (keep iff u16 >= p * 65536)
        uint4 r0 = {0, 0, 0, 0};
        if (drop_p > 0.f)
            r0 = philox4x32((uint32_t)(offset + i), (uint32_t)((offset + i) >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
        const uint32_t rw[4] = {r0.x, r0.y, r0.z, r0.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float x = relu_keep_nan((float)v[j] + bv[j]);
            if (drop_p > 0.f) x = (((rw[j >> 1] >> (16 * (j & 1))) & 0xFFFFu) >= thr) ? x * inv_keep : 0.f;
            v[j] = (__bf16)x;
        }
        h[i] = v;
    }
}
// g = dy * (h > 0 ? 1/(1-p) : 0).  part_colsum (nullable, [gridDim.x][cols]): per-workgroup column sums of g -- the bias
// gradient of the layer -- from the same pass (a thread keeps one 8-column group: the grid stride is a multiple of a row).
__global__ __launch_bounds__(256)
void relu_dropout_bwd_bf16_kernel(const bf16x8* __restrict__ h, const bf16x8* __restrict__ dy, bf16x8* __restrict__ g,
                                  size_t n8, float inv_keep, int cols, float* __restrict__ part_colsum) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
        const bf16x8 hv = h[i], d = dy[i];
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (float)hv[j] > 0.f ? (__bf16)((float)d[j] * inv_keep) : (__bf16)0.f;
        g[i] = o;
        if (part_colsum != nullptr) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += (float)o[j];
        }
    }
    if (part_colsum != nullptr) {
        __shared__ float red[256][9];
        const int tpr = cols / 8, c8 = threadIdx.x % tpr, rl = threadIdx.x / tpr;
#pragma unroll
        for (int j = 0; j < 8; ++j) red[threadIdx.x][j] = acc[j];
        __syncthreads();
        if (rl == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float t = 0.f;
                for (int k = 0; k < 256 / tpr; ++k) t += red[k * tpr + c8][j];
                part_colsum[(size_t)blockIdx.x * cols + 8 * c8 + j] = t;
            }
        }
    }
}

// out[c] = sum_r x[r][c] over a bf16 [rows][cols] tensor (cols = 8 * a divisor of 256): the patch layer's bias gradient.
// Each thread owns 8 fixed columns (16-byte loads), workgroups take row chunks, fp32 atomics merge them.
__global__ __launch_bounds__(256)
void colsum_bf16_kernel(const bf16x8* __restrict__ x, float* __restrict__ out, size_t rows, int cols) {
    const int tpr = cols / 8;                       // threads per row
    const int rpb = 256 / tpr;                      // rows per block-iteration
    const int c8 = threadIdx.x % tpr, rl = threadIdx.x / tpr;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (size_t r = (size_t)blockIdx.x * rpb + rl; r < rows; r += (size_t)gridDim.x * rpb) {
        const bf16x8 v = x[r * tpr + c8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += (float)v[j];
    }
    __shared__ float red[256][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) red[threadIdx.x][j] = acc[j];
    __syncthreads();
    if (rl == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float t = 0.f;
            for (int k = 0; k < rpb; ++k) t += red[k * tpr + c8][j];
            atomicAdd(out + 8 * c8 + j, t);
        }
    }
}

}  // namespace

int mpo_launch_colsum_bf16(const void* x, float* out, size_t rows, int cols, hipStream_t stream) {
    MPO_CHECK(cols % 8 == 0 && 256 % (cols / 8) == 0, "bf16 column sum: width %d must be 8 * a divisor of 256", cols);
    MPO_HIP(hipMemsetAsync(out, 0, (size_t)cols * sizeof(float), stream));
    const size_t rpb = 256 / (cols / 8);
    size_t blocks = (rows + rpb - 1) / rpb;
    if (blocks > 2048) blocks = 2048;
    colsum_bf16_kernel<<<(int)blocks, 256, 0, stream>>>((const bf16x8*)x, out, rows, cols);
    MPO_LAUNCH_CHECK();
    return 0;
}

int mpo_launch_bias_relu_dropout_bf16(void* h, const float* bias, size_t rows, int cols, float drop_p,
                                      unsigned long long seed, unsigned long long offset, const unsigned long long* epoch,
                                      hipStream_t stream) {
    MPO_CHECK(cols % 8 == 0 && 256 % (cols / 8) == 0, "patch epilogue: width %d must be 8 * a divisor of 256", cols);
    const size_t n8 = rows * (size_t)cols / 8;
    const int blocks = (int)((n8 + 255) / 256 < 8192 ? (n8 + 255) / 256 : 8192);   // blocks * 256 is a multiple of cols / 8
    bias_relu_dropout_bf16_kernel<<<blocks, 256, 0, stream>>>((bf16x8*)h, bias, n8, cols, drop_p, seed, offset, epoch);
    MPO_LAUNCH_CHECK();
    return 0;
}
int mpo_relu_dropout_bwd_blocks(size_t n, int with_colsum) {
    const size_t n8 = n / 8;
    const size_t cap = with_colsum ? 512 : 8192;           // column sums: fewer, longer workgroups (one partial row each)
    return (int)((n8 + 255) / 256 < cap ? (n8 + 255) / 256 : cap);
}
int mpo_launch_relu_dropout_bwd_bf16(const void* h, const void* dy, void* g, size_t n, float drop_p, int cols,
                                     float* part_colsum /* nullable [blocks][cols] */, hipStream_t stream) {
    MPO_CHECK(n % 8 == 0, "patch epilogue backward: %zu elements not a multiple of 8", n);
    MPO_CHECK(!part_colsum || (cols >= 8 && cols % 8 == 0 && 256 % (cols / 8) == 0 && n % (size_t)cols == 0),
              "patch epilogue backward: column sums need cols in {8,..,2048} dividing 2048 (got %d)", cols);
    const size_t n8 = n / 8;
    const int blocks = mpo_relu_dropout_bwd_blocks(n, part_colsum != nullptr);
    relu_dropout_bwd_bf16_kernel<<<blocks, 256, 0, stream>>>((const bf16x8*)h, (const bf16x8*)dy, (bf16x8*)g, n8,
                                                             drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f, cols, part_colsum);
    MPO_LAUNCH_CHECK();
    return 0;
}
