// What the patch layers of an fp32-stored and of an fp16-stored window share (patch_fc_f32.hip, patch_fc_f16.hip): the
// tile constants, the operand splits, the LDS swizzles and the range / pack kernels of W_H (the reduction of the weight
// gradient's range partials: patch_wgrad_reduce.h).  Everything has internal linkage: each of the two files carries its own copy.
#pragma once
#include "coattn_tile.h"
#include "mpo_kernels.h"

namespace {

constexpr int FE = 256;                         // embed_dim
constexpr int FK = 1024;                        // patch feature width
constexpr int FBM = 128;                        // rows per block
constexpr int FBK = 32;                         // k per step
constexpr int FSTEPS = FK / FBK;                // 32
constexpr int FIMG = FBM * FBK * 2;             // one bf16 image of a stage: 8 KiB
constexpr int FROWB = FBK * 2;                  // 64 bytes per image row
__device__ __forceinline__ void split8(const f32x4& a, const f32x4& b, bf16x8& hi, bf16x8& lo) {
    const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    pack_hi_lo(v, hi, lo);
}
// fp16 hi / lo split of eight floats, round-to-nearest both (hi + lo carries 22 significand bits, the dropped lo * lo term
// is 2^-22 of the product).  Range: both operands arrive scaled by a power of two that puts their largest magnitude at
// 2^14 .. 2^15 (W_H: from its own maximum, found on the device per call; X: x_scale, which the caller derives from the window's
// maximum -- ops.patch_fc_f32 caches it per tensor -- or leaves on the device, feature_range.hip, for the kernel to read
// through x_scale_dev), so finite data never reach the fp16 limit and small features keep
// their bits (unscaled, features of ~1e-4 sat in fp16 subnormals: ~3e-4 relative).  The clamp only matters for a caller
// that passes no scale (x_scale = 1: |x| up to 1.3e5 is carried by hi + lo, beyond that clipped).  NaN and infinities are
// NOT clamped away: v - v is 0 for finite v and NaN otherwise, so a non-finite feature makes its row of H_bag non-finite,
// as it does in the reference's fp32 GEMM (v_med3 alone returns the bound for a NaN).
__device__ __forceinline__ int fswz(int row) { return ((row >> 1) & 1) ^ ((row >> 2) & 2); }
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void split8h(const f32x4& a, const f32x4& b, float scale, f16x8& hi, f16x8& lo) {
    const float v[8] = {a[0] * scale, a[1] * scale, a[2] * scale, a[3] * scale, b[0] * scale, b[1] * scale, b[2] * scale, b[3] * scale};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const _Float16 h = (_Float16)(__builtin_amdgcn_fmed3f(v[j], -65504.0f, 65504.0f) + (v[j] - v[j]));
        hi[j] = h;
        lo[j] = (_Float16)__builtin_amdgcn_fmed3f(v[j] - (float)h, -65504.0f, 65504.0f);
    }
}
__device__ __forceinline__ f32x4 mfma_f16(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
// scale of W_H for this call -> *scale_out = range_scale (mpo_common.h) of its maximum (one workgroup of 1024 threads over the
// 256 x 1024 weight)
__global__ void weight_range_kernel(const float* __restrict__ w, float* __restrict__ scale_out) {
    __shared__ float red[16];
    float m = 0.f;
    for (int i = threadIdx.x; i < 256 * 1024 / 4; i += 1024) {
        const f32x4 v = reinterpret_cast<const f32x4*>(w)[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 16; ++i) m = fmaxf(m, red[i]);
        *scale_out = range_scale(m);
    }
}

// W_H [256][1024] fp32 (x *w_scale, weight_range_kernel) -> hi / lo fp16 in fragment order: block (((term * 4 + wave) * 32 + step) * 4 + ct) of 1 KiB holds, for lane
// (i = lane & 15, g = lane >> 4), W_H[64 wave + 16 ct + i][32 step + 8 g .. + 7]
__global__ void pack_patch_weight_f32_kernel(const float* __restrict__ w, f16x8* __restrict__ out, const float* __restrict__ w_scale) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;          // one fragment per thread: 256 * 1024 / 8
    if (t >= FE * FK / 8) return;
    const int lane = t & 63, blk = t >> 6;
    const int ct = blk & 3, step = (blk >> 2) & (FSTEPS - 1), wave = blk >> 7;
    const int row = 64 * wave + 16 * ct + (lane & 15), k0 = FBK * step + 8 * (lane >> 4);
    const f32x4 a = *reinterpret_cast<const f32x4*>(w + (size_t)row * FK + k0);
    const f32x4 b = *reinterpret_cast<const f32x4*>(w + (size_t)row * FK + k0 + 4);
    f16x8 hi, lo;
    split8h(a, b, *w_scale, hi, lo);
    out[t] = hi;
    out[FE * FK / 8 + t] = lo;
}

// ------------------------------------------------------------------------------------------------ weight gradient
constexpr int GW = 8;                           // waves
constexpr int GCH = 32;                         // rows per chunk
constexpr int GRANGES = 64, GCOLB = 4;          // row ranges x column blocks of X = 256 workgroups
constexpr int GIMG = GCH * 256 * 2;             // one bf16 image [32 rows][256 columns]: 16 KiB
constexpr int GROWB = 512;

// [32][256] bf16 image, 16-byte chunk c of row r at c ^ (2 (r & 7)) (coattn_tile.h): col_frag<256>() reads it transposed
__device__ __forceinline__ int gimg_off(int r, int c) { return r * GROWB + ((c ^ ((r & 7) << 1)) << 4); }

}  // namespace
