// The reduction of the patch weight gradient's range partials, shared by patch_fc_f32.hip and patch_fc_f16.hip.  Included
// BEHIND each file's own weight-gradient kernel (after patch_fc_split.h), not at the top: a code object lists its kernels in
// definition order, and the fp32 file's is held to its earlier text.
#pragma once
#include "patch_fc_split.h"

namespace {

// d_weight[i] = sum over the 64 range partials; d_bias likewise
__global__ void patch_wgrad_f32_reduce_kernel(const float* __restrict__ part, const float* __restrict__ part_cs,
                                              float* __restrict__ dw, float* __restrict__ db) {
    const int i4 = blockIdx.x * blockDim.x + threadIdx.x;                 // float4 index
    if (i4 < FE * FK / 4) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int s = 0; s < GRANGES; ++s) a += *reinterpret_cast<const f32x4*>(part + (size_t)s * FE * FK + 4 * (size_t)i4);
        *reinterpret_cast<f32x4*>(dw + 4 * (size_t)i4) = a;
    }
    if (db != nullptr && i4 < FE) {
        float a = 0.f;
        for (int s = 0; s < GRANGES; ++s) a += part_cs[s * FE + i4];
        db[i4] = a;
    }
}

}  // namespace
