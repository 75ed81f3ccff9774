// The feature scale of an fp32 window, found on the device: *scale_out = range_scale(max |x|) (mpo_common.h), the power of two
// patch_fc_split.hip multiplies X by before its fp16 operand split.  ops.feature_scale forms the same number on the host
// (a full-size |x| temporary, a library reduction, a blocking read) and hands it over by value, which a captured step bakes
// in; this pass leaves it in device memory, where patch_fc_f32_kernel reads it when it starts -- as it reads W_H's.
//
// A streaming read of n floats.  The maximum is taken over the MAGNITUDE BITS (bits & 0x7fffffff) as unsigned integers:
// finite magnitudes order as their bits, an infinity lies above every finite value and every NaN above infinity, so "some
// element was non-finite" survives the reduction with no second flag (fmaxf drops a NaN), and an integer maximum does not
// depend on the order the workgroups arrive in.  Every thread keeps four 16-byte nontemporal loads in flight (the window is
// read once here and is far larger than the L2; the gather or the patch layer around this pass should keep what they have
// there); the grid is eight workgroups per CU of the device the stream runs on, whatever n; lanes -> wave_max -> LDS -> ONE
// vector atomic max per workgroup onto a word the first launch cleared.  Three launches (clear, reduce, write): nothing
// waits on a "last workgroup", nothing is allocated, nothing synchronises with the host.
#include "../../include/mpo_hip.h"
#include "mpo_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kInFlight = 4;                    // 16-byte loads per thread and trip
constexpr int kBlocksPerCu = 8;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((address_space(1))) u32x4 GlobalVec;

__device__ __forceinline__ uint32_t mag4(const u32x4& v) {
    return max(max(v[0] & 0x7fffffffu, v[1] & 0x7fffffffu), max(v[2] & 0x7fffffffu, v[3] & 0x7fffffffu));
}

__global__ void feature_range_clear_kernel(uint32_t* __restrict__ bits) { *bits = 0u; }

// n4 whole 16-byte vectors at x, then n - 4 n4 (< 4) single floats
__global__ void __launch_bounds__(kThreads)
feature_range_reduce_kernel(const uint32_t* __restrict__ x, long long n, uint32_t* __restrict__ bits) {
    __shared__ uint32_t red[kThreads / 64];
    const GlobalVec* xv = (const GlobalVec*)x;                   // (global, not flat, accesses)
    const long long n4 = n >> 2;
    const long long stride = (long long)gridDim.x * kThreads;
    long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    uint32_t m = 0u;
    for (; i + (kInFlight - 1) * stride < n4; i += kInFlight * stride) {
        u32x4 v[kInFlight];
#pragma unroll
        for (int j = 0; j < kInFlight; ++j) v[j] = __builtin_nontemporal_load(xv + i + j * stride);
#pragma unroll
        for (int j = 0; j < kInFlight; ++j) m = max(m, mag4(v[j]));
    }
    for (; i < n4; i += stride) m = max(m, mag4(__builtin_nontemporal_load(xv + i)));
    if (blockIdx.x == 0 && 4 * n4 + threadIdx.x < n) m = max(m, x[4 * n4 + threadIdx.x] & 0x7fffffffu);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) m = max(m, red[w]);
        if (m != 0u) atomicMax(bits, m);
    }
}

// bits == NULL: an empty matrix
__global__ void feature_range_write_kernel(const uint32_t* __restrict__ bits, float* __restrict__ scale_out) {
    *scale_out = bits != nullptr ? range_scale(__uint_as_float(*bits)) : 1.0f;      // (a NaN or an infinity gives 1)
}

// compute units of the current device (asked once per device; no synchronisation)
int device_cus() {
    static int cus[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
        cus[dev] = n;
    }
    return cus[dev];
}

}  // namespace

extern "C" {

size_t mpo_feature_range_workspace_bytes(void) { return 16; }

int mpo_feature_range_f32(const float* x, int64_t n, float* scale_out, void* workspace, size_t workspace_bytes,
                          mpo_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPO_CHECK(scale_out, "feature range: null scale_out");
    MPO_CHECK(n >= 0, "feature range: n %lld < 0", (long long)n);
    if (n == 0) {
        feature_range_write_kernel<<<1, 1, 0, stream>>>(nullptr, scale_out);
        MPO_LAUNCH_CHECK();
        return 0;
    }
    MPO_CHECK(x, "feature range: null x");
    MPO_CHECK((reinterpret_cast<uintptr_t>(x) & 15) == 0, "feature range: x must be 16-byte aligned");
    MPO_CHECK(workspace && (reinterpret_cast<uintptr_t>(workspace) & 3) == 0 && workspace_bytes >= mpo_feature_range_workspace_bytes(),
              "feature range: workspace null, misaligned or too small (%zu bytes)", workspace_bytes);
    uint32_t* bits = static_cast<uint32_t*>(workspace);
    feature_range_clear_kernel<<<1, 1, 0, stream>>>(bits);
    MPO_LAUNCH_CHECK();
    const long long per_trip = (long long)kThreads * kInFlight;                 // 16-byte vectors a workgroup reads per trip
    const long long want = ((n >> 2) + per_trip - 1) / per_trip;                // (a small matrix: no more workgroups than trips)
    const long long cap = (long long)device_cus() * kBlocksPerCu;
    const unsigned grid = (unsigned)(want < 1 ? 1 : want < cap ? want : cap);
    feature_range_reduce_kernel<<<grid, kThreads, 0, stream>>>(reinterpret_cast<const uint32_t*>(x), (long long)n, bits);
    MPO_LAUNCH_CHECK();
    feature_range_write_kernel<<<1, 1, 0, stream>>>(bits, scale_out);
    MPO_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
