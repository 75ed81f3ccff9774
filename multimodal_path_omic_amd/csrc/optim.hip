// Flat-buffer optimisers of the reference's training.optimizer choices (models/mcat/main.py:284-300) and the deterministic
// sum |p| of its L1 penalty (models/utils.py:33-40).  One grid-stride pass per step over the flat parameter, gradient and
// state buffers, 16-byte accesses when every buffer is 16-byte aligned.  Update rules are torch.optim 2.x single-tensor code
// in fp32:
//   g' = g + l1 sign(p) + wd p                         (l1: the L1 penalty's gradient, folded here; sign(0) = 0)
//   ADAM     m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  p -= lr/(1-b1^t) m / (sqrt(v)/sqrt(1-b2^t) + eps)
//   ADAMAX   m = lerp(m, g', 1-b1);  u = max(b2 u, |g'| + eps);  p -= lr/(1-b1^t) m / u
//   ADADELTA v = rho v + (1-rho) g'^2;  d = sqrt(a+eps)/sqrt(v+eps) g';  a = rho a + (1-rho) d^2;  p -= lr d   (rho = b1)
//   SGD      p -= lr g'
// lr_dev / step_dev (nullable) are read on the device, so a captured step follows a schedule and the bias correction.
#include "mpo_common.h"
#include "mpo_kernels.h"
#include "optim_update.h"                   // OptCoef and opt_update (shared with grad_guard.hip)
#include "../../include/mpo_hip.h"

namespace {

template <int ALG>
__global__ __launch_bounds__(256)
void optim_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1, float* __restrict__ s2,
                       size_t n, size_t n_vec, OptCoef c, const float* __restrict__ lr_dev, const int* __restrict__ step_dev) {
    if (lr_dev) c.lr = *lr_dev;
    if (step_dev && (ALG == MPO_OPTIM_ADAM || ALG == MPO_OPTIM_ADAMAX)) {
        const float t = (float)(*step_dev);
        c.bc1 = 1.0f - powf(c.b1, t);
        c.bc2_sqrt = sqrtf(1.0f - powf(c.b2, t));
    }
    constexpr bool kState = ALG != MPO_OPTIM_SGD;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = tid; i < n_vec; i += stride) {
        float4 pv = reinterpret_cast<float4*>(p)[i];
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
        if constexpr (kState) {
            av = reinterpret_cast<float4*>(s1)[i];
            bv = reinterpret_cast<float4*>(s2)[i];
        }
        opt_update<ALG>(pv.x, gv.x, av.x, bv.x, c);
        opt_update<ALG>(pv.y, gv.y, av.y, bv.y, c);
        opt_update<ALG>(pv.z, gv.z, av.z, bv.z, c);
        opt_update<ALG>(pv.w, gv.w, av.w, bv.w, c);
        reinterpret_cast<float4*>(p)[i] = pv;
        if constexpr (kState) {
            reinterpret_cast<float4*>(s1)[i] = av;
            reinterpret_cast<float4*>(s2)[i] = bv;
        }
    }
    for (size_t i = n_vec * 4 + tid; i < n; i += stride) {       // the unaligned or < 4-element rest, element by element
        float a = 0.f, b = 0.f;
        if constexpr (kState) { a = s1[i]; b = s2[i]; }
        float pi = p[i];
        opt_update<ALG>(pi, g[i], a, b, c);
        p[i] = pi;
        if constexpr (kState) { s1[i] = a; s2[i] = b; }
    }
}

// The benchmark's headline optimiser (mpo_adam_step_flat, dp.FlatAdam): the same Adam rule element by element, without the
// L1 fold, the device learning rate and the 16-byte accesses of optim_flat_kernel<MPO_OPTIM_ADAM>.  The two agree to a few
// ulps, not bit for bit, so it stays a kernel of its own.
// torch.optim.Adam semantics (L2 weight decay folded into the gradient), one pass over the flat buffers
__global__ void adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                 size_t n, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt,
                                 const int* __restrict__ step_dev) {
    if (step_dev) {                                     // graph replay: the step count lives on the device
        const float t = (float)(*step_dev);
        bc1 = 1.0f - powf(b1, t);
        bc2_sqrt = sqrtf(1.0f - powf(b2, t));
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float pi = p[i];
        const float gi = g[i] + wd * pi;
        const float mi = b1 * m[i] + (1.0f - b1) * gi;
        const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] = pi - (lr / bc1) * mi / (sqrtf(vi) / bc2_sqrt + eps);
    }
}

// sum |x|, stage 1: a fixed grid (a function of n only) of per-block partial sums, no atomics
constexpr int kAbsThreads = 256, kAbsMaxBlocks = 1024;
__global__ __launch_bounds__(kAbsThreads)
void abs_sum_partial_kernel(const float* __restrict__ x, size_t n, size_t n_vec, float* __restrict__ partials) {
    __shared__ float red[kAbsThreads];
    const size_t stride = (size_t)gridDim.x * kAbsThreads;
    const size_t tid = (size_t)blockIdx.x * kAbsThreads + threadIdx.x;
    float a = 0.f;
    for (size_t i = tid; i < n_vec; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        a += (fabsf(v.x) + fabsf(v.y)) + (fabsf(v.z) + fabsf(v.w));
    }
    for (size_t i = n_vec * 4 + tid; i < n; i += stride) a += fabsf(x[i]);
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = kAbsThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}
// stage 2: one block adds the partials in a fixed order (fp64), writes the device scalar
__global__ __launch_bounds__(kAbsThreads)
void abs_sum_final_kernel(const float* __restrict__ partials, int n_part, float* __restrict__ out) {
    __shared__ double red[kAbsThreads];
    double a = 0.0;
    for (int i = threadIdx.x; i < n_part; i += kAbsThreads) a += (double)partials[i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = kAbsThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)red[0];
}

inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

}  // namespace

int mpo_launch_adam_flat(float* p, const float* g, float* m, float* v, size_t n, float lr, float b1, float b2, float eps,
                         float wd, int step, const int* step_dev, hipStream_t stream) {
    const float bc1 = 1.0f - powf(b1, (float)step), bc2s = sqrtf(1.0f - powf(b2, (float)step));
    const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    adam_flat_kernel<<<blocks, 256, 0, stream>>>(p, g, m, v, n, lr, b1, b2, eps, wd, bc1, bc2s, step_dev);
    MPO_LAUNCH_CHECK();
    return 0;
}

int mpo_launch_optim_flat(int algorithm, float* p, const float* g, float* s1, float* s2, size_t n, float lr,
                          const float* lr_dev, float b1, float b2, float eps, float wd, float l1, int step,
                          const int* step_dev, hipStream_t stream) {
    if (n == 0) return 0;
    OptCoef c{lr, b1, b2, eps, wd, l1, 1.0f, 1.0f};
    if (algorithm == MPO_OPTIM_ADAM || algorithm == MPO_OPTIM_ADAMAX) {
        c.bc1 = 1.0f - powf(b1, (float)step);
        c.bc2_sqrt = sqrtf(1.0f - powf(b2, (float)step));
    }
    const bool vec = aligned16(p) && aligned16(g) && (algorithm == MPO_OPTIM_SGD || (aligned16(s1) && aligned16(s2)));
    const size_t n_vec = vec ? n / 4 : 0;
    const size_t work = vec ? n_vec + (n - 4 * n_vec) : n;
    const int blocks = (int)((work + 255) / 256 < 2048 ? (work + 255) / 256 : 2048);
    switch (algorithm) {
    case MPO_OPTIM_ADAM:
        optim_flat_kernel<MPO_OPTIM_ADAM><<<blocks, 256, 0, stream>>>(p, g, s1, s2, n, n_vec, c, lr_dev, step_dev);
        break;
    case MPO_OPTIM_ADAMAX:
        optim_flat_kernel<MPO_OPTIM_ADAMAX><<<blocks, 256, 0, stream>>>(p, g, s1, s2, n, n_vec, c, lr_dev, step_dev);
        break;
    case MPO_OPTIM_ADADELTA:
        optim_flat_kernel<MPO_OPTIM_ADADELTA><<<blocks, 256, 0, stream>>>(p, g, s1, s2, n, n_vec, c, lr_dev, step_dev);
        break;
    case MPO_OPTIM_SGD:
        optim_flat_kernel<MPO_OPTIM_SGD><<<blocks, 256, 0, stream>>>(p, g, s1, s2, n, n_vec, c, lr_dev, step_dev);
        break;
    default:
        MPO_CHECK(false, "flat optimiser: unknown algorithm %d", algorithm);
    }
    MPO_LAUNCH_CHECK();
    return 0;
}

size_t mpo_abs_sum_partials(size_t n) {
    const size_t b = (n + 4 * kAbsThreads - 1) / (4 * kAbsThreads);
    return b < 1 ? 1 : (b > kAbsMaxBlocks ? kAbsMaxBlocks : b);
}

int mpo_launch_abs_sum(const float* x, size_t n, float* partials, float* out, hipStream_t stream) {
    const int blocks = (int)mpo_abs_sum_partials(n);
    const size_t n_vec = aligned16(x) ? n / 4 : 0;
    abs_sum_partial_kernel<<<blocks, kAbsThreads, 0, stream>>>(x, n, n_vec, partials);
    MPO_LAUNCH_CHECK();
    abs_sum_final_kernel<<<1, kAbsThreads, 0, stream>>>(partials, blocks, out);
    MPO_LAUNCH_CHECK();
    return 0;
}
