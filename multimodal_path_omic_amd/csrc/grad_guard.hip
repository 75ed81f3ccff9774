// Gradient-norm clipping and the non-finite step skip of the flat optimisers (include/mpo_grad_guard.h), on the device and
// capturable: a step inside a HIP graph has no host to look at its loss, and one non-finite gradient would otherwise reach
// every parameter and both moments for good.
//   mpo_grad_norm_flat            measures g' = g + l1 sign(p): its 2-norm, the clipping coefficient, "some element was not
//                                 finite" -- two launches on the pattern of mpo_abs_sum_flat (optim.hip): a grid that is a
//                                 function of n alone, per-workgroup partials, one workgroup adds them in a fixed order.
//   mpo_optim_step_flat_guarded   optim.hip's pass with the clipped gradient coef g' + wd p (the same opt_update), every
//                                 workgroup leaving before its first store when the step is skipped.
// The two talk through the caller's 16-byte control block; the model has a few million parameters, so both are launch-bound.
#include "mpo_common.h"
#include "optim_update.h"
#include "../../include/mpo_hip.h"

namespace {

struct GradCtl {                                    // the control block of mpo_grad_guard.h
    float norm, coef;
    int32_t nonfinite, skipped;
};
static_assert(sizeof(GradCtl) == 16, "control block: four 32-bit words");

constexpr int kNormThreads = 256, kNormMaxBlocks = 1024;

// one element's share: g' as opt_update forms it (fp32), its exponent bits, its square in fp64
__device__ __forceinline__ void norm_term(float g, float p, float l1, double& acc, uint32_t& bad) {
    float gi = g;
    if (l1 != 0.0f) gi += l1 * (float)((p > 0.0f) - (p < 0.0f));
    bad |= (uint32_t)((__float_as_uint(gi) & 0x7f800000u) == 0x7f800000u);
    acc += (double)gi * (double)gi;
}

// sum of squares and the flag of one workgroup's share, tree over the workgroup in a fixed order -> thread 0 holds both
__device__ __forceinline__ void block_sum_or(double& acc, uint32_t& bad) {
    __shared__ double red[kNormThreads];
    red[threadIdx.x] = acc;
    bad = (uint32_t)__syncthreads_or((int)bad);
    for (int s = kNormThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    acc = red[0];
}

// stage 1: p is read only when l1 != 0 (NULL otherwise)
__global__ __launch_bounds__(kNormThreads)
void grad_norm_partial_kernel(const float* __restrict__ g, const float* __restrict__ p, size_t n, size_t n_vec, float l1,
                              double* __restrict__ part_sum, uint32_t* __restrict__ part_bad) {
    const size_t stride = (size_t)gridDim.x * kNormThreads;
    const size_t tid = (size_t)blockIdx.x * kNormThreads + threadIdx.x;
    double acc = 0.0;
    uint32_t bad = 0u;
    for (size_t i = tid; i < n_vec; i += stride) {
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 pv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (l1 != 0.0f) pv = reinterpret_cast<const float4*>(p)[i];
        norm_term(gv.x, pv.x, l1, acc, bad);
        norm_term(gv.y, pv.y, l1, acc, bad);
        norm_term(gv.z, pv.z, l1, acc, bad);
        norm_term(gv.w, pv.w, l1, acc, bad);
    }
    for (size_t i = n_vec * 4 + tid; i < n; i += stride)         // the unaligned or < 4-element rest, element by element
        norm_term(g[i], l1 != 0.0f ? p[i] : 0.0f, l1, acc, bad);
    block_sum_or(acc, bad);
    if (threadIdx.x == 0) {
        part_sum[blockIdx.x] = acc;
        part_bad[blockIdx.x] = bad;
    }
}

// stage 2: one workgroup adds the partials in a fixed order; one thread writes the control block and settles the step count
__global__ __launch_bounds__(kNormThreads)
void grad_norm_final_kernel(const double* __restrict__ part_sum, const uint32_t* __restrict__ part_bad, int n_part,
                            float max_norm, int skip_nonfinite, int* __restrict__ step_dev, GradCtl* __restrict__ ctl) {
    double acc = 0.0;
    uint32_t bad = 0u;
    for (int i = threadIdx.x; i < n_part; i += kNormThreads) {
        acc += part_sum[i];
        bad |= part_bad[i];
    }
    block_sum_or(acc, bad);
    if (threadIdx.x == 0) {
        const double norm = sqrt(acc);
        double coef = 1.0;
        if (max_norm > 0.0f) {
            const double q = (double)max_norm / (norm + 1e-6);
            coef = q < 1.0 ? q : 1.0;                            // (a NaN norm: 1)
        }
        ctl->norm = (float)norm;
        ctl->coef = (float)coef;
        ctl->nonfinite = bad ? 1 : 0;
        if (skip_nonfinite && bad) {
            ctl->skipped += 1;
            if (step_dev) *step_dev -= 1;                        // the caller counted this step before it knew
        }
    }
}

// The clipped gradient coef (g + l1 sign(p)), the sum formed as opt_update forms it, the product rounded on its own (opaque
// to the compiler, which would otherwise contract it with the weight-decay term behind it).
__device__ __forceinline__ float clipped(float g, float p, float l1, float coef) {
    float gi = g;
    if (l1 != 0.0f) gi += l1 * (float)((p > 0.0f) - (p < 0.0f));
    gi = coef * gi;
    asm volatile("" : "+v"(gi));
    return gi;
}

// optim_flat_kernel's pass (optim.hip).  CLIP: on the clipped gradient, opt_update's own L1 fold switched off (c.l1 == 0: the
// term is inside the clip); otherwise that kernel's loops word for word.
template <int ALG, bool CLIP>
__device__ __forceinline__ void flat_pass(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1,
                                          float* __restrict__ s2, size_t n, size_t n_vec, const OptCoef& c, float l1,
                                          float coef) {
    constexpr bool kState = ALG != MPO_OPTIM_SGD;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = tid; i < n_vec; i += stride) {
        float4 pv = reinterpret_cast<float4*>(p)[i];
        float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
        if constexpr (kState) {
            av = reinterpret_cast<float4*>(s1)[i];
            bv = reinterpret_cast<float4*>(s2)[i];
        }
        if constexpr (CLIP)
            gv = make_float4(clipped(gv.x, pv.x, l1, coef), clipped(gv.y, pv.y, l1, coef), clipped(gv.z, pv.z, l1, coef),
                             clipped(gv.w, pv.w, l1, coef));
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
        float gi = g[i];
        if constexpr (CLIP) gi = clipped(gi, pi, l1, coef);
        opt_update<ALG>(pi, gi, a, b, c);
        p[i] = pi;
        if constexpr (kState) { s1[i] = a; s2[i] = b; }
    }
}

// A skipped step returns before the first store.  A step that is not clipped (coef == 1, the common case, and every step
// of a run that only asks for the skip) takes optim_flat_kernel's own loops: the compiler contracts and packs an update
// differently as soon as anything stands between the gradient's load and it, so "times one" alone would agree with the
// unguarded pass to an ulp, not to the bit.  c.l1 == 0 on entry; `l1` is the L1 term's factor.
template <int ALG>
__global__ __launch_bounds__(256)
void optim_flat_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1,
                               float* __restrict__ s2, size_t n, size_t n_vec, OptCoef c, const float* __restrict__ lr_dev,
                               const int* __restrict__ step_dev, float l1, const GradCtl* __restrict__ ctl,
                               int skip_nonfinite) {
    if (skip_nonfinite && ctl->nonfinite) return;
    const float coef = ctl->coef;
    if (lr_dev) c.lr = *lr_dev;
    if (step_dev && (ALG == MPO_OPTIM_ADAM || ALG == MPO_OPTIM_ADAMAX)) {
        const float t = (float)(*step_dev);
        c.bc1 = 1.0f - powf(c.b1, t);
        c.bc2_sqrt = sqrtf(1.0f - powf(c.b2, t));
    }
    if (coef == 1.0f) {
        c.l1 = l1;
        flat_pass<ALG, false>(p, g, s1, s2, n, n_vec, c, l1, coef);
    } else {
        flat_pass<ALG, true>(p, g, s1, s2, n, n_vec, c, l1, coef);
    }
}

inline bool aligned_to(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; }

size_t norm_blocks(size_t n) {
    const size_t b = (n + 4 * kNormThreads - 1) / (4 * kNormThreads);
    return b < 1 ? 1 : (b > kNormMaxBlocks ? kNormMaxBlocks : b);
}

}  // namespace

extern "C" {

// per workgroup of stage 1: one fp64 partial sum, then (behind all of them) one 32-bit flag
size_t mpo_grad_norm_flat_workspace_bytes(int64_t n) {
    return n < 0 ? 0 : norm_blocks((size_t)n) * (sizeof(double) + sizeof(uint32_t));
}

int mpo_grad_norm_flat(const float* grads, const float* params, int64_t n, float l1, float max_norm, int skip_nonfinite,
                       int32_t* step_dev, void* ctl, void* workspace, size_t workspace_bytes, mpo_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPO_CHECK(n >= 0, "grad norm: n = %lld", (long long)n);
    MPO_CHECK(ctl, "grad norm: null ctl (the 16-byte control block)");
    MPO_CHECK(grads || n == 0, "grad norm: null grads");
    MPO_CHECK(params || l1 == 0.0f || n == 0, "grad norm: l1 = %g needs params", (double)l1);
    MPO_CHECK(aligned_to(grads, 4) && aligned_to(params, 4) && aligned_to(step_dev, 4) && aligned_to(ctl, 4),
              "grad norm: grads, params, step_dev and ctl must be 4-byte aligned");
    MPO_CHECK(workspace && aligned_to(workspace, 8), "grad norm: workspace null or not 8-byte aligned");
    MPO_CHECK(workspace_bytes >= mpo_grad_norm_flat_workspace_bytes(n), "grad norm: workspace too small (%zu bytes, %zu needed)",
              workspace_bytes, mpo_grad_norm_flat_workspace_bytes(n));
    const int blocks = (int)norm_blocks((size_t)n);
    double* part_sum = static_cast<double*>(workspace);
    uint32_t* part_bad = reinterpret_cast<uint32_t*>(part_sum + blocks);
    const bool vec = aligned_to(grads, 16) && (l1 == 0.0f || aligned_to(params, 16));
    const size_t n_vec = vec ? (size_t)n / 4 : 0;
    grad_norm_partial_kernel<<<blocks, kNormThreads, 0, stream>>>(grads, params, (size_t)n, n_vec, l1, part_sum, part_bad);
    MPO_LAUNCH_CHECK();
    grad_norm_final_kernel<<<1, kNormThreads, 0, stream>>>(part_sum, part_bad, blocks, max_norm, skip_nonfinite, step_dev,
                                                           static_cast<GradCtl*>(ctl));
    MPO_LAUNCH_CHECK();
    return 0;
}

int mpo_optim_step_flat_guarded(int algorithm, float* params, const float* grads, float* state1, float* state2, int64_t n,
                                float lr, const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                                float l1, int step, const int32_t* step_dev, const void* ctl, int skip_nonfinite,
                                mpo_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPO_CHECK(algorithm >= MPO_OPTIM_ADAM && algorithm <= MPO_OPTIM_SGD, "guarded flat optimiser: unknown algorithm %d", algorithm);
    MPO_CHECK(n >= 0, "guarded flat optimiser: n = %lld", (long long)n);
    MPO_CHECK(ctl, "guarded flat optimiser: null ctl (the control block mpo_grad_norm_flat wrote)");
    MPO_CHECK(params && grads, "guarded flat optimiser: null parameter or gradient buffer");
    const bool stateful = algorithm != MPO_OPTIM_SGD;
    MPO_CHECK(!stateful || (state1 && state2), "guarded flat optimiser: algorithm %d needs both state buffers", algorithm);
    MPO_CHECK(aligned_to(params, 4) && aligned_to(grads, 4) && aligned_to(state1, 4) && aligned_to(state2, 4) &&
              aligned_to(lr_dev, 4) && aligned_to(step_dev, 4) && aligned_to(ctl, 4),
              "guarded flat optimiser: buffers and ctl must be 4-byte aligned");
    const bool counted = algorithm == MPO_OPTIM_ADAM || algorithm == MPO_OPTIM_ADAMAX;
    MPO_CHECK(!counted || step >= 1 || step_dev, "guarded flat optimiser: step counts from 1 (got %d)", step);
    if (n == 0) return 0;
    OptCoef c{lr, beta1, beta2, eps, weight_decay, 0.0f, 1.0f, 1.0f};     // (l1 travels beside it)
    if (counted) {
        const float t = (float)(step < 1 ? 1 : step);
        c.bc1 = 1.0f - powf(beta1, t);
        c.bc2_sqrt = sqrtf(1.0f - powf(beta2, t));
    }
    // mpo_launch_optim_flat's geometry
    const bool vec = aligned_to(params, 16) && aligned_to(grads, 16) && (!stateful || (aligned_to(state1, 16) && aligned_to(state2, 16)));
    const size_t n_vec = vec ? (size_t)n / 4 : 0;
    const size_t work = vec ? n_vec + ((size_t)n - 4 * n_vec) : (size_t)n;
    const int blocks = (int)((work + 255) / 256 < 2048 ? (work + 255) / 256 : 2048);
    const GradCtl* gc = static_cast<const GradCtl*>(ctl);
    switch (algorithm) {
    case MPO_OPTIM_ADAM:
        optim_flat_guarded_kernel<MPO_OPTIM_ADAM><<<blocks, 256, 0, stream>>>(params, grads, state1, state2, (size_t)n, n_vec, c,
                                                                       lr_dev, step_dev, l1, gc, skip_nonfinite);
        break;
    case MPO_OPTIM_ADAMAX:
        optim_flat_guarded_kernel<MPO_OPTIM_ADAMAX><<<blocks, 256, 0, stream>>>(params, grads, state1, state2, (size_t)n, n_vec, c,
                                                                       lr_dev, step_dev, l1, gc, skip_nonfinite);
        break;
    case MPO_OPTIM_ADADELTA:
        optim_flat_guarded_kernel<MPO_OPTIM_ADADELTA><<<blocks, 256, 0, stream>>>(params, grads, state1, state2, (size_t)n, n_vec, c,
                                                                       lr_dev, step_dev, l1, gc, skip_nonfinite);
        break;
    case MPO_OPTIM_SGD:
        optim_flat_guarded_kernel<MPO_OPTIM_SGD><<<blocks, 256, 0, stream>>>(params, grads, state1, state2, (size_t)n, n_vec, c,
                                                                       lr_dev, step_dev, l1, gc, skip_nonfinite);
        break;
    }
    MPO_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
