// Head of the gene-expression model in its training-step form (declared in include/mpo_hip.h):
//   Y = softmax(h W^T + b)                                   models/ge_nacagat/ge_nacagat.py:63-67
//   loss = nn.CrossEntropyLoss()(Y.unsqueeze(0), label)      models/ge_nacagat/main.py:33 -- on the ALREADY soft-maxed Y
//        = logsumexp(Y) - Y[label]
// one launch each way, plain fp32, one wave per workgroup.
//
// Nothing is kept between the two launches: the state of a bag is its n_classes logits, and forming them again from the
// h row the backward reads anyway (n_classes dot products of d terms) costs less than a buffer would.  Both directions
// run the same ge_head_bag(), so the backward differentiates exactly the values the forward reported.
//
// Gradient (per unit of d_loss):  dL/dY_j = softmax(Y)_j - [j == label];  through Y = softmax(z):
//   dL/dz_i = Y_i (dL/dY_i - sum_j dL/dY_j Y_j)
// then d_h = dz W, dW = dz^T h, db = sum_bags dz, each bag's dz scaled by d_loss[bag].
#include <math.h>

#include "../../include/mpo_hip.h"
#include "mpo_common.h"

namespace {

constexpr int kGeMaxC = 8;        // classes (the reference uses 3)
constexpr int kGeMaxPerLane = 8;  // d <= 512 over the 64 lanes of a wave

__device__ inline float ge_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One bag on one wave: y[] (softmax of the logits), the loss and dz[] = d loss / d logits, identical in every lane.
// hk: this lane's elements of the h row, hk[t] = h[lane + 64 t].  label_ok false: loss NaN, dz 0 (see the header).
__device__ inline void ge_head_bag(const float (&hk)[kGeMaxPerLane], const float* __restrict__ w, const float* __restrict__ bias,
                                   int d, int C, long long label, int lane, float (&y)[kGeMaxC], float& loss,
                                   float (&dz)[kGeMaxC]) {
    const int per_lane = d / 64;
    float z[kGeMaxC];
#pragma unroll
    for (int j = 0; j < kGeMaxC; ++j) {
        float acc = 0.f;
        if (j < C) {
#pragma unroll
            for (int t = 0; t < kGeMaxPerLane; ++t)
                if (t < per_lane) acc = fmaf(hk[t], w[(size_t)j * d + lane + 64 * t], acc);
        }
        acc = ge_wave_sum(acc);
        z[j] = j < C ? acc + bias[j] : -INFINITY;
    }
    float mx = z[0];
#pragma unroll
    for (int j = 1; j < kGeMaxC; ++j) mx = fmaxf(mx, z[j]);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < kGeMaxC; ++j) {
        y[j] = j < C ? expf(z[j] - mx) : 0.f;
        s += y[j];
    }
    const float inv = 1.0f / s;
    float my = 0.f;                                   // Y is in [0, 1]: its maximum is at least 1 / C
#pragma unroll
    for (int j = 0; j < kGeMaxC; ++j) {
        y[j] *= inv;
        if (j < C) my = fmaxf(my, y[j]);
    }
    float p[kGeMaxC], s2 = 0.f;
#pragma unroll
    for (int j = 0; j < kGeMaxC; ++j) {
        p[j] = j < C ? expf(y[j] - my) : 0.f;
        s2 += p[j];
    }
    const float lse = my + logf(s2), inv2 = 1.0f / s2;
    const bool label_ok = label >= 0 && label < C;
    float y_label = 0.f, dot = 0.f, g[kGeMaxC];
#pragma unroll
    for (int j = 0; j < kGeMaxC; ++j) {
        const bool hit = label_ok && j == (int)label;
        if (hit) y_label = y[j];
        g[j] = j < C ? p[j] * inv2 - (hit ? 1.0f : 0.0f) : 0.f;
        dot = fmaf(g[j], y[j], dot);
    }
    loss = label_ok ? lse - y_label : nanf("");
#pragma unroll
    for (int j = 0; j < kGeMaxC; ++j) dz[j] = label_ok ? y[j] * (g[j] - dot) : 0.f;
}

__device__ inline void ge_load_row(const float* __restrict__ h, int bag, int d, int lane, float (&hk)[kGeMaxPerLane]) {
    const int per_lane = d / 64;
#pragma unroll
    for (int t = 0; t < kGeMaxPerLane; ++t) hk[t] = t < per_lane ? h[(size_t)bag * d + lane + 64 * t] : 0.f;
}

// grid = n_bags, block = 64
__global__ void __launch_bounds__(64) ge_head_loss_fwd_kernel(const float* __restrict__ h, const float* __restrict__ w,
                                                              const float* __restrict__ bias, const long long* __restrict__ label,
                                                              float* __restrict__ y_out, float* __restrict__ loss_out, int B, int d,
                                                              int C) {
    const int bag = blockIdx.x, lane = threadIdx.x;
    if (bag >= B) return;
    float hk[kGeMaxPerLane], y[kGeMaxC], dz[kGeMaxC], loss;
    ge_load_row(h, bag, d, lane, hk);
    ge_head_bag(hk, w, bias, d, C, label[bag], lane, y, loss, dz);
    if (lane == 0) loss_out[bag] = loss;
#pragma unroll
    for (int j = 0; j < kGeMaxC; ++j)
        if (lane == j && j < C) y_out[(size_t)bag * C + j] = y[j];
}

// grid = n_bags + n_classes, block = 64.  Workgroup `bag` < n_bags writes row `bag` of d_h; workgroup n_bags + j walks the
// bags in order and writes row j of dW and db[j] (a fixed summation order: no atomics, the same bits on every run).
__global__ void __launch_bounds__(64) ge_head_loss_bwd_kernel(const float* __restrict__ h, const float* __restrict__ w,
                                                              const float* __restrict__ bias, const long long* __restrict__ label,
                                                              const float* __restrict__ d_loss, float* __restrict__ d_h,
                                                              float* __restrict__ d_w, float* __restrict__ d_b, int B, int d, int C) {
    const int lane = threadIdx.x, per_lane = d / 64;
    float hk[kGeMaxPerLane], y[kGeMaxC], dz[kGeMaxC], loss;
    if ((int)blockIdx.x < B) {
        const int bag = blockIdx.x;
        ge_load_row(h, bag, d, lane, hk);
        ge_head_bag(hk, w, bias, d, C, label[bag], lane, y, loss, dz);
        const float g = d_loss[bag];
#pragma unroll
        for (int t = 0; t < kGeMaxPerLane; ++t) {
            if (t >= per_lane) break;
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < kGeMaxC; ++j)
                if (j < C) acc = fmaf(dz[j], w[(size_t)j * d + lane + 64 * t], acc);
            d_h[(size_t)bag * d + lane + 64 * t] = g * acc;
        }
        return;
    }
    const int cls = (int)blockIdx.x - B;
    if (cls >= C) return;
    float acc[kGeMaxPerLane], acc_b = 0.f;
#pragma unroll
    for (int t = 0; t < kGeMaxPerLane; ++t) acc[t] = 0.f;
    for (int bag = 0; bag < B; ++bag) {
        ge_load_row(h, bag, d, lane, hk);
        ge_head_bag(hk, w, bias, d, C, label[bag], lane, y, loss, dz);
        float mine = 0.f;
#pragma unroll
        for (int j = 0; j < kGeMaxC; ++j)
            if (j == cls) mine = dz[j];
        mine *= d_loss[bag];
        acc_b += mine;
#pragma unroll
        for (int t = 0; t < kGeMaxPerLane; ++t) acc[t] = fmaf(mine, hk[t], acc[t]);
    }
#pragma unroll
    for (int t = 0; t < kGeMaxPerLane; ++t)
        if (t < per_lane) d_w[(size_t)cls * d + lane + 64 * t] = acc[t];
    if (lane == 0) d_b[cls] = acc_b;
}

int ge_head_geometry(const char* what, int n_bags, int d, int n_classes) {
    MPO_CHECK(n_bags >= 1 && n_bags <= (1 << 20), "%s: %d bags (1 .. 2^20)", what, n_bags);
    MPO_CHECK(d == 128 || d == 256 || d == 512, "%s: d = %d is not a width the kernel is built for (128, 256 or 512)", what, d);
    MPO_CHECK(n_classes >= 2 && n_classes <= kGeMaxC, "%s: %d classes (2 .. %d)", what, n_classes, kGeMaxC);
    return 0;
}

}  // namespace

extern "C" {

int mpo_ge_head_loss_forward(const float* h, int n_bags, int d, int n_classes, const float* const* params, const int64_t* label,
                             float* y, float* loss, mpo_stream_t stream) {
    MPO_CHECK(h && params && label && y && loss, "ge head + ce loss forward: null argument");
    MPO_CHECK(params[0] && params[1], "ge head + ce loss forward: null parameter");
    RC(ge_head_geometry("ge head + ce loss forward", n_bags, d, n_classes));
    ge_head_loss_fwd_kernel<<<n_bags, 64, 0, static_cast<hipStream_t>(stream)>>>(
        h, params[0], params[1], reinterpret_cast<const long long*>(label), y, loss, n_bags, d, n_classes);
    MPO_LAUNCH_CHECK();
    return 0;
}

int mpo_ge_head_loss_backward(const float* h, int n_bags, int d, int n_classes, const float* const* params, const int64_t* label,
                              const float* d_loss, float* d_h, float* const* grads, mpo_stream_t stream) {
    MPO_CHECK(h && params && label && d_loss && d_h && grads, "ge head + ce loss backward: null argument");
    MPO_CHECK(params[0] && params[1] && grads[0] && grads[1], "ge head + ce loss backward: null parameter or gradient");
    RC(ge_head_geometry("ge head + ce loss backward", n_bags, d, n_classes));
    ge_head_loss_bwd_kernel<<<n_bags + n_classes, 64, 0, static_cast<hipStream_t>(stream)>>>(
        h, params[0], params[1], reinterpret_cast<const long long*>(label), d_loss, d_h, grads[0], grads[1], n_bags, d, n_classes);
    MPO_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
