// Kernels of the two fusion layers beside `concat`, for the heads of include/mpo_fusion_next.h.  fp32 FMA throughout (the
// sigmoids through __expf, as the head kernels of tail.hip).
//
// 1. The gates of GatedConcatFusion (models/fusion.py:22-41) in front of K6: per (slide, branch) row x of d floats
//     g = sigmoid(w . x + b),   hcat[slide][branch * d ..] = x * g
// and their backward.  Rows are a handful (2 per slide of the window) and d <= 512: one wave per row, float4 lanes.
// 2. BilinearFusion (models/fusion.py:44-113), below: the pass over the nn.Bilinear weights each way, the Kronecker product +
// post_fusion_dropout + fc1 each way, and the element-wise glue between the GEMM launches of tail_api.hip.
#include "mpo_common.h"
#include "mpo_kernels.h"

namespace {

constexpr int kGateWaves = 4;                     // rows (waves) per workgroup of the two row kernels
constexpr int kGateThreads = 64 * kGateWaves;
constexpr int kGateParamCols = 64;                // columns (threads) per workgroup of the parameter-gradient kernel

struct GateBranches {
    const float* x[2];        // [n_slides] rows of d floats, row stride ldx
    const float* w[2];        // [d]
    const float* b[2];        // [1]
    float* dx[2];             // backward: like x
    float* dw[2];             // backward: [d]
    float* db[2];             // backward: [1]
};

// row r = slide * 2 + branch
__global__ void __launch_bounds__(kGateThreads)
gate_concat_fwd_kernel(GateBranches P, int ldx, float* __restrict__ hcat, float* __restrict__ g_out, int n_slides, int d) {
    const int row = blockIdx.x * kGateWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= 2 * n_slides) return;
    const int slide = row >> 1, br = row & 1, d4 = d >> 2;
    const float4* x = reinterpret_cast<const float4*>(P.x[br] + (size_t)slide * ldx);
    const float4* w = reinterpret_cast<const float4*>(P.w[br]);
    float4* out = reinterpret_cast<float4*>(hcat + (size_t)slide * 2 * d + (size_t)br * d);
    float dot = 0.f;
    for (int i = lane; i < d4; i += 64) {
        const float4 xv = x[i], wv = w[i];
        dot += xv.x * wv.x + xv.y * wv.y + xv.z * wv.z + xv.w * wv.w;
    }
    dot = wave_sum(dot) + P.b[br][0];
    const float g = 1.f / (1.f + __expf(-dot));
    for (int i = lane; i < d4; i += 64) {
        const float4 xv = x[i];
        out[i] = make_float4(xv.x * g, xv.y * g, xv.z * g, xv.w * g);
    }
    if (lane == 0) g_out[row] = g;
}

// dx = dh g + t w with t = (dh . x) g (1 - g); t goes to t_out [2 n_slides] for the parameter gradients
__global__ void __launch_bounds__(kGateThreads)
gate_concat_bwd_rows_kernel(GateBranches P, int ldx, const float* __restrict__ d_hcat, const float* __restrict__ g_in,
                            float* __restrict__ t_out, int n_slides, int d) {
    const int row = blockIdx.x * kGateWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= 2 * n_slides) return;
    const int slide = row >> 1, br = row & 1, d4 = d >> 2;
    const float4* x = reinterpret_cast<const float4*>(P.x[br] + (size_t)slide * ldx);
    const float4* w = reinterpret_cast<const float4*>(P.w[br]);
    const float4* dh = reinterpret_cast<const float4*>(d_hcat + (size_t)slide * 2 * d + (size_t)br * d);
    float4* dx = reinterpret_cast<float4*>(P.dx[br] + (size_t)slide * ldx);
    float s = 0.f;
    for (int i = lane; i < d4; i += 64) {
        const float4 xv = x[i], dv = dh[i];
        s += xv.x * dv.x + xv.y * dv.y + xv.z * dv.z + xv.w * dv.w;
    }
    const float g = g_in[row];
    const float t = wave_sum(s) * g * (1.f - g);
    for (int i = lane; i < d4; i += 64) {
        const float4 dv = dh[i], wv = w[i];
        dx[i] = make_float4(dv.x * g + t * wv.x, dv.y * g + t * wv.y, dv.z * g + t * wv.z, dv.w * g + t * wv.w);
    }
    if (lane == 0) t_out[row] = t;
}

// dw[j] = sum_b t[b] x[b][j], db = sum_b t[b]: one thread per element, slides in order (a fixed sum, no atomics)
__global__ void __launch_bounds__(kGateParamCols)
gate_concat_bwd_params_kernel(GateBranches P, int ldx, const float* __restrict__ t_in, int n_slides, int d) {
    const int br = blockIdx.y, j = blockIdx.x * kGateParamCols + threadIdx.x;
    if (j > d) return;
    const float* x = P.x[br];
    float acc = 0.f;
    if (j < d) {
        for (int b = 0; b < n_slides; ++b) acc = fmaf(t_in[2 * b + br], x[(size_t)b * ldx + j], acc);
        P.dw[br][j] = acc;
    } else {                                      // the thread after the last column sums the bias gradient
        for (int b = 0; b < n_slides; ++b) acc += t_in[2 * b + br];
        P.db[br][0] = acc;
    }
}

GateBranches branches_of(const float* x0, const float* x1, const float* const* params) {
    GateBranches P = {};
    P.x[0] = x0; P.x[1] = x1;
    for (int br = 0; br < 2; ++br) { P.w[br] = params[2 * br]; P.b[br] = params[2 * br + 1]; }
    return P;
}

}  // namespace

int mpo_check_gate_concat(const float* x0, const float* x1, int ldx, int n_slides, int d) {
    MPO_CHECK(d == 128 || d == 256 || d == 512, "gated concat: d %d is not 128, 256 or 512", d);
    MPO_CHECK(n_slides >= 1 && n_slides <= (1 << 28), "gated concat: n_slides %d not in 1..2^28", n_slides);
    MPO_CHECK(ldx >= d && (ldx & 3) == 0, "gated concat: row stride %d is not a multiple of 4 that is >= d = %d", ldx, d);
    MPO_CHECK(((uintptr_t)x0 & 15) == 0 && ((uintptr_t)x1 & 15) == 0, "gated concat: a row pointer is not 16-byte aligned");
    return 0;
}

int mpo_launch_gate_concat_fwd(const float* x0, const float* x1, int ldx, const float* const* params, float* hcat, float* g,
                               int n_slides, int d, hipStream_t s) {
    RC(mpo_check_gate_concat(x0, x1, ldx, n_slides, d));
    const GateBranches P = branches_of(x0, x1, params);
    gate_concat_fwd_kernel<<<(2 * n_slides + kGateWaves - 1) / kGateWaves, kGateThreads, 0, s>>>(P, ldx, hcat, g, n_slides, d);
    MPO_LAUNCH_CHECK();
    return 0;
}

int mpo_launch_gate_concat_bwd(const float* x0, const float* x1, int ldx, const float* const* params, const float* d_hcat,
                               const float* g, float* t, float* dx0, float* dx1, float* const* grads, int n_slides, int d,
                               hipStream_t s) {
    RC(mpo_check_gate_concat(x0, x1, ldx, n_slides, d));
    RC(mpo_check_gate_concat(dx0, dx1, ldx, n_slides, d));
    GateBranches P = branches_of(x0, x1, params);
    P.dx[0] = dx0; P.dx[1] = dx1;
    for (int br = 0; br < 2; ++br) { P.dw[br] = grads[2 * br]; P.db[br] = grads[2 * br + 1]; }
    gate_concat_bwd_rows_kernel<<<(2 * n_slides + kGateWaves - 1) / kGateWaves, kGateThreads, 0, s>>>(P, ldx, d_hcat, g, t,
                                                                                                    n_slides, d);
    MPO_LAUNCH_CHECK();
    gate_concat_bwd_params_kernel<<<dim3(d / kGateParamCols + 1, 2), kGateParamCols, 0, s>>>(P, ldx, t, n_slides, d);
    MPO_LAUNCH_CHECK();
    return 0;
}


// ================================================================================================ BilinearFusion
namespace {

constexpr int kBilH = 32;          // hidden_size: outputs of linear_h / linear_z / linear_o
constexpr int kBilM = 64;          // mm_hidden_size: outputs of fc1
constexpr int kBilO = kBilH + 1;   // [o | 1]
constexpr int kBilKron = kBilO * kBilO;          // 1089
constexpr int kBilCat = kBilM + 2 * kBilO;       // 130: fc2's input row [u | o1' | o2']
constexpr int kBilChunks = 4;      // row chunks of one W_k: the W pass runs on kBilChunks x 32 x 2 = 256 workgroups
constexpr int kBilTile = 1024;     // float4 of x a workgroup keeps in LDS: kBilTile / (d / 4) slides per slide tile
constexpr int kBilWaves = 8;       // waves of a workgroup of the W pass: a row of the chunk each, two per SIMD
constexpr int kBilThreads = 64 * kBilWaves;

struct BilArgs {
    const float* x[2];             // h_path, h_omic: [B] rows of d floats, stride ld.  Branch br: a = x[br], x = x[br ^ 1]
    const float* wz[2];            // linear_z{1,2}.weight [32][d][d]
    float* dwz[2];                 // backward
};

__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ void fma4(float4& acc, float c, float4 v) {
    acc.x = fmaf(c, v.x, acc.x); acc.y = fmaf(c, v.y, acc.y); acc.z = fmaf(c, v.z, acc.z); acc.w = fmaf(c, v.w, acc.w);
}

// z partials: zp[br][k][chunk][b] = sum_{i in chunk} a[b][i] sum_j W[k][i][j] x[b][j].  Workgroup (chunk, k, br), a wave per row
// i, lanes over j (NS float4 per lane: d = 256 NS, or 128 with half the lanes), TB slides of x in LDS per slide tile.
template <int NS, int TB>
__global__ void __launch_bounds__(kBilThreads)
bilinear_z_fwd_kernel(BilArgs A, int ld, float* __restrict__ zp, int B, int d) {
    __shared__ float4 xs[kBilTile];
    __shared__ float as[kBilTile];             // a[b][i] of the tile's slides and the chunk's rows: TB * d / kBilChunks <= kBilTile
    __shared__ float red[kBilWaves][TB];
    const int ch = blockIdx.x, k = blockIdx.y, br = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, d4 = d >> 2;
    const float* a = A.x[br];
    const float* x = A.x[br ^ 1];
    const float* W = A.wz[br] + (size_t)k * d * d;
    const int rows = d / kBilChunks, i0 = ch * rows;
    for (int b0 = 0; b0 < B; b0 += TB) {
        const int nb = min(TB, B - b0);
        __syncthreads();
        for (int e = threadIdx.x; e < nb * d4; e += kBilThreads) {
            const int b = e / d4, s = e - b * d4;
            xs[e] = reinterpret_cast<const float4*>(x + (size_t)(b0 + b) * ld)[s];
        }
        for (int e = threadIdx.x; e < nb * rows; e += kBilThreads) {
            const int b = e / rows, r = e - b * rows;
            as[e] = a[(size_t)(b0 + b) * ld + i0 + r];
        }
        __syncthreads();
        float acc[TB];
#pragma unroll
        for (int b = 0; b < TB; ++b) acc[b] = 0.f;
        float4 w[NS], wn[NS];                   // this row and the wave's next one (loaded a row ahead)
#pragma unroll
        for (int s = 0; s < NS; ++s)
            wn[s] = lane + 64 * s < d4 ? reinterpret_cast<const float4*>(W + (size_t)(i0 + wave) * d)[lane + 64 * s] : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int r = wave; r < rows; r += kBilWaves) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                w[s] = wn[s];
                if (r + kBilWaves < rows && lane + 64 * s < d4)
                    wn[s] = reinterpret_cast<const float4*>(W + (size_t)(i0 + r + kBilWaves) * d)[lane + 64 * s];
            }
#pragma unroll
            for (int b = 0; b < TB; ++b) {
                if (b < nb) {
                    float t = 0.f;
#pragma unroll
                    for (int s = 0; s < NS; ++s)
                        if (lane + 64 * s < d4) t += dot4(w[s], xs[b * d4 + lane + 64 * s]);
                    acc[b] = fmaf(as[b * rows + r], t, acc[b]);
                }
            }
        }
#pragma unroll
        for (int b = 0; b < TB; ++b) {
            const float v = wave_sum(acc[b]);
            if (lane == 0) red[wave][b] = v;
        }
        __syncthreads();
        if ((int)threadIdx.x < nb) {
            const int t = threadIdx.x;
            float v = red[0][t];
            for (int wv = 1; wv < kBilWaves; ++wv) v += red[wv][t];
            zp[(((size_t)br * kBilH + k) * kBilChunks + ch) * B + b0 + t] = v;
        }
    }
}

// z = bias + the chunk partials in order; sz = sigmoid(z); gated = sz * h.  One thread per (branch, slide, k).
__global__ void __launch_bounds__(256)
bilinear_gate_fwd_kernel(const float* __restrict__ zp, const float* bz0, const float* bz1, const float* __restrict__ h,
                         float* __restrict__ sz, float* __restrict__ gated, int B) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * B * kBilH) return;
    const int k = e % kBilH, b = (e / kBilH) % B, br = e / (kBilH * B);
    float z = (br ? bz1 : bz0)[k];
    for (int ch = 0; ch < kBilChunks; ++ch) z += zp[(((size_t)br * kBilH + k) * kBilChunks + ch) * B + b];
    const float s = 1.f / (1.f + __expf(-z));
    sz[e] = s;
    gated[e] = s * h[e];
}
// dz = dgated h sz (1 - sz), dh = dgated sz (the ReLU of linear_h is the gate of the GEMMs that read dh)
__global__ void __launch_bounds__(256)
bilinear_gate_bwd_kernel(const float* __restrict__ dgated, const float* __restrict__ h, const float* __restrict__ sz,
                         float* __restrict__ dz, float* __restrict__ dh, int B) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * B * kBilH) return;
    const float g = dgated[e], s = sz[e];
    dz[e] = g * h[e] * s * (1.f - s);
    dh[e] = g * s;
}

struct BilDrop {                   // the call's counters: site s starts at off + s * stride (epoch applied by the kernel)
    float p;
    unsigned long long seed, off, stride;
    const unsigned long long* epoch;
};

__device__ __forceinline__ float o_ext(const float* o, int B, int br, int b, int p) {     // [o | 1] of branch br
    return p < kBilH ? o[((size_t)br * B + b) * kBilH + p] : 1.f;
}

// u[b][m] = drop3(relu(sum_e W1[m][e] o1'[p] o2'[q] keep2[b][e] + b1[m])), e = 33 p + q; and the packed fc2 row
// cat[b] = [u | o1' | o2'].  Workgroup (slide, quarter of the 64 outputs): the product lives in LDS only.
__global__ void __launch_bounds__(256)
bilinear_kron_fc1_fwd_kernel(const float* __restrict__ o, const float* __restrict__ W1, const float* __restrict__ b1,
                             float* __restrict__ cat, int B, BilDrop D) {
    __shared__ float kr[kBilKron];
    const int b = blockIdx.x, mq = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float inv_keep = D.p > 0.f ? 1.f / (1.f - D.p) : 1.f;
    const unsigned long long base = epoch_offset(D.off, D.epoch);
    for (int e = threadIdx.x; e < kBilKron; e += 256) {
        const int p = e / kBilO, q = e - p * kBilO;
        float v = o_ext(o, B, 0, b, p) * o_ext(o, B, 1, b, q);
        if (D.p > 0.f) v *= dropout_keep(D.seed, base + 2 * D.stride, (unsigned long long)b * kBilKron + e, D.p, inv_keep);
        kr[e] = v;
    }
    __syncthreads();
    for (int r = 0; r < kBilM / 16; ++r) {
        const int m = mq * (kBilM / 4) + wave * (kBilM / 16) + r;
        float acc = 0.f;
        for (int e = lane; e < kBilKron; e += 64) acc = fmaf(W1[(size_t)m * kBilKron + e], kr[e], acc);
        acc = wave_sum(acc);
        if (lane == 0) {
            float u = relu_keep_nan(acc + b1[m]);
            if (D.p > 0.f) u *= dropout_keep(D.seed, base + 3 * D.stride, (unsigned long long)b * kBilM + m, D.p, inv_keep);
            cat[(size_t)b * kBilCat + m] = u;
        }
    }
    if (mq == 0 && threadIdx.x < 2 * kBilO) {
        const int br = threadIdx.x / kBilO, p = threadIdx.x % kBilO;
        cat[(size_t)b * kBilCat + kBilM + threadIdx.x] = o_ext(o, B, br, b, p);
    }
}

// per slide: du = dcat[:, :64] * relu'/drop3'(u) (kept in dupre for the weight gradient); d_kron[e] = keep2 sum_m du[m] W1[m][e];
// d_o1[p] = sum_q d_kron[p][q] o2'[q] + dcat[64 + p], d_o2[q] = sum_p d_kron[p][q] o1'[p] + dcat[97 + q]   (p, q < 32)
__global__ void __launch_bounds__(256)
bilinear_kron_fc1_bwd_rows_kernel(const float* __restrict__ o, const float* __restrict__ W1, const float* __restrict__ cat,
                                  const float* __restrict__ dcat, float* __restrict__ dupre, float* __restrict__ d_o, int B,
                                  BilDrop D) {
    __shared__ float du[kBilM];
    __shared__ float dkr[kBilKron];
    const int b = blockIdx.x;
    const float inv_keep = D.p > 0.f ? 1.f / (1.f - D.p) : 1.f;
    const unsigned long long base = epoch_offset(D.off, D.epoch);
    if (threadIdx.x < kBilM) {
        const int m = threadIdx.x;
        // (a NaN activation gives a NaN gradient: db1 has no activation factor that would carry the slide's NaN otherwise)
        const float c = cat[(size_t)b * kBilCat + m];
        const float v = c > 0.f ? dcat[(size_t)b * kBilCat + m] * inv_keep : (c == c ? 0.f : c);
        du[m] = v;
        dupre[(size_t)b * kBilM + m] = v;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kBilKron; e += 256) {
        float g = 0.f;
        for (int m = 0; m < kBilM; ++m) g = fmaf(du[m], W1[(size_t)m * kBilKron + e], g);
        if (D.p > 0.f) g *= dropout_keep(D.seed, base + 2 * D.stride, (unsigned long long)b * kBilKron + e, D.p, inv_keep);
        dkr[e] = g;
    }
    __syncthreads();
    if (threadIdx.x < 2 * kBilH) {
        const int br = threadIdx.x / kBilH, p = threadIdx.x % kBilH;
        float acc = dcat[(size_t)b * kBilCat + kBilM + br * kBilO + p];
        for (int q = 0; q < kBilO; ++q)
            acc = fmaf(br == 0 ? dkr[p * kBilO + q] : dkr[q * kBilO + p], o_ext(o, B, br ^ 1, b, q), acc);
        d_o[((size_t)br * B + b) * kBilH + p] = acc;
    }
}
// dW1[m][e] = sum_b du[b][m] o1'[b][p] o2'[b][q] keep2[b][e] (slides in order, one thread per 16 outputs of one e), db1 = sum_b du
__global__ void __launch_bounds__(256)
bilinear_kron_fc1_bwd_params_kernel(const float* __restrict__ o, const float* __restrict__ dupre, float* __restrict__ dW1,
                                    float* __restrict__ db1, int B, BilDrop D) {
    const int e = blockIdx.x * 64 + (threadIdx.x & 63), mg = threadIdx.x >> 6;
    const float inv_keep = D.p > 0.f ? 1.f / (1.f - D.p) : 1.f;
    const unsigned long long base = epoch_offset(D.off, D.epoch);
    if (e < kBilKron) {
        const int p = e / kBilO, q = e - p * kBilO;
        float acc[kBilM / 4];
#pragma unroll
        for (int r = 0; r < kBilM / 4; ++r) acc[r] = 0.f;
        for (int b = 0; b < B; ++b) {
            float v = o_ext(o, B, 0, b, p) * o_ext(o, B, 1, b, q);
            if (D.p > 0.f) v *= dropout_keep(D.seed, base + 2 * D.stride, (unsigned long long)b * kBilKron + e, D.p, inv_keep);
#pragma unroll
            for (int r = 0; r < kBilM / 4; ++r) acc[r] = fmaf(dupre[(size_t)b * kBilM + mg * (kBilM / 4) + r], v, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < kBilM / 4; ++r) dW1[(size_t)(mg * (kBilM / 4) + r) * kBilKron + e] = acc[r];
    }
    if (blockIdx.x == 0 && threadIdx.x < kBilM) {
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += dupre[(size_t)b * kBilM + threadIdx.x];
        db1[threadIdx.x] = acc;
    }
}

// One pass over W for its three gradients.  Workgroup (chunk, k, br), a wave per row i, lanes over j, c[b] = dz[b][k] a[b][i]:
//   dW[k][i][j]        = sum_b c[b] x[b][j]                       (stored by the one thread that owns it; a window of more
//                                                                   than TB slides adds its later tiles to it, in order)
//   da_part[br][k][b][i] = dz[b][k] sum_j W[k][i][j] x[b][j]      (summed over k by bilinear_finish_kernel)
//   dx_part[br][k][chunk][b][j] = sum_{i in chunk} c[b] W[k][i][j] (the waves' sums added in LDS in wave order)
template <int NS, int TB>
__global__ void __launch_bounds__(kBilThreads)
bilinear_z_bwd_kernel(BilArgs A, int ld, const float* __restrict__ dz, float* __restrict__ da_part, float* __restrict__ dx_part,
                      int B, int d) {
    __shared__ float4 xs[kBilTile];
    __shared__ float cs[kBilTile];             // c[b][i] = dz[b][k] a[b][i] of the tile's slides and the chunk's rows
    __shared__ float dzs[TB];
    __shared__ float4 red[kBilWaves][64 * NS];
    const int ch = blockIdx.x, k = blockIdx.y, br = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, d4 = d >> 2;
    const float* a = A.x[br];
    const float* x = A.x[br ^ 1];
    const float* W = A.wz[br] + (size_t)k * d * d;
    float* dW = A.dwz[br] + (size_t)k * d * d;
    const float* dzk = dz + (size_t)br * B * kBilH + k;
    const int rows = d / kBilChunks, i0 = ch * rows;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b0 = 0; b0 < B; b0 += TB) {
        const int nb = min(TB, B - b0);
        __syncthreads();
        for (int e = threadIdx.x; e < nb * d4; e += kBilThreads) {
            const int b = e / d4, s = e - b * d4;
            xs[e] = reinterpret_cast<const float4*>(x + (size_t)(b0 + b) * ld)[s];
        }
        for (int e = threadIdx.x; e < nb * rows; e += kBilThreads) {
            const int b = e / rows, r = e - b * rows;
            cs[e] = dzk[(size_t)(b0 + b) * kBilH] * a[(size_t)(b0 + b) * ld + i0 + r];
        }
        if ((int)threadIdx.x < nb) dzs[threadIdx.x] = dzk[(size_t)(b0 + threadIdx.x) * kBilH];
        __syncthreads();
        float4 dxacc[TB][NS];
#pragma unroll
        for (int b = 0; b < TB; ++b)
#pragma unroll
            for (int s = 0; s < NS; ++s) dxacc[b][s] = zero;
        float4 wn[NS];                          // the wave's next row, loaded a row ahead
#pragma unroll
        for (int s = 0; s < NS; ++s)
            wn[s] = lane + 64 * s < d4 ? reinterpret_cast<const float4*>(W + (size_t)(i0 + wave) * d)[lane + 64 * s] : zero;
        for (int r = wave; r < rows; r += kBilWaves) {
            const int i = i0 + r;
            float4 w[NS], dw[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const bool in = lane + 64 * s < d4;
                w[s] = wn[s];
                if (in && r + kBilWaves < rows) wn[s] = reinterpret_cast<const float4*>(W + (size_t)(i + kBilWaves) * d)[lane + 64 * s];
                dw[s] = in && b0 > 0 ? reinterpret_cast<const float4*>(dW + (size_t)i * d)[lane + 64 * s] : zero;
            }
#pragma unroll
            for (int b = 0; b < TB; ++b) {
                if (b < nb) {
                    const float dzb = dzs[b];
                    const float c = cs[b * rows + r];
                    float t = 0.f;
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        if (lane + 64 * s < d4) {
                            const float4 xv = xs[b * d4 + lane + 64 * s];
                            t += dot4(w[s], xv);
                            fma4(dw[s], c, xv);
                            fma4(dxacc[b][s], c, w[s]);
                        }
                    }
                    t = wave_sum(t);
                    if (lane == 0) da_part[(((size_t)br * kBilH + k) * B + b0 + b) * d + i] = dzb * t;
                }
            }
#pragma unroll
            for (int s = 0; s < NS; ++s)
                if (lane + 64 * s < d4) reinterpret_cast<float4*>(dW + (size_t)i * d)[lane + 64 * s] = dw[s];
        }
#pragma unroll
        for (int b = 0; b < TB; ++b) {
            if (b < nb) {
                __syncthreads();
#pragma unroll
                for (int s = 0; s < NS; ++s) red[wave][lane + 64 * s] = dxacc[b][s];
                __syncthreads();
                float4* out = reinterpret_cast<float4*>(dx_part + ((((size_t)br * kBilH + k) * kBilChunks + ch) * B + b0 + b) * d);
                for (int s = threadIdx.x; s < d4; s += kBilThreads) {
                    float4 v = red[0][s];
                    for (int wv = 1; wv < kBilWaves; ++wv) { v.x += red[wv][s].x; v.y += red[wv][s].y; v.z += red[wv][s].z; v.w += red[wv][s].w; }
                    out[s] = v;
                }
            }
        }
    }
}

// d_x[which][b][j] (holding linear_h's part) += sum_k da_part[which][k][b][j] + sum_{k, chunk} dx_part[which ^ 1][k][chunk][b][j],
// in that order; the 64 threads after the last element: db_z[br][k] = sum_b dz[br][b][k]
__global__ void __launch_bounds__(256)
bilinear_finish_kernel(const float* __restrict__ da_part, const float* __restrict__ dx_part, const float* __restrict__ dz,
                       float* dx0, float* dx1, int ld, float* dbz0, float* dbz1, int B, int d) {
    const size_t n = (size_t)B * d;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < 2 * n) {
        const int which = e >= n;
        const size_t r = e - which * n;
        const size_t b = r / d, j = r - b * d;
        float* out = (which ? dx1 : dx0) + b * ld + j;
        float acc = *out;
        for (int k = 0; k < kBilH; ++k) acc += da_part[((size_t)which * kBilH + k) * n + r];
        for (int kc = 0; kc < kBilH * kBilChunks; ++kc) acc += dx_part[((size_t)(which ^ 1) * kBilH * kBilChunks + kc) * n + r];
        *out = acc;
    } else if (e - 2 * n < 2 * kBilH) {
        const int t = (int)(e - 2 * n), br = t / kBilH, k = t % kBilH;
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += dz[((size_t)br * B + b) * kBilH + k];
        (br ? dbz1 : dbz0)[k] = acc;
    }
}

BilDrop drop_of(float p, unsigned long long seed, unsigned long long off, const unsigned long long* epoch, int B) {
    BilDrop D;
    D.p = p; D.seed = seed; D.off = off; D.epoch = epoch; D.stride = mpo_bilinear_stream_stride(B);
    return D;
}

}  // namespace

unsigned long long mpo_bilinear_stream_stride(int n_slides) { return ((unsigned long long)n_slides * kBilKron + 3) / 4 + 2; }

int mpo_check_bilinear(const float* x0, const float* x1, int ldx, int n_slides, int d, int hidden, int mm_hidden) {
    MPO_CHECK(hidden == kBilH, "bilinear fusion: hidden_size %d is not %d, the one the kernels are built for", hidden, kBilH);
    MPO_CHECK(mm_hidden == kBilM, "bilinear fusion: mm_hidden_size %d is not %d, the one the kernels are built for", mm_hidden, kBilM);
    MPO_CHECK(d == 128 || d == 256 || d == 512, "bilinear fusion: d %d is not 128, 256 or 512", d);
    MPO_CHECK(n_slides >= 1 && n_slides <= (1 << 20), "bilinear fusion: n_slides %d not in 1..2^20", n_slides);
    MPO_CHECK(ldx >= d && (ldx & 3) == 0, "bilinear fusion: row stride %d is not a multiple of 4 that is >= d = %d", ldx, d);
    MPO_CHECK(((uintptr_t)x0 & 15) == 0 && ((uintptr_t)x1 & 15) == 0, "bilinear fusion: a row pointer is not 16-byte aligned");
    return 0;
}

int mpo_launch_bilinear_z_fwd(const float* x0, const float* x1, int ld, const float* wz0, const float* wz1, float* zp, int B, int d,
                              hipStream_t s) {
    BilArgs A = {};
    A.x[0] = x0; A.x[1] = x1; A.wz[0] = wz0; A.wz[1] = wz1;
    const dim3 grid(kBilChunks, kBilH, 2);
    if (d <= 256) bilinear_z_fwd_kernel<1, 16><<<grid, kBilThreads, 0, s>>>(A, ld, zp, B, d);
    else bilinear_z_fwd_kernel<2, 8><<<grid, kBilThreads, 0, s>>>(A, ld, zp, B, d);
    MPO_LAUNCH_CHECK();
    return 0;
}
int mpo_launch_bilinear_gate_fwd(const float* zp, const float* bz0, const float* bz1, const float* h, float* sz, float* gated, int B,
                                 hipStream_t s) {
    bilinear_gate_fwd_kernel<<<(2 * B * kBilH + 255) / 256, 256, 0, s>>>(zp, bz0, bz1, h, sz, gated, B);
    MPO_LAUNCH_CHECK();
    return 0;
}
int mpo_launch_bilinear_gate_bwd(const float* dgated, const float* h, const float* sz, float* dz, float* dh, int B, hipStream_t s) {
    bilinear_gate_bwd_kernel<<<(2 * B * kBilH + 255) / 256, 256, 0, s>>>(dgated, h, sz, dz, dh, B);
    MPO_LAUNCH_CHECK();
    return 0;
}
int mpo_launch_bilinear_kron_fc1_fwd(const float* o, const float* W1, const float* b1, float* cat, int B, float p,
                                     unsigned long long seed, unsigned long long off, const unsigned long long* epoch, hipStream_t s) {
    bilinear_kron_fc1_fwd_kernel<<<dim3(B, 4), 256, 0, s>>>(o, W1, b1, cat, B, drop_of(p, seed, off, epoch, B));
    MPO_LAUNCH_CHECK();
    return 0;
}
int mpo_launch_bilinear_kron_fc1_bwd(const float* o, const float* W1, const float* cat, const float* dcat, float* dupre, float* d_o,
                                     float* dW1, float* db1, int B, float p, unsigned long long seed, unsigned long long off,
                                     const unsigned long long* epoch, hipStream_t s) {
    const BilDrop D = drop_of(p, seed, off, epoch, B);
    bilinear_kron_fc1_bwd_rows_kernel<<<B, 256, 0, s>>>(o, W1, cat, dcat, dupre, d_o, B, D);
    MPO_LAUNCH_CHECK();
    bilinear_kron_fc1_bwd_params_kernel<<<(kBilKron + 63) / 64, 256, 0, s>>>(o, dupre, dW1, db1, B, D);
    MPO_LAUNCH_CHECK();
    return 0;
}
int mpo_launch_bilinear_z_bwd(const float* x0, const float* x1, int ld, const float* wz0, const float* wz1, const float* dz,
                              float* dwz0, float* dwz1, float* dbz0, float* dbz1, float* da_part, float* dx_part, float* dx0,
                              float* dx1, int B, int d, hipStream_t s) {
    BilArgs A = {};
    A.x[0] = x0; A.x[1] = x1; A.wz[0] = wz0; A.wz[1] = wz1; A.dwz[0] = dwz0; A.dwz[1] = dwz1;
    const dim3 grid(kBilChunks, kBilH, 2);
    if (d <= 256) bilinear_z_bwd_kernel<1, 16><<<grid, kBilThreads, 0, s>>>(A, ld, dz, da_part, dx_part, B, d);
    else bilinear_z_bwd_kernel<2, 8><<<grid, kBilThreads, 0, s>>>(A, ld, dz, da_part, dx_part, B, d);
    MPO_LAUNCH_CHECK();
    const size_t blocks = (2 * (size_t)B * d + 2 * kBilH + 255) / 256;
    bilinear_finish_kernel<<<(unsigned)blocks, 256, 0, s>>>(da_part, dx_part, dz, dx0, dx1, ld, dbz0, dbz1, B, d);
    MPO_LAUNCH_CHECK();
    return 0;
}
