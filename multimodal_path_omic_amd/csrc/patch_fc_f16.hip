// The patch layer for an fp16-stored window (feature extractors very commonly write fp16), hand-written forward and weight
// gradient, behind it the fp32 H_bag every fp32-bag kernel already takes.
//
//     H_bag = Dropout(ReLU(X W_H^T + b_H))          X [rows, 1024] fp16, W_H [256, 1024] fp32, H_bag [rows, 256] fp32
//     dW_H  = g^T X,  db_H = colsum(g),  g = dH (.) [H_bag > 0] / (1 - p)          (models/mcat/mcat.py:24-29,87 and its backward)
//
// The fp32 window's kernels (patch_fc_f32.hip) with one operand that needs no split: an fp16 X IS one fp16 MFMA operand.
//   * FORWARD: TWO-TERM products W_hi X + W_lo X with fp32 accumulation.  W_H goes through the fp32 file's range and pack
//     kernels unchanged (W x 2^k split into fp16 hi | lo in fragment order, 2^-k on the accumulator: exact); X is copied
//     global -> registers -> LDS as it is stored: no feature scale, no split, no lo image, no clamp.  The only rounding left
//     against the fp64 product of the stored operands is W's lo tail (2^-22 of a product) and the fp32 accumulation -- the
//     fp32 kernel's own level, so the ReLU mask flips no more often than there.  A NaN or an infinity among the features
//     reaches the MFMA as it is and makes its row of H_bag non-finite (every element of it: the epilogue keeps a -inf sum from
//     becoming a finite zero); fp16 subnormals are operands like any other.
//   * WEIGHT GRADIENT: the fp32 file's three bf16 terms.  An fp16 value splits into bf16 hi + lo EXACTLY (11 significand bits
//     fit 8 + 8, fp16's range lies inside bf16's); g is split as there.  (An fp16 form of g would need a range pass over dH.)
//
// Forward: the fp32 kernel's tiling -- one workgroup of 4 waves walking blocks of 128 rows, K-steps of 32, wave w owns embed
// columns 64 w .. + 63, product taken transposed, one 16-byte store per lane -- over ONE 8 KiB fp16 image per stage (64-byte
// rows, chunk c of row r at c ^ fswz(r)); the same epilogue: bias, NaN-keeping ReLU, the 8-bit dropout hash keyed by (row,
// column group): for the same (seed, offset, epoch) the mask is the fp32 kernel's.
// Weight gradient: patch_wgrad_f32_kernel with X arriving as 16 halves per thread; the same part / part_cs layout, the same
// reduction launch.
//
// Roofline: forward reads 2048 B and writes 1024 B per row (3 072 B / row: 2.5 GB per 8 x 100 000 window against the fp32
// window's 4.1 GB); 2 x 524 288 flop per row.
#include "patch_fc_split.h"

namespace {

constexpr int HNW = 4;                          // waves of the forward's workgroup (one per SIMD)

__global__ __launch_bounds__(64 * HNW, 1)
void patch_fc_f16_kernel(const _Float16* __restrict__ x,          // [total_rows][1024]
                         const f16x8* __restrict__ wpk,           // packed hi | lo (pack_patch_weight_f32_kernel)
                         const float* __restrict__ bias,          // [256]
                         float* __restrict__ h,                   // [total_rows][256]
                         long long total_rows, int rows_per_wg, float drop_p, unsigned long long seed,
                         unsigned long long offset_, const unsigned long long* __restrict__ epoch,
                         const float* __restrict__ w_scale) {
    __shared__ __attribute__((aligned(1024))) char lds[2 * FIMG];             // [stage]: one fp16 image each
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, g = lane >> 4;
    const long long wg_r0 = (long long)blockIdx.x * rows_per_wg;
    const long long wg_r1 = min(total_rows, wg_r0 + rows_per_wg);
    if (wg_r0 >= wg_r1) return;
    const int nblocks = (int)((wg_r1 - wg_r0 + FBM - 1) / FBM);

    constexpr int NCT = 16 / HNW;                                        // 16-column tiles a wave owns
    constexpr int NCHK = 2;                                              // 16-byte image chunks (8 halves) per thread and step
    // staging: thread (row = tid / 2, part = tid % 2) carries 16 consecutive k of its row -- the fp32 kernel's assignment, so
    // the same swizzle keeps the writes and the fragment reads off each other's banks (patch_fc_f32.hip)
    const int srow = tid >> 1, spart = tid & 1;
    const int sswz = fswz(srow);
    int soff[NCHK];
#pragma unroll
    for (int c = 0; c < NCHK; ++c) soff[c] = srow * FROWB + (((NCHK * spart + c) ^ sswz) << 4);
    // fragment reads: row 16 rt + c16, chunk g
    const int foff = c16 * FROWB + ((g ^ fswz(c16)) << 4);
    const f16x8* whi = wpk + (size_t)wave * (FSTEPS * 4 * 64) + lane;
    const f16x8* wlo = whi + FE * FK / 8;
    const uint32_t thr8 = (uint32_t)(drop_p * 256.0f + 0.5f);
    const float inv_keep = drop_p > 0.f ? 256.0f / (256.0f - (float)thr8) : 1.0f;
    const uint32_t drop_key = hash_stream_key(seed, epoch_offset(offset_, epoch));
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const float unscale = 1.0f / *w_scale;                        // (a power of two: exact)

    for (int blk = 0; blk < nblocks; ++blk) {
        const long long rb = wg_r0 + (long long)blk * FBM;
        const long long grow = min(rb + srow, total_rows - 1);           // rows past the end: clamped (never stored)
        const _Float16* xrow = x + (size_t)grow * FK + 8 * NCHK * spart;
        f32x4 acc[NCT][8];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int rt = 0; rt < 8; ++rt) acc[ct][rt] = zero4;
        // Operand pipeline as in the fp32 kernel: three register sets in static rotation, step k multiplies the image of x(k)
        // (LDS stage k & 1) by weight set k % 3, requests x(k + 2) and the weight fragments of step k + 2, and writes
        // x(k + 1) -- requested in the previous step -- into the other stage after the step's MFMAs are issued.
        f16x8 xs[3][NCHK];
        f16x8 wh[3][NCT], wl[3][NCT];
        auto load_x = [&](f16x8 (&dst)[NCHK], int k) {
            k = k < FSTEPS ? k : FSTEPS - 1;                              // (past the end: re-reads the last tile, never used)
#pragma unroll
            for (int j = 0; j < NCHK; ++j) dst[j] = *reinterpret_cast<const f16x8*>(xrow + FBK * k + 8 * j);
        };
        auto load_w = [&](f16x8 (&h_)[NCT], f16x8 (&l_)[NCT], int k) {
            k = k < FSTEPS ? k : FSTEPS - 1;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                h_[ct] = whi[(k * 4 + ct) * 64];
                l_[ct] = wlo[(k * 4 + ct) * 64];
            }
        };
        auto write_tile = [&](const f16x8 (&src)[NCHK], char* st) {
#pragma unroll
            for (int c = 0; c < NCHK; ++c) *reinterpret_cast<f16x8*>(st + soff[c]) = src[c];
        };
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            load_x(xs[j], j);
            load_w(wh[j], wl[j], j);
        }
        write_tile(xs[0], lds);
        // one K-step with the register sets named statically: j = k % 3
        auto step = [&](int k, const f16x8 (&wh_)[NCT], const f16x8 (&wl_)[NCT], f16x8 (&whn)[NCT], f16x8 (&wln)[NCT], f16x8 (&xn)[NCHK],
                        const f16x8 (&xwrite)[NCHK]) {
            const char* st = lds + (k & 1) * FIMG;
            __syncthreads();                                              // the image of x(k) is complete; the other stage is free
            load_x(xn, k + 2);
            load_w(whn, wln, k + 2);
            f16x8 xf[8];
#pragma unroll
            for (int rt = 0; rt < 8; ++rt) xf[rt] = *reinterpret_cast<const f16x8*>(st + rt * 16 * FROWB + foff);
#pragma unroll
            for (int rt = 0; rt < 8; ++rt) {
                // term-major: the two MFMAs of one accumulator are DEPENDENT; with the four column tiles in between every
                // MFMA finds its accumulator ready
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) acc[ct][rt] = mfma_f16(wh_[ct], xf[rt], acc[ct][rt]);
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) acc[ct][rt] = mfma_f16(wl_[ct], xf[rt], acc[ct][rt]);
            }
            // (reads first, two fragments ahead of the MFMAs -- the fp32 kernel's schedule at one read per row tile)
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                __builtin_amdgcn_sched_group_barrier(0x008, 2 * NCT, 0);  // one row tile's MFMAs
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);        // the fragment of row tile j + 2
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 4 * NCT, 0);
            if (k + 1 < FSTEPS) write_tile(xwrite, lds + ((k + 1) & 1) * FIMG);
        };
#pragma unroll 1
        for (int k = 0; k < FSTEPS - 2; k += 3) {                        // 30 steps, then the last two
            step(k, wh[0], wl[0], wh[2], wl[2], xs[2], xs[1]);
            step(k + 1, wh[1], wl[1], wh[0], wl[0], xs[0], xs[2]);
            step(k + 2, wh[2], wl[2], wh[1], wl[1], xs[1], xs[0]);
        }
        step(FSTEPS - 2, wh[0], wl[0], wh[2], wl[2], xs[2], xs[1]);
        step(FSTEPS - 1, wh[1], wl[1], wh[0], wl[0], xs[0], xs[2]);
        // epilogue (the fp32 kernel's): acc[ct][rt][r] = H^T: embed column 64 wave + 16 ct + 4 g + r of patch row 16 rt + c16
        f32x4 bv[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) bv[ct] = *reinterpret_cast<const f32x4*>(bias + 64 * wave + 16 * ct + 4 * g);
#pragma unroll
        for (int rt = 0; rt < 8; ++rt) {
            const long long row = rb + 16 * rt + c16;
            uint4 rnd = {0u, 0u, 0u, 0u};
            if (drop_p > 0.f) rnd = hash4x32(drop_key, (unsigned long long)row * 16ull + (unsigned)(4 * wave + g));
            const uint32_t rw[4] = {rnd.x, rnd.y, rnd.z, rnd.w};
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // (a NaN stays a NaN, as in torch.relu; pre * 0 is 0 for a finite pre and NaN otherwise: an infinite feature
                    //  gives +-inf sums, and without it the ReLU would turn the -inf ones into finite zeros -- the WHOLE row of
                    //  a non-finite feature comes out non-finite, as from the fp32 window's kernel)
                    const float pre = acc[ct][rt][r] * unscale + bv[ct][r];
                    float v = __builtin_elementwise_maximum(pre, 0.f) + pre * 0.f;
                    if (drop_p > 0.f) v = (((rw[ct] >> (8 * r)) & 0xFFu) >= thr8) ? v * inv_keep : 0.f;
                    o[r] = v;
                }
                if (row < wg_r1) *reinterpret_cast<f32x4*>(h + (size_t)row * FE + 64 * wave + 16 * ct + 4 * g) = o;
            }
        }
        __syncthreads();                                                  // (the next block's first write goes to stage 0)
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// eight halves -> bf16 hi / lo: exact (hi keeps the upper 8 significand bits, lo the 3 that remain)
__device__ __forceinline__ void split8x(const f16x8& a, bool live, bf16x8& hi, bf16x8& lo) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = live ? (float)a[j] : 0.f;
    pack_hi_lo(v, hi, lo);
}

__global__ __launch_bounds__(GW * 64, 1)
void patch_wgrad_f16x_kernel(const float* __restrict__ dh,        // [rows][256] gradient arriving at H_bag
                             const float* __restrict__ hbag,      // [rows][256] H_bag itself (zeros = ReLU / dropout mask); NULL: no gate
                             const _Float16* __restrict__ x,      // [rows][1024]
                             long long total_rows, float gate,    // 1 / (1 - realised p) (1: no dropout)
                             float* __restrict__ part,            // [64 ranges][256][1024] partial dW
                             float* __restrict__ part_cs) {       // [64 ranges][256] partial column sums of g
    __shared__ __attribute__((aligned(1024))) char lds[2 * 4 * GIMG];        // [stage][g hi | g lo | x hi | x lo]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // workgroup id -> (row range, column block): the four column blocks of a row range share an XCD (patch_fc_f32.hip)
    static_assert(GRANGES % 8 == 0, "row ranges are dealt to the 8 XCDs");
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int range = xcd + 8 * (slot >> 2), cb = slot & 3;
    const long long per = ((total_rows + GRANGES - 1) / GRANGES + GCH - 1) / GCH * GCH;
    const long long r0 = (long long)range * per, r1 = min(total_rows, r0 + per);
    const int nch = r1 > r0 ? (int)((r1 - r0 + GCH - 1) / GCH) : 0;
    const int gw = wave >> 1, xw = wave & 1;
    f32x4 acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // staging: thread t carries row t >> 4 (32 rows), 16-column group t & 15: four float4 each of dH and H_bag, 16 halves of X
    const int srow = tid >> 4, scg = tid & 15;
    float cs[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) cs[j] = 0.f;
    f32x4 sg[4], sh[4];
    f16x8 sx[2];
    auto load_chunk = [&](int ch) {
        const long long row = min(r0 + (long long)ch * GCH + srow, total_rows - 1);
        const float* pg = dh + (size_t)row * FE + 16 * scg;
        const _Float16* px = x + (size_t)row * FK + 256 * cb + 16 * scg;
#pragma unroll
        for (int j = 0; j < 4; ++j) sg[j] = *reinterpret_cast<const f32x4*>(pg + 4 * j);
#pragma unroll
        for (int j = 0; j < 2; ++j) sx[j] = *reinterpret_cast<const f16x8*>(px + 8 * j);
        if (hbag != nullptr) {
            const float* ph = hbag + (size_t)row * FE + 16 * scg;
#pragma unroll
            for (int j = 0; j < 4; ++j) sh[j] = *reinterpret_cast<const f32x4*>(ph + 4 * j);
        }
    };
    if (nch > 0) load_chunk(0);
    for (int ch = 0; ch < nch; ++ch) {
        char* st = lds + (ch & 1) * (4 * GIMG);
        {   // gate, split, write the four images of this chunk
            const bool live = r0 + (long long)ch * GCH + srow < r1;      // rows past the range contribute zeros
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float gv = sg[j][e];
                    if (hbag != nullptr) gv = sh[j][e] > 0.f ? gv * gate : 0.f;
                    sg[j][e] = live ? gv : 0.f;
                    cs[4 * j + e] += sg[j][e];
                }
            bf16x8 h0, l0, h1, l1;
            split8(sg[0], sg[1], h0, l0);
            split8(sg[2], sg[3], h1, l1);
            *reinterpret_cast<bf16x8*>(st + gimg_off(srow, 2 * scg)) = h0;
            *reinterpret_cast<bf16x8*>(st + gimg_off(srow, 2 * scg + 1)) = h1;
            *reinterpret_cast<bf16x8*>(st + GIMG + gimg_off(srow, 2 * scg)) = l0;
            *reinterpret_cast<bf16x8*>(st + GIMG + gimg_off(srow, 2 * scg + 1)) = l1;
            split8x(sx[0], live, h0, l0);
            split8x(sx[1], live, h1, l1);
            *reinterpret_cast<bf16x8*>(st + 2 * GIMG + gimg_off(srow, 2 * scg)) = h0;
            *reinterpret_cast<bf16x8*>(st + 2 * GIMG + gimg_off(srow, 2 * scg + 1)) = h1;
            *reinterpret_cast<bf16x8*>(st + 3 * GIMG + gimg_off(srow, 2 * scg)) = l0;
            *reinterpret_cast<bf16x8*>(st + 3 * GIMG + gimg_off(srow, 2 * scg + 1)) = l1;
        }
        if (ch + 1 < nch) load_chunk(ch + 1);
        __syncthreads();
        // dW[e][k] += sum_p g[p][e] x[p][k]: both operands read transposed out of the row-major images (patch_fc_f32.hip)
        bf16x8 ah[4], al[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ah[i] = col_frag<256>(st, 4 * gw + i, lane);
            al[i] = col_frag<256>(st + GIMG, 4 * gw + i, lane);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bf16x8 bh = col_frag<256>(st + 2 * GIMG, 8 * xw + j, lane);
            const bf16x8 bl = col_frag<256>(st + 3 * GIMG, 8 * xw + j, lane);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][j] = mfma_bf16(ah[i], bh, acc[i][j]);      // (term-major: dependent MFMAs four apart)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][j] = mfma_bf16(ah[i], bl, acc[i][j]);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][j] = mfma_bf16(al[i], bh, acc[i][j]);
        }
    }
    // partial block: acc[i][j][r] = dW[64 gw + 16 i + 4 g + r][256 cb + 128 xw + 16 j + (lane & 15)]
    const int c16 = lane & 15, g = lane >> 4;
    float* pout = part + (size_t)range * FE * FK;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                pout[(size_t)(64 * gw + 16 * i + 4 * g + r) * FK + 256 * cb + 128 * xw + 16 * j + c16] = acc[i][j][r];
    if (cb == 0 && part_cs != nullptr) {                                  // column sums of g: every thread holds 16 columns of its row
        __syncthreads();
        float* red = reinterpret_cast<float*>(lds);                       // [32 rows][256]
#pragma unroll
        for (int j = 0; j < 16; ++j) red[srow * 256 + 16 * scg + j] = cs[j];
        __syncthreads();
        if (tid < 256) {
            float a = 0.f;
#pragma unroll 8
            for (int r = 0; r < 32; ++r) a += red[r * 256 + tid];
            part_cs[(size_t)range * FE + tid] = a;
        }
    }
}

}  // namespace

#include "patch_wgrad_reduce.h"

// (the fp32 entries' sizes: the same packed weight and scale, the same range partials)
size_t mpo_patch_fc_f16_workspace_floats() { return (size_t)FE * FK + 64; }
size_t mpo_patch_wgrad_f16x_workspace_floats() { return (size_t)GRANGES * FE * FK + (size_t)GRANGES * FE; }

int mpo_launch_patch_fc_f16(const void* x, const float* w, const float* bias, float* h, long long total_rows, int embed,
                            int patch_dim, float drop_p, unsigned long long seed, unsigned long long offset,
                            const unsigned long long* epoch, float* ws, hipStream_t stream) {
    MPO_CHECK(embed == FE && patch_dim == FK, "fp16 patch layer kernel: built for %d -> %d (got %d -> %d)", FK, FE, patch_dim, embed);
    MPO_CHECK(drop_p >= 0.f && drop_p < 1.f, "patch-layer dropout p must be in [0,1) (got %f)", (double)drop_p);
    // (the kernel's own expression: at 256 every byte would be dropped and the keep scale would be 256 / 0)
    MPO_CHECK((uint32_t)(drop_p * 256.0f + 0.5f) <= 255u, "patch-layer dropout p = %g is realised as round(256 p) / 256 = %u/256: "
              "nothing would be kept (p must be below 1 - 1/512)", (double)drop_p, (uint32_t)(drop_p * 256.0f + 0.5f));
    if (total_rows <= 0) return 0;
    float* w_scale = ws + (size_t)FE * FK;
    weight_range_kernel<<<1, 1024, 0, stream>>>(w, w_scale);
    MPO_LAUNCH_CHECK();
    pack_patch_weight_f32_kernel<<<FE * FK / 8 / 256, 256, 0, stream>>>(w, reinterpret_cast<f16x8*>(ws), w_scale);
    MPO_LAUNCH_CHECK();
    const int target = 256;
    long long per = (total_rows + target - 1) / target;
    per = (per + FBM - 1) / FBM * FBM;
    const int grid = (int)((total_rows + per - 1) / per);
    patch_fc_f16_kernel<<<grid, 64 * HNW, 0, stream>>>(reinterpret_cast<const _Float16*>(x), reinterpret_cast<const f16x8*>(ws), bias, h,
                                                      total_rows, (int)per, drop_p, seed, offset, epoch, w_scale);
    MPO_LAUNCH_CHECK();
    return 0;
}

int mpo_launch_patch_wgrad_f16x(const float* dh, const float* hbag, const void* x, long long total_rows, int embed, int patch_dim,
                                float gate, float* d_weight, float* d_bias, float* ws, hipStream_t stream) {
    MPO_CHECK(embed == FE && patch_dim == FK, "fp16 patch weight gradient: built for %d x %d (got %d x %d)", FE, FK, embed, patch_dim);
    MPO_CHECK(total_rows > 0, "fp16 patch weight gradient: no rows");
    float* part = ws;
    float* part_cs = ws + (size_t)GRANGES * FE * FK;
    patch_wgrad_f16x_kernel<<<GRANGES * GCOLB, GW * 64, 0, stream>>>(dh, hbag, reinterpret_cast<const _Float16*>(x), total_rows, gate, part, part_cs);
    MPO_LAUNCH_CHECK();
    patch_wgrad_f32_reduce_kernel<<<FE * FK / 4 / 256, 256, 0, stream>>>(part, part_cs, d_weight, d_bias);
    MPO_LAUNCH_CHECK();
    return 0;
}
