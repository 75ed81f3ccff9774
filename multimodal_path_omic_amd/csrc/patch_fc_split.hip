// The patch layer for a window stored in fp32 (BASELINE cfg 5: 100 000-patch bags in fp32) or in fp16 (feature extractors very
// commonly write fp16), hand-written forward and weight gradient -- replaces the two fp32 library GEMMs that were 8.3 of cfg 5's
// 10.9 ms (r02).  Behind it the fp32 H_bag every fp32-bag kernel already takes.  ONE kernel body per direction, instantiated per
// stored type of X; what a window changes is a policy of a few lines (FwdX, WgradX below).
//
//     H_bag = Dropout(ReLU(X W_H^T + b_H))          X [rows, 1024] fp32 | fp16, W_H [256, 1024] fp32, H_bag [rows, 256] fp32
//     dW_H  = g^T X,  db_H = colsum(g),  g = dH (.) [H_bag > 0] / (1 - p)          (models/mcat/mcat.py:24-29,87 and its backward)
//
// Arithmetic: half-precision products of hi / lo operand splits (x = hi + lo) with fp32 accumulation on the 16x16x32 MFMA.
// With both operands split a product runs as THREE terms hi*hi + lo*hi + hi*lo (48 matrix-pipe cycles per 32 of K where eight
// v_mfma_f32_16x16x4_f32 take 256; the fp32-input MFMA peaks at 157 TF/s: 2.7 ms for this layer's 419 GF at 8 x 100 000 rows,
// forward and again for dW_H).
//   * FORWARD: fp16 splits (11 + 11 significand bits: ~2^-22 per element product, i.e. the fp32 GEMM's own rounding).  The
//     forward decides the ReLU mask: with bf16 splits (2^-17 per product, ~4e-6 absolute on H_bag) a pre-activation within
//     4e-6 of zero flips its mask against the fp32 reference 40 times as often as an fp32 GEMM's does, and ONE flipped
//     element moves a row of dW_H by |dH||x| (measured r03: 1.6-4.6 % of max|dW_H| on 164-row windows, 5.9e-3 at 3 000 rows).
//     fp16's narrow exponent is handled by a power-of-two scale on the weight (W x 2^10 before the split, 2^-10 on the
//     accumulator: exact), and operands clamped to the fp16 range before conversion, so nothing overflows to infinity.
//       - fp32 window: X is scaled (x_scale), split and clamped on the fly: two images per stage, THREE terms.  Features must
//         stay below 1.3e5 in magnitude (hi + lo saturate there), tiny features / weights degrade gracefully to an absolute
//         6e-8 (fp16 subnormals).
//       - fp16 window: an fp16 X IS one fp16 MFMA operand.  X is copied global -> registers -> LDS as it is stored: no feature
//         scale, no split, no lo image, no clamp; one image per stage, TWO terms W_hi X + W_lo X.  The only rounding left
//         against the fp64 product of the stored operands is W's lo tail (2^-22 of a product) and the fp32 accumulation -- the
//         fp32 window's own level, so the ReLU mask flips no more often than there.  A NaN or an infinity among the features
//         reaches the MFMA as it is and makes its row of H_bag non-finite (every element of it: the epilogue keeps a -inf sum
//         from becoming a finite zero); fp16 subnormals are operands like any other.
//   * WEIGHT GRADIENT: bf16 splits (2^-17 per product, fp32's exponent range: gradients span many orders of magnitude and
//     no mask depends on them), three terms for both windows: ~1e-5 relative on dW_H.  An fp16 value splits into bf16 hi + lo
//     EXACTLY (11 significand bits fit 8 + 8, fp16's range lies inside bf16's); g is split the same way for both.  (An fp16
//     form of g would need a range pass over dH.)
// The split of X (and of g) happens on the fly between the global load and the LDS image; W_H is split once per call by a pack
// kernel into MFMA-fragment order (as the bf16 kernel's weight, patch_coattn_fwd.hip).
//
// Forward, one workgroup of 4 waves per CU walking blocks of 128 rows: per K-step of 32 the X tile (128 x 32: 16 KiB of fp32,
// 8 KiB of fp16) comes global -> registers one step ahead and is written to a double-buffered stage of fp16 images (fp32 window:
// hi and lo; fp16 window: the tile itself; 64-byte rows, chunk c of row r at c ^ fswz(r): conflict-free ds_read_b128 fragments),
// one barrier per step; wave w owns embed columns 64 w .. + 63 of all 128 rows (4 x 8 tiles, 128 accumulators, product taken
// TRANSPOSED so that a lane ends with four consecutive embed columns of one patch row = one 16-byte store) and reads its W
// fragments straight from L2 one step ahead.  Epilogue: bias, NaN-keeping ReLU, dropout from the counter hash keyed by (row,
// column group) (8 bits per element, realised p = round(256 p) / 256; the mask lives in H_bag as zeros, the backward reads it
// back from there), fp32 store.  For the same (seed, offset, epoch) the two windows' masks are the same.
//
// Weight gradient, 256 workgroups of 8 waves = 64 row ranges x 4 column blocks of X (256 columns each; the four blocks of a
// range sit on one XCD -- workgroup ids 8 apart --: dH and H_bag are fetched from HBM once and shared through L2, as in
// patch_wgrad.hip): a 256 x 256 fp32 block of dW in registers (wave: 64 x 128, 128 accumulators), 32-row chunks: dH, H_bag
// and X (four float4 or two 8-half vectors per thread) global -> registers one chunk ahead, gate + split, written
// TRANSPOSED-readable (row-major bf16 images read with ds_read_b64_tr_b16), three MFMA terms; fp32 partials per row range +
// one reduction launch.  The column sums of g (= db_H) fall out of the column-block-0 workgroups.
//
// Roofline: the fp32 window's forward reads 4096 B and writes 1024 B per row: HBM-bound at 5 120 B / row (8 x 100 000 rows:
// 4.1 GB per launch); its 3 x 524 288 flop per row (1.26 PF per launch) are the co-limit at the chip's MFMA clock under load.
// The fp16 window's reads 2048 B and writes 1024 B per row (3 072 B / row: 2.5 GB per 8 x 100 000 window); 2 x 524 288 flop
// per row.
#include "coattn_tile.h"
#include "mpo_kernels.h"

namespace {

constexpr int FE = 256;                         // embed_dim
constexpr int FK = 1024;                        // patch feature width
constexpr int FBM = 128;                        // rows per block
constexpr int FBK = 32;                         // k per step
constexpr int FSTEPS = FK / FBK;                // 32
constexpr int FIMG = FBM * FBK * 2;             // one 16-bit image of a stage: 8 KiB
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

// waves of the fp32 window's forward workgroup: 4 (one per SIMD) or 8 (two per SIMD, -DMPO_F32_FWD_WAVES=8 through
// tools/build_variant.py).  Measured the same on the same box (1.27 against 1.24-1.30 ms per 8 x 100 000 window, r03): the
// kernel is not limited by a wave waiting on itself but by the matrix pipe at the clock the chip holds under this load.
#ifndef MPO_F32_FWD_WAVES
#define MPO_F32_FWD_WAVES 4
#endif
constexpr int HNW = 4;                          // waves of the fp16 window's forward workgroup (one per SIMD)

// What the forward's body takes from the stored type of X: the images per stage (with them the MFMA terms, the barrier plan,
// the LDS size and the stage stride), the vector a thread loads, how the 8 staged k of one 16-byte chunk become its images, and
// whether the epilogue has to keep a non-finite row non-finite itself.
template <typename XT> struct FwdX;
template <> struct FwdX<float> {                // scale, split and clamp: hi | lo
    static constexpr int NIMG = 2, VEC = 4;
    static constexpr bool KEEP_NONFINITE = false;                        // (split8h's v - v has made the whole row NaN already)
    typedef f32x4 vec;
    static __device__ __forceinline__ void image(const vec* src, float x_scale, f16x8 (&img)[NIMG]) {
        split8h(src[0], src[1], x_scale, img[0], img[1]);
    }
};
template <> struct FwdX<_Float16> {             // a plain copy: the tile is its own image
    static constexpr int NIMG = 1, VEC = 8;
    static constexpr bool KEEP_NONFINITE = true;
    typedef f16x8 vec;
    static __device__ __forceinline__ void image(const vec* src, float, f16x8 (&img)[NIMG]) { img[0] = src[0]; }
};

// NW waves per workgroup (4: one per SIMD, 64 embed columns each; 8: two per SIMD, 32 each -- the same packed weight, the same
// dropout mask, the same arithmetic per element).  x_scale: a power of two (1 for an fp16 window, which takes none).
template <typename XT, int NW>
__device__ __forceinline__ void patch_fc_split_body(const XT* __restrict__ x, const f16x8* __restrict__ wpk, const float* __restrict__ bias,
                                                    float* __restrict__ h, long long total_rows, int rows_per_wg, float drop_p,
                                                    unsigned long long seed, unsigned long long offset_,
                                                    const unsigned long long* __restrict__ epoch, float x_scale,
                                                    const float* __restrict__ w_scale) {
    typedef FwdX<XT> P;
    typedef typename P::vec xvec;
    constexpr int NIMG = P::NIMG;
    constexpr int STAGE = NIMG * FIMG;
    __shared__ __attribute__((aligned(1024))) char lds[2 * STAGE];           // [stage][image]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, g = lane >> 4;
    const long long wg_r0 = (long long)blockIdx.x * rows_per_wg;
    const long long wg_r1 = min(total_rows, wg_r0 + rows_per_wg);
    if (wg_r0 >= wg_r1) return;
    const int nblocks = (int)((wg_r1 - wg_r0 + FBM - 1) / FBM);

    constexpr int NCT = 16 / NW;                                         // 16-column tiles a wave owns
    constexpr int TPR = NW / 2;                                          // threads per row of the X tile
    constexpr int NCHK = 4 / TPR;                                        // 16-byte image chunks (8 k) per thread and step
    constexpr int VPC = 8 / P::VEC;                                      // loaded vectors per chunk
    constexpr int NV = NCHK * VPC;                                       // loaded vectors per thread and step
    // staging: thread (row = tid / TPR, part = tid % TPR) carries 8 NCHK consecutive k of its row
    const int srow = tid / TPR, spart = tid % TPR;
    // Image rows are 64 bytes; chunk c of row r sits at position c ^ fswz(r).  ds_read_b128 is serviced in four NON-contiguous
    // 16-lane groups ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, + 32: MI355X_MICROARCH.md, LDS): with lane = (row j, chunk g) a
    // group holds rows j, j + 12 at chunk g and rows j + 4, j + 8 at chunk g ^ 1 of every j mod 4 -- four reads inside one
    // 64-byte quarter of the bank line, which bit 3 of the row (x 2) spreads over the four positions; bit 1 of the row keeps the
    // 8-lane groups of the ds_write_b128 that fills the image (4 rows x 2 threads) off each other's banks.  (r03's
    // (row >> 2) & 3 assumed contiguous read groups: every fragment read was 2-way, SQ_LDS_BANK_CONFLICT = 50 % of LDS cycles.)
    const int sswz = fswz(srow);
    int soff[NCHK];
#pragma unroll
    for (int c = 0; c < NCHK; ++c) soff[c] = srow * FROWB + (((NCHK * spart + c) ^ sswz) << 4);
    const int wave4 = wave / (NW / 4), ct0 = NCT * (wave % (NW / 4));   // position in the packed weight's [wave 4][..][ct 4] order
    // fragment reads: row 16 rt + c16, chunk g
    const int foff = c16 * FROWB + ((g ^ fswz(c16)) << 4);
    const f16x8* whi = wpk + (size_t)wave4 * (FSTEPS * 4 * 64) + ct0 * 64 + lane;
    const f16x8* wlo = whi + FE * FK / 8;
    const uint32_t thr8 = (uint32_t)(drop_p * 256.0f + 0.5f);
    const float inv_keep = drop_p > 0.f ? 256.0f / (256.0f - (float)thr8) : 1.0f;
    const uint32_t drop_key = hash_stream_key(seed, epoch_offset(offset_, epoch));
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const float unscale = 1.0f / (x_scale * *w_scale);            // (powers of two: exact)

    for (int blk = 0; blk < nblocks; ++blk) {
        const long long rb = wg_r0 + (long long)blk * FBM;
        const long long grow = min(rb + srow, total_rows - 1);           // rows past the end: clamped (finite; never stored)
        const XT* xrow = x + (size_t)grow * FK + 8 * NCHK * spart;
        f32x4 acc[NCT][8];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int rt = 0; rt < 8; ++rt) acc[ct][rt] = zero4;
        // Operand pipeline, three register sets each in static rotation (three steps per trip, no copies): step k multiplies the
        // images of x(k) (LDS stage k & 1) by weight set k % 3, requests x(k + 2) and the weight fragments of step k + 2, and
        // turns x(k + 1) -- requested in the previous step -- into the other stage's images AFTER the step's MFMAs are issued
        // (four sets each, three steps ahead, spilled 98 registers).  One step of matrix work (~0.8 us) does not
        // cover an HBM or a loaded-L2 round trip: with one step of lookahead every step began by waiting for its operands.
        xvec xs[3][NV];
        f16x8 wh[3][NCT], wl[3][NCT];
        auto load_x = [&](xvec (&dst)[NV], int k) {
            k = k < FSTEPS ? k : FSTEPS - 1;                              // (past the end: re-reads the last tile, never used)
#pragma unroll
            for (int j = 0; j < NV; ++j) dst[j] = *reinterpret_cast<const xvec*>(xrow + FBK * k + P::VEC * j);
        };
        auto load_w = [&](f16x8 (&h_)[NCT], f16x8 (&l_)[NCT], int k) {
            k = k < FSTEPS ? k : FSTEPS - 1;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                h_[ct] = whi[(k * 4 + ct) * 64];
                l_[ct] = wlo[(k * 4 + ct) * 64];
            }
        };
        auto write_tile = [&](const xvec (&src)[NV], char* st) {
#pragma unroll
            for (int c = 0; c < NCHK; ++c) {
                f16x8 img[NIMG];
                P::image(src + VPC * c, x_scale, img);
#pragma unroll
                for (int i = 0; i < NIMG; ++i) *reinterpret_cast<f16x8*>(st + i * FIMG + soff[c]) = img[i];
            }
        };
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            load_x(xs[j], j);
            load_w(wh[j], wl[j], j);
        }
        write_tile(xs[0], lds);
        // one K-step with the register sets named statically: j = k % 3
        auto step = [&](int k, const f16x8 (&wh_)[NCT], const f16x8 (&wl_)[NCT], f16x8 (&whn)[NCT], f16x8 (&wln)[NCT], xvec (&xn)[NV],
                        const xvec (&xwrite)[NV]) {
            const char* st = lds + (k & 1) * STAGE;
            __syncthreads();                                              // the images of x(k) are complete; the other stage is free
            load_x(xn, k + 2);
            load_w(whn, wln, k + 2);
            f16x8 xf[NIMG][8];
#pragma unroll
            for (int rt = 0; rt < 8; ++rt)
#pragma unroll
                for (int i = 0; i < NIMG; ++i) xf[i][rt] = *reinterpret_cast<const f16x8*>(st + i * FIMG + rt * 16 * FROWB + foff);
#pragma unroll
            for (int rt = 0; rt < 8; ++rt) {
                // term-major: the NIMG + 1 MFMAs of one accumulator are DEPENDENT (each waits for the previous result); with the
                // four column tiles in between every MFMA finds its accumulator ready
#pragma unroll
                for (int i = 0; i < NIMG; ++i)                            // W_hi X_hi (, W_hi X_lo)
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) acc[ct][rt] = mfma_f16(wh_[ct], xf[i][rt], acc[ct][rt]);
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) acc[ct][rt] = mfma_f16(wl_[ct], xf[0][rt], acc[ct][rt]);
            }
            // (the scheduler otherwise sinks every read to its first use: reads first, two row tiles' fragments ahead of the MFMAs)
            __builtin_amdgcn_sched_group_barrier(0x100, 2 * NIMG, 0);
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                __builtin_amdgcn_sched_group_barrier(0x008, (NIMG + 1) * NCT, 0);       // one row tile's MFMAs
                __builtin_amdgcn_sched_group_barrier(0x100, NIMG, 0);                   // the fragments of row tile j + 2
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 2 * (NIMG + 1) * NCT, 0);
            if (k + 1 < FSTEPS) write_tile(xwrite, lds + ((k + 1) & 1) * STAGE);        // (vector work behind the queued matrix work)
        };
#pragma unroll 1
        for (int k = 0; k < FSTEPS - 2; k += 3) {                        // 30 steps, then the last two
            step(k, wh[0], wl[0], wh[2], wl[2], xs[2], xs[1]);
            step(k + 1, wh[1], wl[1], wh[0], wl[0], xs[0], xs[2]);
            step(k + 2, wh[2], wl[2], wh[1], wl[1], xs[1], xs[0]);
        }
        step(FSTEPS - 2, wh[0], wl[0], wh[2], wl[2], xs[2], xs[1]);
        step(FSTEPS - 1, wh[1], wl[1], wh[0], wl[0], xs[0], xs[2]);
        // epilogue: acc[ct][rt][r] = H^T: embed column 64 wave + 16 ct + 4 g + r of patch row 16 rt + c16
        f32x4 bv[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) bv[ct] = *reinterpret_cast<const f32x4*>(bias + 64 * wave4 + 16 * (ct0 + ct) + 4 * g);
#pragma unroll
        for (int rt = 0; rt < 8; ++rt) {
            const long long row = rb + 16 * rt + c16;
            uint4 rnd = {0u, 0u, 0u, 0u};
            if (drop_p > 0.f) rnd = hash4x32(drop_key, (unsigned long long)row * 16ull + (unsigned)(4 * wave4 + g));
            const uint32_t rw[4] = {rnd.x, rnd.y, rnd.z, rnd.w};
            uint32_t rwc[NCT];                                           // words ct0 .. ct0 + NCT - 1 (ct0 is wave-uniform: selects, no indexing)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) rwc[ct] = NCT == 4 ? rw[ct] : (ct0 == 0 ? rw[ct] : rw[(2 + ct) & 3]);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pre = acc[ct][rt][r] * unscale + bv[ct][r];
                    float v = __builtin_elementwise_maximum(pre, 0.f);   // (v_maximum3_f32: a NaN stays a NaN, as in torch.relu)
                    // (pre * 0 is 0 for a finite pre and NaN otherwise: an infinite feature that reached the MFMA gives +-inf
                    //  sums, and without it the ReLU would turn the -inf ones into finite zeros -- the WHOLE row of a
                    //  non-finite feature comes out non-finite, as from the window whose split makes it so)
                    if constexpr (P::KEEP_NONFINITE) v += pre * 0.f;
                    if (drop_p > 0.f) v = (((rwc[ct] >> (8 * r)) & 0xFFu) >= thr8) ? v * inv_keep : 0.f;
                    o[r] = v;
                }
                if (row < wg_r1) *reinterpret_cast<f32x4*>(h + (size_t)row * FE + 64 * wave4 + 16 * (ct0 + ct) + 4 * g) = o;
            }
        }
        __syncthreads();                                                  // (the next block's first write goes to stage 0)
    }
}

template <int NW>
__global__ __launch_bounds__(64 * NW, 1)
void patch_fc_f32_kernel(const float* __restrict__ x,             // [total_rows][1024]
                         const f16x8* __restrict__ wpk,           // packed hi | lo (pack_patch_weight_f32_kernel)
                         const float* __restrict__ bias,          // [256]
                         float* __restrict__ h,                   // [total_rows][256]
                         long long total_rows, int rows_per_wg, float drop_p, unsigned long long seed,
                         unsigned long long offset_, const unsigned long long* __restrict__ epoch,
                         float x_scale_arg, const float* __restrict__ x_scale_dev,      // the scale by value, or (non-NULL) read here
                         const float* __restrict__ w_scale) {
    // (wave-uniform either way: one scalar load at kernel start, as *w_scale in the body)
    const float x_scale = x_scale_dev != nullptr ? *x_scale_dev : x_scale_arg;
    patch_fc_split_body<float, NW>(x, wpk, bias, h, total_rows, rows_per_wg, drop_p, seed, offset_, epoch, x_scale, w_scale);
}

__global__ __launch_bounds__(64 * HNW, 1)
void patch_fc_f16_kernel(const _Float16* __restrict__ x, const f16x8* __restrict__ wpk, const float* __restrict__ bias,
                         float* __restrict__ h, long long total_rows, int rows_per_wg, float drop_p, unsigned long long seed,
                         unsigned long long offset_, const unsigned long long* __restrict__ epoch,
                         const float* __restrict__ w_scale) {
    patch_fc_split_body<_Float16, HNW>(x, wpk, bias, h, total_rows, rows_per_wg, drop_p, seed, offset_, epoch, 1.0f, w_scale);
}

// ------------------------------------------------------------------------------------------------ weight gradient
constexpr int GW = 8;                           // waves
constexpr int GCH = 32;                         // rows per chunk
constexpr int GRANGES = 64, GCOLB = 4;          // row ranges x column blocks of X = 256 workgroups
constexpr int GIMG = GCH * 256 * 2;             // one bf16 image [32 rows][256 columns]: 16 KiB
constexpr int GROWB = 512;

// [32][256] bf16 image, 16-byte chunk c of row r at c ^ (2 (r & 7)) (coattn_tile.h): col_frag<256>() reads it transposed
__device__ __forceinline__ int gimg_off(int r, int c) { return r * GROWB + ((c ^ ((r & 7) << 1)) << 4); }

// A thread's 16 columns of X in one chunk, as stored: the load, and the split into the bf16 hi / lo chunks (h0, l0: columns
// 0-7; h1, l1: 8-15; a row past the range contributes zeros).
template <typename XT> struct WgradX;
template <> struct WgradX<float> {
    f32x4 v[4];
    __device__ __forceinline__ void load(const float* p) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const f32x4*>(p + 4 * j);
    }
    __device__ __forceinline__ void split(bool live, bf16x8& h0, bf16x8& l0, bf16x8& h1, bf16x8& l1) {
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = live ? v[j] : zero4;
        split8(v[0], v[1], h0, l0);
        split8(v[2], v[3], h1, l1);
    }
};
template <> struct WgradX<_Float16> {           // exact: hi keeps the upper 8 significand bits, lo the 3 that remain
    f16x8 v[2];
    __device__ __forceinline__ void load(const _Float16* p) {
#pragma unroll
        for (int j = 0; j < 2; ++j) v[j] = *reinterpret_cast<const f16x8*>(p + 8 * j);
    }
    static __device__ __forceinline__ void split8x(const f16x8& a, bool live, bf16x8& hi, bf16x8& lo) {
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = live ? (float)a[j] : 0.f;
        pack_hi_lo(f, hi, lo);
    }
    __device__ __forceinline__ void split(bool live, bf16x8& h0, bf16x8& l0, bf16x8& h1, bf16x8& l1) {
        split8x(v[0], live, h0, l0);
        split8x(v[1], live, h1, l1);
    }
};

template <typename XT>
__device__ __forceinline__ void patch_wgrad_split_body(const float* __restrict__ dh, const float* __restrict__ hbag,
                                                       const XT* __restrict__ x, long long total_rows, float gate,
                                                       float* __restrict__ part, float* __restrict__ part_cs) {
    __shared__ __attribute__((aligned(1024))) char lds[2 * 4 * GIMG];        // [stage][g hi | g lo | x hi | x lo]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // workgroup id -> (row range, column block): the four column blocks of a row range read the same dH / H_bag rows and must
    // share an L2, i.e. an XCD (blockIdx -> XCD is round-robin, id mod 8).  r03 PMC: with the blocks of a range on FOUR
    // NEIGHBOURING ids (= four XCDs) the kernel fetched 9.90 GB per 8 x 100 000 window against 4.92 GB algorithmic -- every
    // block its own copy of dH and H_bag (profiles/r03_pmc_mcat_f32_100k.json)
    static_assert(GRANGES % 8 == 0, "row ranges are dealt to the 8 XCDs");
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int range = xcd + 8 * (slot >> 2), cb = slot & 3;
    const long long per = ((total_rows + GRANGES - 1) / GRANGES + GCH - 1) / GCH * GCH;
    const long long r0 = (long long)range * per, r1 = min(total_rows, r0 + per);
    const int nch = r1 > r0 ? (int)((r1 - r0 + GCH - 1) / GCH) : 0;
    // wave (gw = wave >> 1: 64 rows of dW = embed columns 64 gw .. + 63 of g; xw = wave & 1: 128 of this block's X columns)
    const int gw = wave >> 1, xw = wave & 1;
    f32x4 acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // staging: thread t carries row t >> 4 (32 rows), 16-column group t & 15 (16 x 16 = 256 columns): four float4 each of dH
    // and H_bag, and its 16 columns of X
    const int srow = tid >> 4, scg = tid & 15;
    float cs[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) cs[j] = 0.f;
    f32x4 sg[4], sh[4];
    WgradX<XT> sx;
    auto load_chunk = [&](int ch) {
        const long long row = min(r0 + (long long)ch * GCH + srow, total_rows - 1);
        const float* pg = dh + (size_t)row * FE + 16 * scg;
#pragma unroll
        for (int j = 0; j < 4; ++j) sg[j] = *reinterpret_cast<const f32x4*>(pg + 4 * j);
        sx.load(x + (size_t)row * FK + 256 * cb + 16 * scg);
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
            sx.split(live, h0, l0, h1, l1);
            *reinterpret_cast<bf16x8*>(st + 2 * GIMG + gimg_off(srow, 2 * scg)) = h0;
            *reinterpret_cast<bf16x8*>(st + 2 * GIMG + gimg_off(srow, 2 * scg + 1)) = h1;
            *reinterpret_cast<bf16x8*>(st + 3 * GIMG + gimg_off(srow, 2 * scg)) = l0;
            *reinterpret_cast<bf16x8*>(st + 3 * GIMG + gimg_off(srow, 2 * scg + 1)) = l1;
        }
        if (ch + 1 < nch) load_chunk(ch + 1);
        __syncthreads();
        // dW[e][k] += sum_p g[p][e] x[p][k]: A = g^T (rows = embed column, k = patch), B = x^T ... both read transposed out of
        // the row-major images: col_frag(t) gives, for column 16 t + (lane & 15), the 8 patches of k-order(g, j) -- the same
        // order on both sides
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

__global__ __launch_bounds__(GW * 64, 1)
void patch_wgrad_f32_kernel(const float* __restrict__ dh,         // [rows][256] gradient arriving at H_bag
                            const float* __restrict__ hbag,       // [rows][256] H_bag itself (zeros = ReLU / dropout mask); NULL: no gate
                            const float* __restrict__ x,          // [rows][1024]
                            long long total_rows, float gate,     // 1 / (1 - realised p) (1: no dropout)
                            float* __restrict__ part,             // [64 ranges][256][1024] partial dW
                            float* __restrict__ part_cs) {        // [64 ranges][256] partial column sums of g
    patch_wgrad_split_body<float>(dh, hbag, x, total_rows, gate, part, part_cs);
}

__global__ __launch_bounds__(GW * 64, 1)
void patch_wgrad_f16x_kernel(const float* __restrict__ dh, const float* __restrict__ hbag, const _Float16* __restrict__ x,
                             long long total_rows, float gate, float* __restrict__ part, float* __restrict__ part_cs) {
    patch_wgrad_split_body<_Float16>(dh, hbag, x, total_rows, gate, part, part_cs);
}

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

size_t mpo_patch_fc_split_workspace_floats() { return (size_t)FE * FK + 64; }     // packed hi | lo fp16 weight = 1 MiB, then its scale
size_t mpo_patch_wgrad_split_workspace_floats() { return (size_t)GRANGES * FE * FK + (size_t)GRANGES * FE; }

int mpo_launch_patch_fc_split(const void* x, bool x_f16, const float* w, const float* bias, float* h, long long total_rows,
                              int embed, int patch_dim, float drop_p, unsigned long long seed, unsigned long long offset,
                              const unsigned long long* epoch, float x_scale, const float* x_scale_dev, float* ws,
                              hipStream_t stream) {
    const char* window = x_f16 ? "fp16" : "fp32";
    MPO_CHECK(embed == FE && patch_dim == FK, "%s patch layer kernel: built for %d -> %d (got %d -> %d)", window, FK, FE, patch_dim, embed);
    MPO_CHECK(drop_p >= 0.f && drop_p < 1.f, "patch-layer dropout p must be in [0,1) (got %f)", (double)drop_p);
    // (the kernel's own expression: at 256 every byte would be dropped and the keep scale would be 256 / 0)
    MPO_CHECK((uint32_t)(drop_p * 256.0f + 0.5f) <= 255u, "patch-layer dropout p = %g is realised as round(256 p) / 256 = %u/256: "
              "nothing would be kept (p must be below 1 - 1/512)", (double)drop_p, (uint32_t)(drop_p * 256.0f + 0.5f));
    if (!x_f16 && x_scale_dev == nullptr) {    // (a device scale cannot be looked at here: it must hold what mpo_feature_range_f32 wrote)
        int e = 0;
        MPO_CHECK(x_scale > 0.f && x_scale < INFINITY && frexpf(x_scale, &e) == 0.5f, "fp32 patch layer: x_scale must be a power of two (got %g)", (double)x_scale);
    }
    if (total_rows <= 0) return 0;
    float* w_scale = ws + (size_t)FE * FK;
    const f16x8* wpk = reinterpret_cast<const f16x8*>(ws);
    weight_range_kernel<<<1, 1024, 0, stream>>>(w, w_scale);
    MPO_LAUNCH_CHECK();
    pack_patch_weight_f32_kernel<<<FE * FK / 8 / 256, 256, 0, stream>>>(w, reinterpret_cast<f16x8*>(ws), w_scale);
    MPO_LAUNCH_CHECK();
    const int target = 256;
    long long per = (total_rows + target - 1) / target;
    per = (per + FBM - 1) / FBM * FBM;
    const int grid = (int)((total_rows + per - 1) / per);
    if (x_f16)
        patch_fc_f16_kernel<<<grid, 64 * HNW, 0, stream>>>(static_cast<const _Float16*>(x), wpk, bias, h, total_rows, (int)per, drop_p, seed,
                                                          offset, epoch, w_scale);
    else
        patch_fc_f32_kernel<MPO_F32_FWD_WAVES><<<grid, 64 * MPO_F32_FWD_WAVES, 0, stream>>>(static_cast<const float*>(x), wpk, bias, h, total_rows,
                                                                                          (int)per, drop_p, seed, offset, epoch, x_scale, x_scale_dev, w_scale);
    MPO_LAUNCH_CHECK();
    return 0;
}

int mpo_launch_patch_wgrad_split(const float* dh, const float* hbag, const void* x, bool x_f16, long long total_rows, int embed,
                                 int patch_dim, float gate, float* d_weight, float* d_bias, float* ws, hipStream_t stream) {
    const char* window = x_f16 ? "fp16" : "fp32";
    MPO_CHECK(embed == FE && patch_dim == FK, "%s patch weight gradient: built for %d x %d (got %d x %d)", window, FE, FK, embed, patch_dim);
    MPO_CHECK(total_rows > 0, "%s patch weight gradient: no rows", window);
    float* part = ws;
    float* part_cs = ws + (size_t)GRANGES * FE * FK;
    if (x_f16)
        patch_wgrad_f16x_kernel<<<GRANGES * GCOLB, GW * 64, 0, stream>>>(dh, hbag, static_cast<const _Float16*>(x), total_rows, gate, part, part_cs);
    else
        patch_wgrad_f32_kernel<<<GRANGES * GCOLB, GW * 64, 0, stream>>>(dh, hbag, static_cast<const float*>(x), total_rows, gate, part, part_cs);
    MPO_LAUNCH_CHECK();
    patch_wgrad_f32_reduce_kernel<<<FE * FK / 4 / 256, 256, 0, stream>>>(part, part_cs, d_weight, d_bias);
    MPO_LAUNCH_CHECK();
    return 0;
}
