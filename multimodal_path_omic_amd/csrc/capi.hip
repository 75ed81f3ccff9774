// extern "C" entry points of libmpo_hip.so (declared in include/mpo_hip.h) and the host-side
// orchestration of each one: a fixed sequence of kernel launches on the caller's stream, working
// only in caller-provided buffers.  No allocation, no synchronisation, graph-capturable.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "../../include/mpo_hip.h"
#include "coattn_tile.h"
#include "mpo_common.h"
#include "mpo_kernels.h"
#include "mpo_layout.h"

static thread_local char g_err[512] = "";

void mpo_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ------------------------------------------------------------------------------------------- buffer layouts (mpo_layout.h)
// R = n_slides * n_q rows of width E on the query side; `parts` = split-M partials of the bag plan
template <typename T> struct K1Saved { T *qs, *qk2, *ctx, *attn, *lse2; };       // qs | qk2 | ctx | attn [R,E] | lse2 [R]
template <class A> K1Saved<typename A::elem> k1_saved(A& a, size_t R, size_t E) {
    return {a.floats(R * E), a.floats(R * E), a.floats(R * E), a.floats(R * E), a.floats(R)};
}
struct K1FwdWs { float *part_ml, *part_ctx, *w_bf16; };
// weight_floats: the packed bf16 copy of W_H when the patch layer runs in the same call (0: none)
template <class A> K1FwdWs k1_fwd_ws(A& a, size_t parts, size_t n_q, size_t E, size_t weight_floats) {
    return {a.floats(parts * 32), a.floats(parts * n_q * E), weight_floats ? a.floats(weight_floats) : nullptr};
}
struct K1BwdWs { float *dattn, *dctx, *dqk, *dq_pre, *delta, *part_dqk, *part_cs; };
template <class A> K1BwdWs k1_bwd_ws(A& a, size_t R, size_t parts, size_t n_q, size_t E, bool colsum) {
    return {a.floats(R * E), a.floats(R * E), a.floats(R * E), a.floats(R * E), a.floats(R), a.floats(parts * n_q * E),
            colsum ? a.floats(parts * E) : nullptr};
}

template <typename T> struct K2Saved { T *qt, *qs2, *tq, *ctx, *attn, *lse2, *asum; };   // five [R,E] | lse2 [R] | asum [R]
template <class A> K2Saved<typename A::elem> k2_saved(A& a, size_t R, size_t E) {
    return {a.floats(R * E), a.floats(R * E), a.floats(R * E), a.floats(R * E), a.floats(R * E), a.floats(R), a.floats(R)};
}
// embed 512 runs every bag pass once per 256-column half (see copy_cols below): [R][E/2] operand copies and a second pair of maps
struct K2FwdWs { float *part, *hq1, *hq2, *hctx, *tmp_maps; };
template <class A> K2FwdWs k2_fwd_ws(A& a, size_t R, size_t parts, size_t n_q, size_t E, size_t total_rows) {
    K2FwdWs w{a.floats(parts * n_q * E), nullptr, nullptr, nullptr, nullptr};
    if (E == 512) { w.hq1 = a.floats(R * E / 2); w.hq2 = a.floats(R * E / 2); w.hctx = a.floats(R * E / 2); w.tmp_maps = a.floats(2 * n_q * total_rows); }
    return w;
}
struct K2BwdWs { float *dattn, *dctx, *dqt, *dtq, *dq, *spare, *dasum, *part, *part2, *part_cs, *ds1_map, *dg_map, *hb[6], *tmp_map; };
template <class A> K2BwdWs k2_bwd_ws(A& a, size_t R, size_t parts, size_t n_q, size_t E, size_t total_rows, bool colsum) {
    K2BwdWs w{a.floats(R * E), a.floats(R * E), a.floats(R * E), a.floats(R * E), a.floats(R * E), a.floats(R * E), a.floats(R),
              a.floats(parts * n_q * E), a.floats(parts * n_q * E), colsum ? a.floats(parts * E) : nullptr,
              a.floats(n_q * total_rows), a.floats(n_q * total_rows), {}, nullptr};
    if (E == 512) {
        for (float*& h : w.hb) h = a.floats(R * E / 2);
        w.tmp_map = a.floats(2 * n_q * total_rows);
    }
    return w;
}
// the patch-gradient entries: per-workgroup column sums when the bias gradient is asked for
template <class A> float* k2_patch_grad_ws(A& a, size_t parts, size_t E, bool colsum) { return colsum ? a.floats(parts * E) : nullptr; }

// the single-block workspaces of the patch layer: floats of the block
static size_t patch_weight_floats(int embed, int patch_dim) { return (size_t)(embed < 256 ? 256 : embed) * patch_dim / 2; }   // W_H as bf16
static size_t patch_epilogue_bwd_floats(int64_t n, int cols) { return (size_t)mpo_relu_dropout_bwd_blocks((size_t)n, 1) * (size_t)cols; }
static size_t one_block_workspace_bytes(size_t n_floats) {
    WsCount c;
    c.floats(n_floats);
    return c.workspace_bytes();
}

namespace {
bool g_k2_one_pass_key = true;     // K2 backward: the whole key gradient in one pass over K (bag_key_grad_kernel; mpo_set_nacagat_one_pass_key_grad)
}

// ONE workgroup per CU over the window (256 CUs): long row ranges amortise the per-workgroup prologue
// (query fragments) and epilogue (LDS merge, partial write); measured r01 on 32 x 15k bf16:
// 256 WGs 51.6 us, 512 59.0, 1024 73.0, 2048 98.9.
extern "C" int mpo_coattn_target_workgroups(void) {
    return 256;
}

extern "C" int mpo_coattn_splits(int n_slides, int max_rows) {
    // uniform cut: the same number of row ranges for every slide; at least one 32-row tile per wave of a workgroup
    const int target = mpo_coattn_target_workgroups();
    int s = (target + n_slides - 1) / n_slides;
    if (s > 512) s = 512;
    const int cap = (max_rows + 127) / 128;
    if (s > cap) s = cap;
    if (s < 1) s = 1;
    return s;
}

// C-ABI plan -> kernel plan.  NULL (or a NULL wg_start) selects the uniform cut.
static BagPlan make_plan(const mpo_bag_plan* p, int n_slides, int max_rows) {
    BagPlan pl;
    pl.n_slides = n_slides;
    if (p != nullptr && p->wg_start != nullptr) {
        pl.wg_start = p->wg_start;
        pl.n_wg = p->n_wg;
        pl.rows_per_wg = p->rows_per_wg;
    } else {
        pl.splits = mpo_coattn_splits(n_slides, max_rows);
    }
    return pl;
}
static int check_plan(const BagPlan& pl, int n_slides) {
    if (pl.wg_start == nullptr) return 0;
    MPO_CHECK(pl.rows_per_wg >= kTileRows && pl.rows_per_wg % kTileRows == 0, "bag plan: rows_per_wg %d must be a positive multiple of %d",
              pl.rows_per_wg, kTileRows);
    MPO_CHECK(pl.n_wg >= n_slides && pl.n_wg <= mpo_coattn_target_workgroups() + n_slides,
              "bag plan: n_wg %d outside [n_slides, target + n_slides]", pl.n_wg);
    return 0;
}
// upper bound on the number of split-M partials of any plan for this window
static size_t max_parts(int n_slides) { return (size_t)mpo_coattn_target_workgroups() + (size_t)n_slides; }

extern "C" {

int mpo_abi_version(void) { return MPO_ABI_VERSION; }
const char* mpo_last_error(void) { return g_err; }

int mpo_linear_forward(const float* x, const float* weight, const float* bias, float* y, int rows, int in_features,
                       int out_features, float alpha, int act, mpo_stream_t stream) {
    return mpo_linear_fwd(x, weight, bias, y, rows, in_features, out_features, alpha, act, stream);
}
int mpo_linear_backward_input(const float* dy, const float* weight, float* dx, int rows, int in_features,
                              int out_features, float alpha, int accumulate, mpo_stream_t stream) {
    return mpo_linear_bwd_input(dy, weight, dx, rows, in_features, out_features, alpha, accumulate, stream);
}
int mpo_linear_backward_weight(const float* dy, const float* x, float* dweight, float* dbias, int rows,
                               int in_features, int out_features, float alpha, mpo_stream_t stream) {
    return mpo_linear_bwd_weight(dy, x, dweight, dbias, rows, in_features, out_features, alpha, stream);
}
// ------------------------------------------------------------------------------------------- K1
size_t mpo_coattn_saved_floats(int n_slides, int n_q, int embed) {
    Count<kPacked> c;
    k1_saved(c, (size_t)n_slides * n_q, embed);
    return c.n_floats();
}

size_t mpo_coattn_workspace_bytes(int n_slides, int n_q, int embed, int max_rows) {
    (void)max_rows;
    WsCount f, b;                                    // one workspace serves the forward and the backward
    k1_fwd_ws(f, max_parts(n_slides), n_q, embed, 0);
    k1_bwd_ws(b, (size_t)n_slides * n_q, max_parts(n_slides), n_q, embed, true);
    return std::max(f.end, b.end) + kWorkspaceSlack;
}

static int check_common(int bag_dtype, int n_slides, int total_rows, int max_rows, int n_q, int embed) {
    MPO_CHECK(bag_dtype == MPO_F32 || bag_dtype == MPO_BF16, "bag dtype %d is neither MPO_F32 nor MPO_BF16", bag_dtype);
    MPO_CHECK(n_slides >= 1, "n_slides must be >= 1 (got %d)", n_slides);
    MPO_CHECK(n_q >= 1 && n_q <= 16, "number of omic queries must be in 1..16 (got %d)", n_q);
    MPO_CHECK(embed == 128 || embed == 256 || embed == 512, "embed_dim %d not in {128,256,512}", embed);
    MPO_CHECK(max_rows >= 1 && total_rows >= n_slides, "every slide needs at least one patch (total_rows %d, max_rows %d)",
              total_rows, max_rows);
    return 0;
}

// The patch layer in front of K1 (row f1): H_bag = dropout(relu(X W_H^T + b_H)) is written by its own bag launch and read back
// by the co-attention's partial pass.
struct PatchStep {
    const void* patches;
    const float *weight, *bias;
    int patch_dim;
    float drop_p;
    uint64_t seed, offset;
    const uint64_t* rng_epoch;
    void* h_bag;
};

// K1's forward launch sequence.  patch == nullptr: over the caller's bag; else the patch layer produces the (bf16) bag on the way.
static int k1_forward(const void* bag, int bag_f32, const PatchStep* patch, const int32_t* cu_rows, int n_slides, int max_rows,
                      const float* query, int n_q, int E, const float* in_w, const float* in_b, const float* out_w,
                      const float* out_b, float* out, float* attn_map, float* saved, const BagPlan& plan, const K1FwdWs& ws,
                      hipStream_t stream) {
    const int R = n_slides * n_q;
    Carve<kPacked> sv(saved);
    const K1Saved<float> S = k1_saved(sv, R, E);
    if (patch) RC(mpo_launch_pack_patch_weight(patch->weight, ws.w_bf16, E, patch->patch_dim, stream));
    // qs = (query W_q^T + b_q) / sqrt(E)
    RC(mpo_linear_fwd(query, in_w, in_b, S.qs, R, E, E, 1.0f / sqrtf((float)E), MPO_ACT_NONE, stream));
    // qk2 = log2(e) * qs W_k     (fold of the key projection into the query; key bias cancels in softmax)
    RC(mpo_linear_bwd_input(S.qs, in_w + (size_t)E * E, S.qk2, R, E, E, kLog2e, 0, stream));
    if (patch) {
        RC(mpo_launch_patch_fc_fwd(patch->patches, ws.w_bf16, patch->bias, cu_rows, patch->h_bag, E, patch->patch_dim, patch->drop_p, patch->seed,
                                   patch->offset, reinterpret_cast<const unsigned long long*>(patch->rng_epoch), plan, stream));
        bag = patch->h_bag;
    }
    RC(mpo_launch_coattn_fwd_partial(bag, bag_f32, cu_rows, n_slides, E, S.qk2, ws.part_ml, ws.part_ctx, attn_map, n_q, plan, stream));
    RC(mpo_launch_coattn_combine(ws.part_ml, ws.part_ctx, S.ctx, S.lse2, n_slides, n_q, E, plan, stream));
    // attn = ctx W_v^T + b_v   (rows of A sum to one);  out = attn W_o^T + b_o
    RC(mpo_linear_fwd(S.ctx, in_w + (size_t)2 * E * E, in_b + 2 * E, S.attn, R, E, E, 1.0f, MPO_ACT_NONE, stream));
    RC(mpo_linear_fwd(S.attn, out_w, out_b, out, R, E, E, 1.0f, MPO_ACT_NONE, stream));
    if (attn_map) RC(mpo_launch_coattn_normalize(attn_map, S.lse2, cu_rows, n_slides, n_q, max_rows, 0.f, 0, 0, stream));
    return 0;
}

int mpo_coattn_mcat_forward(const void* bag, int bag_dtype, const int32_t* cu_rows, int n_slides, int total_rows,
                            int max_rows, const float* query, int n_q, int embed, const float* in_w,
                            const float* in_b, const float* out_w, const float* out_b, float* out, float* attn_map,
                            float* saved, const mpo_bag_plan* plan_, void* workspace, size_t workspace_bytes,
                            mpo_stream_t stream) {
    RC(check_common(bag_dtype, n_slides, total_rows, max_rows, n_q, embed));
    const BagPlan plan = make_plan(plan_, n_slides, max_rows);
    RC(check_plan(plan, n_slides));
    WsCarve ws(workspace, workspace_bytes);
    const K1FwdWs W = k1_fwd_ws(ws, plan_parts(plan), n_q, embed, 0);
    MPO_CHECK(ws.ok(), "coattn forward: workspace too small (%zu bytes)", workspace_bytes);
    return k1_forward(bag, bag_dtype == MPO_F32, nullptr, cu_rows, n_slides, max_rows, query, n_q, embed, in_w, in_b, out_w, out_b,
                      out, attn_map, saved, plan, W, stream);
}

// ------------------------------------------------------------------------------------------- row f1: patch layer + K1
// ONE C-ABI call, two bag launches: the patch-layer kernel writes H_bag, K1's partial pass reads it back (L2-warm per slide).
size_t mpo_patch_coattn_workspace_bytes(int n_slides, int n_q, int embed, int patch_dim) {
    WsCount c;
    k1_fwd_ws(c, max_parts(n_slides), n_q, embed, (size_t)embed * patch_dim / 2);
    return c.workspace_bytes();
}

int mpo_patch_coattn_mcat_forward(const void* patches, const int32_t* cu_rows, int n_slides, int total_rows, int max_rows,
                                  int patch_dim, const float* patch_weight, const float* patch_bias, float drop_p,
                                  uint64_t seed, uint64_t offset, const uint64_t* rng_epoch,
                                  const float* query, int n_q, int embed, const float* in_w, const float* in_b,
                                  const float* out_w, const float* out_b, void* h_bag, float* out, float* attn_map,
                                  float* saved, const mpo_bag_plan* plan_, void* workspace, size_t workspace_bytes,
                                  mpo_stream_t stream) {
    RC(check_common(MPO_BF16, n_slides, total_rows, max_rows, n_q, embed));
    MPO_CHECK(embed == 256 && patch_dim == 1024, "fused patch layer + co-attention is built for 1024 -> 256 (got %d -> %d)",
              patch_dim, embed);
    const BagPlan plan = make_plan(plan_, n_slides, max_rows);
    RC(check_plan(plan, n_slides));
    WsCarve ws(workspace, workspace_bytes);
    const K1FwdWs W = k1_fwd_ws(ws, plan_parts(plan), n_q, embed, (size_t)embed * patch_dim / 2);
    MPO_CHECK(ws.ok(), "fused patch layer + co-attention: workspace too small (%zu bytes)", workspace_bytes);
    const PatchStep patch{patches, patch_weight, patch_bias, patch_dim, drop_p, seed, offset, rng_epoch, h_bag};
    // (same saved layout as mpo_coattn_mcat_forward: its backward applies)
    return k1_forward(nullptr, 0, &patch, cu_rows, n_slides, max_rows, query, n_q, embed, in_w, in_b, out_w, out_b, out, attn_map,
                      saved, plan, W, stream);
}

// The patch layer alone, H_bag = dropout(relu(X W_H^T + b_H)) (models/mcat/mcat.py:24-29,87), as ONE pass of the same
// kernel: for the models whose co-attention needs more than H_bag (NaCAGaT's key projection) and for MCAT outside the
// 1024 -> 256 configuration.  patch_dim 512, 1024 or 2048 (the kernel's schedule is built per width).  Workspace: the packed
// bf16 copy of the weight.
size_t mpo_patch_fc_workspace_bytes(int embed, int patch_dim) { return one_block_workspace_bytes(patch_weight_floats(embed, patch_dim)); }
int mpo_patch_fc_forward(const void* patches, const int32_t* cu_rows, int n_slides, int total_rows, int max_rows, int patch_dim,
                         const float* patch_weight, const float* patch_bias, int embed, float drop_p, uint64_t seed,
                         uint64_t offset, const uint64_t* rng_epoch, void* h_bag, const mpo_bag_plan* plan_, void* workspace,
                         size_t workspace_bytes, mpo_stream_t stream) {
    RC(check_common(MPO_BF16, n_slides, total_rows, max_rows, 1, embed));
    MPO_CHECK((embed == 128 || embed == 256 || embed == 512) && (patch_dim == 512 || patch_dim == 1024 || patch_dim == 2048),
              "patch layer kernel is built for patch_dim in {512, 1024, 2048} -> embed in {128, 256, 512} (got %d -> %d)", patch_dim, embed);
    MPO_CHECK((int64_t)max_rows * embed * 2 < ((int64_t)1 << 31), "patch layer: a slide's H_bag of 2 GiB or more (%d rows)", max_rows);
    const BagPlan plan = make_plan(plan_, n_slides, max_rows);
    RC(check_plan(plan, n_slides));
    WsCarve ws(workspace, workspace_bytes);
    float* w_bf16 = ws.floats(patch_weight_floats(embed, patch_dim));
    MPO_CHECK(ws.ok(), "patch layer: workspace too small (%zu bytes)", workspace_bytes);
    RC(mpo_launch_pack_patch_weight(patch_weight, w_bf16, embed, patch_dim, stream));
    return mpo_launch_patch_fc_fwd(patches, w_bf16, patch_bias, cu_rows, h_bag, embed, patch_dim, drop_p, seed, offset,
                                   reinterpret_cast<const unsigned long long*>(rng_epoch), plan, stream);
}

// fp32- and fp16-stored windows: the patch layer on patch_fc_split.hip.  One helper per direction behind both windows' entries;
// the fp16 entries are the fp32 ones without a feature scale, their rate an integer.
size_t mpo_patch_fc_f32_workspace_bytes(int backward) {
    return one_block_workspace_bytes(backward ? mpo_patch_wgrad_split_workspace_floats() : mpo_patch_fc_split_workspace_floats());
}
size_t mpo_patch_fc_f16_workspace_bytes(int backward) { return mpo_patch_fc_f32_workspace_bytes(backward); }
// drop_256 = round(256 p) -> the p the launcher rounds back to that integer (exact: 256ths); refusals in the fp32 entry's words
static int patch_f16_rate(int drop_256, float* p) {
    *p = (float)drop_256 / 256.0f;
    MPO_CHECK(drop_256 >= 0 && drop_256 <= 256, "patch-layer dropout p must be in [0,1) (got %f)", (double)*p);
    MPO_CHECK(drop_256 <= 255, "patch-layer dropout p = %g is realised as round(256 p) / 256 = %u/256: "
              "nothing would be kept (p must be below 1 - 1/512)", (double)*p, (unsigned)drop_256);
    return 0;
}
// x_f16: an fp16 window -- the rate is drop_256 (drop_p is not read) and there is no feature scale.  An fp32 window: drop_p, and
// x_scale by value or (x_scale_dev non-NULL) read on the device when the kernel starts: one kernel, the same bits.
static int patch_split_forward(const void* patches, bool x_f16, int64_t total_rows, int patch_dim, const float* patch_weight,
                               const float* patch_bias, int embed, float drop_p, int drop_256, uint64_t seed, uint64_t offset,
                               const uint64_t* rng_epoch, float x_scale, const float* x_scale_dev, float* h_bag, void* workspace,
                               size_t workspace_bytes, mpo_stream_t stream) {
    const char* window = x_f16 ? "fp16" : "fp32";
    MPO_CHECK(patches && patch_weight && patch_bias && h_bag, "%s patch layer: null operand", window);
    if (x_f16) RC(patch_f16_rate(drop_256, &drop_p));
    MPO_CHECK(total_rows >= 1, "%s patch layer: total_rows %lld", window, (long long)total_rows);
    WsCarve ws(workspace, workspace_bytes);
    float* wpk = ws.floats(mpo_patch_fc_split_workspace_floats());
    MPO_CHECK(ws.ok(), "%s patch layer: workspace too small (%zu bytes)", window, workspace_bytes);
    return mpo_launch_patch_fc_split(patches, x_f16, patch_weight, patch_bias, h_bag, total_rows, embed, patch_dim, drop_p, seed, offset,
                                     reinterpret_cast<const unsigned long long*>(rng_epoch), x_scale, x_scale_dev, wpk, stream);
}
// x_f16: the gate is formed from drop_256 (gate is not read)
static int patch_split_backward(const float* d_h_bag, const float* h_bag, const void* patches, bool x_f16, int64_t total_rows,
                                int embed, int patch_dim, float gate, int drop_256, float* d_weight, float* d_bias,
                                void* workspace, size_t workspace_bytes, mpo_stream_t stream) {
    const char* window = x_f16 ? "fp16" : "fp32";
    MPO_CHECK(d_h_bag && patches && d_weight, "%s patch layer backward: null operand", window);
    if (x_f16) {
        float drop_p;
        RC(patch_f16_rate(drop_256, &drop_p));
        gate = 256.0f / (256.0f - (float)drop_256);                  // (the forward kernel's inv_keep; 1 at drop_256 = 0)
    }
    MPO_CHECK(total_rows >= 1, "%s patch layer backward: total_rows %lld", window, (long long)total_rows);
    WsCarve ws(workspace, workspace_bytes);
    float* part = ws.floats(mpo_patch_wgrad_split_workspace_floats());
    MPO_CHECK(ws.ok(), "%s patch layer backward: workspace too small (%zu bytes)", window, workspace_bytes);
    return mpo_launch_patch_wgrad_split(d_h_bag, h_bag, patches, x_f16, total_rows, embed, patch_dim, gate, d_weight, d_bias, part, stream);
}
int mpo_patch_fc_f32_forward(const float* patches, int64_t total_rows, int patch_dim, const float* patch_weight,
                             const float* patch_bias, int embed, float drop_p, uint64_t seed, uint64_t offset,
                             const uint64_t* rng_epoch, float x_scale, float* h_bag, void* workspace, size_t workspace_bytes,
                             mpo_stream_t stream) {
    return patch_split_forward(patches, false, total_rows, patch_dim, patch_weight, patch_bias, embed, drop_p, 0, seed, offset, rng_epoch,
                               x_scale, nullptr, h_bag, workspace, workspace_bytes, stream);
}
int mpo_patch_fc_f32_forward_dev(const float* patches, int64_t total_rows, int patch_dim, const float* patch_weight,
                                 const float* patch_bias, int embed, float drop_p, uint64_t seed, uint64_t offset,
                                 const uint64_t* rng_epoch, const float* x_scale, float* h_bag, void* workspace,
                                 size_t workspace_bytes, mpo_stream_t stream) {
    MPO_CHECK(x_scale, "fp32 patch layer: null device scale (mpo_feature_range_f32 writes it)");
    return patch_split_forward(patches, false, total_rows, patch_dim, patch_weight, patch_bias, embed, drop_p, 0, seed, offset, rng_epoch,
                               1.0f, x_scale, h_bag, workspace, workspace_bytes, stream);
}
int mpo_patch_fc_f32_backward(const float* d_h_bag, const float* h_bag, const float* patches, int64_t total_rows, int embed,
                              int patch_dim, float gate, float* d_weight, float* d_bias, void* workspace, size_t workspace_bytes,
                              mpo_stream_t stream) {
    return patch_split_backward(d_h_bag, h_bag, patches, false, total_rows, embed, patch_dim, gate, 0, d_weight, d_bias, workspace,
                                workspace_bytes, stream);
}
int mpo_patch_fc_f16_forward(const void* patches, int64_t total_rows, int patch_dim, const float* patch_weight,
                             const float* patch_bias, int embed, int drop_256, uint64_t seed, uint64_t offset,
                             const uint64_t* rng_epoch, float* h_bag, void* workspace, size_t workspace_bytes, mpo_stream_t stream) {
    return patch_split_forward(patches, true, total_rows, patch_dim, patch_weight, patch_bias, embed, 0.f, drop_256, seed, offset, rng_epoch,
                               1.0f, nullptr, h_bag, workspace, workspace_bytes, stream);
}
int mpo_patch_fc_f16_backward(const float* d_h_bag, const float* h_bag, const void* patches, int64_t total_rows, int embed,
                              int patch_dim, int drop_256, float* d_weight, float* d_bias, void* workspace, size_t workspace_bytes,
                              mpo_stream_t stream) {
    return patch_split_backward(d_h_bag, h_bag, patches, true, total_rows, embed, patch_dim, 1.0f, drop_256, d_weight, d_bias, workspace,
                                workspace_bytes, stream);
}

// the patch layer's bag pass alone, and with the co-attention's partial pass behind it (bench.py's roofline leg, profiling workloads)
int mpo_patch_coattn_fwd_bagpass(const void* patches, const void* w_packed, const float* bias, const int32_t* cu_rows, int n_slides,
                                 const float* qk2, void* h_bag, float* part_ml, float* part_ctx, int n_q, int max_rows,
                                 float drop_p, uint64_t seed, uint64_t offset, const mpo_bag_plan* plan_, mpo_stream_t stream) {
    const BagPlan plan = make_plan(plan_, n_slides, max_rows);
    RC(check_plan(plan, n_slides));
    RC(mpo_launch_patch_fc_fwd(patches, w_packed, bias, cu_rows, h_bag, 256, 1024, drop_p, seed, offset, nullptr, plan, stream));
    if (qk2 == nullptr) return 0;
    return mpo_launch_coattn_fwd_partial(h_bag, 0, cu_rows, n_slides, 256, qk2, part_ml, part_ctx, nullptr, n_q, plan, stream);
}
int mpo_pack_patch_weight(const float* weight, void* packed, int embed, int patch_dim, mpo_stream_t stream) {
    return mpo_launch_pack_patch_weight(weight, packed, embed, patch_dim, stream);
}

int mpo_coattn_mcat_backward(const void* bag, int bag_dtype, const int32_t* cu_rows, int n_slides, int total_rows,
                             int max_rows, const float* query, int n_q, int embed, const float* in_w,
                             const float* out_w, const float* saved, const float* attn_map, const float* d_out,
                             const float* d_attn_map, float* d_query, int d_query_accumulate, void* d_bag,
                             float* d_bag_colsum, float* d_in_w,
                             float* d_in_b, float* d_out_w, float* d_out_b, float bag_relu_gate, const mpo_bag_plan* plan_,
                             void* workspace, size_t workspace_bytes, mpo_stream_t stream) {
    RC(check_common(bag_dtype, n_slides, total_rows, max_rows, n_q, embed));
    MPO_CHECK(!d_attn_map || attn_map, "coattn backward: a gradient on the attention map needs the forward's map");
    const int E = embed, R = n_slides * n_q;
    const BagPlan plan = make_plan(plan_, n_slides, max_rows);
    RC(check_plan(plan, n_slides));
    WsCarve ws(workspace, workspace_bytes);
    const K1BwdWs W = k1_bwd_ws(ws, R, plan_parts(plan), n_q, E, d_bag_colsum != nullptr);
    MPO_CHECK(ws.ok(), "coattn backward: workspace too small (%zu bytes)", workspace_bytes);
    Carve<kPacked, const float> sv(saved);
    const K1Saved<const float> S = k1_saved(sv, R, E);
    const float* w_q = in_w;
    const float* w_k = in_w + (size_t)E * E;
    const float* w_v = in_w + (size_t)2 * E * E;
    const float scale = 1.0f / sqrtf((float)E);
    // out = attn W_o^T + b_o
    RC(mpo_linear_bwd_pair(mpo_args_bwd_input(d_out, out_w, W.dattn, R, E, E, 1.0f, 0),
                           mpo_args_bwd_weight(d_out, S.attn, d_out_w, d_out_b, R, E, E, 1.0f), stream));
    // attn = ctx W_v^T + b_v
    RC(mpo_linear_bwd_pair(mpo_args_bwd_input(W.dattn, w_v, W.dctx, R, E, E, 1.0f, 0),
                           mpo_args_bwd_weight(W.dattn, S.ctx, d_in_w + (size_t)2 * E * E, d_in_b + 2 * E, R, E, E, 1.0f), stream));
    // delta = rowsum(dctx * ctx) [+ rowsum(A * dA_ext)]: inside the bag pass unless a map gradient adds its term
    if (d_attn_map) {
        RC(mpo_launch_rowdot(W.dctx, S.ctx, W.delta, R, E, stream));
        RC(mpo_launch_map_rowdot(attn_map, d_attn_map, cu_rows, W.delta, n_slides, n_q, 1, stream));
    }
    // the bag pass
    RC(mpo_launch_coattn_bwd(bag, bag_dtype == MPO_F32, cu_rows, n_slides, E, S.qk2, S.lse2, W.dctx, d_attn_map ? W.delta : nullptr,
                             S.ctx, attn_map, d_attn_map, d_bag, W.part_dqk, W.part_cs, n_q, plan, bag_relu_gate, stream));
    {   // one launch: dqk = sum of the split-M partials, the bag's column sums, db_k = 0 (softmax is shift-invariant)
        BagFinish f{};
        f.part[0] = W.part_dqk; f.out[0] = W.dqk; f.n_red = 1;
        f.part_cs = W.part_cs; f.colsum = d_bag_colsum; f.cs_cols = E;
        f.zero[0] = d_in_b + E; f.n_zero[0] = E;
        RC(mpo_launch_bag_finish(f, n_slides, n_q, E, plan, stream));
    }
    // qk = qs W_k :  dqs = dqk W_k^T (folded with the 1/sqrt(E) of qs = scale * (...)),  dW_k = qs^T dqk
    RC(mpo_gemm_together(stream, mpo_args_fwd(W.dqk, w_k, nullptr, W.dq_pre, R, E, E, scale, MPO_ACT_NONE),
                         mpo_args_bwd_weight(S.qs, W.dqk, d_in_w + (size_t)E * E, nullptr, R, E, E, 1.0f)));
    // q_pre = query W_q^T + b_q
    return mpo_linear_bwd_pair(mpo_args_bwd_input(W.dq_pre, w_q, d_query, R, E, E, 1.0f, d_query_accumulate ? 1 : 0),
                               mpo_args_bwd_weight(W.dq_pre, query, d_in_w, d_in_b, R, E, E, 1.0f), stream);
}

// ------------------------------------------------------------------------------------------- K2
size_t mpo_nacagat_saved_floats(int n_slides, int n_q, int embed) {
    Count<kPacked> c;
    k2_saved(c, (size_t)n_slides * n_q, embed);
    return c.n_floats();
}
size_t mpo_nacagat_workspace_bytes(int n_slides, int n_q, int embed, int max_rows, int total_rows) {
    (void)max_rows;
    const size_t R = (size_t)n_slides * n_q, parts = max_parts(n_slides);
    WsCount f, b, p;                                 // one workspace serves the forward, the backward and the patch-gradient entries
    k2_fwd_ws(f, R, parts, n_q, embed, total_rows);
    k2_bwd_ws(b, R, parts, n_q, embed, total_rows, true);
    k2_patch_grad_ws(p, parts, embed, true);
    return std::max({f.end, b.end, p.end}) + kWorkspaceSlack;
}

// embed_dim 512 ('big', models/nacagat/nacagat.py:17-18): the bag kernels are built for embed <= 256, so the two bags travel in
// the SPLIT-HALVES layout [2][total_rows][256] (columns 0..255 | 256..511) and every bag pass runs once per column half on
// the 256-wide kernels: the score / gradient maps are sums over the halves (linear in the embed index), the column-indexed
// results (context, query-side sums, dK, dH) are the halves side by side.  The 6 x 512 query-side tensors keep their natural
// layout; their halves are strided copies.  Functional, not tuned (four small copies and one map-sized add per pass).
static int copy_cols(float* dst, size_t dst_ld, const float* src, size_t src_ld, int rows, int cols, hipStream_t s) {
    MPO_HIP(hipMemcpy2DAsync(dst, dst_ld * 4, src, src_ld * 4, (size_t)cols * 4, rows, hipMemcpyDeviceToDevice, s));
    return 0;
}

// What the two K2 entries start with: the checked geometry, the work plan, and column half h of a natural-layout [R][E]
// query-side tensor.  take: the half of `src` a bag pass reads (a copy in `scratch`); put_to / put: where the producer of a half
// of `dst` writes, and the copy that moves it home; map_to / map_add: maps are sums over the halves, the first half writes `map`,
// a later one writes `tmp` and is added.  At NH == 1 a half is the tensor itself and nothing is copied or added.
struct K2Call {
    BagPlan splits;
    int E, R, NH, EH, f32;                 // NH column halves of EH columns: 2 x 256 at embed 512, else the whole row
    size_t half_k, half_h, half_dk;        // bytes from one half to the next of K, of the bag and of dK
    hipStream_t stream;
    int take(const float*& half, const float* src, float* scratch, int h) const {
        half = NH > 1 ? scratch : src;
        return NH > 1 ? copy_cols(scratch, EH, src + h * EH, E, R, EH, stream) : 0;
    }
    float* put_to(float* dst, float* scratch) const { return NH > 1 ? scratch : dst; }
    int put(float* dst, const float* scratch, int h) const { return NH > 1 ? copy_cols(dst + h * EH, E, scratch, EH, R, EH, stream) : 0; }
    static float* map_to(float* map, float* tmp, int h) { return h == 0 ? map : tmp; }
    int map_add(float* map, const float* tmp, size_t n, int h) const { return h > 0 ? mpo_launch_ew_add(map, tmp, n, stream) : 0; }
};
// the shared checks in the entries' order (dk_dtype: the backward's; the forward passes MPO_F32)
static int k2_begin(K2Call& c, int k_dtype, int bag_dtype, int dk_dtype, int n_slides, int total_rows, int max_rows, int n_q, int embed,
                    float drop_p, const mpo_bag_plan* plan_, hipStream_t stream) {
    RC(check_common(bag_dtype, n_slides, total_rows, max_rows, n_q, embed));
    MPO_CHECK(drop_p >= 0.f && drop_p < 1.f, "attention dropout p must be in [0,1) (got %f)", (double)drop_p);
    MPO_CHECK(k_dtype == MPO_F32, "nacagat co-attention: K must be fp32 (k_dtype %d): the narrow gate amplifies key rounding", k_dtype);
    MPO_CHECK(dk_dtype == MPO_F32 || dk_dtype == MPO_BF16, "d_kbag dtype %d is neither MPO_F32 nor MPO_BF16", dk_dtype);
    const int f32 = bag_dtype == MPO_F32, NH = embed == 512 ? 2 : 1, EH = embed / NH;      // (split-halves bag layout at 512)
    const size_t half = (size_t)total_rows * EH;                                            // elements of one half of a bag
    c = {make_plan(plan_, n_slides, max_rows), embed, n_slides * n_q, NH, EH, f32, half * 4, half * (f32 ? 4 : 2),
         half * (dk_dtype == MPO_F32 ? 4 : 2), stream};
    return check_plan(c.splits, n_slides);
}

int mpo_coattn_nacagat_forward(const void* kbag, int k_dtype, const void* hbag, int bag_dtype, const int32_t* cu_rows, int n_slides,
                               int total_rows, int max_rows, const float* query, int n_q, int embed,
                               const float* in_w, const float* in_b, const float* out_w, const float* out_b,
                               float drop_p, uint64_t seed, uint64_t offset, const uint64_t* rng_epoch,
                               float* q_proj, float* out, float* attn_map, float* score_maps,
                               float* saved, const mpo_bag_plan* plan_, void* workspace, size_t workspace_bytes,
                               mpo_stream_t stream) {
    K2Call c;
    RC(k2_begin(c, k_dtype, bag_dtype, MPO_F32, n_slides, total_rows, max_rows, n_q, embed, drop_p, plan_, stream));
    const int E = c.E, R = c.R, NH = c.NH, EH = c.EH, f32 = c.f32;
    const BagPlan& splits = c.splits;
    WsCarve ws(workspace, workspace_bytes);
    const K2FwdWs W = k2_fwd_ws(ws, R, plan_parts(splits), n_q, E, total_rows);
    MPO_CHECK(ws.ok(), "nacagat forward: workspace too small (%zu bytes)", workspace_bytes);
    Carve<kPacked> sv(saved);
    const K2Saved<float> S = k2_saved(sv, R, E);
    const size_t map_n = (size_t)n_q * total_rows;
    float* a_map = score_maps;
    float* g_map = score_maps + map_n;
    // q = query W_q^T + b_q  (returned: the reference hands it to the CAG, models/blocks.py:110,206)
    RC(mpo_linear_fwd(query, in_w, in_b, q_proj, R, E, E, 1.0f, MPO_ACT_NONE, stream));
    RC(mpo_launch_qprep(q_proj, S.qt, S.qs2, S.tq, R * E, 1.0f / sqrtf((float)E), stream));
    // one pass over K: a = qs2 . K and g = tanh(q) . tanh(K)   (tanh(K) is never materialised)
    for (int h = 0; h < NH; ++h) {
        const float *r1, *r2;
        RC(c.take(r1, S.qs2, W.hq1, h));
        RC(c.take(r2, S.tq, W.hq2, h));
        RC(mpo_launch_bag_rowdot_gated(static_cast<const char*>(kbag) + h * c.half_k, 1, cu_rows, n_slides, EH, r1, r2,
                                       c.map_to(a_map, W.tmp_maps, h), c.map_to(g_map, W.tmp_maps + map_n, h), n_q, splits, stream));
        RC(c.map_add(score_maps, W.tmp_maps, 2 * map_n, h));
    }
    RC(mpo_launch_gated_softmax_fwd(a_map, g_map, cu_rows, attn_map, S.lse2, S.asum, n_slides, n_q, drop_p, seed, offset,
                                    reinterpret_cast<const unsigned long long*>(rng_epoch), stream));
    for (int h = 0; h < NH; ++h) {
        RC(mpo_launch_bag_colacc(static_cast<const char*>(hbag) + h * c.half_h, f32, cu_rows, n_slides, EH, attn_map, W.part, n_q,
                                 splits, stream));
        RC(mpo_launch_coattn_bwd_reduce(W.part, c.put_to(S.ctx, W.hctx), n_slides, n_q, EH, splits, stream));
        RC(c.put(S.ctx, W.hctx, h));
    }
    // attn = ctx W_v^T + (sum_m A_drop) b_v ;  out = attn W_o^T + b_o
    RC(mpo_linear_fwd(S.ctx, in_w + (size_t)2 * E * E, nullptr, S.attn, R, E, E, 1.0f, MPO_ACT_NONE, stream));
    RC(mpo_launch_row_scaled_bias(S.attn, S.asum, in_b + 2 * E, R, E, stream));
    return mpo_linear_fwd(S.attn, out_w, out_b, out, R, E, E, 1.0f, MPO_ACT_NONE, stream);
}

int mpo_coattn_nacagat_backward(const void* kbag, int k_dtype, const void* hbag, int bag_dtype,
                                const int32_t* cu_rows, int n_slides, int total_rows, int max_rows,
                                const float* query, int n_q, int embed, const float* in_w, const float* in_b,
                                const float* out_w, float drop_p, uint64_t seed, uint64_t offset, const uint64_t* rng_epoch,
                                const float* saved, const float* score_maps, const float* attn_map,
                                const float* d_out, const float* d_attn_map, const float* d_q_proj,
                                float* d_query, int d_query_accumulate, void* d_kbag, int dk_dtype, float* d_kbag_colsum, void* d_hbag,
                                float* d_ctx, float* d_in_w, float* d_in_b, float* d_out_w, float* d_out_b,
                                const mpo_bag_plan* plan_, void* workspace, size_t workspace_bytes, mpo_stream_t stream) {
    K2Call c;
    RC(k2_begin(c, k_dtype, bag_dtype, dk_dtype, n_slides, total_rows, max_rows, n_q, embed, drop_p, plan_, stream));
    const int E = c.E, R = c.R, NH = c.NH, EH = c.EH, f32 = c.f32;
    const BagPlan& splits = c.splits;
    MPO_CHECK(d_ctx != nullptr || d_hbag != nullptr, "nacagat backward: neither d_hbag nor d_ctx given");
    WsCarve ws(workspace, workspace_bytes);
    const K2BwdWs W = k2_bwd_ws(ws, R, plan_parts(splits), n_q, E, total_rows, d_kbag_colsum != nullptr);
    MPO_CHECK(ws.ok(), "nacagat backward: workspace too small (%zu bytes)", workspace_bytes);
    float* dctx = d_ctx ? d_ctx : W.dctx;                  // a caller that finishes dH itself keeps dL/dctx
    float* const* hb = W.hb;                               // [R][EH] scratch of the column-half passes
    Carve<kPacked, const float> sv(saved);
    const K2Saved<const float> S = k2_saved(sv, R, E);
    const float* a_map = score_maps;
    const float* g_map = score_maps + (size_t)n_q * total_rows;
    const float* w_q = in_w;
    const float* w_v = in_w + (size_t)2 * E * E;
    const float* b_v = in_b + 2 * E;
    // out = attn W_o^T + b_o
    RC(mpo_linear_bwd_pair(mpo_args_bwd_input(d_out, out_w, W.dattn, R, E, E, 1.0f, 0),
                           mpo_args_bwd_weight(d_out, S.attn, d_out_w, d_out_b, R, E, E, 1.0f), stream));
    // attn = ctx W_v^T + asum (x) b_v
    {
        const GemmArgs dbv = mpo_args_bwd_weight(S.asum, W.dattn, d_in_b + 2 * E, nullptr, R, E, 1, 1.0f);     // db_v = asum^T dattn
        const GemmArgs das = mpo_args_fwd(W.dattn, b_v, nullptr, W.dasum, R, E, 1, 1.0f, MPO_ACT_NONE);        // dasum = dattn b_v
        RC(mpo_gemm_together(stream, mpo_args_bwd_input(W.dattn, w_v, dctx, R, E, E, 1.0f, 0),
                             mpo_args_bwd_weight(W.dattn, S.ctx, d_in_w + (size_t)2 * E * E, nullptr, R, E, E, 1.0f), &dbv, &das));
    }
    // map side: dA = dctx . H^T (summed over the column halves at 512; dch keeps the two halves of dctx for the last pass)
    const float* dch[2];
    for (int h = 0; h < NH; ++h) {
        RC(c.take(dch[h], dctx, hb[h], h));
        RC(mpo_launch_bag_rowdot(static_cast<const char*>(hbag) + h * c.half_h, f32, cu_rows, n_slides, EH, dch[h],
                                 c.map_to(W.ds1_map, W.tmp_map, h), 1.0f, n_q, splits, stream));
        RC(c.map_add(W.ds1_map, W.tmp_map, (size_t)n_q * total_rows, h));
    }
    RC(mpo_launch_gated_softmax_bwd(a_map, g_map, cu_rows, S.lse2, W.dasum, d_attn_map, W.ds1_map, W.dg_map, n_slides, n_q, drop_p,
                                    seed, offset, reinterpret_cast<const unsigned long long*>(rng_epoch), stream));
    // query side: dq~ = ds1 K, dtq = dg TK
    // (one pass over K, tanh on the fly) -- or, for N <= 6 at embed <= 256, out of the bag-side pass below: both need K and
    // the two maps and nothing of each other, so K (491 MB per 32 x 15 000 window) is read once for the two
    const bool one_pass = g_k2_one_pass_key && NH == 1 && n_q <= 6;
    for (int h = 0; h < NH && !one_pass; ++h) {
        RC(mpo_launch_bag_colacc_gated(static_cast<const char*>(kbag) + h * c.half_k, 1, cu_rows, n_slides, EH, W.ds1_map, W.dg_map,
                                       W.part, W.part2, n_q, splits, stream));
        BagFinish f{};
        f.part[0] = W.part; f.out[0] = c.put_to(W.dqt, hb[2]); f.part[1] = W.part2; f.out[1] = c.put_to(W.dtq, hb[3]); f.n_red = 2;
        RC(mpo_launch_bag_finish(f, n_slides, n_q, EH, splits, stream));
        RC(c.put(W.dqt, hb[2], h));
        RC(c.put(W.dtq, hb[3], h));
    }
    auto query_side = [&]() -> int {
        RC(mpo_launch_qprep_bwd(W.dqt, W.dtq, S.tq, d_q_proj, W.dq, R * E, 1.0f / sqrtf((float)E), stream));
        return mpo_linear_bwd_pair(mpo_args_bwd_input(W.dq, w_q, d_query, R, E, E, 1.0f, d_query_accumulate ? 1 : 0),
                                   mpo_args_bwd_weight(W.dq, query, d_in_w, d_in_b, R, E, E, 1.0f), stream);
    };
    if (!one_pass) RC(query_side());
    // bag side: dK = ds1^T q~ + (dg^T tq) * (1 - TK^2),  dH = A_drop^T dctx
    // (one pass: tanh' from the staged K tile)
    for (int h = 0; h < NH; ++h) {
        const float *qth, *tqh;
        RC(c.take(qth, S.qt, hb[4], h));
        RC(c.take(tqh, S.tq, hb[5], h));
        if (one_pass)
            RC(mpo_launch_bag_key_grad(reinterpret_cast<const float*>(kbag), cu_rows, n_slides, EH, W.ds1_map, qth, W.dg_map, tqh,
                                       d_kbag, dk_dtype == MPO_F32, W.part_cs, W.part, W.part2, n_q, splits, stream));
        else
            RC(mpo_launch_bag_outer_gated(reinterpret_cast<const float*>(static_cast<const char*>(kbag) + h * c.half_k), cu_rows,
                                          n_slides, EH, W.ds1_map, qth, W.dg_map, tqh, static_cast<char*>(d_kbag) + h * c.half_dk,
                                          dk_dtype == MPO_F32, W.part_cs, n_q, splits, stream));
        // one launch: the key bag's column sums, and (first half) zeros for the key slice of the packed in-projection (it
        // belongs to the caller's K = H W_k^T + b_k; a caller may have the key-bias gradient written straight into its slice)
        BagFinish f{};
        f.part_cs = d_kbag_colsum ? W.part_cs : nullptr; f.colsum = d_kbag_colsum ? d_kbag_colsum + h * EH : nullptr; f.cs_cols = EH;
        if (h == 0) {
            f.zero[0] = d_in_w + (size_t)E * E; f.n_zero[0] = E * E;
            if (d_kbag_colsum != d_in_b + E) { f.zero[1] = d_in_b + E; f.n_zero[1] = E; }
        }
        if (one_pass) { f.part[0] = W.part; f.out[0] = W.dqt; f.part[1] = W.part2; f.out[1] = W.dtq; f.n_red = 2; }
        RC(mpo_launch_bag_finish(f, n_slides, n_q, EH, splits, stream));
    }
    if (one_pass) RC(query_side());
    if (d_ctx == nullptr)
        for (int h = 0; h < NH; ++h)
            RC(mpo_launch_bag_outer(cu_rows, n_slides, EH, attn_map, dch[h], nullptr, nullptr,
                                    static_cast<char*>(d_hbag) + h * c.half_h, f32, n_q, splits, stream));
    return 0;
}

// The two patch-gradient entries share their plan, their workspace (per-workgroup column sums) and the column sum behind the bag pass.
struct K2PatchGrad {
    BagPlan splits;
    float* part_cs;
};
static int k2_patch_grad_begin(K2PatchGrad& pg, int n_slides, int max_rows, int embed, bool colsum, const mpo_bag_plan* plan_,
                               void* workspace, size_t workspace_bytes) {
    pg.splits = make_plan(plan_, n_slides, max_rows);
    RC(check_plan(pg.splits, n_slides));
    WsCarve ws(workspace, workspace_bytes);
    pg.part_cs = k2_patch_grad_ws(ws, plan_parts(pg.splits), embed, colsum);
    MPO_CHECK(ws.ok(), "nacagat patch grad: workspace too small (%zu bytes)", workspace_bytes);
    return 0;
}
static int k2_patch_grad_end(const K2PatchGrad& pg, float* d_bias, int embed, hipStream_t stream) {
    return d_bias ? mpo_launch_colsum(pg.part_cs, d_bias, (int)plan_parts(pg.splits), embed, embed, 0, stream) : 0;
}

int mpo_nacagat_patch_grad(const int32_t* cu_rows, int n_slides, int total_rows, int max_rows, int n_q, int embed,
                           const float* attn_map, const float* d_ctx, const void* addend_bf16, const void* hbag_bf16,
                           void* d_bag_bf16, float relu_gate, float* d_bias, const mpo_bag_plan* plan_,
                           void* workspace, size_t workspace_bytes, mpo_stream_t stream) {
    RC(check_common(MPO_BF16, n_slides, total_rows, max_rows, n_q, embed));
    MPO_CHECK(attn_map && d_ctx && addend_bf16 && hbag_bf16 && d_bag_bf16, "nacagat patch grad: null operand");
    MPO_CHECK(((reinterpret_cast<uintptr_t>(addend_bf16) | reinterpret_cast<uintptr_t>(hbag_bf16) |
                reinterpret_cast<uintptr_t>(d_bag_bf16)) & 15) == 0, "nacagat patch grad: bag operands must be 16-byte aligned");
    K2PatchGrad pg;
    RC(k2_patch_grad_begin(pg, n_slides, max_rows, embed, d_bias != nullptr, plan_, workspace, workspace_bytes));
    RC(mpo_launch_bag_outer_gate(cu_rows, n_slides, embed, attn_map, d_ctx, addend_bf16, hbag_bf16, d_bag_bf16, relu_gate,
                                 pg.part_cs, n_q, pg.splits, stream));
    return k2_patch_grad_end(pg, d_bias, embed, stream);
}

int mpo_nacagat_patch_grad_fused(const int32_t* cu_rows, int n_slides, int total_rows, int max_rows, int n_q, int embed,
                                 const float* attn_map, const float* d_ctx, const void* d_kbag_bf16, const float* w_k,
                                 const void* hbag_bf16, void* d_bag_bf16, float relu_gate, float* d_bias,
                                 const mpo_bag_plan* plan_, void* workspace, size_t workspace_bytes, mpo_stream_t stream) {
    RC(check_common(MPO_BF16, n_slides, total_rows, max_rows, n_q, embed));
    MPO_CHECK(attn_map && d_ctx && d_kbag_bf16 && w_k && hbag_bf16 && d_bag_bf16, "nacagat patch grad: null operand");
    MPO_CHECK(d_bag_bf16 != d_kbag_bf16, "nacagat patch grad (fused): d_bag must not alias d_kbag");
    MPO_CHECK(((reinterpret_cast<uintptr_t>(d_kbag_bf16) | reinterpret_cast<uintptr_t>(hbag_bf16) |
                reinterpret_cast<uintptr_t>(d_bag_bf16)) & 15) == 0, "nacagat patch grad: bag operands must be 16-byte aligned");
    K2PatchGrad pg;
    RC(k2_patch_grad_begin(pg, n_slides, max_rows, embed, d_bias != nullptr, plan_, workspace, workspace_bytes));
    RC(mpo_launch_k2_patch_grad(cu_rows, d_kbag_bf16, w_k, attn_map, d_ctx, hbag_bf16, d_bag_bf16, relu_gate, pg.part_cs, n_q, embed,
                                pg.splits, stream));
    return k2_patch_grad_end(pg, d_bias, embed, stream);
}

int mpo_coattn_fwd_bagpass(const void* bag, int bag_dtype, const int32_t* cu_rows, int n_slides, int embed,
                           const float* qk2, float* part_ml, float* part_ctx, float* raw_logits, int n_q, int max_rows,
                           const mpo_bag_plan* plan_, mpo_stream_t stream) {
    const BagPlan plan = make_plan(plan_, n_slides, max_rows);
    RC(check_plan(plan, n_slides));
    return mpo_launch_coattn_fwd_partial(bag, bag_dtype == MPO_F32, cu_rows, n_slides, embed, qk2, part_ml, part_ctx,
                                         raw_logits, n_q, plan, stream);
}
// per-(query, slide) dot products over the ragged maps, and the per-slide scaling that is the backward of a map norm
int mpo_map_block_dot(const float* a_map, const float* b_map, const int32_t* cu_rows, int n_slides, int n_q, float* out,
                      mpo_stream_t stream) {
    MPO_CHECK(a_map && b_map && cu_rows && out && n_slides >= 1 && n_q >= 1, "map block dot: bad argument");
    return mpo_launch_map_rowdot(a_map, b_map, cu_rows, out, n_slides, n_q, 0, stream);
}
int mpo_map_block_scale(const float* a_map, const float* scale, const int32_t* cu_rows, int n_slides, int n_q, float* out,
                        mpo_stream_t stream) {
    MPO_CHECK(a_map && scale && cu_rows && out && n_slides >= 1 && n_q >= 1, "map block scale: bad argument");
    return mpo_launch_map_block_scale(a_map, scale, cu_rows, out, n_slides, n_q, stream);
}
int mpo_key_projection(const void* hbag_bf16, int64_t rows, int embed, const float* w_k, const float* b_k, float* kbag,
                       mpo_stream_t stream) {
    MPO_CHECK(rows >= 1 && rows <= 0x7fffffff, "key projection: %lld rows out of range", (long long)rows);
    return mpo_launch_key_proj(hbag_bf16, w_k, b_k, kbag, (int)rows, embed, stream);
}
int mpo_nacagat_fwd_bagpass(const float* kbag, const int32_t* cu_rows, int n_slides, int embed, const float* qs2,
                            const float* tq, float* a_map, float* g_map, int n_q, int max_rows, const mpo_bag_plan* plan_,
                            mpo_stream_t stream) {
    const BagPlan plan = make_plan(plan_, n_slides, max_rows);
    RC(check_plan(plan, n_slides));
    return mpo_launch_bag_rowdot_gated(kbag, 1, cu_rows, n_slides, embed, qs2, tq, a_map, g_map, n_q, plan, stream);
}
int mpo_coattn_bwd_bagpass(const void* bag, int bag_dtype, const int32_t* cu_rows, int n_slides, int embed,
                           const float* qk2, const float* lse2, const float* dctx, const float* delta,
                           const float* d_attn_map, void* d_bag, float* part_dqk, int n_q, int max_rows,
                           const mpo_bag_plan* plan_, mpo_stream_t stream) {
    const BagPlan plan = make_plan(plan_, n_slides, max_rows);
    RC(check_plan(plan, n_slides));
    MPO_CHECK(delta, "coattn backward bag pass: delta is required here");
    return mpo_launch_coattn_bwd(bag, bag_dtype == MPO_F32, cu_rows, n_slides, embed, qk2, lse2, dctx, delta, nullptr, nullptr,
                                 d_attn_map, d_bag, part_dqk, nullptr, n_q, plan, 0.f, stream);
}

// ------------------------------------------------------------------------------------------- patch layer epilogue
int mpo_patch_epilogue_forward(void* h_bf16, const float* bias, int64_t rows, int cols, float drop_p, uint64_t seed,
                               uint64_t offset, const uint64_t* rng_epoch, mpo_stream_t stream) {
    MPO_CHECK(h_bf16 && bias, "patch epilogue: null operand");
    MPO_CHECK(rows >= 0, "patch epilogue: %lld rows", (long long)rows);
    // (the kernel moves h as bf16 x 8 and the bias as fp32 x 4: 16-byte loads)
    MPO_CHECK(((reinterpret_cast<uintptr_t>(h_bf16) | reinterpret_cast<uintptr_t>(bias)) & 15) == 0,
              "patch epilogue: h and bias must be 16-byte aligned");
    return mpo_launch_bias_relu_dropout_bf16(h_bf16, bias, (size_t)rows, cols, drop_p, seed, offset,
                                             reinterpret_cast<const unsigned long long*>(rng_epoch), stream);
}
int mpo_colsum_bf16(const void* x_bf16, float* out, int64_t rows, int cols, mpo_stream_t stream) {
    MPO_CHECK(x_bf16 && out, "bf16 column sum: null operand");
    MPO_CHECK(rows >= 0, "bf16 column sum: %lld rows", (long long)rows);
    MPO_CHECK((reinterpret_cast<uintptr_t>(x_bf16) & 15) == 0, "bf16 column sum: x must be 16-byte aligned (bf16 x 8 loads)");
    return mpo_launch_colsum_bf16(x_bf16, out, (size_t)rows, cols, stream);
}
size_t mpo_patch_epilogue_backward_workspace_bytes(int64_t n, int cols) { return one_block_workspace_bytes(patch_epilogue_bwd_floats(n, cols)); }
int mpo_patch_epilogue_backward(const void* h_bf16, const void* dy_bf16, void* g_bf16, int64_t n, int cols, float drop_p,
                                float* d_bias, void* workspace, size_t workspace_bytes, mpo_stream_t stream) {
    MPO_CHECK(h_bf16 && dy_bf16 && g_bf16, "patch epilogue backward: null operand");
    MPO_CHECK(((reinterpret_cast<uintptr_t>(h_bf16) | reinterpret_cast<uintptr_t>(dy_bf16) |
                reinterpret_cast<uintptr_t>(g_bf16)) & 15) == 0,
              "patch epilogue backward: h, dy and g must be 16-byte aligned (bf16 x 8 loads)");
    if (!d_bias) return mpo_launch_relu_dropout_bwd_bf16(h_bf16, dy_bf16, g_bf16, (size_t)n, drop_p, cols, nullptr, stream);
    WsCarve ws(workspace, workspace_bytes);
    float* part = ws.floats(patch_epilogue_bwd_floats(n, cols));
    MPO_CHECK(workspace && ws.ok(), "patch epilogue backward: workspace too small (%zu bytes)", workspace_bytes);
    RC(mpo_launch_relu_dropout_bwd_bf16(h_bf16, dy_bf16, g_bf16, (size_t)n, drop_p, cols, part, stream));
    return mpo_launch_colsum(part, d_bias, mpo_relu_dropout_bwd_blocks((size_t)n, 1), cols, cols, 0, stream);
}

// dW_H = g^T X (models/mcat/mcat.py:24-29 backward): g = d(pre-activation) [rows, embed] bf16, X [rows, patch_dim] bf16
size_t mpo_patch_weight_grad_workspace_bytes(int embed, int patch_dim) {
    return one_block_workspace_bytes(mpo_patch_wgrad_partial_floats(embed, patch_dim));
}
int mpo_patch_weight_grad(const void* g_bf16, const void* patches_bf16, int64_t total_rows, int embed, int patch_dim,
                          float* d_weight, int workgroups, void* workspace, size_t workspace_bytes, mpo_stream_t stream) {
    MPO_CHECK(g_bf16 && patches_bf16 && d_weight, "patch weight gradient: null argument");
    MPO_CHECK(total_rows >= 1 && total_rows < (int64_t)1 << 31, "patch weight gradient: %lld rows", (long long)total_rows);
    WsCarve ws(workspace, workspace_bytes);
    float* part = ws.floats(mpo_patch_wgrad_partial_floats(embed, patch_dim));
    MPO_CHECK(ws.ok(), "patch weight gradient: workspace too small (%zu bytes)", workspace_bytes);
    return mpo_launch_patch_wgrad(g_bf16, patches_bf16, total_rows, embed, patch_dim, part, d_weight, workgroups,
                                  static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------- optimiser
int mpo_adam_step_flat(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                       float beta1, float beta2, float eps, float weight_decay, int step, const int32_t* step_dev,
                       mpo_stream_t stream) {
    MPO_CHECK(step >= 1 || step_dev, "adam: step counts from 1 (got %d)", step);
    return mpo_launch_adam_flat(params, grads, exp_avg, exp_avg_sq, (size_t)n, lr, beta1, beta2, eps, weight_decay,
                                step < 1 ? 1 : step, step_dev, stream);
}

// The other training.optimizer choices and the L1 penalty's fold (include/mpo_hip.h); additive to ABI 14.
int mpo_optim_step_flat(int algorithm, float* params, const float* grads, float* state1, float* state2, int64_t n, float lr,
                        const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, float l1, int step,
                        const int32_t* step_dev, mpo_stream_t stream) {
    MPO_CHECK(algorithm >= MPO_OPTIM_ADAM && algorithm <= MPO_OPTIM_SGD, "flat optimiser: unknown algorithm %d", algorithm);
    MPO_CHECK(n >= 0, "flat optimiser: n = %lld", (long long)n);
    MPO_CHECK(params && grads, "flat optimiser: null parameter or gradient buffer");
    const bool stateful = algorithm != MPO_OPTIM_SGD;
    MPO_CHECK(!stateful || (state1 && state2), "flat optimiser: algorithm %d needs both state buffers", algorithm);
    const auto misaligned = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3u) != 0; };
    MPO_CHECK(!misaligned(params) && !misaligned(grads) && !misaligned(state1) && !misaligned(state2) && !misaligned(lr_dev) &&
              !misaligned(step_dev), "flat optimiser: buffers must be 4-byte aligned");
    const bool counted = algorithm == MPO_OPTIM_ADAM || algorithm == MPO_OPTIM_ADAMAX;
    MPO_CHECK(!counted || step >= 1 || step_dev, "flat optimiser: step counts from 1 (got %d)", step);
    return mpo_launch_optim_flat(algorithm, params, grads, state1, state2, (size_t)n, lr, lr_dev, beta1, beta2, eps,
                                 weight_decay, l1, step < 1 ? 1 : step, step_dev, static_cast<hipStream_t>(stream));
}
size_t mpo_abs_sum_flat_workspace_bytes(int64_t n) {
    return n < 0 ? 0 : mpo_abs_sum_partials((size_t)n) * sizeof(float);
}
int mpo_abs_sum_flat(const float* x, int64_t n, float* out, void* workspace, size_t workspace_bytes, mpo_stream_t stream) {
    MPO_CHECK(n >= 1, "abs sum: n = %lld", (long long)n);
    MPO_CHECK(x && out && workspace, "abs sum: null argument");
    MPO_CHECK((reinterpret_cast<uintptr_t>(x) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0 &&
              (reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, "abs sum: pointers must be 4-byte aligned");
    MPO_CHECK(workspace_bytes >= mpo_abs_sum_flat_workspace_bytes(n), "abs sum: workspace too small (%zu bytes)",
              workspace_bytes);
    return mpo_launch_abs_sum(x, (size_t)n, static_cast<float*>(workspace), out, static_cast<hipStream_t>(stream));
}

// Verification hook: the small-row GEMMs have a branch-free body for regular products and a general body; both must
// give the same bits.  enabled = 0 routes every product through the general body.  Returns the previous setting.
int mpo_set_gemm_fast_path(int enabled) { return mpo_gemm_fast_path(enabled); }
int mpo_gemm_last_route(void) { return mpo_gemm_route_last(); }
int mpo_gemm_last_group_routes(void) { return mpo_gemm_route_group_take(); }
int mpo_set_coattn_bwd_two_wave(int enabled) { return mpo_coattn_bwd8_enable(enabled); }
// verification hook: 0 = fp32 bags take the general (matrix-pipe) K1 backward
int mpo_set_coattn_bwd_f32_vector(int enabled) { return mpo_coattn_bwd_f32_enable(enabled); }
// verification hook: 0 = K2's backward reads K twice (bag_colacc_gated, then bag_outer_gated, both on the matrix pipe) as in rounds 1-2
int mpo_set_nacagat_one_pass_key_grad(int enabled) {
    const int was = g_k2_one_pass_key ? 1 : 0;
    g_k2_one_pass_key = enabled != 0;
    return was;
}

// The two device-resident per-step counters of a captured training step, bumped by one launch.
int mpo_step_counters_bump(uint64_t* rng_epoch, int32_t* adam_step, mpo_stream_t stream) {
    MPO_CHECK(rng_epoch || adam_step, "step counters: nothing to bump");
    return mpo_launch_counters_bump(reinterpret_cast<unsigned long long*>(rng_epoch), adam_step, static_cast<hipStream_t>(stream));
}

}  // extern "C"