/* Gated-concat and bilinear fusion + classifier + survival head as one call each way -- entries of libmpo_hip.so's C ABI (conventions:
 * mpo_hip.h, which includes this file; include that one).  Additive to ABI 14: no earlier entry changed, mpo_abi_version()
 * stays 14. */
#ifndef MPO_FUSION_NEXT_H
#define MPO_FUSION_NEXT_H
#ifndef MPO_HIP_H
#error "include mpo_hip.h: it defines mpo_stream_t and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* GatedConcatFusion (models/fusion.py:22-41, with its gates as parameters) in front of K6's MLP, classifier and head:
 *   g_i = sigmoid(w_i . x_i + b_i),  hcat = [x_0 g_0 | x_1 g_1],  then exactly what mpo_fusion_head_* does on hcat
 *   (din = 2 d, hidden = dout = d).
 *   h_path, h_omic   DEVICE [n_slides] rows of d floats, 16-byte aligned, BOTH with the row stride `row_stride` (floats,
 *            >= d, a multiple of 4): row_stride = 2 d and h_omic = h_path + d is the interleaved (B, [h_path | h_omic])
 *            row the pooling launch writes; row_stride = d is two separate (B, d) matrices.  No copy either way.
 *   d_h_path, d_h_omic   the gradients, same shape, same row stride; every element of every row is written.
 *   d        128, 256 or 512;  n_classes 1..16 (the head kernels' range);  n_slides >= 1, any.
 *   params   10 DEVICE pointers: gates.0.0.weight [1][d], gates.0.0.bias [1], gates.1.0.weight, gates.1.0.bias,
 *            fusion_layer.0.weight [d][2 d], .bias, fusion_layer.2.weight [d][d], .bias, classifier.weight [C][d], .bias.
 *   grads    10 DEVICE pointers in the same order; each gradient is overwritten (not accumulated).  The gate gradients
 *            dw_i[j] = sum_b t_b x_i[b][j], db_i = sum_b t_b (t_b = (d_hcat_b . x_b) g_b (1 - g_b)) are summed over the
 *            slides b = 0, 1, ... in that order by one thread per element: no atomics, bit-equal from run to run.
 *   saved    *_saved_floats() floats, written by the forward and read by the backward (the loss form keeps d_logits
 *            there as mpo_fusion_head_loss_forward does; it has its own size).
 *   workspace   *_workspace_bytes() bytes for either backward; a shorter one is refused ("workspace too small").
 *   rng_span    counters a training-mode call takes from the generator: 0 -- the layer has no dropout.
 *   loss_kind   0 = `ces` (models/loss.py:5-28, weight alpha), 1 = `sct` (models/loss.py:62-85 on Y; alpha unused).
 * The loss form is the training step: head, loss and the backward of both in one launch, loss[b] and risk[b] per slide, the
 * gradient that enters loss[b] is slide_weight[b]; its backward continues from the stored d_logits.
 * A null argument and a geometry outside the ranges above are refused with a reason before any launch. */
size_t mpo_gated_concat_head_saved_floats(int n_slides, int d, int n_classes);
size_t mpo_gated_concat_head_loss_saved_floats(int n_slides, int d, int n_classes);
size_t mpo_gated_concat_head_workspace_bytes(int n_slides, int d, int n_classes);
uint64_t mpo_gated_concat_head_rng_span(int n_slides, int d);
int mpo_gated_concat_head_forward(const float* h_path, const float* h_omic, int row_stride, int n_slides, int d, int n_classes,
                                  const float* const* params, float* hazards, float* survs, float* y, float* saved,
                                  mpo_stream_t stream);
int mpo_gated_concat_head_backward(const float* h_path, const float* h_omic, int row_stride, int n_slides, int d, int n_classes,
                                   const float* const* params, const float* saved, const float* hazards, const float* survs,
                                   const float* y, const float* d_hazards /* nullable */, const float* d_survs /* nullable */,
                                   const float* d_y /* nullable */, float* d_h_path, float* d_h_omic, float* const* grads,
                                   void* workspace, size_t workspace_bytes, mpo_stream_t stream);
int mpo_gated_concat_head_loss_forward(const float* h_path, const float* h_omic, int row_stride, int n_slides, int d,
                                       int n_classes, const float* const* params, const int64_t* label,
                                       const float* censorship, const float* slide_weight, float alpha, float eps,
                                       int loss_kind, float* hazards, float* survs, float* y, float* loss, float* risk,
                                       float* saved, mpo_stream_t stream);
int mpo_gated_concat_head_loss_backward(const float* h_path, const float* h_omic, int row_stride, int n_slides, int d,
                                        int n_classes, const float* const* params, const float* saved, float* d_h_path,
                                        float* d_h_omic, float* const* grads, void* workspace, size_t workspace_bytes,
                                        mpo_stream_t stream);

/* BilinearFusion (models/fusion.py:44-113 with gates, bilinear products and skip connection on -- what the models build) +
 * classifier + head, in the same four forms.  Differences from the entries above:
 *   hidden, mm_hidden   the layer's hidden_size and mm_hidden_size: 32 and 64 (the reference's defaults) or the call is refused.
 *   params / grads   18 DEVICE pointers: linear_h1.0.weight [32][d], .bias, linear_z1.weight [32][d][d], .bias, linear_o1.0.weight
 *            [32][32], .bias, the same six of branch 2 (z2 = bilinear(h_omic, h_path)), fc1.0.weight [64][1089], .bias,
 *            fc2.0.weight [d][130], .bias, classifier.weight [C][d], .bias.  Every gradient is overwritten; every sum over
 *            slides, rows or partial results runs in a fixed order (no atomics).
 *   drop_p, seed, offset, rng_epoch (nullable)   training-mode dropout as mpo_gated_pool_forward takes it (0 = eval); the
 *            backward takes the same four and regenerates the masks, none is stored.  rng_span(n_slides, d) = 5 * stride,
 *            stride = ceil(n_slides * 1089 / 4) + 2; site s draws from the stream that starts at counter
 *            offset + *rng_epoch * 2^40 + s * stride, element idx of a stream = word idx % 4 of counter idx / 4 (dropout_keep):
 *              s = 0, 1   linear_o1 / linear_o2's dropout, idx = slide * 32 + column
 *              s = 2      post_fusion_dropout on the Kronecker product, idx = slide * 1089 + 33 p + q
 *              s = 3      fc1's dropout, idx = slide * 64 + column
 *              s = 4      fc2's dropout, idx = slide * d + column
 * n_slides any (1 .. 2^20): the pass over the bilinear weights keeps 16 slides (8 at d = 512) in LDS at a time and walks longer
 * windows tile by tile. */
size_t mpo_bilinear_head_saved_floats(int n_slides, int d, int n_classes);
size_t mpo_bilinear_head_loss_saved_floats(int n_slides, int d, int n_classes);
size_t mpo_bilinear_head_workspace_bytes(int n_slides, int d, int n_classes);
uint64_t mpo_bilinear_head_rng_span(int n_slides, int d);
int mpo_bilinear_head_forward(const float* h_path, const float* h_omic, int row_stride, int n_slides, int d, int hidden, int mm_hidden,
                              int n_classes, const float* const* params, float drop_p, uint64_t seed, uint64_t offset,
                              const uint64_t* rng_epoch, float* hazards, float* survs, float* y, float* saved, mpo_stream_t stream);
int mpo_bilinear_head_backward(const float* h_path, const float* h_omic, int row_stride, int n_slides, int d, int hidden, int mm_hidden,
                               int n_classes, const float* const* params, float drop_p, uint64_t seed, uint64_t offset,
                               const uint64_t* rng_epoch, const float* saved, const float* hazards, const float* survs, const float* y,
                               const float* d_hazards, const float* d_survs, const float* d_y, float* d_h_path, float* d_h_omic,
                               float* const* grads, void* workspace, size_t workspace_bytes, mpo_stream_t stream);
int mpo_bilinear_head_loss_forward(const float* h_path, const float* h_omic, int row_stride, int n_slides, int d, int hidden,
                                   int mm_hidden, int n_classes, const float* const* params, float drop_p, uint64_t seed,
                                   uint64_t offset, const uint64_t* rng_epoch, const int64_t* label, const float* censorship,
                                   const float* slide_weight, float alpha, float eps, int loss_kind, float* hazards, float* survs,
                                   float* y, float* loss, float* risk, float* saved, mpo_stream_t stream);
int mpo_bilinear_head_loss_backward(const float* h_path, const float* h_omic, int row_stride, int n_slides, int d, int hidden,
                                    int mm_hidden, int n_classes, const float* const* params, float drop_p, uint64_t seed,
                                    uint64_t offset, const uint64_t* rng_epoch, const float* saved, float* d_h_path, float* d_h_omic,
                                    float* const* grads, void* workspace, size_t workspace_bytes, mpo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPO_FUSION_NEXT_H */
