/* The feature scale of an fp32 window, found on the device -- entries of libmpo_hip.so's C ABI (conventions: mpo_hip.h, which
 * includes this file; include that one).  Additive to ABI 14: no earlier entry changed, mpo_abi_version() stays 14. */
#ifndef MPO_FEATURE_RANGE_H
#define MPO_FEATURE_RANGE_H
#ifndef MPO_HIP_H
#error "include mpo_hip.h: it defines mpo_stream_t and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* mpo_patch_fc_f32_forward takes x_scale, a power of two derived from max |X|, BY VALUE: a host read per window, and a
 * constant of any HIP graph the call is captured into.  These entries keep the scale on the device
 * (csrc/feature_range.hip): a step captured once follows whatever the window holds when it is replayed.
 *   feature_range_f32   *scale_out = 2^(15 - e) for max |x[0 .. n)| = m 2^e, m in [0.5, 1), the exponent clamped to +-100;
 *               1.0 when the maximum is zero or any element is an infinity or a NaN (the maximum is taken over the
 *               magnitude BITS, where every NaN orders above infinity, so one non-finite element decides), and when
 *               n == 0 (x may be NULL then; only the write of scale_out is launched).  Exactly the value
 *               mpo_patch_fc_f32_forward documents for x_scale.  Three tiny launches on `stream` (clear, reduce, write),
 *               no host synchronisation, no allocation: capturable.  x: DEVICE, 16-byte aligned; scale_out: DEVICE,
 *               one float; workspace: DEVICE, caller-owned, 4-byte aligned, mpo_feature_range_workspace_bytes() bytes,
 *               not shared with a call that may run at the same time.
 *   patch_fc_f32_forward_dev   mpo_patch_fc_f32_forward with x_scale read through a DEVICE pointer when the kernel
 *               starts (as the kernel reads W_H's scale): the same kernel, the same checks otherwise, the same bits
 *               for the same scale.  The host cannot look at the value: x_scale must hold what mpo_feature_range_f32
 *               wrote (a power of two), by a launch ordered before this one on the stream.  The backward entry takes
 *               no scale: mpo_patch_fc_f32_backward serves both. */
size_t mpo_feature_range_workspace_bytes(void);
int mpo_feature_range_f32(const float* x, int64_t n, float* scale_out, void* workspace, size_t workspace_bytes,
                          mpo_stream_t stream);
int mpo_patch_fc_f32_forward_dev(const float* patches, int64_t total_rows, int patch_dim, const float* patch_weight,
                                 const float* patch_bias, int embed, float drop_p, uint64_t seed, uint64_t offset,
                                 const uint64_t* rng_epoch, const float* x_scale, float* h_bag, void* workspace,
                                 size_t workspace_bytes, mpo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPO_FEATURE_RANGE_H */
