/* The patch layer of an fp16-stored window -- entries of libmpo_hip.so's C ABI (conventions: mpo_hip.h, which includes this
 * file; include that one).  Additive to ABI 14: no earlier entry changed, mpo_abi_version() stays 14. */
#ifndef MPO_PATCH_F16_H
#define MPO_PATCH_F16_H
#ifndef MPO_HIP_H
#error "include mpo_hip.h: it defines mpo_stream_t and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* mpo_patch_fc_f32_forward / _backward for a window whose patch features are stored in fp16 (models/mcat/mcat.py:24-29,87 with
 * fp16 patch features), 1024 -> 256 (csrc/patch_fc_split.hip):
 *   forward   H_bag = Dropout(ReLU(X W^T + b)) in fp32 storage, X [total_rows][1024] fp16.  An fp16 feature is one fp16 MFMA
 *             operand as it is stored, so there is NO feature scale and no split of X: products as two fp16 MFMA terms
 *             W_hi X + W_lo X with fp32 accumulation (W_H scaled by its own maximum inside the call and split, as in the fp32
 *             entry).  The only rounding against the fp64 product of the stored operands is W's dropped tail (2^-22 of a
 *             product) and the accumulation.  Dropout: the fp32 entry's counter hash, 8 bits per element (realised p =
 *             round(256 p) / 256), keyed by (row, column group): the same (seed, offset, epoch) gives the fp32 entry's mask;
 *             the mask lives in H_bag as zeros.  Non-finite features stay non-finite in their rows of H_bag.
 *   backward  d_weight = g^T X, d_bias = colsum(g) with g = d_h_bag (.) [H_bag > 0] * gate; gate = 256 / (256 - drop_256)
 *             (1 without dropout); h_bag NULL: g = d_h_bag.  Three bf16 MFMA terms; X splits into bf16 hi + lo exactly.
 *             X needs no gradient (it is data).
 * drop_256: the dropout rate as the kernel realises it, in 256ths -- round(256 p), what the fp32 entry forms from its drop_p
 *             (ops._realised_drop(p) * 256): an element is dropped when its hash byte is below drop_256, a kept one scaled by
 *             256 / (256 - drop_256); 0 = no dropout.  Forward and backward take the SAME integer, and the backward forms
 *             its gate 256 / (256 - drop_256) from it: the realised rate is exact by construction and the two directions
 *             cannot disagree about the keep scale.  0 .. 255; 256 (p >= 1 - 1/512) and anything outside [0, 256] are
 *             refused in the fp32 entry's words, before anything is launched.
 * patches: DEVICE, fp16, 16-byte aligned rows (contiguous [total_rows][1024]); every other pointer as in the fp32 entries.
 * workspace: caller-owned, mpo_patch_fc_f16_workspace_bytes(backward) bytes (the fp32 entries' sizes).  Launches on `stream`
 * only: no allocation, no host synchronisation -- capturable. */
size_t mpo_patch_fc_f16_workspace_bytes(int backward);
int mpo_patch_fc_f16_forward(const void* patches, int64_t total_rows, int patch_dim, const float* patch_weight,
                             const float* patch_bias, int embed, int drop_256, uint64_t seed, uint64_t offset,
                             const uint64_t* rng_epoch, float* h_bag, void* workspace, size_t workspace_bytes,
                             mpo_stream_t stream);
int mpo_patch_fc_f16_backward(const float* d_h_bag, const float* h_bag /* nullable */, const void* patches, int64_t total_rows,
                              int embed, int patch_dim, int drop_256, float* d_weight, float* d_bias, void* workspace,
                              size_t workspace_bytes, mpo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPO_PATCH_F16_H */
