/* Gradient-norm clipping and the non-finite step skip of the flat optimisers -- entries of libmpo_hip.so's C ABI (conventions:
 * mpo_hip.h, which includes this file; include that one).  Additive to ABI 14: no earlier entry changed, mpo_abi_version()
 * stays 14. */
#ifndef MPO_GRAD_GUARD_H
#define MPO_GRAD_GUARD_H
#ifndef MPO_HIP_H
#error "include mpo_hip.h: it defines mpo_stream_t and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* A step measures its gradient and then applies it, both on the device (csrc/grad_guard.hip): nothing is read by the host,
 * so both calls sit inside a captured step.  They talk through the CONTROL BLOCK `ctl`: DEVICE, caller-owned, 16 bytes,
 * 4-byte aligned, four 32-bit words
 *     word 0  norm       fp32   || g' || of the last measured gradient, g' = g + l1 sign(p)
 *     word 1  coef       fp32   the clipping coefficient of that gradient (1 when clipping is off)
 *     word 2  nonfinite  int32  1 when an element of that g' was an infinity or a NaN, else 0
 *     word 3  skipped    int32  running count of steps skipped for that reason; the caller zeroes it once
 * mpo_grad_norm_flat writes words 0-2 and adds to word 3; mpo_optim_step_flat_guarded only reads.
 *
 *   grad_norm_flat   norm = sqrt(sum_i g'_i^2) over g' = g + l1 sign(p) (sign(0) = 0; the L1 penalty's gradient is part of
 *               what is clipped; l1 == 0: p may be NULL), each g' formed in fp32 as the optimiser forms it, squared and
 *               summed in fp64 (a finite fp32 gradient cannot overflow the sum) and rounded to fp32 once after the root.
 *               coef = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1 (torch.nn.utils.clip_grad_norm_), in fp64, rounded
 *               once; a NaN norm gives 1.  nonfinite comes from the exponent bits of the elements, not from the sum.
 *               skip_nonfinite != 0 and nonfinite: skipped += 1 and, step_dev not NULL, *step_dev -= 1 -- the step count a
 *               caller advanced before the gradient was known counts applied steps only.  Two launches (per-workgroup
 *               partial sums on a grid that is a function of n alone, then one workgroup adds them in a fixed order):
 *               no atomics, the same bits every time; no allocation, no host synchronisation.  g, p: DEVICE, 4-byte
 *               aligned (16-byte aligned: 16-byte loads); workspace: DEVICE, caller-owned, 8-byte aligned,
 *               mpo_grad_norm_flat_workspace_bytes(n) bytes.
 *   optim_step_flat_guarded   mpo_optim_step_flat (same arguments, algorithms, checks and update rules) on the gradient
 *               g' = coef (g + l1 sign(p)) + weight_decay p with coef = ctl.coef: weight decay is added after the clip, as
 *               torch.optim adds it.  coef == 1 gives mpo_optim_step_flat's bits (the kernel then runs that pass's own
 *               loops; a clipped step agrees with it on coef * g to the last few ulps).  skip_nonfinite != 0 and ctl.nonfinite:
 *               nothing is written -- parameters, both states and the padding keep their bits.  ctl must hold what an
 *               mpo_grad_norm_flat ordered before this call on the stream wrote, with the same g, p and l1. */
size_t mpo_grad_norm_flat_workspace_bytes(int64_t n);
int mpo_grad_norm_flat(const float* grads, const float* params, int64_t n, float l1, float max_norm, int skip_nonfinite,
                       int32_t* step_dev, void* ctl, void* workspace, size_t workspace_bytes, mpo_stream_t stream);
int mpo_optim_step_flat_guarded(int algorithm, float* params, const float* grads, float* state1, float* state2, int64_t n,
                                float lr, const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                                float l1, int step, const int32_t* step_dev, const void* ctl, int skip_nonfinite,
                                mpo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPO_GRAD_GUARD_H */
