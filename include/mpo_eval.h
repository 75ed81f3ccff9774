/* Validation and test epochs on the device: the concordance index of a cohort and the per-slide statistics of a ragged
 * attention map -- entries of libmpo_hip.so's C ABI (conventions: mpo_hip.h, which includes this file; include that one).
 * Additive to ABI 14: no earlier entry changed, mpo_abi_version() stays 14. */
#ifndef MPO_EVAL_H
#define MPO_EVAL_H
#ifndef MPO_HIP_H
#error "include mpo_hip.h: it defines mpo_stream_t and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* concordance_index   Harrell's C of n subjects with scikit-survival's conventions (csrc/concordance.hip).  Over every ordered
 *               pair i != j:  event_i = (1 - censorship_i) != 0;  comparable = event_i and (time_j > time_i or (time_j ==
 *               time_i and not event_j));  diff = (double)risk_i - (double)risk_j;  tie = |diff| <= 1e-8 (the tolerance is
 *               scikit-survival's default and is not an argument);  concordant = comparable and diff > 0 and not tie;  tied =
 *               comparable and tie.  A NaN risk fails every comparison.  counts[0..3) = concordant, tied, comparable;
 *               *c_index = (concordant + 0.5 tied) / comparable in fp64, NaN when comparable == 0.  Integer counting:
 *               the same bits whatever the launch geometry.  Two launches on `stream` (per-workgroup counts into the
 *               workspace, then one workgroup adds them and divides): no atomics, nothing zeroed, no allocation, no host
 *               synchronisation -- capturable.  1 <= n <= 2^24.  time (fp64), censorship, risk (fp32), counts (int64[3]),
 *               c_index (fp64[1]): DEVICE, naturally aligned; workspace: DEVICE, caller-owned, 8-byte aligned,
 *               mpo_concordance_workspace_bytes(n) bytes (0 for an n out of range), not shared with a call that may run at
 *               the same time.
 * concordance_tile    subjects per tile of that kernel (its workgroup size): the sizes at which its loops change shape.
 * map_block_stats     out[b] = [min, max, mean] of slide b's block of a ragged attention map: the n_q * M_b values from
 *               n_q * cu_rows[b] on, as mpo_map_block_dot reads them (csrc/map_stats.hip).  Sums are carried in fp64 in a
 *               fixed order and rounded to fp32 once; min and max propagate a NaN.  Two launches on `stream`, whatever
 *               n_slides; no atomics, no allocation, no host synchronisation.  max_rows: the longest slide (sizes the grid; a
 *               longer slide's tail would go unread).  a_map, cu_rows, out (fp32 [n_slides][3]): DEVICE; workspace: DEVICE,
 *               caller-owned, 8-byte aligned, mpo_map_block_stats_workspace_bytes(n_slides, n_q, max_rows) bytes. */
size_t mpo_concordance_workspace_bytes(int64_t n);
int mpo_concordance_tile(void);
int mpo_concordance_index(const double* time, const float* censorship, const float* risk, int64_t n, int64_t* counts,
                          double* c_index, void* workspace, size_t workspace_bytes, mpo_stream_t stream);
size_t mpo_map_block_stats_workspace_bytes(int n_slides, int n_q, int max_rows);
int mpo_map_block_stats(const float* a_map, const int32_t* cu_rows, int n_slides, int n_q, int max_rows, float* out,
                        void* workspace, size_t workspace_bytes, mpo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPO_EVAL_H */
