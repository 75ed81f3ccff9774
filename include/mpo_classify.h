/* Classification metrics of a set of slides on the device: what the gene-expression model's validation and test epochs end
 * with -- an entry of libmpo_hip.so's C ABI (conventions: mpo_hip.h, which includes this file; include that one).
 * Additive to ABI 14: no earlier entry changed, mpo_abi_version() stays 14. */
#ifndef MPO_CLASSIFY_H
#define MPO_CLASSIFY_H
#ifndef MPO_HIP_H
#error "include mpo_hip.h: it defines mpo_stream_t and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* class_metrics       Predictions, confusion matrix, accuracy, balanced accuracy and mean loss of n rows of class scores
 *               (csrc/class_metrics.hip).  pred[b] = argmax of y[b] as torch.argmax takes it: the first index of a NaN if the
 *               row holds one, otherwise the first index of the maximum.  A label is valid when 0 <= label[b] < n_classes;
 *               confusion[label[b]][pred[b]] += 1 over the valid rows.  counts[0..4) = valid rows, correct rows, rows with an
 *               invalid label, rows that hold a NaN (valid or not).  summary[0] = correct / valid in fp64, NaN when valid ==
 *               0;  summary[1] = the mean of confusion[c][c] / support_c over the classes with support_c = sum_p
 *               confusion[c][p] > 0, added in class order, NaN when there is none;  summary[2] = sum(loss) / n over all n
 *               rows, carried in fp64 from the first addition in an order that depends on n alone, NaN when loss is null (a
 *               NaN loss propagates).  Integer counting: the same bits whatever the launch geometry.  Two launches on
 *               `stream` (per-workgroup partials into the workspace, then one workgroup finishes): no global atomics, nothing
 *               the caller zeroes, no allocation, no host synchronisation -- capturable.  1 <= n <= 2^24, 2 <= n_classes <= 8.
 *               y (fp32 [n][n_classes]), loss (fp32 [n], nullable), label, pred (int64 [n]; pred nullable), confusion (int64
 *               [n_classes][n_classes]), counts (int64 [4]), summary (fp64 [3]): DEVICE, naturally aligned; workspace: DEVICE,
 *               caller-owned, 8-byte aligned, mpo_class_metrics_workspace_bytes(n, n_classes) bytes (0 for an n or n_classes
 *               out of range), not shared with a call that may run at the same time.
 * class_metrics_tile  rows per tile of that kernel (its workgroup size): the sizes at which its loops change shape. */
size_t mpo_class_metrics_workspace_bytes(int64_t n, int n_classes);
int mpo_class_metrics_tile(void);
int mpo_class_metrics(const float* y, const int64_t* label, const float* loss /* nullable */, int64_t n, int n_classes,
                      int64_t* pred /* nullable */, int64_t* confusion, int64_t* counts, double* summary, void* workspace,
                      size_t workspace_bytes, mpo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPO_CLASSIFY_H */
