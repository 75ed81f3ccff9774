/* Fixed-budget patch sampling from a cohort resident on the device -- entries of libmpo_hip.so's C ABI (conventions: mpo_hip.h,
 * which includes this file; include that one).  Additive to ABI 14: no earlier entry changed, mpo_abi_version() stays 14. */
#ifndef MPO_COHORT_H
#define MPO_COHORT_H
#ifndef MPO_HIP_H
#error "include mpo_hip.h: it defines mpo_stream_t and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* The gather of mpo_bag_sample.h for a window whose slides are stored SEPARATELY: a window is n_slides ids into a table of
 * slides that lives on the device, so a shuffled epoch never assembles a contiguous window (csrc/bag_sample.hip).
 * The draw is the same: pi_b keyed by the slide's POSITION b in the window and its length M_b, so the same slides in the
 * same order with the same (seed, offset, *rng_epoch) give the bits mpo_bag_sample_rows gives on their concatenation.
 * Slides are addressed by pointer: the cohort's total row count has no 32-bit limit (a slide's own rows and the window's
 * n_slides * k output rows are int32).
 *   desc        DEVICE memory, 8-byte aligned, mpo_bag_sample_slides_desc_bytes(n_slides) bytes (0 for n_slides < 1), owned
 *               by the caller: uint64 ptr[n_slides], int32 len[n_slides], int32 ocu[n_slides + 1], rounded up to 16 bytes;
 *               written by bind_slides, read by the gather AT RUN TIME -- a launch captured into a HIP graph gathers from
 *               whichever slides were bound last before the replay.
 *   bind_slides one tiny launch on `stream`, no host synchronisation, no staging memory (a bind for the next window may be
 *               enqueued while this window's replay is still running).  table_ptrs: DEVICE uint64 [n_table], the address
 *               of every cohort slide's first row, 16-byte aligned; table_lens: DEVICE int32 [n_table]; ids: DEVICE int32
 *               [n_slides], the window.  ptr / len of the named slides are copied into desc; ocu[b + 1] - ocu[b] = k for
 *               every slide with `cycle`, min(k, M_b) without.  An id outside [0, n_table), a length < 1 or a misaligned
 *               pointer gives the slide length 0: the gather writes nothing for it and reads nothing.  The tables, ids'
 *               values as read by this launch, and the slides' rows must stay valid until the last gather that reads this
 *               binding has finished.
 *   slides      the gather; arguments, checks and messages as mpo_bag_sample_rows.  Output row ocu[b] + j is source row
 *               pi_b(j mod M_b) of slide b: for j < M_b (all there is without `cycle`) the sample without replacement; with
 *               `cycle` a slide shorter than k is lapped in its permuted order, every row floor(k / M_b) or ceil(k / M_b)
 *               times, each lap complete before any row repeats.  The lapped indices are the prefix
 *               mpo_bag_sample_indices_host gives, tiled.  Rows past ocu[n_slides] are not written. */
size_t mpo_bag_sample_slides_desc_bytes(int n_slides);
int mpo_bag_sample_bind_slides(void* desc, const uint64_t* table_ptrs, const int32_t* table_lens, int n_table, const int32_t* ids,
                               int n_slides, int k, int cycle, mpo_stream_t stream);
int mpo_bag_sample_slides(const void* desc, int n_slides, int k, int width, int elem_bytes, uint64_t seed, uint64_t offset,
                          const uint64_t* rng_epoch /* nullable */, void* out, mpo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPO_COHORT_H */
