/* Fixed-budget patch sampling -- entries of libmpo_hip.so's C ABI (conventions: mpo_hip.h, which includes this file; include
 * that one).  Additive to ABI 14: no earlier entry changed, mpo_abi_version() stays 14. */
#ifndef MPO_BAG_SAMPLE_H
#define MPO_BAG_SAMPLE_H
#ifndef MPO_HIP_H
#error "include mpo_hip.h: it defines mpo_stream_t and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Beyond the reference, which feeds every patch of a slide.
 * Output row j < min(k, M_b) of slide b is source row pi_b(j) of that slide, pi_b a permutation of [0, M_b) that is a pure
 * function of (seed, offset + *rng_epoch * 2^40, b, M_b) (csrc/bag_sample.h: four-round Feistel network on fmix32 with
 * cycle-walking): k rows without replacement, a slide shorter than k whole (in permuted order).  The output is ragged like
 * any window: slide b owns output rows ocu[b] .. ocu[b+1]-1, ocu[b+1] - ocu[b] = min(k, M_b) -- (n_slides * k, width) of
 * static shape when every slide has at least k rows.  One offset per call (the offset is a key, not a range of counters).
 *   desc     DEVICE memory, 8-byte aligned, mpo_bag_sample_desc_bytes(n_slides) bytes, owned by the caller: the window's
 *            base pointer, cu_rows and ocu as mpo_bag_sample_bind writes them and mpo_bag_sample_rows reads them AT RUN
 *            TIME -- a launch captured into a HIP graph gathers from whichever window was bound last before the replay.
 *   bind     one tiny launch on `stream`: the base pointer is a kernel argument, cu_rows (DEVICE int32 [n_slides + 1], the
 *            window's own) is copied device to device.  No host synchronisation and no staging memory.  `rows` 16-byte
 *            aligned; it and cu_rows must stay valid until the last gather that reads this binding has finished.
 *   rows     the gather: width elements of elem_bytes (2 = bf16, 4 = fp32) per row, width * elem_bytes a multiple of 16;
 *            `out` 16-byte aligned with room for n_slides * k rows; rows past ocu[n_slides] are not written.
 *   indices_host  pure host code, no GPU: indices[b * k + j] = pi_b(j) (slide-local) for j < min(k, lengths[b]), else -1;
 *            `epoch` is the VALUE *rng_epoch would hold (0 without one).  lengths: HOST int32 [n_slides], every one >= 1. */
size_t mpo_bag_sample_desc_bytes(int n_slides);
int mpo_bag_sample_bind(void* desc, const void* rows, const int32_t* cu_rows, int n_slides, int k, mpo_stream_t stream);
int mpo_bag_sample_rows(const void* desc, int n_slides, int k, int width, int elem_bytes, uint64_t seed, uint64_t offset,
                        const uint64_t* rng_epoch /* nullable */, void* out, mpo_stream_t stream);
int mpo_bag_sample_indices_host(const int32_t* lengths, int n_slides, int k, uint64_t seed, uint64_t offset, uint64_t epoch,
                                int32_t* indices);

#ifdef __cplusplus
}
#endif
#endif /* MPO_BAG_SAMPLE_H */
