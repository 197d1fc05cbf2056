/* include/deodr_hip_basis.h -- companion header of include/deodr_hip.h: a dense linear basis (PCA / blend shapes / eigen-textures) on the device.
 *
 * Same library (libdeodr_hip.so), same conventions: device pointers, asynchronous on `stream` (hipStream_t as void*), no allocation, no
 * synchronisation, errors returned (0 = ok) with the message in deodr_hip_last_error().  It is versioned on its own
 * (DEODR_HIP_BASIS_ABI_VERSION) so that deodr_hip.h and the other companion headers stay what they are.
 *
 * A morphable model is `mean + coefficients . basis`: K coefficients give the N rendered values (N = 3 V for a shape model, Ht Wt C for an
 * eigen-texture), and the gradient of the K coefficients is `basis . gradient of the N values`.  `basis` is [K, N] row-major (the layout of a PCA's
 * components_) in `basis_dtype` (DEODR_HIP_F32 / DEODR_HIP_F64); `mean` is [N] in `basis_dtype`, or NULL for zero.  Coefficients and their gradient
 * are always double, [batch, K].
 *
 * CONTRACT of both directions
 *   - Arithmetic is double whatever the storage, one rounding per stored value.
 *   - No atomics on values: every sum is taken in an order fixed by (K, N, batch) alone, results are bit-identical from run to run.
 *   - Pointers need the alignment of ONE element only (a basis, a texture, a vertex array may be a slice of a larger buffer); N need not be a
 *     multiple of anything.
 *   - Limits: 1 <= K <= 1024, 1 <= batch <= 64, 1 <= N <= 2^30, K N <= 2^31 - 1 (offsets are formed in size_t all the same).
 *   - Refused before any launch, with a message: a NULL among the required pointers, each range above, an unknown dtype tag, a pointer
 *     misaligned for its element, an overlap named below, scratch_bytes below deodr_hip_basis_scratch_bytes.
 */
#ifndef DEODR_HIP_BASIS_H
#define DEODR_HIP_BASIS_H

#include "deodr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*     y[b][j] = mean[j] + sum over k < K of coeffs[b][k] * basis[k][j]          j < N, b < batch
 * y is [batch, N] contiguous in `y_dtype` (DEODR_HIP_F32 / DEODR_HIP_F64).  A value is summed in the order mean, k = 0, 1, ..; every stored element
 * has one writer.  batch = 1 streams `basis` once; a larger batch is done in chunks of 4 coefficient vectors, each of which streams it once.
 * y must not overlap basis, mean or coeffs. */
int deodr_hip_basis_apply(const void *basis, const void *mean, const double *coeffs, int K, int N, int batch, int basis_dtype, void *y, int y_dtype,
						  void *stream);

/*     coeffs_b[b][k] (= | +=) sum over j < N of basis[k][j] * g[b][j]          k < K, b < batch
 * g is [batch, N] contiguous in `g_dtype`; accumulate != 0: added to what coeffs_b holds.  A row of `basis` is cut into
 * deodr_hip_basis_segments(K, N) pieces; a workgroup sums one piece of 8 rows (threads, then lanes, then wavefronts, in a fixed order) into one
 * partial per (row, piece, b), and the last workgroup to arrive for those 8 rows adds their partials in piece order.
 * coeffs_b must not overlap basis or g.
 * scratch: device memory of deodr_hip_basis_scratch_bytes(K, N, batch) bytes, 8-byte aligned, ZERO-FILLED ONCE by the caller (the kernel leaves
 * its counter words zero), used by one stream at a time. */
int deodr_hip_basis_apply_b(const void *basis, const void *g, int g_dtype, int K, int N, int batch, int basis_dtype, double *coeffs_b, int accumulate,
							void *scratch, size_t scratch_bytes, void *stream);

/* Bytes of scratch deodr_hip_basis_apply_b needs; 0 for arguments outside the limits above. */
size_t deodr_hip_basis_scratch_bytes(int K, int N, int batch);

/* The number of pieces into which deodr_hip_basis_apply_b cuts a row of `basis`: one for small problems, enough to fill the chip for large ones;
 * non-decreasing in N for a fixed K.  A pure host function of (K, N); 0 for arguments outside the limits above. */
int deodr_hip_basis_segments(int K, int N);

/* ABI version of this header; bumped on any incompatible change. */
int deodr_hip_basis_abi_version(void);
#define DEODR_HIP_BASIS_ABI_VERSION 1

#ifdef __cplusplus
}
#endif
#endif /* DEODR_HIP_BASIS_H */
