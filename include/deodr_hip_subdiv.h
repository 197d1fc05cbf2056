/* include/deodr_hip_subdiv.h -- companion header of include/deodr_hip.h: Loop subdivision on the device, as the product of a sparse matrix.
 *
 * Same library (libdeodr_hip.so), same conventions: device pointers, asynchronous on `stream` (hipStream_t as void*), no allocation, no
 * synchronisation, errors returned (0 = ok) with the message in deodr_hip_last_error().  It is versioned on its own
 * (DEODR_HIP_SUBDIV_ABI_VERSION) so that deodr_hip.h and deodr_hip_texture.h stay what they are.
 *
 * The fine vertices of a Loop subdivision surface are S control, S a fixed sparse matrix of the mesh's connectivity (k levels composed into one
 * matrix on the host, deodr_amd/subdivision.py); the adjoint is S^T gradient.  Both are one call of deodr_hip_subdiv_apply on a matrix in
 * compressed rows: offsets [n_rows + 1], cols and vals [nnz], nnz = offsets[n_rows].
 */
#ifndef DEODR_HIP_SUBDIV_H
#define DEODR_HIP_SUBDIV_H

#include "deodr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*     y[b][r][:] (= | +=) sum over k in [offsets[r], offsets[r+1]) of vals[k] * x[b][cols[k]][:]          b < batch, r < n_rows
 * x is [batch, n_cols, D], y is [batch, n_rows, D], contiguous, in `dtype` (DEODR_HIP_F32 / DEODR_HIP_F64); accumulate != 0: added to what y holds.
 * Arithmetic in double whatever the storage type, one rounding per stored value.  1 <= D <= DEODR_HIP_MAX_COLORS (a compile-time instance for
 * D = 3, a run-time loop otherwise), batch <= 65535.  Every row is summed in an order fixed by the row alone (no atomics): bit-identical from run
 * to run.  y must not overlap x.
 * nnz: the number of entries, offsets[n_rows] -- the library cannot read it without waiting for the device, and it decides (with n_rows) how
 * many adjacent lanes walk a row: deodr_hip_subdiv_lanes.
 * PRECONDITIONS the call cannot check (the tables are device memory): offsets non-decreasing with offsets[0] = 0 and offsets[n_rows] = nnz, every
 * entry of cols < n_cols.  deodr_amd/subdivision.py checks them on the host when it builds the tables. */
int deodr_hip_subdiv_apply(const uint32_t *offsets, const uint32_t *cols, const double *vals, int n_rows, int n_cols, uint32_t nnz, const void *x, void *y,
						   int batch, int D, int dtype, int accumulate, void *stream);

/* The kernel instance deodr_hip_subdiv_apply launches for a matrix of n_rows rows and nnz entries: 8 (adjacent lanes per row: the short rows of S)
 * or 64 (a whole wavefront per row: the long rows of S^T); 0 for n_rows <= 0. */
int deodr_hip_subdiv_lanes(int n_rows, uint32_t nnz);

/* ABI version of this header; bumped on any incompatible change. */
int deodr_hip_subdiv_abi_version(void);
#define DEODR_HIP_SUBDIV_ABI_VERSION 1

#ifdef __cplusplus
}
#endif
#endif /* DEODR_HIP_SUBDIV_H */
