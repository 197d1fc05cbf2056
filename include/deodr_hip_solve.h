/* include/deodr_hip_solve.h -- companion header of include/deodr_hip.h: a sparse symmetric positive definite solve on the device, by conjugate
 * gradients with a fixed number of steps.  What the mesh fitters smooth a vertex gradient with: u = (I + lambda L)^-1 g, L the mesh Laplacian
 * (deodr_amd/smoothing.py).
 *
 * Same library (libdeodr_hip.so), same conventions: device pointers, asynchronous on `stream` (hipStream_t as void*), no allocation, no
 * synchronisation, errors returned (0 = ok) with the message in deodr_hip_last_error().  It is versioned on its own
 * (DEODR_HIP_SOLVE_ABI_VERSION) so that deodr_hip.h and the other companion headers stay what they are.
 *
 * THE OPERATION.  A: n x n, symmetric positive definite, in compressed rows: offsets [n + 1] and cols [nnz] uint32, vals [nnz] double, the diagonal
 * stored like any other entry.  b, x: [n, D] doubles, contiguous, 1 <= D <= 4.  The D columns are solved independently from x = 0; every sum
 * below is over the rows of ONE column d:
 *     r = b,  p = r,  rho = sum r^2,  rho_b = rho
 *     `iterations` times:   q = A p;   sigma = sum p q
 *                           active = (rho > rel_tol^2 rho_b) and (sigma > 0)
 *                           alpha = active ? rho / sigma : 0;    x += alpha p;    r -= alpha q
 *                           rho' = sum r^2;    beta = active ? rho' / rho : 0;    rho = active ? rho' : rho
 *                           p = r + beta p
 *     residual[d] = rho_b > 0 ? rho / rho_b : 0                      (the SQUARED relative residual of the recurrence)
 * A column of b that is all zeros, a column that has reached rel_tol, and a column whose rho has reached 0 (in exact arithmetic: after n steps)
 * is frozen: its x no longer changes, and no division by zero is ever made.  A truncated run is still a descent direction: b^T x = x^T A x >= 0.
 *
 * CONTRACT
 *   - All arithmetic is double, without contraction.  No atomics on values: the order of every sum is fixed by (n, nnz, D) and the rows alone, so two
 *     calls give the same bits.
 *   - The number of launches depends on (n, nnz, D, iterations) alone -- deodr_hip_spd_solve_launches --, nothing is read back: the call can be
 *     captured into a graph, and a replay follows b and vals as they are at that moment.
 *   - offsets and cols aligned to 4 bytes, everything else to 8.
 *   - Refused before any launch, with a message: n <= 0, nnz < n, D outside 1 .. 4, iterations < 1, rel_tol < 0 or NaN, a NULL pointer, a misaligned
 *     pointer, scratch_bytes below deodr_hip_spd_solve_scratch_bytes, x overlapping b, an output or the scratch overlapping anything else.
 *   - PRECONDITIONS the call cannot check (the tables are device memory): A symmetric and positive definite; offsets non-decreasing with
 *     offsets[0] = 0 and offsets[n] = nnz; every entry of cols < n.  deodr_amd/smoothing.py checks them on the host when it builds a system.
 */
#ifndef DEODR_HIP_SOLVE_H
#define DEODR_HIP_SOLVE_H

#include "deodr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Systems of at most this many rows run as ONE launch (below); larger ones as 2 + 2 iterations launches. */
#define DEODR_HIP_SOLVE_N_SMALL 1024

/* x [n, D] and residual [D] are overwritten.  scratch: device memory of deodr_hip_spd_solve_scratch_bytes(n, D) bytes, 8-byte aligned, used by one
 * stream at a time.  It need NOT be zeroed: the call clears the counter words at its start (a kernel of its own) where it uses them and writes
 * every other word before it reads it.
 * n <= DEODR_HIP_SOLVE_N_SMALL: one launch of D workgroups, one per column, a thread per row: p in LDS, x, r and q in registers, the sums through
 * the workgroup; no workgroup waits for another.
 * n >  DEODR_HIP_SOLVE_N_SMALL: one launch that clears the counter words, one that sets r = b, x = 0, rho; then two per iteration --
 * q = A (r + beta p) with eight adjacent lanes per row, sigma and alpha; then x, r, rho', beta -- whose sums are brought together by the last
 * workgroup to arrive; r, q and two copies of p live in the scratch. */
int deodr_hip_spd_solve(const uint32_t *offsets, const uint32_t *cols, const double *vals, int n, uint32_t nnz, const double *b, double *x, int D,
						int iterations, double rel_tol, double *residual, void *scratch, size_t scratch_bytes, void *stream);

/* Bytes of scratch deodr_hip_spd_solve needs: 64 + 8 (24 + 4 * 512 + 4 n D); 0 for n <= 0 or D outside 1 .. 4.  Monotone in both arguments. */
size_t deodr_hip_spd_solve_scratch_bytes(int n, int D);

/* The number of kernel launches of a call (the rule the call follows): 1 for n <= DEODR_HIP_SOLVE_N_SMALL, 2 + 2 iterations above; 0 for arguments
 * the call refuses. */
int deodr_hip_spd_solve_launches(int n, uint32_t nnz, int D, int iterations);

/* ABI version of this header; bumped on any incompatible change. */
int deodr_hip_solve_abi_version(void);
#define DEODR_HIP_SOLVE_ABI_VERSION 1

#ifdef __cplusplus
}
#endif
#endif /* DEODR_HIP_SOLVE_H */
