/* include/deodr_hip_arap.h -- companion header of include/deodr_hip.h: the as-rigid-as-possible energy of Sorkine and Alexa (2007) on the device,
 * with its gradient and the per-vertex rotations.  What the mesh fitters regularise a deforming mesh with under rigidity="arap"
 * (deodr_amd/arap.py).
 *
 * Same library (libdeodr_hip.so), same conventions: device pointers, asynchronous on `stream` (hipStream_t as void*), no allocation, no
 * synchronisation, errors returned (0 = ok) with the message in deodr_hip_last_error().  It is versioned on its own
 * (DEODR_HIP_ARAP_ABI_VERSION) so that deodr_hip.h and the other companion headers stay what they are.
 *
 * THE OPERATION.  The vertex adjacency of the mesh in compressed rows: offsets [V + 1] and cols [nnz] uint32, weights [nnz] double; the weights
 * >= 0, the pattern and the weights symmetric, no diagonal, nnz = 0 allowed.  q = vertices_ref [V, 3], p = vertices [n, V, 3], doubles, contiguous,
 * n >= 1 independent poses.  For every pose and every vertex i, the sums over the entries j of row i in order, e^p_ij = p_i - p_j,
 * e^q_ij = q_i - q_j:
 *     S_i = sum_j w_ij e^p_ij (e^q_ij)^T                                  (entry (a, b): sum_j w_ij * (e^p_a * e^q_b))
 *     R_i = argmax over SO(3) of tr(R^T S_i)                              (a proper rotation, also when det S_i < 0)
 *     d_ij = e^p_ij - R_i e^q_ij,    d'_ij = e^p_ij - R_j e^q_ij
 *     energy      = 1/2 cregu sum_i sum_j w_ij |d_ij|^2
 *     gradient_i  = cregu sum_j w_ij (d_ij + d'_ij)                       (= cregu sum_j w_ij [2 e^p_ij - (R_i + R_j) e^q_ij])
 * The gradient is the exact gradient of the energy wherever every R_i is unique (the envelope theorem: the rotations are optimal, their own
 * derivative does not enter).
 * R_i: Horn's symmetric 4 x 4 matrix N of S_i (N00 = tr S, N01 = Szy - Syz, N02 = Sxz - Szx, N03 = Syx - Sxy, N11 = Sxx - Syy - Szz,
 * N12 = Sxy + Syx, N13 = Szx + Sxz, N22 = Syy - Sxx - Szz, N23 = Syz + Szy, N33 = Szz - Sxx - Syy), DEODR_HIP_ARAP_SWEEPS sweeps of cyclic Jacobi
 * over the pivots (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) in this order, and the eigenvector (w, x, y, z) of the largest diagonal entry, ties to the
 * lowest index, negated if w < 0.  A rotation of the pivot a_pq: theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1))
 * with sign(0) = 1, t = 1 / (2 theta) where |theta| > 1e150 (theta^2 would overflow), c = 1 / sqrt(t^2 + 1), s = t c.  A pivot that is exactly 0
 * is skipped (t = 0: the rotation is the identity, bit for bit).  The quaternion is used as it comes out (the eigenvectors are orthonormal to
 * rounding), R = the usual matrix of (x, y, z, w).
 *
 * CONTRACT
 *   - All arithmetic is double, without contraction.  No atomics on values: the order of every sum is fixed by (V, nnz, n) and the rows alone --
 *     a row's entries in order; the cell energies: the vertices of a thread in order, the lanes of a wavefront, the wavefronts, the workgroups --,
 *     so two calls give the same bits.
 *   - Two exact consequences of the skipped pivot and the tie rule: S_i = 0 (a vertex without neighbours, weights that are all 0, coincident
 *     points) gives R_i = identity; vertices bit-equal to vertices_ref give every R_i = identity, energy == 0.0 and gradient == 0.0 exactly,
 *     wherever S_i has rank >= 2 or is 0 (a ring that is a single direction leaves the half turn about it in a tie that rounding may break).
 *     Never a NaN for finite input whose products do not overflow.
 *   - The number of launches and their geometry depend on (V, nnz, n) alone -- deodr_hip_arap_launches, deodr_hip_arap_blocks --, nothing is read
 *     back: the call can be captured into a graph, and a replay follows vertices, vertices_ref and weights as they are at that moment.
 *   - offsets and cols aligned to 4 bytes, everything else to 8.
 *   - Refused before any launch, with a message: V <= 0, n outside 1 .. 65535 (the poses are the second dimension of the grid), cregu < 0 or NaN,
 *     a NULL pointer other than rotations (cols and weights may be NULL when nnz = 0), a misaligned pointer,
 *     scratch_bytes below deodr_hip_arap_scratch_bytes, an output overlapping an input, the scratch or another output.
 *   - PRECONDITIONS the call cannot check (the tables are device memory): offsets non-decreasing with offsets[0] = 0 and offsets[V] = nnz; every
 *     entry of cols < V; no diagonal entry; the pattern symmetric; the weights symmetric and >= 0.  deodr_amd/arap.py checks them on the host.
 */
#ifndef DEODR_HIP_ARAP_H
#define DEODR_HIP_ARAP_H

#include "deodr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sweeps of cyclic Jacobi.  Largest off-diagonal norm relative to the matrix norm after 3 / 4 / 5 / 6 sweeps over the cells of the test tables, in
 * long double: 7.0e-3 / 3.1e-7 / 2.3e-22 / 6.3e-71 (tools/arap_times.py --table): 5 is the first count below double's rounding. */
#define DEODR_HIP_ARAP_SWEEPS 5

/* The launch geometry: threads of a workgroup, a thread per vertex; workgroups per pose at most (the threads stride beyond). */
#define DEODR_HIP_ARAP_BLOCK 256
#define DEODR_HIP_ARAP_MAX_BLOCKS 512

/* energy [n] and gradient [n, V, 3] are overwritten, and rotations [n, V, 4] -- unit quaternions (x, y, z, w), w >= 0 -- unless it is NULL.
 * scratch: device memory of deodr_hip_arap_scratch_bytes(V, n) bytes, 8-byte aligned, used by one stream at a time.  It need NOT be zeroed: the
 * first kernel clears the arrival tickets of the second, and every other word is written before it is read.
 * Two launches over a grid of deodr_hip_arap_blocks(V) x n workgroups, a thread per (pose, vertex): the rotations (S, Horn, Jacobi; the quaternion
 * and the cell's energy to the scratch), then the gradient (the neighbours' quaternions gathered from the scratch) and the sum of the cell energies,
 * brought together by the last workgroup of a pose to arrive. */
int deodr_hip_arap_energy(const uint32_t *offsets, const uint32_t *cols, const double *weights, int V, uint32_t nnz, const double *vertices_ref,
						  const double *vertices, int n, double cregu, double *energy, double *gradient, double *rotations, void *scratch,
						  size_t scratch_bytes, void *stream);

/* Bytes of scratch deodr_hip_arap_energy needs: 64 + 8 (5 n V + DEODR_HIP_ARAP_MAX_BLOCKS n + (n + 1) / 2); 0 for V <= 0 or n outside 1 .. 65535.
 * Monotone in both arguments. */
size_t deodr_hip_arap_scratch_bytes(int V, int n);

/* The launch rule.  _launches: the number of kernel launches of a call, 2; 0 for arguments the call refuses.  _blocks: the workgroups per pose of
 * both launches, min(ceil(V / DEODR_HIP_ARAP_BLOCK), DEODR_HIP_ARAP_MAX_BLOCKS); 0 for V <= 0.  The grid is (_blocks(V), n). */
int deodr_hip_arap_launches(int V, uint32_t nnz, int n);
int deodr_hip_arap_blocks(int V);

/* ABI version of this header; bumped on any incompatible change. */
int deodr_hip_arap_abi_version(void);
#define DEODR_HIP_ARAP_ABI_VERSION 1

#ifdef __cplusplus
}
#endif
#endif /* DEODR_HIP_ARAP_H */
