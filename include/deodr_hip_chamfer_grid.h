/* include/deodr_hip_chamfer_grid.h -- companion header of include/deodr_hip.h: the closest-point (ICP / Chamfer) energy of
 * include/deodr_hip_chamfer.h with the nearest neighbours found over a uniform grid of hashed cells instead of by brute force, and the stable
 * sort by key that it is built on.  What deodr_amd/chamfer.py (PointCloudTerm(search="grid")) and MeshPointCloudFitter(search="grid") call.
 *
 * Same library (libdeodr_hip.so), same conventions: device pointers, asynchronous on `stream` (hipStream_t as void*), no allocation, no
 * synchronisation, errors returned (0 = ok) with the message in deodr_hip_last_error().  Versioned on its own
 * (DEODR_HIP_CHAMFER_GRID_ABI_VERSION).
 *
 * THE OPERATION is the one of include/deodr_hip_chamfer.h, word for word: the arrays, d2 operation by operation, the lowest index on a tie,
 * tau2 = max_distance * max_distance, the terms, the loss, vertices_b, the `directions` mask, NULL weights.  One precondition more and one
 * difference:
 *   - max_distance (params[2], device memory) must be FINITE.  The call cannot check it; deodr_amd/chamfer.py does.  The precondition is one
 *     on the values, not on safety: with an infinite or NaN max_distance h is infinite or NaN, every reference falls into one bucket, every
 *     index stays inside its array and the search walks all references -- slow and without the guarantees above, but nothing is read or
 *     written out of bounds.
 *   - a query whose brute-force nearest neighbour has d2 > tau2 reports DEODR_HIP_CHAMFER_GRID_NONE in nearest_vertex / nearest_point (such a
 *     pair contributes w tau2 and no gradient, as before).  For every other query nearest_* is EQUAL to deodr_hip_chamfer's, so the set of
 *     truncated pairs is equal too, and terms, loss and vertices_b are the same mathematical sums.
 * The order of the sums.  The terms: the order of deodr_hip_chamfer (the queries of a thread in increasing ORIGINAL index with the stride of the
 * grid, the lanes of a wavefront, the wavefronts, the workgroups).  The gradient of the points of vertex i: its points k_0 < k_1 < ... (the ones
 * with j*(k) = i and d2 <= tau2, in increasing k) are dealt to 64 lanes, lane l adds w_k (v_i - p_k) over k_l, k_(l+64), ... in that order, then
 * the 64 lane sums are added by the wavefront's fixed tree; that sum is doubled and scaled by mix_0, and the mesh -> points part is added to
 * it.  The order depends on the data alone (which points a vertex owns), never on timing: two calls give the same bits.
 *
 * THE GRID.  h = max(cell_size, max_distance / DEODR_HIP_CHAMFER_GRID_RINGS), formed on the device from params when the kernels run.  The cell
 * of a coordinate x is floor(x / h) clamped to [-DEODR_HIP_CHAMFER_GRID_CELL_LIMIT, DEODR_HIP_CHAMFER_GRID_CELL_LIMIT], per axis.  Cells are
 * addressed through a hash table of 2^table_bits buckets (deodr_hip_chamfer_grid_table_bits of the number of references); two cells in one bucket
 * only add candidates.  There is no bounding box.  A grid is built for the vertices when points -> mesh is on and for the points when mesh ->
 * points is on: bucket of every reference, deodr_hip_sort_keys, bucket bounds from adjacent sorted keys and the records (x, y, z, index) gathered
 * in sorted order.  A query expands ring by ring (Chebyshev distance in cells) around its own cell up to ring min(ceil(max_distance / h) + 1,
 * RINGS + 1) -- one ring more than the real-number bound, for the rounding of x / h -- and keeps the strict lexicographic minimum of (d2, index);
 * it stops after ring s >= 1 once its best d2 is < (h s (1 - 2^-20))^2, below which no reference outside the rings 0 .. s can be.
 *
 * CONTRACT: the one of include/deodr_hip_chamfer.h (double arithmetic without contraction, no floating-point atomics, launches and geometry a
 * function of (V, P, n, directions) alone, nothing read back: capturable, a replay follows every array and params as they are then; alignment;
 * the first kernel clears the arrival tickets, the scratch need not be zeroed).  Refused before any launch, with a message: V or P <= 0 or above
 * DEODR_HIP_CHAMFER_GRID_MAX_ITEMS, n outside 1 .. 65535, directions outside 1 .. 3, cell_size not finite or <= 0, a NULL pointer other than
 * point_weights, vertex_weights, nearest_vertex and nearest_point, a misaligned pointer, scratch_bytes below
 * deodr_hip_chamfer_grid_scratch_bytes, an output overlapping an input, the scratch or another output.  There is no cap on V * P.
 */
#ifndef DEODR_HIP_CHAMFER_GRID_H
#define DEODR_HIP_CHAMFER_GRID_H

#include "deodr_hip_chamfer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the stable sort by key.
 * n independent rows of N keys [n, N].  Only the low `bits` (1 .. 32) of a key take part.  order [n, N]: per row the permutation that sorts it,
 * order[i] = the index in the row of the i-th smallest key; equal keys keep increasing index (stable).  sorted_keys [n, N] (NULL: not wanted):
 * keys[order[i]], all 32 bits of them.  A least-significant-digit radix sort, DEODR_HIP_SORT_DIGIT_BITS bits per pass, ceil(bits / DIGIT_BITS)
 * passes of three launches each: the digit histogram of every workgroup (DEODR_HIP_SORT_ITEMS consecutive keys each, grid ceil(N / ITEMS) x n),
 * an exclusive scan over (digit, workgroup) in that order (one workgroup per row: thread d walks the workgroups of digit d in order), and a
 * scatter that ranks its keys stably inside the workgroup (DEODR_HIP_SORT_BLOCK keys at a time: wavefront ballots, then the wavefronts in
 * order).  No workgroup waits for another, no atomic decides a position, nothing is read back (capturable), the launches depend on (N, n, bits)
 * alone, the scratch need not be zeroed.  keys, sorted_keys, order and scratch must not overlap; all aligned to 4 bytes.
 * Refused with a message: N <= 0 or above DEODR_HIP_SORT_MAX_ITEMS, n outside 1 .. 65535, bits outside 1 .. 32, a NULL keys, order or scratch, a
 * misaligned pointer, a short scratch, overlapping buffers. */
#define DEODR_HIP_SORT_DIGIT_BITS 8
#define DEODR_HIP_SORT_BLOCK 256
#define DEODR_HIP_SORT_ITEMS 2048
#define DEODR_HIP_SORT_MAX_ITEMS 16777216
int deodr_hip_sort_keys(const uint32_t *keys, int N, int n, int bits, uint32_t *sorted_keys, uint32_t *order, void *scratch, size_t scratch_bytes,
						void *stream);
/* 4 n (4 N + 2^DIGIT_BITS ceil(N / ITEMS)) bytes: two buffers of keys and two of indices that the passes alternate between, and the histograms;
 * 0 for arguments the call refuses. */
size_t deodr_hip_sort_keys_scratch_bytes(int N, int n, int bits);
/* 3 ceil(bits / DIGIT_BITS); 0 for arguments the call refuses. */
int deodr_hip_sort_keys_launches(int N, int n, int bits);

/* ---- the closest-point energy over the grid */
#define DEODR_HIP_CHAMFER_GRID_NONE 4294967295
#ifndef DEODR_HIP_CHAMFER_GRID_RINGS /* (tools/chamfer_grid_times.py builds variants of the library to sweep these two) */
#define DEODR_HIP_CHAMFER_GRID_RINGS 4
#endif
#ifndef DEODR_HIP_CHAMFER_GRID_TABLE_LOAD
#define DEODR_HIP_CHAMFER_GRID_TABLE_LOAD 2
#endif
#define DEODR_HIP_CHAMFER_GRID_CELL_LIMIT 1073741824
#define DEODR_HIP_CHAMFER_GRID_MAX_ITEMS 16777216
#define DEODR_HIP_CHAMFER_GRID_MIN_TABLE_BITS 6
#define DEODR_HIP_CHAMFER_GRID_MAX_TABLE_BITS 25
/* a wavefront adds the points of a vertex: vertices per workgroup of the gather */
#define DEODR_HIP_CHAMFER_GRID_GATHER_VERTICES 4

/* The arrays are those of deodr_hip_chamfer; cell_size > 0, finite, on the host.  terms [n, 2], loss [n] and vertices_b [n, V, 3] are
 * overwritten; nearest_vertex [n, P] (with points -> mesh) and nearest_point [n, V] (with mesh -> points) unless NULL.
 * Launches, with sort(b) = deodr_hip_sort_keys_launches(.., b), tv = table_bits(V), tp = table_bits(P), bv = ceil(log2(V + 1)):
 *   points -> mesh: keys of the vertices (the first kernel of the call: it clears the tickets), sort(tv), build;
 *   mesh -> points: keys of the points (the first kernel when points -> mesh is off), sort(tp), build;
 *   points -> mesh: search of the points (in the sorted order of the points' own grid when it exists), the points' combine step (term_0, the
 *                   assignment), sort(bv) of the assignment, the gather (a wavefront per vertex);
 *   mesh -> points: search of the vertices (in the sorted order of the vertices' own grid when it exists);
 *   always: the vertices' combine step (vertices_b, term_1, loss). */
int deodr_hip_chamfer_grid(const double *vertices, int V, const double *points, int P, const double *point_weights, const double *vertex_weights,
						   const double *params, double cell_size, int n, int directions, double *terms, double *loss, double *vertices_b,
						   uint32_t *nearest_vertex, uint32_t *nearest_point, void *scratch, size_t scratch_bytes, void *stream);

/* Bytes of scratch, with M = DEODR_HIP_CHAMFER_MAX_BLOCKS, Tv = 2^table_bits(V), Tp = 2^table_bits(P) and S = the largest
 * deodr_hip_sort_keys_scratch_bytes of the three sorts: 64 + 8 n (8 V + 5 P + 2 M) + 4 n (7 P + 4 V + 2 Tv + 2 Tp + 2) + S; 0 for arguments
 * the call refuses. */
size_t deodr_hip_chamfer_grid_scratch_bytes(int V, int P, int n);

/* The number of kernel launches of a call (the list above); 0 for arguments the call refuses. */
int deodr_hip_chamfer_grid_launches(int V, int P, int n, int directions);

/* log2 of the number of buckets for `references` references: the smallest b with 2^b >= TABLE_LOAD references (2 of them), within MIN_TABLE_BITS .. MAX_TABLE_BITS;
 * 0 for references <= 0 or above MAX_ITEMS. */
int deodr_hip_chamfer_grid_table_bits(int references);

/* ABI version of this header; bumped on any incompatible change. */
int deodr_hip_chamfer_grid_abi_version(void);
#define DEODR_HIP_CHAMFER_GRID_ABI_VERSION 1

#ifdef __cplusplus
}
#endif
#endif /* DEODR_HIP_CHAMFER_GRID_H */
