/* include/deodr_hip_chamfer.h -- companion header of include/deodr_hip.h: the closest-point (ICP / Chamfer) energy between the vertices of a mesh and
 * an unorganised 3-D point set, with its gradient to the vertices and the correspondences.  What deodr_amd/chamfer.py (PointCloudTerm) and
 * MeshPointCloudFitter fit a mesh to a scan with.
 *
 * Same library (libdeodr_hip.so), same conventions: device pointers, asynchronous on `stream` (hipStream_t as void*), no allocation, no
 * synchronisation, errors returned (0 = ok) with the message in deodr_hip_last_error().  It is versioned on its own
 * (DEODR_HIP_CHAMFER_ABI_VERSION) so that deodr_hip.h and the other companion headers stay what they are.
 *
 * THE OPERATION.  All arrays contiguous doubles: vertices [n, V, 3], points [n, P, 3], point_weights [n, P] >= 0 (NULL: ones), vertex_weights [V]
 * >= 0, shared by the poses (NULL: ones), params [3] IN DEVICE MEMORY = (mix_0, mix_1, max_distance), max_distance > 0 (+inf allowed), read when
 * the kernels run; n >= 1 independent poses.  Per pose, p_k the points, v_i the vertices, w_k / u_i the weights:
 *     d2(a, b)   = ((a.x-b.x)*(a.x-b.x) + (a.y-b.y)*(a.y-b.y)) + (a.z-b.z)*(a.z-b.z)      (each operation rounded, no contraction)
 *     j*(k)      = the lowest j that minimises d2(p_k, v_j)                               (nearest vertex of point k)
 *     k*(i)      = the lowest k that minimises d2(v_i, p_k)                               (nearest point of vertex i)
 *     tau2       = max_distance * max_distance
 *     term_0     = sum_k w_k min(d2(p_k, v_j*(k)), tau2)                                  (points -> mesh)
 *     term_1     = sum_i u_i min(d2(v_i, p_k*(i)), tau2)                                  (mesh -> points)
 *     loss       = mix_0 term_0 + mix_1 term_1
 *     vertices_b_i = mix_0 * sum over k with j*(k) = i and d2 <= tau2, in increasing k, of 2 w_k (v_i - p_k)
 *                  + mix_1 * [d2 <= tau2] 2 u_i (v_i - p_k*(i))
 * The nearest neighbour is chosen on the unweighted, untruncated d2.  A pair beyond max_distance contributes the constant w tau2 and no gradient
 * (the truncated ICP rule).  vertices_b is the exact gradient of loss wherever every nearest neighbour is unique and no pair sits at exactly
 * max_distance.  A point that is bit-equal to its nearest vertex has d2 == 0 and contributes exactly 0 to vertices_b.
 *
 * `directions`, a bit mask on the host: DEODR_HIP_CHAMFER_POINTS_TO_MESH, DEODR_HIP_CHAMFER_MESH_TO_POINTS, or both (3).  A direction that is off
 * is not computed: its term is written as 0, it adds nothing to loss and vertices_b, and its nearest_* array is not written.
 *
 * THE SEARCH IS BRUTE FORCE: every (point, vertex) pair is visited, once per direction that is on -- V * P distance evaluations per pose and
 * direction, no grid, no tree.  V * P is therefore capped (DEODR_HIP_CHAMFER_MAX_PAIRS).
 *
 * CONTRACT
 *   - All arithmetic is double, without contraction.  No floating-point atomics.  Comparison is strict < with the references visited in increasing
 *     index, so the lowest index wins a tie.  Every sum is in an order fixed by (V, P, n, directions) alone -- the gradient of the points of a
 *     vertex: increasing k within a segment of the points, then the segments in order (deodr_hip_chamfer_segments); the terms: the queries of a
 *     thread in order, the lanes of a wavefront, the wavefronts, the workgroups --, so two calls give the same bits.
 *   - The number of launches and their geometry depend on (V, P, n, directions) alone -- deodr_hip_chamfer_launches, deodr_hip_chamfer_segments --,
 *     nothing is read back: the call can be captured into a graph, and a replay follows vertices, points, the weights and params as they are at
 *     that moment.
 *   - nearest_vertex and nearest_point aligned to 4 bytes, everything else to 8.
 *   - Refused before any launch, with a message: V <= 0 or P <= 0, n outside 1 .. 65535 (the poses are the third dimension of the grid), directions
 *     outside 1 .. 3, V * P above DEODR_HIP_CHAMFER_MAX_PAIRS, a NULL pointer other than point_weights, vertex_weights, nearest_vertex and
 *     nearest_point, a misaligned pointer, scratch_bytes below deodr_hip_chamfer_scratch_bytes, an output overlapping an input, the scratch or
 *     another output.
 *   - PRECONDITIONS the call cannot check (device memory): params as above, the weights >= 0, finite coordinates.  deodr_amd/chamfer.py checks
 *     them on the host.
 */
#ifndef DEODR_HIP_CHAMFER_H
#define DEODR_HIP_CHAMFER_H

#include "deodr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the bits of `directions` */
#define DEODR_HIP_CHAMFER_POINTS_TO_MESH 1
#define DEODR_HIP_CHAMFER_MESH_TO_POINTS 2

/* The launch geometry.  BLOCK: threads of a workgroup of the searches, a query per thread, and of the combine steps.  TILE: references staged in
 * LDS at a time (every lane reads the same address: a broadcast).  MAX_BLOCKS: workgroups per pose of the combine steps at most (the threads
 * stride beyond).  TARGET_BLOCKS / MAX_SEGMENTS: the split rule below. */
#define DEODR_HIP_CHAMFER_BLOCK 256
#define DEODR_HIP_CHAMFER_TILE 256
#define DEODR_HIP_CHAMFER_MAX_BLOCKS 512
#define DEODR_HIP_CHAMFER_TARGET_BLOCKS 1024
#define DEODR_HIP_CHAMFER_MAX_SEGMENTS 64

/* The cap on V * P, per pose.  One search launch visits n * V * P pairs.  Measured on an MI355X at the largest size of tools/chamfer_times.py,
 * V * P = 10 002 * 40 000 = 4.0e8: both directions take 454 us at n = 1, 0.57 ps per pair and direction, and 2 425 us at n = 8,
 * 0.38 ps, where the device is full.  2^36 = 6.9e10 pairs are then 26 ms to 39 ms per pose and launch: a launch of 8 poses at the cap stays near
 * 0.2 s, well under a second (a caller with many more poses at the cap splits them over calls). */
#define DEODR_HIP_CHAMFER_MAX_PAIRS 68719476736

/* terms [n, 2], loss [n] and vertices_b [n, V, 3] are overwritten; nearest_vertex [n, P] (with points -> mesh) and nearest_point [n, V] (with
 * mesh -> points) unless NULL.
 * scratch: device memory of deodr_hip_chamfer_scratch_bytes(V, P, n) bytes, 8-byte aligned, used by one stream at a time.  It need NOT be zeroed:
 * the first kernel clears the arrival tickets (a kernel, not a memset node), and every other word is written before it is read.
 * Launches: with points -> mesh the point-major search (grid: ceil(P / BLOCK) x segments(P, V) x n) and its combine step (nearest vertex, term_0);
 * then always the vertex-major walk (grid: ceil(V / BLOCK) x segments(V, P) x n: the search for the nearest point with mesh -> points, and in the
 * same walk the gather of w_k (v_i - p_k) over the points whose nearest vertex is i with points -> mesh) and its combine step (vertices_b, term_1,
 * loss). */
int deodr_hip_chamfer(const double *vertices, int V, const double *points, int P, const double *point_weights, const double *vertex_weights,
					  const double *params, int n, int directions, double *terms, double *loss, double *vertices_b, uint32_t *nearest_vertex,
					  uint32_t *nearest_point, void *scratch, size_t scratch_bytes, void *stream);

/* Bytes of scratch deodr_hip_chamfer needs, with Sp = segments(P, V), Sv = segments(V, P), M = DEODR_HIP_CHAMFER_MAX_BLOCKS:
 * 64 + 8 (n (Sp P + 4 Sv V + 2 M) + ceil(n (Sp P + Sv V + P + 2) / 2)); 0 for arguments the call refuses. */
size_t deodr_hip_chamfer_scratch_bytes(int V, int P, int n);

/* The number of kernel launches of a call: 4 with points -> mesh (directions 1 and 3), 2 with mesh -> points alone; 0 for arguments the call refuses. */
int deodr_hip_chamfer_launches(int V, int P, int n, int directions);

/* The split rule: into how many contiguous parts the `references` are cut for a search of `queries` queries, so that few queries against many
 * references still fill the device: min(tiles, DEODR_HIP_CHAMFER_MAX_SEGMENTS, ceil(DEODR_HIP_CHAMFER_TARGET_BLOCKS / ceil(queries / BLOCK))) with
 * tiles = ceil(references / TILE); part s holds the tiles [s tiles / S, (s + 1) tiles / S) (integer division), never none.  Non-increasing in
 * queries, non-decreasing in references; 0 for queries <= 0 or references <= 0. */
int deodr_hip_chamfer_segments(int queries, int references);

/* ABI version of this header; bumped on any incompatible change. */
int deodr_hip_chamfer_abi_version(void);
#define DEODR_HIP_CHAMFER_ABI_VERSION 1

#ifdef __cplusplus
}
#endif
#endif /* DEODR_HIP_CHAMFER_H */
