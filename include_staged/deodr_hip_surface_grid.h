/* include_staged/deodr_hip_surface_grid.h -- STAGED companion header of include/deodr_hip.h (deodr_amd/_abi.py, STAGED: it moves into include/
 * with the next change of the table of companions): the point-to-surface distance of include/deodr_hip_surface.h with the closest face found over
 * a uniform grid of hashed cells holding the posed triangles instead of by brute force.  What deodr_amd/surface.py
 * (PointSurfaceTerm(search="grid")) and MeshPointCloudFitter(metric="surface", surface_search="grid") call.
 *
 * Same library (libdeodr_hip.so), same conventions: device pointers, asynchronous on `stream` (hipStream_t as void*), no allocation, no
 * synchronisation, errors returned (0 = ok) with the message in deodr_hip_last_error().  Versioned on its own
 * (DEODR_HIP_SURFACE_GRID_ABI_VERSION).
 *
 * THE OPERATION is the one of include/deodr_hip_surface.h, word for word: the arrays, d2(p, f) operation by operation, the LOWEST face index on a
 * tie, tau2 = max_distance * max_distance, the terms, the loss, vertices_b, the `directions` mask, NULL weights.  One precondition more and one
 * difference, as include/deodr_hip_chamfer_grid.h has them against include/deodr_hip_chamfer.h:
 *   - max_distance (params[2], device memory) must be FINITE.  The call cannot check it; deodr_amd/surface.py does.  The precondition is one on
 *     the values, not on safety: with an infinite or NaN max_distance the cell edge is infinite or NaN, every face falls into one bucket, every
 *     index stays inside its array and the search walks all faces -- slow and without the guarantees below, but nothing is read or written out
 *     of bounds.
 *   - a point whose brute-force closest face has d2 > tau2 reports DEODR_HIP_SURFACE_GRID_NONE in nearest_face and (0, 0, 0) in barycentric (it
 *     contributes w tau2 and no gradient, as before); a vertex whose nearest point is beyond tau2 reports it in nearest_point.  For every other
 *     point nearest_face is EQUAL to deodr_hip_surface_distance's and barycentric has its bits (the same closest-point text on the same record),
 *     so the set of truncated pairs is equal too, term_0, term_1 and loss have the brute-force operator's bits (the same combine steps over the
 *     same values in the same order), and vertices_b is the same mathematical sum in the order below.
 *
 * THE FACE GRID.  One record per face.  Per pose, E = the longest side of any face's axis-aligned bounding box (each side max - min, rounded
 * once), found on the device, and h_f = max(cell_size, max_distance / DEODR_HIP_CHAMFER_GRID_RINGS, E), formed when the kernels run: a replay
 * follows vertices that moved and a max_distance that changed.  The key of a face is the cell of the MINIMUM corner of its box -- floor(x / h_f)
 * per axis, clamped to +- DEODR_HIP_CHAMFER_GRID_CELL_LIMIT, the hash of include/deodr_hip_chamfer_grid.h, 2^table_bits(F) buckets
 * (deodr_hip_chamfer_grid_table_bits) -- so, its box being no longer than a cell, the face lies in the cells key .. key + 1 per axis up to the
 * rounding of the quotients.  Build: keys, deodr_hip_sort_keys, bucket bounds from adjacent sorted keys, the 128-byte records gathered in sorted
 * order with their original index: a bucket is a run of whole cache lines.  ONE VERY LONG TRIANGLE makes h_f large for the whole pose: everything
 * falls into a few heavy cells -- correct, and slow (DESIGN.md 4p has the measurement, 10 what would mend it).
 *
 * THE SEARCH.  A thread per point, in the sorted order of the points' own grid when mesh -> points builds one.  With c the point's cell, shell s
 * is the key cells of the box [c - s - 1, c + s] per axis that shell s - 1 did not hold (8 cells, then 56, 152, ...): the keys a face with a point
 * within s cells of the query can have.  Every record of every bucket goes through the closest-point sequence; the strict lexicographic minimum of
 * (d2, original face index) is kept -- neither the visiting order nor a bucket probed twice changes it.  The last shell is min(ceil(max_distance /
 * h_f) + 1, RINGS + 1) -- one more than the real-number bound, for the rounding of x / h_f --, and the search stops after shell s >= 1 once its
 * best d2 is < (h_f s (1 - 2^-20))^2, below which no face of an unvisited key can be (both statements with the rounding of x / h_f,
 * of E and of a box corner on a cell face, for coordinates up to 2^27 h_f in size).
 *
 * THE MESH -> POINTS SIDE is include/deodr_hip_chamfer_grid.h's, unchanged: the points' grid with ITS cell edge max(cell_size, max_distance /
 * RINGS) (the two grids do not share h), the ring search of the vertices (in index order), the same per-vertex step.
 *
 * THE ORDER OF THE SUMS.  The terms: the order of deodr_hip_surface_distance (the queries of a thread in increasing ORIGINAL index with the
 * stride of the grid, the lanes of a wavefront, the wavefronts, the workgroups).  G(f, c): the points of face f, k_0 < k_1 < ... (those with
 * f*(k) = f and d2 <= tau2, in increasing k: the assignment sorted stably on ceil(log2(F + 1)) bits, NONE last) are dealt to 64 lanes, lane l
 * adds its products over k_l, k_(l + 64), ... in that order, then the 64 lane sums are added by the wavefront's fixed tree.  vertices_b_i: the
 * corners of i in table order, one chain, scaled by mix_0, then the mesh -> points part added.  The order depends on the data alone (which points
 * a face owns), never on timing: two calls give the same bits.
 *
 * CONTRACT: the one of the two parents (double arithmetic without contraction, no floating-point atomics and no integer atomics on values,
 * launches and geometry a function of (V, F, P, n, directions) alone, nothing read back: capturable, a replay follows every array and params as
 * they are then; faces, corner_offsets, corners, nearest_face and nearest_point aligned to 4 bytes, everything else to 8; the first kernel
 * clears the arrival tickets (a kernel, not a memset node), the scratch need not be zeroed).  Refused before any launch, with a message: V, F or
 * P <= 0 or above DEODR_HIP_CHAMFER_GRID_MAX_ITEMS, n outside 1 .. 65535, directions outside 1 .. 3, cell_size not finite or <= 0, a NULL pointer
 * other than point_weights, vertex_weights, nearest_face, barycentric and nearest_point, a misaligned pointer, scratch_bytes below
 * deodr_hip_surface_grid_scratch_bytes, an output overlapping an input, the scratch or another output.  There is no cap on F * P and none on
 * V * P.  PRECONDITIONS the call cannot check: those of include/deodr_hip_surface.h, and the finite max_distance.
 */
#ifndef DEODR_HIP_SURFACE_GRID_H
#define DEODR_HIP_SURFACE_GRID_H

#include "../include/deodr_hip_chamfer_grid.h"
#include "../include/deodr_hip_surface.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DEODR_HIP_SURFACE_GRID_NONE 4294967295
/* a wavefront adds the points of a face: faces per workgroup of the gather */
#define DEODR_HIP_SURFACE_GRID_GATHER_FACES 4
/* (the rings, the cell limit and the largest set are DEODR_HIP_CHAMFER_GRID_RINGS, _CELL_LIMIT and _MAX_ITEMS) */

/* The arrays are those of deodr_hip_surface_distance; cell_size > 0, finite, on the host.  terms [n, 2], loss [n] and vertices_b [n, V, 3] are
 * overwritten; with points -> mesh nearest_face [n, P] (uint32) and barycentric [n, P, 3] unless NULL; with mesh -> points nearest_point [n, V]
 * (uint32) unless NULL.
 * Launches, with sort(b) = deodr_hip_sort_keys_launches(.., b), tf = table_bits(F), tp = table_bits(P), bf = ceil(log2(F + 1)):
 *   points -> mesh: the prep kernel (the first kernel of the call: it clears the tickets; the records; the longest box side per workgroup), the
 *                   keys of the faces (every workgroup takes the maximum of those sides: E, h_f), sort(tf), build;
 *   mesh -> points: keys of the points (the first kernel when points -> mesh is off), sort(tp), build;
 *   points -> mesh: search of the points, the points' combine step (nearest_face, barycentric, term_0, the assignment), sort(bf) of the
 *                   assignment, the gather (a wavefront per face);
 *   mesh -> points: search of the vertices;
 *   always: the vertices' combine step (vertices_b, nearest_point, term_1, loss). */
int deodr_hip_surface_grid(const double *vertices, int V, const int32_t *faces, int F, const int32_t *corner_offsets, const int32_t *corners,
						   const double *points, int P, const double *point_weights, const double *vertex_weights, const double *params, double cell_size,
						   int n, int directions, double *terms, double *loss, double *vertices_b, uint32_t *nearest_face, double *barycentric,
						   uint32_t *nearest_point, void *scratch, size_t scratch_bytes, void *stream);

/* Bytes of scratch, with M = DEODR_HIP_CHAMFER_MAX_BLOCKS, Tf = 2^table_bits(F), Tp = 2^table_bits(P) and S =
 * deodr_hip_sort_keys_scratch_bytes(max(F, P), n, 32): 64 + 8 n (41 F + 11 P + V + 3 M + 1) + 4 n (3 F + 7 P + V + 2 Tf + 2 Tp + 2) + S; 0 for
 * arguments the call refuses. */
size_t deodr_hip_surface_grid_scratch_bytes(int V, int F, int P, int n);

/* The number of kernel launches of a call (the list above): 1, plus 6 + sort(tf) + sort(bf) with points -> mesh, plus 3 + sort(tp) with mesh ->
 * points; 0 for arguments the call refuses. */
int deodr_hip_surface_grid_launches(int V, int F, int P, int n, int directions);

/* ABI version of this header; bumped on any incompatible change. */
int deodr_hip_surface_grid_abi_version(void);
#define DEODR_HIP_SURFACE_GRID_ABI_VERSION 1

#ifdef __cplusplus
}
#endif
#endif /* DEODR_HIP_SURFACE_GRID_H */
