/* include/deodr_hip_surface.h -- companion header of include/deodr_hip.h: the point-to-SURFACE distance between an unorganised 3-D point set and the
 * triangles of a mesh (the closest point of the closest triangle, not the closest vertex), with its gradient to the vertices and the
 * correspondences.  What deodr_amd/surface.py (PointSurfaceTerm) and MeshPointCloudFitter(metric="surface") fit a mesh to a dense scan with.
 *
 * Same library (libdeodr_hip.so), same conventions: device pointers, asynchronous on `stream` (hipStream_t as void*), no allocation, no
 * synchronisation, nothing read back, errors returned (0 = ok) with the message in deodr_hip_last_error().  It is versioned on its own
 * (DEODR_HIP_SURFACE_ABI_VERSION) so that deodr_hip.h and the other companion headers stay what they are.  The bits of `directions`, the launch
 * geometry constants (BLOCK, TILE, MAX_BLOCKS) and THE SPLIT RULE are those of include/deodr_hip_chamfer.h: deodr_hip_chamfer_segments(queries,
 * references) cuts every search and gather of this header too (a tile is 256 face records here, 256 points there), so no rule is exported here.
 *
 * THE INPUTS.  Contiguous; doubles unless said: vertices [n, V, 3]; faces [F, 3] int32, shared by the poses, values in [0, V); the static
 * transposed table corner_offsets [V + 1] and corners [3 F], int32: for vertex i the entries 3 f + c with faces[f][c] == i, in increasing order,
 * at corners[corner_offsets[i] .. corner_offsets[i + 1]) (deodr_amd.surface.corner_table builds and checks it on the host); points [n, P, 3];
 * point_weights [n, P] >= 0 (NULL: ones); vertex_weights [V] >= 0 (NULL: ones); params [3] IN DEVICE MEMORY = (mix_0, mix_1, max_distance),
 * max_distance > 0 (+inf allowed), read when the kernels run; n >= 1 independent poses.
 *
 * THE OPERATION, operation by operation, each one rounded to double, no contraction (the library is built with -ffp-contract=off).  A dot product
 * is (x.x * y.x + x.y * y.y) + x.z * y.z.  For a point p and the triangle (a, b, c) = the posed vertices of faces[f]:
 *     ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c
 *     d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp, d5 = ab.cp, d6 = ac.cp
 *     vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4
 *     e_ab = d1 - d3, e_ac = d2 - d6, e_b = d4 - d3, e_c = d5 - d6, e_bc = e_b + e_c, den = (va + vb) + vc
 * and the FIRST region that holds, in Ericson's order, gives (v, w):
 *     A        d1 <= 0 and d2 <= 0                                  v = 0, w = 0
 *     B        d3 >= 0 and d4 <= d3                                 v = 1, w = 0
 *     AB       vc <= 0 and d1 >= 0 and d3 <= 0 and e_ab > 0         v = d1 / e_ab, w = 0
 *     C        d6 >= 0 and d5 <= d6                                 v = 0, w = 1
 *     AC       vb <= 0 and d2 >= 0 and d6 <= 0 and e_ac > 0         v = 0, w = d2 / e_ac
 *     BC       va <= 0 and e_b >= 0 and e_c >= 0 and e_bc > 0       w = e_b / e_bc, v = 1 - w
 *     interior otherwise                                            v = vb / den, w = vc / den; v = w = 0 where den == 0
 * An edge region is taken only where its denominator is STRICTLY positive: with that and the select on den no NaN arises from finite input, and
 * a triangle of zero area (two or three equal corners, three collinear ones) gives the distance to the segment or point it is.  Then
 *     q        = (a + v ab) + w ac                  per component: (a.x + v * ab.x) + w * ac.x
 *     bary     = (1 - v - w, v, w)                  (1 - v) - w
 *     e        = q - p,  d2(p, f) = (e.x e.x + e.y e.y) + e.z e.z
 *     f*(k)    = the LOWEST face index that minimises d2(p_k, f)     (strict <, faces visited in increasing index)
 *     tau2     = max_distance * max_distance
 *     term_0   = sum_k w_k min(d2(p_k, f*(k)), tau2)                                       (points -> mesh)
 *     term_1   = sum_i u_i min(d2(v_i, p_k*(i)), tau2)      EXACTLY the mesh -> points side of include/deodr_hip_chamfer.h: vertex to nearest
 *                point, the lowest k of the minimum, run by the same kernel
 *     loss     = mix_0 term_0 + mix_1 term_1
 *     vertices_b_i = mix_0 * sum over (f, c) in corners(i), in table order, of G(f, c)
 *                  + mix_1 * [d2 <= tau2] 2 u_i (v_i - p_k*(i))
 *     G(f, c)  = sum over k with f*(k) = f and d2 <= tau2, in increasing k, of ((2 w_k) * bary_c) * e_k      (the envelope theorem: corner c of
 *                the face of the closest point receives bary_c times the pull 2 w_k (q_k - p_k))
 * The nearest face is chosen on the unweighted, untruncated d2.  A pair beyond max_distance contributes the constant w tau2 and no gradient.  A
 * point that is bit-equal to its closest point has e == 0 and contributes exactly 0.  vertices_b is the exact gradient of loss wherever every
 * closest face's closest point is unique and no pair sits at exactly max_distance.
 *
 * TIES ARE THE GENERIC CASE HERE, not a corner case: the closest point of a point outside a convex part of a mesh is often a vertex or lies on
 * an edge, and every face around that vertex or edge then has the same closest point -- on a 396-face convex mesh 37 % of the outside points had
 * two faces with bit-identical d2 (a shared vertex) and another 2.5 % two within 2 ulp (a shared edge reached through two corner orders).  The
 * lowest-index rule together with the operation-by-operation definition above is what makes nearest_face (and with it barycentric and the
 * distribution of the gradient over the corners) reproducible: an implementation that rounds one product differently picks other faces.
 *
 * `directions`: DEODR_HIP_CHAMFER_POINTS_TO_MESH (1), DEODR_HIP_CHAMFER_MESH_TO_POINTS (2), or both (3).  A direction that is off is not
 * computed: its term is written as 0, it adds nothing to loss and vertices_b, and its nearest_* / barycentric arrays are not written.
 *
 * THE SEARCH IS BRUTE FORCE: every (point, face) pair is visited with points -> mesh, every (vertex, point) pair with mesh -> points; no grid, no
 * tree, no culling.  F * P is therefore capped (DEODR_HIP_SURFACE_MAX_PAIRS), and V * P by DEODR_HIP_CHAMFER_MAX_PAIRS with mesh -> points.
 *
 * CONTRACT
 *   - All arithmetic is double, without contraction.  No floating-point atomics.  Every sum is in an order fixed by (V, F, P, n, directions)
 *     alone -- G(f, c): increasing k within a segment of the points; vertices_b_i: the corners of i in table order and, per corner, the segments
 *     in order (deodr_hip_chamfer_segments(F, P)), one chain; the terms: the queries of a thread in order, the lanes of a wavefront, the
 *     wavefronts, the workgroups --, so two calls give the same bits.
 *   - The number of launches and their geometry depend on (V, F, P, n, directions) alone -- deodr_hip_surface_distance_launches --, nothing is
 *     read back: the call can be captured into a graph, and a replay follows vertices, points, the weights and params as they are at that moment
 *     (faces and the corner table too, but they are static by their meaning).
 *   - faces, corner_offsets, corners, nearest_face and nearest_point aligned to 4 bytes, everything else to 8.
 *   - Refused before any launch, with a message: V <= 0, F <= 0 or P <= 0, F above 715 827 882 (3 F is an int32), n outside 1 .. 65535,
 *     directions outside 1 .. 3, F * P above DEODR_HIP_SURFACE_MAX_PAIRS, V * P above DEODR_HIP_CHAMFER_MAX_PAIRS when mesh -> points is on, a
 *     NULL pointer other than point_weights, vertex_weights, nearest_face, barycentric and nearest_point, a misaligned pointer, scratch_bytes
 *     below deodr_hip_surface_distance_scratch_bytes, an output overlapping an input, the scratch or another output.
 *   - PRECONDITIONS the call cannot check (device memory): the values of faces in [0, V), the corner table as defined above, params as above, the
 *     weights >= 0, finite coordinates.  deodr_amd/surface.py checks them on the host.
 */
#ifndef DEODR_HIP_SURFACE_H
#define DEODR_HIP_SURFACE_H

#include "deodr_hip_chamfer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The cap on F * P, per pose.  The point-major search visits n * F * P pairs in one launch.  Measured on an MI355X at the largest size of
 * tools/surface_times.py, F * P = 20 000 * 40 000 = 8.0e8: points -> mesh alone takes 4 850 us at n = 1, 6.1 ps per pair, and
 * 28 375 us at n = 8, 4.4 ps per pair, where the device is full.  2^32 = 4.3e9 pairs are then 19 ms to 26 ms per pose and launch: a launch of 8
 * poses at the cap stays near 0.2 s (a caller with many more poses at the cap splits them over calls). */
#define DEODR_HIP_SURFACE_MAX_PAIRS 4294967296

/* terms [n, 2], loss [n] and vertices_b [n, V, 3] are overwritten; with points -> mesh nearest_face [n, P] (uint32) and barycentric [n, P, 3]
 * unless NULL; with mesh -> points nearest_point [n, V] (uint32) unless NULL.
 * scratch: device memory of deodr_hip_surface_distance_scratch_bytes(V, F, P, n) bytes, 8-byte aligned, used by one stream at a time.  It need
 * NOT be zeroed: the first kernel clears the arrival tickets (a kernel, not a memset node), and every other word is written before it is read.
 * Launches, with BLOCK = DEODR_HIP_CHAMFER_BLOCK and segments = deodr_hip_chamfer_segments: with points -> mesh (1) the prep kernel (tickets; one
 * record a, b, c, ab, ac per pose and face), (2) the point-major search (grid: ceil(P / BLOCK) x segments(P, F) x n), (3) its combine step
 * (nearest_face, barycentric, term_0), (4) the face-major gather of G (grid: ceil(F / BLOCK) x segments(F, P) x n); with mesh -> points the
 * vertex-major search of include/deodr_hip_chamfer.h (grid: ceil(V / BLOCK) x segments(V, P) x n); then always the per-vertex combine step
 * (vertices_b, nearest_point, term_1, loss). */
int deodr_hip_surface_distance(const double *vertices, int V, const int32_t *faces, int F, const int32_t *corner_offsets, const int32_t *corners,
							   const double *points, int P, const double *point_weights, const double *vertex_weights, const double *params, int n,
							   int directions, double *terms, double *loss, double *vertices_b, uint32_t *nearest_face, double *barycentric,
							   uint32_t *nearest_point, void *scratch, size_t scratch_bytes, void *stream);

/* Bytes of scratch deodr_hip_surface_distance needs, with Sp = segments(P, F), Sg = segments(F, P), Sv = segments(V, P),
 * M = DEODR_HIP_CHAMFER_MAX_BLOCKS: 64 + 8 (n (16 F + Sp P + 6 P + 9 Sg F + Sv V + 2 M) + ceil(n (Sp P + Sv V + P + 2) / 2)); 0 for arguments
 * the call refuses whatever the directions (the cap on V * P is not among them). */
size_t deodr_hip_surface_distance_scratch_bytes(int V, int F, int P, int n);

/* The number of kernel launches of a call: 5 with points -> mesh alone, 6 with both directions, 2 with mesh -> points alone; 0 for arguments the
 * call refuses. */
int deodr_hip_surface_distance_launches(int V, int F, int P, int n, int directions);

/* ABI version of this header; bumped on any incompatible change. */
int deodr_hip_surface_abi_version(void);
#define DEODR_HIP_SURFACE_ABI_VERSION 1

#ifdef __cplusplus
}
#endif
#endif /* DEODR_HIP_SURFACE_H */
