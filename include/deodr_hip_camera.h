/* include/deodr_hip_camera.h -- companion header of include/deodr_hip.h: the camera as a differentiable input (calibration) on the device.
 *
 * Same library (libdeodr_hip.so), same conventions: device pointers, asynchronous on `stream` (hipStream_t as void*), no allocation, no
 * synchronisation, errors returned (0 = ok) with the message in deodr_hip_last_error().  It is versioned on its own
 * (DEODR_HIP_CAMERA_ABI_VERSION) so that deodr_hip.h and the other companion headers stay what they are.
 *
 * deodr_hip_project_points (deodr_hip.h) maps points [n,V,3] through the n cameras (extrinsic [n,3,4], intrinsic [n,3,3], distortion [n,5] =
 * (k1, k2, p1, p2, k3) or NULL) to image coordinates ij [n,V,2] and depths [n,V]:
 *     c = E (p, 1);  (x, y) = c.xy / c.z;  r2 = x^2 + y^2;  radial = 1 + k1 r2 + k2 r2^2 + k3 r2^3
 *     x_d = x radial + 2 p1 x y + p2 (r2 + 2 x^2);  y_d = y radial + p1 (r2 + 2 y^2) + 2 p2 x y        (x_d, y_d) = (x, y) without distortion
 *     ij = K[:2,:2] (x_d, y_d) + K[:2,2];  depth = c.z
 * deodr_hip_project_points_b gives the adjoint of the points only.  Here is the adjoint of everything, and the map from the parameters a
 * calibration moves (a quaternion and a translation per view; focal lengths, principal point and distortion) to those matrices, with its adjoint.
 *
 * CONTRACT
 *   - All arrays are contiguous float64; every pointer is 8-byte aligned.
 *   - Double arithmetic, no atomics on values: the order of every sum is fixed by (V, n) alone, so results are bit-identical from run to run and
 *     do not depend on which optional outputs are asked for.
 *   - Limits: 1 <= n <= 64, 1 <= V <= 2^24.
 *   - Refused before any launch, with a message: a NULL among the required pointers, distortion given without distortion_b or the reverse, each
 *     range above, a misaligned pointer, scratch_bytes below deodr_hip_camera_scratch_bytes, an output that overlaps an input.
 */
#ifndef DEODR_HIP_CAMERA_H
#define DEODR_HIP_CAMERA_H

#include "deodr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The full adjoint of deodr_hip_project_points.  ij_b [n,V,2]; depths_b [n,V] or NULL (zero).
 *   points_b [n,V,3] or NULL: exactly what deodr_hip_project_points_b writes (the same bits).
 *   extrinsic_b [n,3,4]: per view the 12 sums over the vertices of c_b (x) (p, 1), c_b the adjoint of the camera-space point.
 *   intrinsic_b [n,3,3]: rows 0 and 1 the sums of ij_b (x) (x_d, y_d, 1); row 2 is written as zero.
 *   distortion_b [n,5]: the sums of the adjoints of (k1, k2, p1, p2, k3); required exactly when `distortion` is given.
 * accumulate != 0: added to what extrinsic_b, intrinsic_b and distortion_b hold (points_b is always written).
 * A view is cut into deodr_hip_camera_blocks(V, n) workgroups of 256 threads; thread t of workgroup w takes the vertices
 * 256 w + t + 256 blocks i, i = 0, 1, ..; the 23 sums of a view go threads -> lanes -> wavefronts -> workgroups in an order fixed by (V, n)
 * (the 12 of the extrinsic and the other 11 as two sums, each with its own counter word).
 * scratch: device memory of deodr_hip_camera_scratch_bytes(V, n) bytes, 8-byte aligned, ZERO-FILLED ONCE by the caller (the kernel leaves its
 * counter words zero), used by one stream at a time. */
int deodr_hip_camera_project_b(const double *points, const double *extrinsic, const double *intrinsic, const double *distortion, const double *ij_b,
							   const double *depths_b, double *points_b, double *extrinsic_b, double *intrinsic_b, double *distortion_b, int V, int n,
							   int accumulate, void *scratch, size_t scratch_bytes, void *stream);

/* Workgroups per view of deodr_hip_camera_project_b: one for small meshes, enough to fill the chip for large V n, capped; non-decreasing in V.
 * A pure host function; 0 for arguments outside the limits above. */
int deodr_hip_camera_blocks(int V, int n);

/* Bytes of scratch deodr_hip_camera_project_b needs (two counter words per view, then 23 doubles per workgroup); 0 outside the limits above. */
size_t deodr_hip_camera_scratch_bytes(int V, int n);

/* The per-view matrices from the parameters of a calibration.  quaternions [n,4] = (x, y, z, w), normalised here; translations [n,3]:
 *     extrinsic[b] = [R(q_b / |q_b|) | t_b], R p + t = qrot(q, p) + t of deodr_hip_rigid_transform
 *     intrinsic[b] = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]
 *     distortion_out[b] = distortion_in
 * shared != 0: focal [2] = (fx, fy), center [2] = (cx, cy) and distortion_in [5] are one physical camera used by all n views; otherwise they are
 * [n,2], [n,2], [n,5].  distortion_in and distortion_out are both given or both NULL.  Outputs must not overlap inputs. */
int deodr_hip_camera_assemble(const double *quaternions, const double *translations, const double *focal, const double *center,
							  const double *distortion_in, int shared, double *extrinsic, double *intrinsic, double *distortion_out, int n, void *stream);

/* The adjoint of deodr_hip_camera_assemble (all outputs written).  quaternions_b [n,4] is with respect to the RAW quaternions (through the
 * normalisation), translations_b [n,3]; focal_b, center_b, distortion_in_b have the shapes of their parameters; the skew and lower-row entries of
 * intrinsic_b are dropped.  shared != 0: the intrinsic and distortion adjoints are summed over the views in view order by one thread.
 * distortion_b and distortion_in_b are both given or both NULL.  Outputs must not overlap inputs. */
int deodr_hip_camera_assemble_b(const double *quaternions, const double *extrinsic_b, const double *intrinsic_b, const double *distortion_b, int shared,
								double *quaternions_b, double *translations_b, double *focal_b, double *center_b, double *distortion_in_b, int n,
								void *stream);

/* ABI version of this header; bumped on any incompatible change. */
int deodr_hip_camera_abi_version(void);
#define DEODR_HIP_CAMERA_ABI_VERSION 1

#ifdef __cplusplus
}
#endif
#endif /* DEODR_HIP_CAMERA_H */
