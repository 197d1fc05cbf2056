/* include/deodr_hip_lighting.h -- companion header of include/deodr_hip.h: spherical-harmonic lighting (bands 0 - 2) and per-vertex albedo on the device.
 *
 * Same library (libdeodr_hip.so), same conventions: device pointers, asynchronous on `stream` (hipStream_t as void*), no allocation, no
 * synchronisation, errors returned (0 = ok) with the message in deodr_hip_last_error().  It is versioned on its own
 * (DEODR_HIP_LIGHTING_ABI_VERSION) so that deodr_hip.h and the other companion headers stay what they are.
 *
 * THE MODEL.  N = (x, y, z) is the vertex normal of deodr_hip_vertex_shade (deodr_hip.h), of the posed vertices of view b: sign times the sum of the
 * unit normals of the faces around the vertex, normalised; sign = -1 for clockwise meshes.  The nine real SH basis functions of bands 0 - 2:
 *     Y0 = c0      Y1 = c1 y    Y2 = c1 z    Y3 = c1 x
 *     Y4 = c2 x y  Y5 = c2 y z  Y6 = c3 (3 z^2 - 1)  Y7 = c2 x z  Y8 = c4 (x^2 - y^2)
 *     c0 = 1/(2 sqrt(pi))  c1 = sqrt(3)/(2 sqrt(pi))  c2 = sqrt(15)/(2 sqrt(pi))  c3 = sqrt(5)/(4 sqrt(pi))  c4 = sqrt(15)/(4 sqrt(pi))
 * sh is [9,S], S = 1 (monochrome light) or S = C.  The irradiance, NOT clamped (differentiable everywhere), and the colours:
 *     E[b,v,c] = sum_k sh[k, min(c, S-1)] Y_k(N[b,v])          colors[b,v,c] = albedo[v,c] E[b,v,c]
 * albedo is [C] (albedo_per_vertex = 0: one colour for the mesh) or [V,C] (albedo_per_vertex = 1).  Without an albedo (S = 1) the output is
 * luminosity[b,v] = E[b,v,0]: what the `shade` input of a textured mesh takes.
 * A vertex without faces, or whose accumulated normal is zero, behaves as in deodr_hip_vertex_shade (a division by zero; not handled).
 *
 * CONTRACT
 *   - posed [n,V,3], sh, albedo and every output are contiguous float64, 8-byte aligned; faces [T,3], vf_offsets [V+1], vf_corners [3T] are the
 *     uint32 arrays of deodr_hip_vertex_shade, 4-byte aligned.
 *   - Double arithmetic, no atomics on values: the order of every sum is fixed by (V, n) alone, so results are bit-identical from run to run and
 *     do not depend on which optional outputs are asked for.
 *   - Limits: 1 <= n <= 64, 1 <= V <= 2^24, 1 <= C <= 3, S = 1 or S = C.
 *   - Refused before any launch, with a message: a NULL among the required pointers, no output requested, albedo without colors / colors_b or the
 *     reverse, luminosity / luminosity_b with S != 1, a value out of range, a misaligned pointer, scratch_bytes below deodr_hip_sh_scratch_bytes,
 *     an output that overlaps an input (faces and vf_corners, whose length is not an argument, are tested with their first 12 bytes).
 */
#ifndef DEODR_HIP_LIGHTING_H
#define DEODR_HIP_LIGHTING_H

#include "deodr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One launch, grid (ceil(8 V / 256), n): eight adjacent lanes gather the faces around a vertex.  luminosity [n,V] or NULL (needs S = 1); colors [n,V,C] or
 * NULL (needs albedo); at least one of them. */
int deodr_hip_sh_shade(const double *posed, const uint32_t *faces, const uint32_t *vf_offsets, const uint32_t *vf_corners, const double *sh, int S,
					   const double *albedo, int albedo_per_vertex, int C, double *luminosity, double *colors, int V, int n, int clockwise, void *stream);

/* The adjoint.  luminosity_b [n,V] or NULL (needs S = 1), colors_b [n,V,C] or NULL (given exactly when albedo is); at least one of them.  Outputs,
 * each may be NULL but not all:
 *   posed_b [n,V,3]: always overwritten.
 *   sh_b [9,S]: the sums over views and vertices of E_b[b,v,c] Y_k (S = 1: E_b summed over the channels, luminosity_b added).
 *   albedo_b [C]: sums over views and vertices of colors_b E (albedo_per_vertex = 0); [V,C]: albedo_b[v,c] = sum_b colors_b[b,v,c] E[b,v,c], added in
 *     view order by one thread per element (albedo_per_vertex = 1).
 * accumulate != 0: added to what sh_b and albedo_b hold (a caller with more than 64 views calls once per slice).
 * Up to three launches: the per-(view, vertex) kernel on deodr_hip_sh_blocks(V, n) workgroups of 256 threads -- workgroup w takes the pairs
 * 32 (w + blocks i) + 0 .. 31 of the n V pairs (view-major), i = 0, 1, ..; the 9 S + C sums go threads -> lanes -> wavefronts -> workgroups as up
 * to three sums (12, 9, 9 values), each with its own counter word --; for a per-vertex albedo_b and n > 1 the sum over the views; for posed_b the
 * gather over the faces around each vertex that deodr_hip_vertex_shade_b runs.
 * scratch: device memory of deodr_hip_sh_scratch_bytes(V, n, C) bytes, 8-byte aligned, ZERO-FILLED ONCE by the caller (the kernels leave their
 * counter words zero), used by one stream at a time.
 * The scratch after the call (part of this ABI version): 64 bytes of counter words, then doubles -- [n,V,3] the adjoint of the un-normalised
 * accumulated normals, then, with albedo_per_vertex != 0 and n > 1, [n,V,C] the products colors_b E (written whether or not albedo_b is asked for:
 * albedo_b is their sum over the views, and a caller that sums over the views in a launch of its own -- deodr_hip_fit_pose_project_b's colors_sum --
 * passes albedo_b = NULL and saves this call's third launch). */
int deodr_hip_sh_shade_b(const double *posed, const uint32_t *faces, const uint32_t *vf_offsets, const uint32_t *vf_corners, const double *sh, int S,
						 const double *albedo, int albedo_per_vertex, int C, const double *luminosity_b, const double *colors_b, double *posed_b,
						 double *sh_b, double *albedo_b, int accumulate, void *scratch, size_t scratch_bytes, int V, int n, int clockwise, void *stream);

/* Bytes of scratch deodr_hip_sh_shade_b needs (64 bytes of counter words, then n V (3 + C) doubles and 30 per workgroup); 0 outside the limits above. */
size_t deodr_hip_sh_scratch_bytes(int V, int n, int C);

/* Workgroups of the per-(view, vertex) kernel of deodr_hip_sh_shade_b: ceil(n V / 32), at most 1024; non-decreasing in V and in n.  A pure host function;
 * 0 for arguments outside the limits above. */
int deodr_hip_sh_blocks(int V, int n);

/* ABI version of this header; bumped on any incompatible change. */
int deodr_hip_lighting_abi_version(void);
#define DEODR_HIP_LIGHTING_ABI_VERSION 1

#ifdef __cplusplus
}
#endif
#endif /* DEODR_HIP_LIGHTING_H */
