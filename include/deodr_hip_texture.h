/* include/deodr_hip_texture.h -- companion header of include/deodr_hip.h: texture estimation on the device.
 *
 * Same library (libdeodr_hip.so), same conventions: device pointers, asynchronous on `stream` (hipStream_t as void*), no allocation, errors
 * returned (0 = ok) with the message in deodr_hip_last_error().  It is versioned on its own (DEODR_HIP_TEXTURE_ABI_VERSION) so that
 * deodr_hip.h stays what it is.
 *
 * The rasterizer delivers the gradient of the data term with respect to the texture (DeodrHipScene::texture_b, summed over the views); the
 * two calls below are what turns it into a texture fit that never leaves the device:
 *
 *     deodr_hip_render_scene_fit_ex (clear_gradients = 1)    texture_b  = d data / d texture
 *     deodr_hip_texture_smoothness                           texture_b += d smoothness / d texture,  energy[0] = smoothness
 *     deodr_hip_texture_step                                 texture, speed updated in place
 *
 * A texture is [Ht, Wt, C] contiguous in the pixel type (`pixel_dtype` = DEODR_HIP_F32 / DEODR_HIP_F64), as DeodrHipScene::texture; `speed` and
 * `gradient` have its shape and type.  Arithmetic is in double whatever the storage type, one rounding per stored value.  The pointers need the
 * alignment of one element only (a texture may be a slice of a larger buffer), and Wt * C need not be a multiple of anything.
 * Ht, Wt >= 2 (as the rasterizer asks), 1 <= C <= DEODR_HIP_MAX_COLORS, Ht * Wt * C <= 2^30.
 */
#ifndef DEODR_HIP_TEXTURE_H
#define DEODR_HIP_TEXTURE_H

#include "deodr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Smoothness of a texture, with a free boundary:
 *     E = 0.5 weight sum over channels c of [ sum_{x < Wt-1} (t[y,x+1,c] - t[y,x,c])^2 + sum_{y < Ht-1} (t[y+1,x,c] - t[y,x,c])^2 ]
 * energy[0] = E (double, device), deterministic: per-workgroup partials added in a fixed order by the last workgroup to arrive, bit-identical
 * from run to run.  dE/dt = weight (deg t - sum of the 2 .. 4 neighbours) is ACCUMULATED into `gradient` (pixel type), as the *_b arrays of the
 * rasterizer are; every texel is owned by one thread (no atomics).  `texture` is only read and must not overlap `gradient`.  Texels no view sees
 * have a zero data gradient: this term in-paints them.
 * scratch: device memory of deodr_hip_texture_scratch_bytes(Ht, Wt, C) bytes (0 for invalid dimensions), ZERO-FILLED ONCE by the caller (the
 * kernel leaves its counter word zero), used by one stream at a time. */
size_t deodr_hip_texture_scratch_bytes(int Ht, int Wt, int C);
int deodr_hip_texture_smoothness(const void *texture, int Ht, int Wt, int C, int pixel_dtype, double weight, void *gradient, double *energy, void *scratch,
								 size_t scratch_bytes, void *stream);

/* Momentum step of a pixel-typed array (deodr_hip_momentum_update takes double arrays only):
 *     s = (1 - damping) (inertia s + (1 - inertia) clamp(-factor g, +-step_max));   t = t + s          step_max <= 0: no clamp of the step
 * clamp != 0: t is then clipped to [clamp_lo, clamp_hi] and s is set to 0 where it clipped (the momentum does not keep pushing into the wall).
 * In place on `texture` and `speed`; `gradient` is only read (and not cleared: the next fit step does that, clear_gradients) and must not
 * overlap `texture`. */
int deodr_hip_texture_step(void *texture, void *speed, const void *gradient, int Ht, int Wt, int C, int pixel_dtype, double factor, double step_max,
						   double inertia, double damping, int clamp, double clamp_lo, double clamp_hi, void *stream);

/* ABI version of this header; bumped on any incompatible change. */
int deodr_hip_texture_abi_version(void);
#define DEODR_HIP_TEXTURE_ABI_VERSION 1

#ifdef __cplusplus
}
#endif
#endif /* DEODR_HIP_TEXTURE_H */
