/* include/deodr_hip_pyramid.h -- companion header of include/deodr_hip.h: the multi-scale (pyramid) L2 data term on the device.
 *
 * Same library (libdeodr_hip.so), same conventions: device pointers, asynchronous on `stream` (hipStream_t as void*), no allocation, no
 * synchronisation, errors returned (0 = ok) with the message in deodr_hip_last_error().  It is versioned on its own
 * (DEODR_HIP_PYRAMID_ABI_VERSION) so that deodr_hip.h and the other companion headers stay what they are.
 *
 * THE TERM.  image, obs [n,H,W,C] in the pixel dtype, weights [n,H,W] in the pixel dtype (>= 0) or NULL (1 everywhere); levels = L coarse levels.
 * Level 0 is the frame, level l+1 has ceil(H_l / 2) x ceil(W_l / 2) cells, the children of cell (i, j) are the cells (2i .. 2i+1, 2j .. 2j+1) that
 * exist; a level that is 1 x 1 stays 1 x 1.  (A cell of level l is the aligned 2^l x 2^l block of pixels, clipped to the frame.)
 *     q_0 = w (image - obs)  per channel          w_0 = w
 *     q_{l+1}(cell) = sum of its children's q_l   w_{l+1}(cell) = sum of its children's w_l
 *     term_l = sum over cells and channels of q_l^2 / w_l        (a cell with w_l = 0 adds 0)
 *     loss   = sum over l = 0 .. L of level_weights[l] term_l
 * term_0 is sum w (image - obs)^2; term_l is sum over cells of w_l (weighted mean residual of the cell)^2; term_{l+1} <= term_l.
 * The adjoint, with iw_l = 1 / w_l (0 where w_l = 0) and lambda = level_weights:
 *     g_L = 2 lambda_L q_L iw_L      g_l = 2 lambda_l q_l iw_l + g_{l+1}(parent cell)      image_b = w g_0
 *
 * CONTRACT
 *   - All arithmetic is double whatever the pixel dtype; image_b is rounded once when it is stored.
 *   - No floating-point atomics: the order of every sum is fixed by (n, H, W, C, levels) alone.  Two calls give the same bits, and terms and loss do
 *     not depend on whether image_b is asked for.
 *   - level_weights [levels + 1] doubles in DEVICE memory, read by the kernels when they run: a captured graph that is replayed sees the values of the
 *     moment.  They are expected to be >= 0 (not checked: they are not on the host).
 *   - image, obs, weights, image_b aligned to their element, the double arrays and the scratch to 8 bytes.
 *   - Limits: 1 <= levels <= DEODR_HIP_PYRAMID_MAX_LEVELS, C >= 1, n, H, W >= 1, n H W C < 2^40.
 *   - Refused before any launch, with a message: image, obs, level_weights, terms or scratch == NULL, a value outside the limits, an unknown dtype
 *     tag, a misaligned pointer, scratch_bytes below deodr_hip_pyramid_scratch_bytes, an output that overlaps an input, the scratch or another output.
 */
#ifndef DEODR_HIP_PYRAMID_H
#define DEODR_HIP_PYRAMID_H

#include "deodr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DEODR_HIP_PYRAMID_MAX_LEVELS 8

/* terms [levels + 1]: the unweighted term_l.  loss (may be NULL): one double.  image_b (may be NULL) [n,H,W,C] in the pixel dtype, overwritten.
 * Launches: one wavefront per 8 x 8 tile of pixels reduces levels 0 .. 3 (and with levels <= 3 writes image_b in the same pass); with levels > 3 one
 * workgroup per 32 x 32 tiles does levels 4 .. L and their adjoint on the tile sums, and a third pass over the frame writes image_b.
 * scratch: device memory of deodr_hip_pyramid_scratch_bytes(n, H, W, C, levels) bytes, 8-byte aligned, used by one stream at a time.  It need NOT be
 * zeroed: a call clears the 64 bytes of counter words at its start (on the stream) and writes every other word before it reads it. */
int deodr_hip_pyramid_l2(const void *image, const void *obs, const void *weights, int n, int H, int W, int C, int pixel_dtype, int levels,
						 const double *level_weights, double *terms, double *loss, void *image_b, void *scratch, size_t scratch_bytes, void *stream);

/* Bytes of scratch deodr_hip_pyramid_l2 needs; 0 outside the limits above.  Monotone in every argument. */
size_t deodr_hip_pyramid_scratch_bytes(int n, int H, int W, int C, int levels);

/* ABI version of this header; bumped on any incompatible change. */
int deodr_hip_pyramid_abi_version(void);
#define DEODR_HIP_PYRAMID_ABI_VERSION 1

#ifdef __cplusplus
}
#endif
#endif /* DEODR_HIP_PYRAMID_H */
