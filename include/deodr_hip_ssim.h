/* include/deodr_hip_ssim.h -- companion header of include/deodr_hip.h: the structural (SSIM) data term on the device, mixed with the pixel term.
 *
 * Same library (libdeodr_hip.so), same conventions: device pointers, asynchronous on `stream` (hipStream_t as void*), no allocation, no
 * synchronisation, errors returned (0 = ok) with the message in deodr_hip_last_error().  It is versioned on its own
 * (DEODR_HIP_SSIM_ABI_VERSION) so that deodr_hip.h and the other companion headers stay what they are.
 *
 * THE TERM.  image = x, obs = y [n,H,W,C] in the pixel dtype, weights = w [n,H,W] in the pixel dtype (>= 0) or NULL (1 everywhere), data_range = R
 * > 0, mix = (alpha, beta).  G is the normalised separable Gaussian window of DEODR_HIP_SSIM_WINDOW = 11 taps per axis, g_k ~ exp(-k^2 / (2 1.5^2)),
 * k = -5 .. 5, sum g = 1 (evaluated in double), applied per view and per channel with ZERO PADDING: a window over the border of the frame sees
 * zeros in both images (the convention of conv2d(padding=5)).  With C1 = (0.01 R)^2, C2 = (0.03 R)^2:
 *     mx = G*x   my = G*y   sxx = G*x^2 - mx^2   syy = G*y^2 - my^2   sxy = G*xy - mx my
 *     SSIM = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sxx + syy + C2))                    per pixel and channel
 *     term_0 = sum w (x - y)^2       term_1 = sum w (1 - SSIM)       loss = alpha term_0 + beta term_1
 * The adjoint, with a1 = 2 mx my + C1, a2 = 2 sxy + C2, b1 = mx^2 + my^2 + C1, b2 = sxx + syy + C2:
 *     S_xy = 2 a1 / (b1 b2)     S_xx = -SSIM / b2     S_m = 2 my a2 / (b1 b2) - 2 mx SSIM / b1 - 2 mx S_xx - my S_xy
 *     A = -w S_m     B = -w S_xx     Cm = -w S_xy                                                  (three maps, per pixel and channel)
 *     image_b = 2 alpha w (x - y) + beta (G*A + 2 x (G*B) + y (G*Cm))                              (G is symmetric; zero padding again)
 * sxx, syy come out of a cancellation and are NOT clamped (b1 >= C1 > 0 always, b2 >= C2 > 0 mathematically).
 *
 * THE WEIGHTS multiply the SSIM MAP; they do not enter the windows.  A window next to a hole in the weights still sees the observation inside the
 * hole, and image_b is in general NOT 0 where w = 0 (the pixels within 5 of a weighted pixel get a gradient).  A caller who needs more dilates the
 * mask by 5 pixels.
 *
 * CONTRACT
 *   - All arithmetic is double whatever the pixel dtype; image_b is rounded once when it is stored.
 *   - No floating-point atomics: the order of every sum is fixed by (n, H, W, C) alone.  Two calls give the same bits, and terms and loss do not
 *     depend on whether image_b is asked for.
 *   - mix [2] doubles in DEVICE memory, read by the kernels when they run: a captured graph that is replayed sees the values of the moment.
 *   - image, obs, weights, image_b aligned to their element, the double arrays and the scratch to 8 bytes.
 *   - Limits: n, H, W, C >= 1, n H W C < 2^40; data_range finite and > 0.
 *   - Refused before any launch, with a message: image, obs, mix, terms or scratch == NULL, a value outside the limits, an unknown dtype tag, a
 *     misaligned pointer, scratch_bytes below deodr_hip_ssim_scratch_bytes, an output that overlaps an input, the scratch or another output.
 */
#ifndef DEODR_HIP_SSIM_H
#define DEODR_HIP_SSIM_H

#include "deodr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DEODR_HIP_SSIM_WINDOW 11

/* terms [2]: the unweighted term_0, term_1.  loss (may be NULL): one double.  image_b (may be NULL) [n,H,W,C] in the pixel dtype, overwritten.
 * Launches: one workgroup per 16 x 32 tile of pixels and view (the grid strides beyond 1024 workgroups), channel by channel: the tile and its halo
 * of 5 pixels to LDS, the window along the rows, then down the columns -> the two sums and, with image_b, the maps A, B, Cm in the scratch; a second
 * launch of the same tiling applies the window to the three maps and writes image_b.  With image_b == NULL: one launch, no maps written.
 * scratch: device memory of deodr_hip_ssim_scratch_bytes(n, H, W, C) bytes, 8-byte aligned, used by one stream at a time.  It need NOT be zeroed:
 * a call clears the 64 bytes of counter words at its start (on the stream) and writes every other word before it reads it. */
int deodr_hip_ssim_l2(const void *image, const void *obs, const void *weights, int n, int H, int W, int C, int pixel_dtype, double data_range,
					  const double *mix, double *terms, double *loss, void *image_b, void *scratch, size_t scratch_bytes, void *stream);

/* Bytes of scratch deodr_hip_ssim_l2 needs: 64 + 8 (2 * 1024 + 3 n H W C); 0 outside the limits above.  Monotone in every argument. */
size_t deodr_hip_ssim_scratch_bytes(int n, int H, int W, int C);

/* ABI version of this header; bumped on any incompatible change. */
int deodr_hip_ssim_abi_version(void);
#define DEODR_HIP_SSIM_ABI_VERSION 1

#ifdef __cplusplus
}
#endif
#endif /* DEODR_HIP_SSIM_H */
