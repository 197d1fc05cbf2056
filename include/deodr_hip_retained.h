/* include/deodr_hip_retained.h -- companion header of include/deodr_hip.h: the fit step of a loop that renders into the same buffers every time.
 *
 * Same library (libdeodr_hip.so), same conventions: device pointers, asynchronous on `stream` (hipStream_t as void*), no allocation, errors
 * returned (0 = ok) with the message in deodr_hip_last_error().  It is versioned on its own (DEODR_HIP_RETAINED_ABI_VERSION) so that
 * deodr_hip.h stays what it is.
 *
 * Two tiles out of three of a typical frame receive no primitive, and a fit step writes the background colour (or image) and depth = +inf
 * into them again at every iteration: half of the bytes the step moves.  In a fit loop the buffers already hold those values -- the
 * mesh moves by a fraction of a tile per iteration -- so a step that is TOLD that they do fills only the tiles that have just become empty.
 */
#ifndef DEODR_HIP_RETAINED_H
#define DEODR_HIP_RETAINED_H

#include "deodr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* deodr_hip_render_scene_fit_ex (`options` may be NULL: deodr_hip_render_scene_fit) with one more argument.  retained == 0: exactly that call.
 *
 * retained != 0 is the CALLER'S STATEMENT that
 *   (1) `image` and `z_buffer` still hold exactly what the previous forward launched with this workspace wrote into them (any entry point
 *       of the library that renders: deodr_hip_render_scene, a fit step, the forward inside deodr_hip_render_scene_b), and
 *   (2) the background (DeodrHipScene::background_color values, or the background_image) is what it was for that forward.
 * The step then writes background and depth = +inf only into the tiles that are empty now and held a primitive in that forward; every other
 * empty tile keeps what it has.  Image, depth buffer and gradients are those of the plain call.
 *
 * What the library verifies itself, on the device, before it believes the statement (otherwise every empty tile is filled, as with
 * retained == 0 -- a wrong or premature claim costs time, not a stale frame):
 *   - the workspace holds the tile bitmap of the previous forward: not a new (zero-filled) or regrown workspace, and not a forward of the
 *     un-staged kernel family (more than 4 channels, the deterministic mode, deodr_hip_force_generic), which keeps no bitmap;
 *   - that forward was given the same `image` and `z_buffer` addresses, both non-NULL, the same pixel type, the same n_views and the same height and width.
 * What it cannot verify, and the caller answers for: the CONTENTS of the two buffers (nothing else wrote them since -- not the caller, not
 * another workspace rendering into them) and the VALUES of the background.
 *
 * The statement is only used by a fit step whose background fill rides on its own kernels (a scene with triangles, at most 4 channels, not
 * deterministic); any other call ignores it.  Do not state it for a launch that is captured into a graph and replayed unless it holds at
 * every replay.  workspace_bytes is deodr_hip_workspace_bytes(), which includes the second bitmap. */
int deodr_hip_render_scene_fit_retained(const DeodrHipScene *scene, void *image, void *z_buffer, double sigma, const void *obs, int clear_gradients,
										const DeodrHipFitOptions *options, int retained, void *workspace, size_t workspace_bytes, void *stream);

/* ABI version of this header; bumped on any incompatible change. */
int deodr_hip_retained_abi_version(void);
#define DEODR_HIP_RETAINED_ABI_VERSION 1

#ifdef __cplusplus
}
#endif
#endif /* DEODR_HIP_RETAINED_H */
