// deodr_amd/csrc/dr_kernels.hip -- the translation unit of libdeodr_hip.so: HIP kernels (gfx950 / CDNA4, wave64; in the
// headers listed after the kernels below) + the host side and the C ABI (this file).
//
// Kernels (n_views views per launch; DESIGN.md section 4 has the why of every choice below):
//
//   setup_bin_kernel        blocks of 256 threads on a 1-D grid, the edge blocks first: 256 edge slots compacted to the flagged
//                           ones, or one triangle per thread.  Cull, depth sum, stencil + attribute planes in double and in
//                           registers (dr_prims.h), edge records (+ the EdgeFin record finalize reads), the index checks of
//                           checkSceneValid, binning into 8 x 8 tiles (all slot requests of a 3 x 3 block of tiles in flight; a
//                           thread bins the first block of its primitive, the other blocks of all primitives of a wavefront
//                           are dealt out evenly over its lanes), optional gradient clearing
//   tile_scan_kernel        one thread per tile: counters -> work list of the NON-EMPTY tiles (entries carry the first triangle
//                           ids; many-primitive tiles first), tile bitmap, three lists of edge tiles by edge count, sweep slots
//   raster_fwd_fast_kernel  1 wavefront / work-list entry, lane = pixel.  Pass 1 (z-buffered triangles staged 16 at a time
//                           through LDS, exact scanline spans, winner = min (Z, index)), shading of the winner, pass 2 (ordered
//                           edge overdraw) fused in registers, ONE write of image / z (/ owner) per pixel.  FUSED
//                           (deodr_hip_render_scene_fit): also the adjoint for the sum-of-squares residual of EVERY tile (tiles with
//                           silhouette edges: reverse sweep + pass 1 by a second instance of the walker on the head of the work
//                           list; untextured scenes: pairs of adjacent edge-free tiles share a wavefront; textured scenes, round 5:
//                           instances of their own at three waves per SIMD, from 8 views per launch on as two kernels on two
//                           streams -- the head walkers / everybody else)
//   fill_kernel / fill_word background + depth = inf of the empty tiles, runs of tiles written as contiguous 16-byte pieces:
//                           a kernel on a forked stream (forward-only calls) or extra workgroups of the forward raster and of
//                           finalize, dealt 2 : 1 (fit step)
//   raster_bwd_fast_kernel  (two-call path) adjoint of pass 1 in every non-empty tile without edges
//   raster_bwd_edge_kernel  (two-call path) persistent waves over the listed edge tiles: adjoint of pass 2 (un-blend in reverse order, moments
//                           by a transposing butterfly, one 15-lane atomic per edge and tile), then of pass 1
//   finalize_kernel         per primitive: moments -> plane adjoints -> 3x3-inverse adjoint -> vertex gradients
//   raster_fwd_kernel / raster_bwd_kernel   the same algorithm without LDS staging: nb_colors > 4, antialiase_error
//   dr_fronthalf.h, dr_fititer.h   the O(V) kernels either side of the rasterizer in a fit iteration (pose + projection, shading,
//                           silhouette flags, their adjoints, rigid energy, data terms, momentum update): deterministic sums
//
// Where: dr_dispatch.h (host only: which template instance of a kernel a call runs, the tables of the instances) . dr_workspace.h (layout, KParams,
// wave primitives) . dr_setup.h (setup_bin_kernel) . dr_forward.h (tile_scan_kernel, fill,
// raster_fwd_fast_kernel) . dr_backward.h (raster_bwd_fast_kernel, raster_bwd_edge_kernel) . dr_finalize.h (finalize_kernel) .
// dr_forward_generic.h / dr_backward_generic.h (the un-staged family, edge ordering) . dr_math.h / dr_prims.h (per-primitive math) .
// dr_fronthalf.h / dr_fititer.h (fit iteration) . dr_host.h (host only: what the entry points ask of their arguments -- element size of a dtype tag,
// overlap of two buffers, capped grids -- and the layout of the scratch buffers).
//
// No MFMA anywhere: the path is gather / scatter + streaming writes.  The workspace is self-cleaning (tile counters are
// zeroed by the scan kernel, spill counters are double-buffered by the parity of the forward count, list counters are zeroed
// by set-up, the moment accumulators by finalize) so a call never needs a memset node.  Every global atomic of the path is
// executed at the memory side on this part (TCC_EA0_ATOMIC == TCC_ATOMIC): their number, not their addresses, is what counts.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <type_traits>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../../include/deodr_hip.h"
#include "dr_dispatch.h"
#include "dr_host.h"
#include "../../include/deodr_hip_texture.h"
#include "../../include/deodr_hip_subdiv.h"
#include "../../include/deodr_hip_retained.h"
#include "../../include/deodr_hip_basis.h"
#include "../../include/deodr_hip_camera.h"
#include "../../include/deodr_hip_lighting.h"
#include "../../include/deodr_hip_skinning.h"
#include "../../include/deodr_hip_pyramid.h"
#include "../../include/deodr_hip_ssim.h"
#include "../../include/deodr_hip_solve.h"
#include "../../include/deodr_hip_arap.h"
#include "../../include/deodr_hip_chamfer.h"
#include "../../include/deodr_hip_surface.h"
#include "../../include/deodr_hip_chamfer_grid.h"
#include "../../include_staged/deodr_hip_surface_grid.h"
#include "dr_fititer.h" // <- dr_finalize.h <- dr_backward.h <- dr_backward_generic.h <- dr_forward.h <- dr_forward_generic.h <- dr_setup.h <- dr_workspace.h <- dr_prims.h
#include "dr_texfit.h"  // texture smoothness + step (include/deodr_hip_texture.h); uses grid_sum of dr_fronthalf.h
#include "dr_subdiv.h"  // rows of a sparse matrix applied to [batch, n, D] blocks (include/deodr_hip_subdiv.h): Loop subdivision and its adjoint
#include "dr_basis.h"   // a dense [K, N] basis applied to coefficient vectors, and its adjoint (include/deodr_hip_basis.h): morphable models
#include "dr_camera.h"  // the camera as a differentiable input: full adjoint of the projection, calibration parameters <-> matrices (include/deodr_hip_camera.h)
#include "dr_lighting.h" // spherical-harmonic lighting and per-vertex albedo beside vertex_shade_* of dr_fititer.h (include/deodr_hip_lighting.h)
#include "dr_skinning.h" // linear blend skinning: joint chain, blend of the influences of a vertex, their adjoints (include/deodr_hip_skinning.h)
#include "dr_pyramid.h"	 // the multi-scale L2 data term and its adjoint: levels 0 .. 3 per 8 x 8 tile, the levels above on the tile grid (include/deodr_hip_pyramid.h)
#include "dr_ssim.h"	 // the structural (SSIM) data term and its adjoint: two stencil kernels over 16 x 32 tiles with a halo in LDS (include/deodr_hip_ssim.h)
#include "dr_solve.h"	 // sparse SPD solve by conjugate gradients: one workgroup per column for small systems, two launches per step above (include/deodr_hip_solve.h)
#include "dr_arap.h"	 // as-rigid-as-possible energy: a 3 x 3 polar decomposition per vertex by Jacobi on Horn's matrix, then the gradient (include/deodr_hip_arap.h)
#include "dr_chamfer.h" // closest-point (Chamfer) energy: a brute-force tiled nearest-neighbour search both ways, the gradient gathered in the same walk (include/deodr_hip_chamfer.h)
#include "dr_surface.h" // point-to-surface distance: the closest point of the closest triangle by a brute-force tiled search over face records, on the machinery of dr_chamfer.h (include/deodr_hip_surface.h)
#include "dr_sort.h"	// a stable LSD radix sort by key: histograms, a scan over (digit, workgroup), a scatter ranked by ballots (include/deodr_hip_chamfer_grid.h)
#include "dr_chamfer_grid.h" // the closest-point energy over a uniform grid of hashed cells: keys, sort, build, ring search, gather; the combine steps of dr_chamfer.h (include/deodr_hip_chamfer_grid.h)
#include "dr_surface_grid.h" // point-to-surface distance over a uniform grid of triangles: one record per face keyed by its box's minimum corner, shell search, gather (include_staged/deodr_hip_surface_grid.h)

using namespace dr;
using namespace dr::dispatch;
using namespace dr::host;

namespace
{

// ------------------------------------------------------------------------------------------------------ host side

thread_local char g_error[256] = "";

int fail(const char *msg)
{
	snprintf(g_error, sizeof g_error, "%s", msg);
	return 1;
}

int fail(const char *what, const char *why) // "what: why"
{
	snprintf(g_error, sizeof g_error, "%s: %s", what, why);
	return 1;
}

int check_hip(hipError_t e, const char *what)
{
	if (e == hipSuccess)
		return 0;
	snprintf(g_error, sizeof g_error, "%s: %s", what, hipGetErrorString(e));
	return 1;
}

int fill_params(const DeodrHipScene *sc, double sigma, void *workspace, size_t workspace_bytes, KParams &p, bool backward)
{
	if (!sc)
		return fail("scene == NULL");
	// the checks of checkSceneValid (H.h:2664-2715) that do not need to read device memory
	if (!sc->faces || !sc->faces_uv || !sc->depths || !sc->uv || !sc->ij || !sc->shade || !sc->colors || !sc->edgeflags || !sc->textured ||
		!sc->shaded)
		return fail("scene array == NULL");
	if ((sc->background_image == nullptr) == (sc->background_color == nullptr))
		return fail("exactly one of scene.background_image / scene.background_color must be given");
	if (sc->nb_triangles < 0 || sc->nb_vertices <= 0 || sc->nb_uv <= 0 || sc->height <= 0 || sc->width <= 0 || sc->n_views <= 0)
		return fail("invalid scene dimensions");
	if (sc->nb_colors <= 0 || sc->nb_colors > DEODR_HIP_MAX_COLORS)
		return fail("nb_colors out of range");
	if (sc->nb_triangles >= (1 << 30))
		return fail("more than 2^30 triangles");
	if (sc->height > 32767 || sc->width > 32767)
		return fail("image larger than 32767 pixels (pixel coordinates are 16-bit, as in the reference)");
	if (!elem_bytes(sc->vertex_dtype) || !elem_bytes(sc->pixel_dtype))
		return fail("unknown dtype tag");
	if (sc->texture && (sc->texture_height < 2 || sc->texture_width < 2))
		return fail("texture must be at least 2 x 2");
	if (backward)
	{
		if (!sc->backface_culling)
			return fail("You have to use backface_culling true if you ant to compute gradients"); // H.h:2924
		if (sc->perspective_correct)
			return fail("backward gradient propagation not supported yet with perspective_correct=True"); // H.h:810
		if (!sc->uv_b || !sc->ij_b || !sc->shade_b || !sc->colors_b)
			return fail("scene gradient array == NULL");
		if (sc->texture && !sc->texture_b)
			return fail("scene.texture_b == NULL although scene.texture is given"); // H.h:2694
	}
	if (!workspace)
		return fail("workspace == NULL");
	memset(&p, 0, sizeof p);
	{ // the spill-pool capacity is implied by the workspace size: the largest pool_pairs whose layout fits
		const size_t per_view = workspace_bytes / (size_t)sc->n_views;
		if (make_layout(sc->nb_triangles, sc->height, sc->width, sc->nb_colors, 1).view_bytes > per_view)
			return fail("workspace too small (see deodr_hip_workspace_bytes)");
		size_t lo = 1, hi = 0x7fffffffu;
		while (lo < hi)
		{
			size_t mid = lo + (hi - lo + 1) / 2;
			if (make_layout(sc->nb_triangles, sc->height, sc->width, sc->nb_colors, mid).view_bytes <= per_view)
				lo = mid;
			else
				hi = mid - 1;
		}
		p.L = make_layout(sc->nb_triangles, sc->height, sc->width, sc->nb_colors, lo);
	}
	p.faces = sc->faces;
	p.faces_uv = sc->faces_uv;
	p.textured = sc->textured;
	p.shaded = sc->shaded;
	p.edgeflags = sc->edgeflags;
	p.depths = sc->depths;
	p.ij = sc->ij;
	p.shade = sc->shade;
	p.colors = sc->colors;
	p.uv = sc->uv;
	p.texture = sc->texture;
	p.bg_image = sc->background_image;
	p.bg_color = sc->background_color;
	p.uv_b = sc->uv_b;
	p.ij_b = sc->ij_b;
	p.shade_b = sc->shade_b;
	p.colors_b = sc->colors_b;
	p.texture_b = sc->texture_b;
	p.T = sc->nb_triangles;
	p.V = sc->nb_vertices;
	p.Vuv = sc->nb_uv;
	p.H = sc->height;
	p.W = sc->width;
	p.C = sc->nb_colors;
	p.tex_h = sc->texture_height;
	p.tex_w = sc->texture_width;
	p.clockwise = sc->clockwise != 0;
	p.culling = sc->backface_culling != 0;
	p.strict = sc->strict_edge != 0;
	p.persp = sc->perspective_correct != 0;
	p.vtx_f64 = sc->vertex_dtype == DEODR_HIP_F64;
	p.pix_f64 = sc->pixel_dtype == DEODR_HIP_F64;
	p.offset = sc->integer_pixel_centers ? 0.0 : 0.5;
	p.sigma = sigma;
	p.ws = (char *)workspace;
	p.row_group = ROW_GROUP;
	// (see KParams::prim_tables; measured on the 20 k-triangle benchmark scene: 1 view loses 1.7 us to the tables, 8 views gain 6)
	constexpr long long PRIM_TABLES_MIN = 40000;
	p.prim_tables = (long long)sc->n_views * sc->nb_triangles >= PRIM_TABLES_MIN;
	return 0;
}

// ---- optional per-kernel timing (bench.py's roofline leg): hipEvents recorded on the launch stream around each kernel
enum KernelId
{
	KID_SETUP = 0,
	KID_RASTER_FWD = 1,
	KID_RASTER_BWD = 2,
	KID_FINALIZE = 3,
	KID_COUNT = 4
};
struct ProfEvent
{
	hipEvent_t start, stop;
	int kid;
};
bool g_profile = false;	  // the launches of the current call are bracketed by events
int g_profile_every = 0;	  // deodr_hip_profile_enable(n): 0 off, n > 0: every n-th forward (and the adjoint that follows it)
unsigned g_profile_calls = 0; // forwards seen since profiling was enabled
unsigned long long *g_stamps = nullptr; // deodr_hip_profile_stamps: device buffer of g_stamp_rows x 4 words, one row per forward
int g_stamp_rows = 0;
unsigned g_stamp_calls = 0;
bool g_force_generic = false; // deodr_hip_force_generic(1): run the un-staged kernels (the parity suite covers both families)
bool g_det = false;			  // deodr_hip_set_deterministic(1): un-staged kernels + integer accumulation (KParams::det) for EVERY scene
inline bool det_mode(const DeodrHipScene *sc) { return g_det || sc->deterministic != 0; } // (DeodrHipScene::deterministic: for this scene)

// int64 shadows of the gradient arrays in the deterministic mode: one library-owned buffer per (device, stream), grown on demand (the only
// allocation the library ever makes, and only in this mode: a test mode), zero between calls (det_convert clears what it reads).  Per
// STREAM: calls on one stream are ordered, so they may share the shadows; two fit steps on two streams (or threads) of one device each
// get their own -- with one buffer per device their sums mixed.  Never freed (a handful of streams per process).
struct DetScratch
{
	int dev = -1;
	hipStream_t stream = nullptr;
	long long *ptr = nullptr;
	size_t words = 0;
};
std::mutex g_det_mutex;
std::vector<DetScratch> g_det_scratch;
int det_shadows(KParams &p, int n_views, hipStream_t st)
{
	const size_t n_ij = (size_t)n_views * p.V * 2, n_col = (size_t)n_views * p.V * p.C, n_sh = (size_t)n_views * p.V, n_uv = (size_t)p.Vuv * 2,
				 n_tex = p.texture_b ? (size_t)p.tex_h * p.tex_w * p.C : 0, need = n_ij + n_col + n_sh + n_uv + n_tex;
	int dev = 0;
	if (check_hip(hipGetDevice(&dev), "hipGetDevice"))
		return 1;
	std::lock_guard<std::mutex> lock(g_det_mutex);
	size_t at = 0;
	while (at < g_det_scratch.size() && !(g_det_scratch[at].dev == dev && g_det_scratch[at].stream == st))
		at++;
	if (at == g_det_scratch.size())
	{
		g_det_scratch.emplace_back();
		g_det_scratch[at].dev = dev, g_det_scratch[at].stream = st;
	}
	DetScratch &sc = g_det_scratch[at];
	if (sc.words < need)
	{
		hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
		(void)hipStreamIsCapturing(st, &cap);
		if (cap != hipStreamCaptureStatusNone)
			return fail("deterministic mode: the shadow buffer has to grow, which cannot happen under stream capture (run the step once before capturing)");
		if (check_hip(hipDeviceSynchronize(), "deterministic mode: synchronise"))
			return 1;
		if (sc.ptr)
			(void)hipFree(sc.ptr);
		sc.ptr = nullptr, sc.words = 0;
		if (check_hip(hipMalloc((void **)&sc.ptr, 8 * need), "deterministic mode: shadow buffer") || check_hip(hipMemset(sc.ptr, 0, 8 * need), "deterministic mode: clear"))
			return 1;
		sc.words = need;
	}
	p.det = 1;
	p.det_err = &((WsHeader *)(p.ws + p.L.hdr))->scene_errors; // (view 0: what deodr_hip_workspace_status reads; det_convert copies it to the polled word)
	hipLaunchKernelGGL(det_status_kernel, dim3(1), dim3(1), 0, st, (WsHeader *)(p.ws + p.L.hdr), 1); // (the range bit of the PREVIOUS deterministic adjoint goes)
	p.det_ij = sc.ptr;
	p.det_colors = p.det_ij + n_ij;
	p.det_shade = p.det_colors + n_col;
	p.det_uv = p.det_shade + n_sh;
	p.det_texture = n_tex ? p.det_uv + n_uv : nullptr;
	return 0;
}
void det_convert(const KParams &p, int n_views, hipStream_t st)
{
	const size_t n_ij = (size_t)n_views * p.V * 2, n_col = (size_t)n_views * p.V * p.C, n_sh = (size_t)n_views * p.V, n_uv = (size_t)p.Vuv * 2,
				 n_tex = p.det_texture ? (size_t)p.tex_h * p.tex_w * p.C : 0;
	auto run = [&](long long *shadow, void *out, size_t n, int f64) {
		if (n && out)
			hipLaunchKernelGGL(det_convert_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, shadow, out, n, f64);
		else if (n && shadow) // (an array the caller did not ask for: whatever the kernels added to its shadow must not reach the next call)
			(void)hipMemsetAsync(shadow, 0, 8 * n, st);
	};
	run(p.det_ij, p.ij_b, n_ij, p.vtx_f64);
	run(p.det_colors, p.colors_b, n_col, p.vtx_f64);
	run(p.det_shade, p.shade_b, n_sh, p.vtx_f64);
	run(p.det_uv, p.uv_b, n_uv, p.vtx_f64);
	run(p.det_texture, p.texture_b, n_tex, p.pix_f64);
	hipLaunchKernelGGL(det_status_kernel, dim3(1), dim3(1), 0, st, (WsHeader *)(p.ws + p.L.hdr), 0);
}
// Tuning constants (measured in round 1, profiles/README.md); deliberately NOT read from the environment: nothing outside the
// arguments of a call may change what the call launches.
constexpr int EDGE_WAVES = 1024; // persistent waves per view of the adjoint's edge kernel

// ---- which instance of a kernel a call runs: the rule and the tables of dr_dispatch.h; here the tables become kernels
static_assert(STAGED_CHANNELS == CH && TWO_KERNEL_VIEWS == TEX_TWO_KERNELS && WALKER_UNIT == 8 * WORK_CHUNK, "dr_dispatch.h restates the kernels' constants");

// Runs launch(std::integral_constant<size_t, i>{}) for the entry i of `table` that equals `want`.  The tables are the only place that names an
// instance: a generic lambda turns entry i into template arguments (and so instantiates every entry).  An instance the table does not hold (or that
// launch refuses: returns false) is the error `no_instance`, never a fall into some default.
template <size_t I = 0, class Inst, size_t N, class Launch>
int launch_from(const char *no_instance, const Inst (&table)[N], const Inst &want, Launch launch)
{
	if constexpr (I < N)
		return table[I] == want && launch(std::integral_constant<size_t, I>{}) ? 0 : launch_from<I + 1>(no_instance, table, want, launch);
	return fail(no_instance);
}

// The pixel-dtype tag as a type: f(double{}) or f(float{}) for a generic lambda.
template <class F>
auto with_pixel_type(bool f64, F f) { return f64 ? f(double{}) : f(float{}); }

// A dtype tag of the ABI (one that elem_bytes knows: the entry points check first) as a type, for the operators whose arrays each carry a tag of their
// own.  (with_pixel_type is not a call of this: the order of the two branches is the order of the kernels in the code object, float first here.)
static_assert(elem_bytes(DEODR_HIP_F32) == sizeof(float) && elem_bytes(DEODR_HIP_F64) == sizeof(double), "dr_host.h restates the dtype tags");
template <class F>
auto with_dtype(int tag, F f) { return tag == DEODR_HIP_F32 ? f(float{}) : f(double{}); }

// One of two template arguments: f(std::integral_constant<int, A>{}), or with B when `second`.
template <int A, int B, class F>
auto with_constant(bool second, F f) { return !second ? f(std::integral_constant<int, A>{}) : f(std::integral_constant<int, B>{}); }

template <class PixT>
int launch_adjoint_raster(const KParams &p, bool fast, bool owner_tiles, dim3 grid4, dim3 edge_grid, hipStream_t st)
{
	if (!fast)
	{
		if (fit_weights(p)) // (a weighted fit step on the un-staged kernels: more than CH channels, the deterministic mode)
			hipLaunchKernelGGL(raster_bwd_weighted_kernel<PixT>, grid4, dim3(256), 0, st, p);
		else
			hipLaunchKernelGGL(raster_bwd_kernel<PixT>, grid4, dim3(256), 0, st, p);
		return 0;
	}
	constexpr bool f64 = sizeof(PixT) == 8;
	// raster_bwd_edge_kernel (edge: std::true_type) or raster_bwd_fast_kernel, the instance for this scene
	auto launch = [&](auto edge, dim3 grid, const KParams &args) {
		return launch_from("internal: no instance of the adjoint raster kernels for this call", BWD_INSTANCES, select_adjoint_raster(f64, p.texture != nullptr, p.C), [&](auto i) {
			constexpr BwdInst k = BWD_INSTANCES[decltype(i)::value];
			if constexpr (bwd_exists(k, f64) && decltype(edge)::value)
				hipLaunchKernelGGL((raster_bwd_edge_kernel<PixT, k.tex, k.nc>), grid, dim3(64), 0, st, args);
			else if constexpr (bwd_exists(k, f64))
				hipLaunchKernelGGL((raster_bwd_fast_kernel<PixT, k.tex, k.nc>), grid, dim3(64), 0, st, args);
			return bwd_exists(k, f64);
		});
	};
	if (owner_tiles) // (after a fused forward the tiles without edges have already been back-propagated)
	{
		KParams q = p;
		q.tile_blocks = fwd_tile_blocks(p.L.ntiles, p.n_views, false); // the grid of the forward that built the work list (never a fused one)
		q.heavy_share = heavy_share_for(p.n_views, q.tile_blocks, false);
		q.split_part = 16; // (no fit step here: nothing is split)
		if (launch(std::false_type{}, dim3((unsigned)p.n_views * (unsigned)q.tile_blocks), q))
			return 1;
	}
	// (running the two kernels side by side on a forked stream was measured: no gain, the edge kernel just stretches)
	if (p.sigma > 0 && p.aa_err)
	{ // antialiase_error: the sweep ran over the error buffer, and so does its adjoint (bwd_err_tile, dr_backward.h)
		const dim3 grid(edge_grid.x, edge_grid.y);
		if (p.texture != nullptr)
			hipLaunchKernelGGL((raster_bwd_edge_err_kernel<PixT, true>), grid, dim3(64), 0, st, p);
		else
			hipLaunchKernelGGL((raster_bwd_edge_err_kernel<PixT, false>), grid, dim3(64), 0, st, p);
	}
	else if (p.sigma > 0 && !p.fuse_edges) // (a fit step back-propagates the tiles with edges inside its forward raster)
		return launch(std::true_type{}, edge_grid, p);
	return 0;
}

std::vector<ProfEvent> g_prof_events;
std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_free;

struct ScopedKernelTimer
{
	hipStream_t stream;
	ProfEvent ev;
	bool on;
	ScopedKernelTimer(int kid, hipStream_t st) : stream(st), on(g_profile)
	{
		if (!on)
			return;
		if (g_prof_free.empty())
		{
			(void)hipEventCreate(&ev.start);
			(void)hipEventCreate(&ev.stop);
		}
		else
		{
			ev.start = g_prof_free.back().first;
			ev.stop = g_prof_free.back().second;
			g_prof_free.pop_back();
		}
		ev.kid = kid;
		(void)hipEventRecord(ev.start, stream);
	}
	~ScopedKernelTimer()
	{
		if (!on)
			return;
		(void)hipEventRecord(ev.stop, stream);
		g_prof_events.push_back(ev);
	}
};

// The side stream the background fill runs on (one per device, created at first use), with the two events that fork it from
// and join it back to the caller's stream.  Re-recording an event does not disturb a wait already enqueued on its previous
// record, so one pair serves every call; the mutex keeps the record / wait pairs of concurrent host threads together.  Under
// stream capture the fork / join become edges of the captured graph.
struct SideStream
{
	hipStream_t stream = nullptr;
	hipEvent_t fork = nullptr, join = nullptr;
};
std::mutex g_side_mutex;
std::vector<SideStream> g_side;

int side_stream(SideStream &out)
{
	int dev = 0;
	if (check_hip(hipGetDevice(&dev), "hipGetDevice"))
		return 1;
	if ((size_t)dev >= g_side.size())
		g_side.resize(dev + 1);
	SideStream &ss = g_side[dev];
	if (!ss.stream)
	{
		if (check_hip(hipStreamCreateWithFlags(&ss.stream, hipStreamNonBlocking), "side stream") ||
			check_hip(hipEventCreateWithFlags(&ss.fork, hipEventDisableTiming), "side event") ||
			check_hip(hipEventCreateWithFlags(&ss.join, hipEventDisableTiming), "side event"))
			return 1;
	}
	out = ss;
	return 0;
}

// KParams::fwd_* / views_magic: what every workgroup of the staged forward would otherwise derive for itself (tile_blocks, heavy_share, fill_mode,
// n_views are set).  Only the staged forward reads them: the adjoint's launches do not call this.
void forward_launch_constants(KParams &q)
{
	const bool chunked = q.tile_blocks % (8 * WORK_CHUNK) == 0;
	q.fwd_heads = chunked ? (uint32_t)(q.tile_blocks / q.heavy_share) : 0u;
	q.fwd_walkers = (uint32_t)q.tile_blocks;
	const uint32_t n_walk = (uint32_t)q.n_views * q.fwd_walkers;
	q.fwd_n_fill = (uint32_t)q.n_views * (uint32_t)fill_units(q.retained, q.fill_mode, 2, q.L.nwords);
	q.fwd_dealt = (q.fuse_edges && n_walk >= 8 * q.fwd_n_fill) ? q.fwd_n_fill / 8 : 0u;
	q.views_magic = q.n_views == 1 ? 0xffffffffu : (uint32_t)(0x100000000ull / (unsigned long long)q.n_views) + 1u; // (see div_views)
}

constexpr long long SPARSE_MAX = 16384; // triangles (all views) up to which the per-primitive kernels spread their work over more wavefronts (KParams::setup_sparse)
// KParams::setup_sparse and the workgroups of a per-primitive kernel over all views: the edge blocks (one edge slot per thread in a small launch) + the
// triangle blocks (set-up: `spread_triangles`, a small launch gives every triangle setup_sparse threads; finalize: one thread per triangle)
unsigned prim_grid(KParams &p, int n_views, bool spread_triangles)
{
	p.setup_sparse = (long long)p.T * n_views <= SPARSE_MAX ? 4 : 1;
	return (unsigned)(prim_tri_blocks(spread_triangles ? p.T * p.setup_sparse : p.T) + prim_edge_blocks(p.T, p.setup_sparse > 1 ? 1 : EDGE_SLOTS)) * (unsigned)n_views;
}

// Which family of kernels a call runs.  The staged one (LDS staging, work lists) for up to CH channels, unless the un-staged one is forced or the
// deterministic mode is on: this is the test of the adjoint and of the fused fit step ...
bool staged_adjoint(const DeodrHipScene *sc, const KParams &p) { return p.C <= CH && !g_force_generic && !det_mode(sc); }
// ... and a forward on its own is also staged with more than CH channels (the second operand of ||) when the frame has no silhouette edge and no texture
// and nothing is fused -- Scene3D.render_deferred's frame, sigma = 0 -- through fwd_manyc_tile (the adjoint has no such path).  antialiase_error: staged
// since round 6, the AA instances of the forward raster.
bool staged_forward(const DeodrHipScene *sc, const KParams &p, bool fused)
{
	return (p.C <= CH || (!(p.sigma > 0) && !p.aa_err && !p.texture && !fused)) && !g_force_generic && !det_mode(sc);
}

// Staged forward: counters -> work list + tile bitmap (scan), then the raster on the caller's stream and, forked from it, the
// background fill on the side stream.  *join receives the event the caller's stream has to wait for before the call returns
// control to it (the fill overlaps whatever the call launches in between).
template <class PixT>
int launch_forward_staged(const KParams &p, bool fused, hipStream_t stream, hipEvent_t *join)
{
	KParams q = p;
	q.tile_blocks = fwd_tile_blocks(p.L.ntiles, p.n_views, fused && p.fuse_edges);
	q.heavy_share = heavy_share_for(p.n_views, q.tile_blocks, fused && p.fuse_edges);
	q.split_part = split_part_for(p.n_views, q.tile_blocks);
	q.pair_tex = p.texture != nullptr && p.n_views < TEX_TWO_KERNELS;
	forward_launch_constants(q);
	hipLaunchKernelGGL(tile_scan_kernel, dim3((p.L.ntiles + SCAN_BLOCK - 1) / SCAN_BLOCK, p.n_views), dim3(SCAN_BLOCK), 0, stream, q);
	if (p.fill_mode == 0)
	{
		std::lock_guard<std::mutex> lock(g_side_mutex);
		SideStream ss;
		if (side_stream(ss) || check_hip(hipEventRecord(ss.fork, stream), "fork") || check_hip(hipStreamWaitEvent(ss.stream, ss.fork, 0), "fork"))
			return 1;
		const unsigned words = (unsigned)(p.n_views * p.L.nwords);
		hipLaunchKernelGGL(fill_kernel<PixT>, dim3((words + FILL_WAVES - 1) / FILL_WAVES), dim3(64 * FILL_WAVES), 0, ss.stream, q, fused ? 0 : 1);
		if (check_hip(hipEventRecord(ss.join, ss.stream), "join"))
			return 1;
		*join = ss.join;
	}
	// (+ the workgroups that stream this kernel's share of the background of the empty tiles, one unit each: a bitmap word, or 64 in a retained step)
	const dim3 grid((unsigned)p.n_views * (unsigned)q.fwd_walkers + (unsigned)q.fwd_n_fill);
	const bool tex = p.texture != nullptr;
	hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
	if (fused && tex && p.fuse_edges)
		(void)hipStreamIsCapturing(stream, &capturing);
	constexpr bool f64 = sizeof(PixT) == 8;
	const FwdInst inst = select_forward(FwdCall{f64, fused, tex, p.fuse_edges != 0, p.clamp != 0, fit_weights(p) != nullptr, p.aa_err != 0,
												p.strict && p.W % TILE == 0 && p.H % TILE == 0, capturing != hipStreamCaptureStatusNone, p.C, p.n_views,
												q.tile_blocks, q.heavy_share});
	auto launch = [&](const FwdInst &want, dim3 g, hipStream_t on, const KParams &args) {
		return launch_from("internal: no instance of raster_fwd_fast_kernel for this call", FWD_INSTANCES, want, [&](auto i) {
			constexpr FwdInst k = FWD_INSTANCES[decltype(i)::value];
			if constexpr (fwd_exists(k, f64))
				hipLaunchKernelGGL((raster_fwd_fast_kernel<PixT, k.fused, k.tex, k.clamp, k.nc, k.common, k.texe, k.var>), g, dim3(64), 0, on, args);
			return fwd_exists(k, f64);
		});
	};
	if (inst.texe != 2)
		return launch(inst, grid, stream, q);
	// the two-kernel form: the head walkers (edge adjoint: many registers) on the side stream, everybody else (+ the fill workgroups) on the caller's,
	// both behind the scan
	const unsigned head = (unsigned)p.n_views * (unsigned)(q.tile_blocks / q.heavy_share);
	std::lock_guard<std::mutex> lock(g_side_mutex);
	SideStream ss;
	if (side_stream(ss) || check_hip(hipEventRecord(ss.fork, stream), "fork") || check_hip(hipStreamWaitEvent(ss.stream, ss.fork, 0), "fork"))
		return 1;
	KParams rest = q;
	FwdInst others = inst;
	rest.block_base = head, others.texe = 3;
	if (launch(inst, dim3(head), ss.stream, q) || launch(others, dim3(grid.x - head), stream, rest))
		return 1;
	return check_hip(hipEventRecord(ss.join, ss.stream), "join") || check_hip(hipStreamWaitEvent(stream, ss.join, 0), "join");
}

// grid of the un-staged kernels: four tiles (wavefronts) per workgroup
dim3 generic_grid(const KParams &p, int n_views) { return dim3((unsigned)(((p.L.tiles_x + 3) / 4) * p.L.tiles_y), (unsigned)n_views); }

// fused: the forward also back-propagates L = sum (image - obs)^2 through the tiles that have no silhouette edge (staged
// kernels only; the caller checks).  *join: see launch_forward_staged (nullptr when nothing was forked).
int launch_forward(const DeodrHipScene *sc, KParams &p, hipStream_t stream, hipEvent_t *join, bool fused = false)
{
	const int n_views = sc->n_views;
	*join = nullptr;
	g_profile = g_profile_every > 0 && (g_profile_calls++ % (unsigned)g_profile_every) == 0;
	p.stamp = (g_stamps && g_stamp_calls < (unsigned)g_stamp_rows) ? g_stamps + 4 * (size_t)g_stamp_calls++ : nullptr;
	p.n_views = n_views;
	const bool f64 = sc->pixel_dtype == DEODR_HIP_F64;
	if (p.T > 0)
	{
		const dim3 grid(prim_grid(p, n_views, true));
		ScopedKernelTimer t(KID_SETUP, stream);
		if (launch_from("internal: no instance of setup_bin_kernel for this call", SETUP_INSTANCES, select_setup(p.vtx_f64 != 0, p.C), [&](auto i) {
				constexpr PrimInst k = SETUP_INSTANCES[decltype(i)::value];
				hipLaunchKernelGGL((setup_bin_kernel<k.vtx_f64, k.nc>), grid, dim3(PRIM_BLOCK), 0, stream, p);
				return true;
			}))
			return 1;
	}
	{
		ScopedKernelTimer t(KID_RASTER_FWD, stream);
		if (!staged_forward(sc, p, fused))
			with_pixel_type(f64, [&](auto pix) { hipLaunchKernelGGL(raster_fwd_kernel<decltype(pix)>, generic_grid(p, n_views), dim3(256), 0, stream, p); });
		else if (with_pixel_type(f64, [&](auto pix) { return launch_forward_staged<decltype(pix)>(p, fused, stream, join); }))
			return 1;
	}
	return check_hip(hipGetLastError(), "forward launch");
}

// the caller's stream waits for the side stream's work of this call
int join_side(hipStream_t stream, hipEvent_t join) { return join ? check_hip(hipStreamWaitEvent(stream, join, 0), "join") : 0; }

// adjoint raster and the per-primitive finalize; owner_tiles = false after a fused forward
int launch_adjoint(const DeodrHipScene *sc, KParams &p, hipStream_t st, bool owner_tiles)
{
	// (antialiase_error, round 6: the tiles without silhouette edges through raster_bwd_fast_kernel -- their gradient is -2 (obs - image) err_buffer_b,
	// H.h:3054-3060 --, the tiles with edges through the un-staged tile code, called tile by tile from raster_bwd_edge_kernel's work lists)
	const bool fast = staged_adjoint(sc, p);
	p.n_views = sc->n_views;
	if (det_mode(sc) && det_shadows(p, sc->n_views, st))
		return 1;
	// persistent waves of the edge kernel: enough to cover a silhouette-heavy single view, few enough that with many views
	// the waves that find their sub-list exhausted cost nothing
	const int edge_waves = p.L.ntiles < EDGE_WAVES ? p.L.ntiles : EDGE_WAVES;
	dim3 edge_grid(sc->n_views, edge_waves + (fast ? fill_share_blocks(fill_units(p.retained, p.fill_mode, 0, p.L.nwords)) : 0));
	if (!fast || owner_tiles || (p.sigma > 0 && !p.fuse_edges)) // (a fit step with fused edge tiles launches nothing here)
	{
		ScopedKernelTimer t(KID_RASTER_BWD, st);
		auto raster = [&](auto pix) { return launch_adjoint_raster<decltype(pix)>(p, fast, owner_tiles, generic_grid(p, sc->n_views), edge_grid, st); };
		if (with_pixel_type(sc->pixel_dtype == DEODR_HIP_F64, raster))
			return 1;
	}
	if (p.T > 0)
	{
		const int fill_words = fast ? sc->n_views * fill_units(p.retained, p.fill_mode, 1, p.L.nwords) : 0; // (units: one wavefront each)
		dim3 g2(prim_grid(p, sc->n_views, false) + (unsigned)((fill_words + PRIM_BLOCK / 64 - 1) / (PRIM_BLOCK / 64)) +
				(p.loss_out ? 1u : 0u)); // (+ the workgroup that adds up the loss)
		ScopedKernelTimer t(KID_FINALIZE, st);
		if (launch_from("internal: no instance of finalize_kernel for this call", FINALIZE_INSTANCES, select_finalize(p.vtx_f64 != 0, p.C, p.det != 0, p.prim_tables != 0), [&](auto i) {
				constexpr PrimInst k = FINALIZE_INSTANCES[decltype(i)::value];
				hipLaunchKernelGGL((finalize_kernel<k.vtx_f64, k.nc, k.det, k.table>), g2, dim3(PRIM_BLOCK), 0, st, p);
				return true;
			}))
			return 1;
	}
	if (p.det)
		det_convert(p, sc->n_views, st);
	return check_hip(hipGetLastError(), "backward launch");
}

// Workspaces whose last forward was the fused one: their owner buffer is incomplete (tiles without edges are not written), so a
// later deodr_hip_render_scene_b that claims to have the forward state must rebuild it.
std::mutex g_fused_mutex;
std::unordered_set<const void *> g_fused_ws;
void note_forward(const void *workspace, bool fused)
{
	std::lock_guard<std::mutex> lock(g_fused_mutex);
	if (fused)
		g_fused_ws.insert(workspace);
	else
		g_fused_ws.erase(workspace);
}
bool last_forward_was_fused(const void *workspace)
{
	std::lock_guard<std::mutex> lock(g_fused_mutex);
	return g_fused_ws.count(workspace) != 0;
}

// Streaming copy / fill / read with 16-byte non-temporal accesses, the access pattern of the rasterizer's own frame stores and
// background fill (deodr_hip_copy_probe: the copy ceiling of the box a roofline fraction may also be quoted against).
typedef uint32_t probe_u4 __attribute__((ext_vector_type(4)));
constexpr int PROBE_MODES[] = {0, 1, 2}; // copy, fill, read
template <int MODE>
__global__ __launch_bounds__(256) void copy_probe_kernel(probe_u4 *dst, const probe_u4 *src, size_t n16)
{
	const size_t stride = (size_t)gridDim.x * 256 * 4;
	probe_u4 acc = {0, 0, 0, 0};
	for (size_t i = (size_t)blockIdx.x * 256 * 4 + threadIdx.x; i < n16; i += stride)
	{ // four independent 16-byte pieces per thread and round, consecutive lanes on consecutive pieces
		probe_u4 v[4];
#pragma unroll
		for (int u = 0; u < 4; u++)
			if (MODE != 1 && i + u * 256 < n16)
				v[u] = __builtin_nontemporal_load(src + i + u * 256);
			else
				v[u] = probe_u4{1, 2, 3, 4};
#pragma unroll
		for (int u = 0; u < 4; u++)
			if (i + u * 256 < n16)
			{
				if (MODE == 2)
					acc ^= v[u];
				else
					__builtin_nontemporal_store(v[u], dst + i + u * 256);
			}
	}
	if (MODE == 2 && (acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x9e3779b9u)
		((uint32_t *)dst)[0] = acc.x; // (never true for real data: keeps the loads alive)
}

// ---- scratch of the fit-iteration kernels and the data terms: Scratch of dr_host.h, one counter word per kernel
size_t fh_blocks(long long count) { return (size_t)((count + FH_BLOCK - 1) / FH_BLOCK); }
size_t fit_scratch_need_pose_b(int, int n) { return scratch_need((size_t)POSE_B_BLOCKS * (size_t)(7 * n + 3)); }
size_t fit_scratch_need_shade_b(int V, int n) { return scratch_need(3 * (size_t)n * V + 7 * fh_blocks((long long)n * V * GATHER_LANES)); }
size_t fit_scratch_need_rigid(int V) { return scratch_need(fh_blocks((long long)V * GATHER_LANES)); }
size_t fit_scratch_need_l2(void) { return scratch_need((size_t)L2_BLOCKS); }
size_t fit_scratch_need_momentum(int most) { return scratch_need((size_t)MOMENTUM_MAX * 3 * fh_blocks(most)); }
enum FitCounter
{
	FC_POSE_B = 0,
	FC_SHADE_B = 1,
	FC_RIGID = 2,
	FC_L2 = 3,
	FC_MOMENTUM = 4 // ... + MOMENTUM_MAX
};
static_assert(FC_MOMENTUM + MOMENTUM_MAX <= SCRATCH_COUNTER_WORDS, "the counter words of the scratch");

// The kernels that walk the views of a vertex: one thread per vertex for a single view, GATHER_LANES adjacent lanes otherwise.
// launch(the lane count as a constant, the workgroups that gives for V vertices).
template <class F>
auto with_gather_lanes(int V, int n, F launch)
{
	return n == 1 ? launch(std::integral_constant<int, 1>{}, fh_blocks(V)) : launch(std::integral_constant<int, GATHER_LANES>{}, fh_blocks((long long)V * GATHER_LANES));
}

} // namespace

extern "C" {

int deodr_hip_abi_version(void) { return DEODR_HIP_ABI_VERSION; }

int deodr_hip_force_generic(int on)
{
	g_force_generic = on != 0;
	return 0;
}

int deodr_hip_set_deterministic(int on)
{
	g_det = on != 0;
	return 0;
}

int deodr_hip_profile_enable(int every)
{
	g_profile_every = every > 0 ? every : 0;
	g_profile_calls = 0;
	g_profile = false;
	return 0;
}

int deodr_hip_profile_stamps(void *device_buffer, int rows)
{
	g_stamps = (unsigned long long *)device_buffer;
	g_stamp_rows = device_buffer && rows > 0 ? rows : 0;
	g_stamp_calls = 0;
	return 0;
}

int deodr_hip_profile_read(double ms_sum[4], unsigned long long launches[4])
{
	for (int i = 0; i < KID_COUNT; i++)
	{
		ms_sum[i] = 0;
		launches[i] = 0;
	}
	for (ProfEvent &e : g_prof_events)
	{
		if (check_hip(hipEventSynchronize(e.stop), "profile sync"))
			return 1;
		float ms = 0;
		if (check_hip(hipEventElapsedTime(&ms, e.start, e.stop), "profile elapsed"))
			return 1;
		ms_sum[e.kid] += ms;
		launches[e.kid] += 1;
		g_prof_free.push_back({e.start, e.stop});
	}
	g_prof_events.clear();
	return 0;
}

int deodr_hip_copy_probe(void *dst, const void *src, size_t bytes, int mode, int reps, void *stream)
{
	if (!dst || (mode != 1 && !src) || bytes < 16 || (bytes & 15) || ((uintptr_t)dst & 15) || ((uintptr_t)src & 15) || mode < 0 || mode > 2 || reps <= 0)
		return fail("copy_probe: bad arguments");
	const size_t n16 = bytes / 16;
	size_t blocks = (n16 + 1023) / 1024;
	if (blocks > 256 * 32)
		blocks = 256 * 32; // 32 workgroups per CU, grid-stride beyond
	for (int r = 0; r < reps; r++)
	{
		(void)launch_from("internal: no instance of copy_probe_kernel for this mode", PROBE_MODES, mode, [&](auto i) { // (mode was checked above)
			hipLaunchKernelGGL(copy_probe_kernel<PROBE_MODES[decltype(i)::value]>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (probe_u4 *)dst, (const probe_u4 *)src, n16);
			return true;
		});
	}
	return check_hip(hipGetLastError(), "copy_probe launch");
}

const char *deodr_hip_last_error(void) { return g_error; }

size_t deodr_hip_workspace_bytes(int nb_triangles, int height, int width, int nb_colors, int n_views, size_t pool_pairs)
{
	if (nb_triangles < 0 || height <= 0 || width <= 0 || nb_colors <= 0 || n_views <= 0)
		return 0;
	return make_layout(nb_triangles, height, width, nb_colors, pool_pairs).view_bytes * (size_t)n_views;
}

int deodr_hip_render_scene(const DeodrHipScene *sc, void *image, void *z_buffer, double sigma, int antialiase_error, const void *obs,
						   void *err_buffer, void *workspace, size_t workspace_bytes, void *stream)
{
	KParams p;
	if (fill_params(sc, sigma, workspace, workspace_bytes, p, false))
		return 1;
	if (antialiase_error && (!obs || !err_buffer))
		return fail("antialiase_error needs obs and err_buffer");
	p.image = image;
	p.zbuf = z_buffer;
	p.aa_err = antialiase_error != 0;
	p.obs = obs;
	p.err = err_buffer;
	note_forward(workspace, false);
	hipEvent_t join = nullptr;
	if (launch_forward(sc, p, (hipStream_t)stream, &join))
		return 1;
	return join_side((hipStream_t)stream, join);
}

int deodr_hip_render_scene_b(const DeodrHipScene *sc, const void *image, const void *z_buffer, const void *image_b, double sigma,
							 int antialiase_error, const void *obs, const void *err_buffer, const void *err_buffer_b, void *workspace,
							 size_t workspace_bytes, int have_forward_state, void *stream)
{
	(void)z_buffer;
	(void)err_buffer;
	KParams p;
	if (fill_params(sc, sigma, workspace, workspace_bytes, p, true))
		return 1;
	if (antialiase_error)
	{
		if (!obs || !err_buffer_b)
			return fail("antialiase_error needs obs and err_buffer_b");
		// (the staged kernels read the frame of the tiles without silhouette edges from `image`, bwd_fast_tile; refused for the un-staged
		// family too, which recomputes the colour: one contract for the mode)
		if (!image)
			return fail("antialiase_error needs image: the frame deodr_hip_render_scene wrote in this mode");
	}
	else if (!image_b && !(image && obs))
		return fail("image_b == NULL (or, for the residual mode, image and obs)");
	hipStream_t st = (hipStream_t)stream;
	hipEvent_t join = nullptr;
	if (!have_forward_state || last_forward_was_fused(workspace))
	{ // stateless use (or a fused forward, which leaves no complete owner buffer): rebuild records, tile lists and the owner
	  // buffer (no image / z written)
		note_forward(workspace, false);
		KParams f = p;
		f.image = nullptr;
		f.zbuf = nullptr;
		f.aa_err = 0;
		if (launch_forward(sc, f, st, &join) || join_side(st, join)) // (the generic adjoint reads the owner ids of every tile)
			return 1;
	}
	p.image_b = image_b;
	p.image_in = image;
	p.obs = obs;
	p.err_b = antialiase_error ? err_buffer_b : nullptr; // (ignored without antialiase_error, as ever; the slot is KParams::weights then: never a caller's pointer)
	p.aa_err = antialiase_error != 0;
	return launch_adjoint(sc, p, st, true);
}

static int l2_loss_impl(const void *image, const void *obs, int pixel_dtype, size_t count, double *out, void *scratch, size_t scratch_bytes, void *stream,
					   int clamp, double clamp_lo, double clamp_hi, const void *weights = nullptr, int nb_colors = 1);

static int render_scene_fit_impl(const DeodrHipScene *sc, void *image, void *z_buffer, double sigma, const void *obs, int clear_gradients,
								 const DeodrHipFitOptions *opt, void *workspace, size_t workspace_bytes, void *stream, int retained = 0)
{
	const double *tile_loss = opt ? opt->tile_loss : nullptr;
	double *loss_out = opt ? opt->loss : nullptr, *loss_scratch = opt ? (double *)opt->loss_scratch : nullptr;
	if (opt && opt->clamp && !(opt->clamp_lo <= opt->clamp_hi))
		return fail("render_scene_fit: clamp_lo > clamp_hi");
	if (loss_out && (!tile_loss || !loss_scratch))
		return fail("render_scene_fit: the loss needs the background table (deodr_hip_background_loss) and its scratch");
	KParams p;
	if (fill_params(sc, sigma, workspace, workspace_bytes, p, true))
		return 1;
	if (!image || !obs)
		return fail("render_scene_fit needs image and obs");
	hipStream_t st = (hipStream_t)stream;
	p.image = image;
	p.zbuf = z_buffer;
	p.obs = obs;
	p.image_in = image;
	if (clear_gradients)
	{
		p.clear_grads = 1; // vertex arrays: zeroed by the set-up kernel; the texture gradient (large, if any) by a fill
		if (p.texture_b && check_hip(hipMemsetAsync(p.texture_b, 0, (size_t)p.tex_h * p.tex_w * p.C * elem_bytes(sc->pixel_dtype), st), "clear texture_b"))
			return 1;
	}
	const bool fused = staged_adjoint(sc, p);
	const bool loss_in_kernels = loss_out && fused && p.T > 0; // (the tile walkers of the staged forward + finalize's last workgroup)
	if (loss_in_kernels)
		p.loss_tile_bg = tile_loss, p.loss_wave = loss_scratch, p.loss_out = loss_out;
	if (opt && opt->clamp)
		p.clamp = 1, p.clamp_lo = opt->clamp_lo, p.clamp_hi = opt->clamp_hi;
	p.weights = opt ? opt->weights : nullptr;
	// the background of the empty tiles rides on the adjoint's kernels (fill_share); without any of them: the side stream
	// The forward raster also back-propagates the tiles with silhouette edges (no edge-tile kernel, no saved sweeps) and streams a share
	// of the background.  Textured scenes too since round 5 (round 2 measured 0.264 -> 0.407 ms for one 2048^2 view of 100 k triangles:
	// 400 spilled registers on the edge path at four waves per SIMD; with the instances of their own at three waves, the many-edge tiles
	// split into parts and the quadrant windows of the texture gradient it is 0.195 -> 0.168 ms, 2 / 4 / 8 views 0.257 -> 0.243 /
	// 0.448 -> 0.451 / 0.890 -> 0.893: profiles/r05y_ab_fused_textured_edge_tiles.txt).  (sigma = 0: no edge anywhere, the lighter instances)
	p.fuse_edges = fused && (!p.texture || sigma > 0);
	p.fill_mode = fused ? (((sigma > 0 && !p.fuse_edges) ? 1 : 0) | (p.T > 0 ? 2 : 0) | ((p.T > 0 && p.fuse_edges) ? 4 : 0)) : 0;
	// the caller's claim that the buffers still hold the frame of the forward before this one: only where the fill rides on the step's kernels
	// (the stand-alone fill_kernel fills every empty tile whatever is claimed), and only believed by a fill wavefront that finds it confirmed
	p.retained = (retained && p.fill_mode != 0) ? 1 : 0;
	note_forward(workspace, fused);
	hipEvent_t join = nullptr;
	if (launch_forward(sc, p, st, &join, fused))
		return 1;
	// The step-done flag: stored by the last wavefront of finalize_kernel to finish when that kernel is the step's last (the usual fit
	// step), by a one-thread kernel behind everything otherwise.
	uint32_t *done_flag = opt ? opt->done_flag : nullptr;
	const bool fin_signals = done_flag && p.T > 0 && !det_mode(sc) && !join && !(loss_out && !loss_in_kernels);
	if (fin_signals)
		p.done_flag = done_flag, p.done_value = opt->done_value;
	if (launch_adjoint(sc, p, st, !fused))
		return 1;
	if (join_side(st, join)) // the background fill has been overlapping the adjoint
		return 1;
	if (loss_out && !loss_in_kernels)
	{ // un-staged kernels (more than 4 channels) or a scene without triangles: one pass over the finished frame
		if (check_hip(hipMemsetAsync(loss_scratch, 0, fit_scratch_need_l2(), st), "loss scratch"))
			return 1;
		if (l2_loss_impl(image, obs, sc->pixel_dtype, (size_t)sc->n_views * sc->height * sc->width * sc->nb_colors, loss_out, loss_scratch,
						 fit_scratch_need_l2(), stream, p.clamp, p.clamp_lo, p.clamp_hi, fit_weights(p), sc->nb_colors))
			return 1;
	}
	if (done_flag && !fin_signals)
	{
		hipLaunchKernelGGL(store_flag_kernel, dim3(1), dim3(1), 0, st, done_flag, opt->done_value);
		return check_hip(hipGetLastError(), "done flag launch");
	}
	return 0;
}

int deodr_hip_render_scene_fit(const DeodrHipScene *sc, void *image, void *z_buffer, double sigma, const void *obs, int clear_gradients,
							   void *workspace, size_t workspace_bytes, void *stream)
{
	return render_scene_fit_impl(sc, image, z_buffer, sigma, obs, clear_gradients, nullptr, workspace, workspace_bytes, stream);
}

int deodr_hip_render_scene_fit_ex(const DeodrHipScene *sc, void *image, void *z_buffer, double sigma, const void *obs, int clear_gradients,
								  const DeodrHipFitOptions *options, void *workspace, size_t workspace_bytes, void *stream)
{
	return render_scene_fit_impl(sc, image, z_buffer, sigma, obs, clear_gradients, options, workspace, workspace_bytes, stream);
}

// ---- include/deodr_hip_retained.h
int deodr_hip_retained_abi_version(void) { return DEODR_HIP_RETAINED_ABI_VERSION; }

int deodr_hip_render_scene_fit_retained(const DeodrHipScene *sc, void *image, void *z_buffer, double sigma, const void *obs, int clear_gradients,
										const DeodrHipFitOptions *options, int retained, void *workspace, size_t workspace_bytes, void *stream)
{
	return render_scene_fit_impl(sc, image, z_buffer, sigma, obs, clear_gradients, options, workspace, workspace_bytes, stream, retained);
}

static size_t loss_table_doubles(int height, int width, int n_views)
{ // [0] the whole frame, then one value per view and tile; never less than the partials of the one-pass fallback
	const size_t tiles = (size_t)((width + TILE - 1) / TILE) * ((height + TILE - 1) / TILE);
	size_t n = 1 + (size_t)n_views * tiles;
	const size_t floors[2] = {(size_t)L2_BLOCKS + 16, (size_t)n_views * LOSS_SLOTS};
	for (size_t f : floors)
		n = n > f ? n : f;
	return n;
}

size_t deodr_hip_fit_loss_bytes(int height, int width, int n_views)
{
	return height > 0 && width > 0 && n_views > 0 ? sizeof(double) * loss_table_doubles(height, width, n_views) : 0;
}

int deodr_hip_background_loss(const DeodrHipScene *sc, const void *obs, const DeodrHipFitOptions *options, double *tile_loss, void *workspace,
							  size_t workspace_bytes, void *stream)
{
	KParams p;
	if (fill_params(sc, 1.0, workspace, workspace_bytes, p, false))
		return 1;
	if (!obs || !tile_loss)
		return fail("background_loss needs obs and the table");
	if (options && options->clamp)
		p.clamp = 1, p.clamp_lo = options->clamp_lo, p.clamp_hi = options->clamp_hi;
	p.weights = options ? options->weights : nullptr;
	p.obs = obs;
	p.n_views = sc->n_views;
	hipStream_t st = (hipStream_t)stream;
	const dim3 grid((unsigned)p.L.ntiles, (unsigned)sc->n_views);
	with_pixel_type(sc->pixel_dtype == DEODR_HIP_F64, [&](auto pix) {
		if (fit_weights(p))
			hipLaunchKernelGGL(background_loss_weighted_kernel<decltype(pix)>, grid, dim3(64), 0, st, p, tile_loss);
		else
			hipLaunchKernelGGL(background_loss_kernel<decltype(pix)>, grid, dim3(64), 0, st, p, tile_loss);
	});
	hipLaunchKernelGGL(background_loss_total_kernel, dim3(1), dim3(FH_BLOCK), 0, st, tile_loss, (size_t)sc->n_views * p.L.ntiles);
	return check_hip(hipGetLastError(), "background_loss launch");
}

// ---- front half of a fit iteration (dr_fronthalf.h): plain double arrays on the device, asynchronous on `stream`

int deodr_hip_rigid_transform(const double *vertices, const double *quaternions, const double *translations, double *out, int V, int n, void *stream)
{
	if (!vertices || !quaternions || !translations || !out || V <= 0 || n <= 0)
		return fail("rigid_transform: bad arguments");
	hipLaunchKernelGGL(rigid_transform_kernel, dim3((V + FH_BLOCK - 1) / FH_BLOCK, n), dim3(FH_BLOCK), 0, (hipStream_t)stream, vertices, quaternions, translations, out, V, n);
	return check_hip(hipGetLastError(), "rigid_transform launch");
}

int deodr_hip_rigid_transform_b(const double *vertices, const double *quaternions, const double *out_b, double *vertices_b, double *pose_b, int V, int n,
								void *stream)
{ // pose_b [n,7] = (quaternion adjoint 4, translation adjoint 3) per view, overwritten
	if (!vertices || !quaternions || !out_b || !vertices_b || !pose_b || V <= 0 || n <= 0)
		return fail("rigid_transform_b: bad arguments");
	hipStream_t st = (hipStream_t)stream;
	if (check_hip(hipMemsetAsync(pose_b, 0, sizeof(double) * 7 * (size_t)n, st), "rigid_transform_b clear"))
		return 1;
	// (the kernel addresses the two adjoints separately: quaternions first [n,4], then translations [n,3])
	hipLaunchKernelGGL(rigid_transform_b_kernel, dim3((V + FH_BLOCK - 1) / FH_BLOCK), dim3(FH_BLOCK), 0, st, vertices, quaternions, out_b, vertices_b, pose_b,
					   pose_b + 4 * (size_t)n, V, n);
	return check_hip(hipGetLastError(), "rigid_transform_b launch");
}

int deodr_hip_project_points(const double *points, const double *extrinsic, const double *intrinsic, const double *distortion, double *ij, double *depths,
							 int V, int n, void *stream)
{
	if (!points || !extrinsic || !intrinsic || !ij || !depths || V <= 0 || n <= 0)
		return fail("project_points: bad arguments");
	hipLaunchKernelGGL(project_points_kernel, dim3((V + FH_BLOCK - 1) / FH_BLOCK, n), dim3(FH_BLOCK), 0, (hipStream_t)stream, points, extrinsic, intrinsic,
					   distortion, ij, depths, V, n);
	return check_hip(hipGetLastError(), "project_points launch");
}

int deodr_hip_project_points_b(const double *points, const double *extrinsic, const double *intrinsic, const double *distortion, const double *ij_b,
							   const double *depths_b, double *points_b, int V, int n, void *stream)
{
	if (!points || !extrinsic || !intrinsic || !ij_b || !points_b || V <= 0 || n <= 0)
		return fail("project_points_b: bad arguments");
	hipLaunchKernelGGL(project_points_b_kernel, dim3((V + FH_BLOCK - 1) / FH_BLOCK, n), dim3(FH_BLOCK), 0, (hipStream_t)stream, points, extrinsic, intrinsic,
					   distortion, ij_b, depths_b, points_b, V, n);
	return check_hip(hipGetLastError(), "project_points_b launch");
}

int deodr_hip_silhouette_flags(const double *ij, const uint32_t *faces, const uint32_t *edge_faces, uint8_t *flags, int T, int V, int n, int clockwise,
							   void *stream)
{
	if (!ij || !faces || !edge_faces || !flags || T <= 0 || V <= 0 || n <= 0)
		return fail("silhouette_flags: bad arguments");
	hipLaunchKernelGGL(silhouette_flags_kernel, dim3((T + FH_BLOCK - 1) / FH_BLOCK, n), dim3(FH_BLOCK), 0, (hipStream_t)stream, ij, faces, edge_faces, flags, T, V,
					   clockwise);
	return check_hip(hipGetLastError(), "silhouette_flags launch");
}

size_t deodr_hip_fit_scratch_bytes(int V, int n)
{
	if (V <= 0 || n <= 0)
		return 0;
	size_t need = fit_scratch_need_pose_b(V, n);
	const size_t others[4] = {fit_scratch_need_shade_b(V, n), fit_scratch_need_rigid(V), fit_scratch_need_momentum(3 * V > 7 * n ? 3 * V : 7 * n),
							  fit_scratch_need_l2()};
	for (size_t o : others)
		need = o > need ? o : need;
	return need;
}

int deodr_hip_momentum_update(int n_tensors, double *const *x, double *const *speed, const double *const *grad, const double *const *grad2,
							  const double *factor, const double *step_max, const int *count, const int *normalize_rows, double inertia, double damping,
							  const double *grad_scale, const double *const *grad_mean, double *const *mean_out, double *energy, const double *data_energy,
							  double data_weight, void *scratch, size_t scratch_bytes, void *stream)
{
	if (energy && !data_energy)
		return fail("momentum_update: energy[1] = data_weight * data_energy[0] + energy[0] needs data_energy");
	if (n_tensors <= 0 || n_tensors > MOMENTUM_MAX || !x || !speed || !grad || !factor || !step_max || !count)
		return fail("momentum_update: bad arguments (at most 8 tensors per call)");
	MomentumArgs a;
	memset(&a, 0, sizeof a);
	int most = 0;
	bool means = false;
	for (int k = 0; k < n_tensors; k++)
	{
		if (!x[k] || !speed[k] || !grad[k] || count[k] <= 0)
			return fail("momentum_update: NULL tensor");
		a.x[k] = x[k], a.speed[k] = speed[k], a.grad[k] = grad[k], a.grad2[k] = grad2 ? grad2[k] : nullptr;
		a.factor[k] = factor[k], a.step_max[k] = step_max[k], a.count[k] = count[k], a.normalize_rows[k] = normalize_rows ? normalize_rows[k] : 0;
		a.grad_scale[k] = grad_scale ? grad_scale[k] : 1.0;
		a.grad_mean[k] = grad_mean ? grad_mean[k] : nullptr;
		a.mean_out[k] = mean_out ? mean_out[k] : nullptr;
		if ((a.grad_mean[k] || a.mean_out[k]) && (count[k] % 3 || a.normalize_rows[k]))
			return fail("momentum_update: grad_mean / mean_out are for [count/3, 3] tensors without row normalisation");
		means = means || a.mean_out[k];
		most = count[k] > most ? count[k] : most;
	}
	const Scratch sc = {scratch, scratch_bytes};
	if (means && !sc.holds(fit_scratch_need_momentum(most)))
		return fail("momentum_update: mean_out needs the fit scratch (deodr_hip_fit_scratch_bytes)");
	a.n = n_tensors, a.inertia = inertia, a.damping = damping;
	a.energy = energy, a.data_energy = data_energy, a.data_weight = data_weight;
	a.counters = scratch ? sc.counter(FC_MOMENTUM) : nullptr;
	a.partials = scratch ? sc.doubles() : nullptr;
	hipLaunchKernelGGL(momentum_update_kernel, dim3((most + FH_BLOCK - 1) / FH_BLOCK, n_tensors), dim3(FH_BLOCK), 0, (hipStream_t)stream, a);
	return check_hip(hipGetLastError(), "momentum_update launch");
}

int deodr_hip_fit_pose_project(double *vertices, const double *vertices_mean, const double *quaternions, const double *translations, const double *extrinsic,
							   const double *intrinsic, const double *distortion, double *posed, double *ij, double *depths, double *depth_colors,
							   double depth_scale, int V, int n, void *stream)
{
	if (!vertices || !quaternions || !translations || !extrinsic || !intrinsic || !posed || !ij || !depths || V <= 0 || n <= 0)
		return fail("fit_pose_project: bad arguments");
	with_gather_lanes(V, n, [&](auto lanes, size_t blocks) {
		hipLaunchKernelGGL(fit_pose_project_kernel<decltype(lanes)::value>, dim3(blocks), dim3(FH_BLOCK), 0, (hipStream_t)stream, vertices, vertices_mean, quaternions,
						   translations, extrinsic, intrinsic, distortion, posed, ij, depths, depth_colors, depth_scale, V, n);
	});
	return check_hip(hipGetLastError(), "fit_pose_project launch");
}

int deodr_hip_fit_pose_project_b(const double *vertices, const double *quaternions, const double *posed, const double *extrinsic, const double *intrinsic,
								 const double *distortion, const double *posed_b, const double *ij_b, const double *depths_b, double depths_b_scale,
								 double *vertices_b, double *out, void *scratch, size_t scratch_bytes, int V, int n, const double *colors_b, int nb_colors,
								 double *colors_sum, void *stream)
{
	if (!vertices || !quaternions || !posed || !extrinsic || !intrinsic || !ij_b || !vertices_b || !out || V <= 0 || n <= 0)
		return fail("fit_pose_project_b: bad arguments");
	if (n > FIT_MAX_VIEWS)
		return fail("fit_pose_project_b: at most 64 views per call");
	if (colors_sum && (!colors_b || nb_colors <= 0 || nb_colors > 4))
		return fail("fit_pose_project_b: colors_sum needs colors_b with 1 - 4 channels");
	const Scratch sc = {scratch, scratch_bytes};
	if (!sc.holds(fit_scratch_need_pose_b(V, n)))
		return fail("fit_pose_project_b: scratch too small (deodr_hip_fit_scratch_bytes)");
	with_gather_lanes(V, n, [&](auto lanes, size_t blocks) {
		hipLaunchKernelGGL(fit_pose_project_b_kernel<decltype(lanes)::value>, dim3(capped_blocks(blocks, 1, POSE_B_BLOCKS)), dim3(FH_BLOCK), 0, (hipStream_t)stream,
						   vertices, quaternions, posed, extrinsic, intrinsic, distortion, posed_b, ij_b, depths_b, depths_b_scale, vertices_b, out, sc.doubles(),
						   sc.counter(FC_POSE_B), V, n, colors_b, nb_colors, colors_sum);
	});
	return check_hip(hipGetLastError(), "fit_pose_project_b launch");
}

int deodr_hip_views_gradient_sum(const double *posed, const double *extrinsic, const double *intrinsic, const double *distortion, const double *ij_b,
								 const double *depths_b, double depths_b_scale, double *vertices_b, int V, int n, const double *colors_b, int nb_colors,
								 double *colors_sum, void *stream)
{
	if (!posed || !extrinsic || !intrinsic || !ij_b || !vertices_b || V <= 0 || n <= 0)
		return fail("views_gradient_sum: bad arguments");
	if (colors_sum && (!colors_b || nb_colors <= 0 || nb_colors > 4))
		return fail("views_gradient_sum: colors_sum needs colors_b with 1 - 4 channels");
	with_gather_lanes(V, n, [&](auto lanes, size_t blocks) {
		hipLaunchKernelGGL(views_gradient_sum_kernel<decltype(lanes)::value>, dim3(blocks), dim3(FH_BLOCK), 0, (hipStream_t)stream, posed, extrinsic, intrinsic,
						   distortion, ij_b, depths_b, depths_b_scale, vertices_b, V, n, colors_b, nb_colors, colors_sum);
	});
	return check_hip(hipGetLastError(), "views_gradient_sum launch");
}

int deodr_hip_wait_flag(const uint32_t *flag, uint32_t value, uint32_t *status, double timeout_seconds, void *stream)
{
	if (!flag || !(timeout_seconds > 0))
		return fail("wait_flag: bad arguments");
	hipLaunchKernelGGL(wait_flag_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, flag, value, status, (unsigned long long)(timeout_seconds * 1e8));
	return check_hip(hipGetLastError(), "wait_flag launch");
}

static int shade_args(ShadeArgs &a, const double *posed, const uint32_t *faces, const uint32_t *vf_offsets, const uint32_t *vf_corners, const double *light,
					  const double *ambient, const double *color, int C, int V, int n, int clockwise)
{
	if (!posed || !faces || !vf_offsets || !vf_corners || !light || !ambient || V <= 0 || n <= 0 || (color && (C < 1 || C > 3)))
		return fail("vertex_shade: bad arguments (one colour of 1 - 3 channels, or none)");
	a = ShadeArgs{posed, faces, vf_offsets, vf_corners, light, ambient, color, color ? C : 0, V, n, clockwise ? -1.0 : 1.0};
	return 0;
}

int deodr_hip_vertex_shade(const double *posed, const uint32_t *faces, const uint32_t *vf_offsets, const uint32_t *vf_corners, const double *light,
						   const double *ambient, const double *color, int C, double *luminosity, double *colors, int V, int n, int clockwise, void *stream)
{
	ShadeArgs a;
	if (shade_args(a, posed, faces, vf_offsets, vf_corners, light, ambient, color, C, V, n, clockwise))
		return 1;
	if ((!luminosity && !colors) || (colors && !color))
		return fail("vertex_shade: nothing to write, or colours asked for without a colour");
	hipLaunchKernelGGL(vertex_shade_kernel, dim3(fh_blocks((long long)V * GATHER_LANES), n), dim3(FH_BLOCK), 0, (hipStream_t)stream, a, luminosity, colors);
	return check_hip(hipGetLastError(), "vertex_shade launch");
}

int deodr_hip_vertex_shade_b(const double *posed, const uint32_t *faces, const uint32_t *vf_offsets, const uint32_t *vf_corners, const double *light,
							 const double *ambient, const double *color, int C, const double *luminosity_b, const double *colors_b, double *posed_b, double *out,
							 void *scratch, size_t scratch_bytes, int V, int n, int clockwise, void *stream)
{
	ShadeArgs a;
	if (shade_args(a, posed, faces, vf_offsets, vf_corners, light, ambient, color, C, V, n, clockwise))
		return 1;
	if ((!luminosity_b && !colors_b) || (colors_b && !color) || !posed_b || !out)
		return fail("vertex_shade_b: bad arguments");
	const Scratch sc = {scratch, scratch_bytes};
	if (!sc.holds(fit_scratch_need_shade_b(V, n)))
		return fail("vertex_shade_b: scratch too small (deodr_hip_fit_scratch_bytes)");
	hipStream_t st = (hipStream_t)stream;
	double *acc_b = sc.doubles(), *partials = acc_b + 3 * (size_t)n * V;
	hipLaunchKernelGGL(vertex_shade_b1_kernel, dim3(fh_blocks((long long)n * V * GATHER_LANES)), dim3(FH_BLOCK), 0, st, a, luminosity_b, colors_b, acc_b, out, partials,
					   sc.counter(FC_SHADE_B));
	hipLaunchKernelGGL(vertex_shade_b2_kernel, dim3(fh_blocks((long long)V * GATHER_LANES), n), dim3(FH_BLOCK), 0, st, a, (const double *)acc_b, posed_b);
	return check_hip(hipGetLastError(), "vertex_shade_b launch");
}

int deodr_hip_rigid_energy(const double *vertices, const double *vertices_ref, const uint32_t *m_offsets, const uint32_t *m_cols, const double *m_vals,
						   double cregu, double *gradient, double *energy, const double *data_energy, double data_weight, void *scratch, size_t scratch_bytes,
						   int V, void *stream)
{
	if (!vertices || !vertices_ref || !m_offsets || !m_cols || !m_vals || !gradient || !energy || V <= 0)
		return fail("rigid_energy: bad arguments");
	const Scratch sc = {scratch, scratch_bytes};
	if (!sc.holds(fit_scratch_need_rigid(V)))
		return fail("rigid_energy: scratch too small (deodr_hip_fit_scratch_bytes)");
	const RigidArgs a = {vertices, vertices_ref, m_offsets, m_cols, m_vals, cregu, gradient, energy, data_energy, data_weight, sc.doubles(), sc.counter(FC_RIGID), V};
	hipLaunchKernelGGL(rigid_energy_kernel, dim3(fh_blocks((long long)V * GATHER_LANES)), dim3(FH_BLOCK), 0, (hipStream_t)stream, a);
	return check_hip(hipGetLastError(), "rigid_energy launch");
}

int deodr_hip_fit_front(const double *ij, const uint32_t *faces, const uint32_t *edge_faces, uint8_t *flags, int T, const double *posed,
						const uint32_t *vf_offsets, const uint32_t *vf_corners, const double *light, const double *ambient, const double *color, int C,
						double *luminosity, double *colors, const double *vertices, const double *vertices_ref, const uint32_t *m_offsets, const uint32_t *m_cols,
						const double *m_vals, double cregu, double *gradient, double *energy, void *scratch, size_t scratch_bytes, int V, int n, int clockwise,
						void *stream)
{
	if (!faces || V <= 0 || n <= 0)
		return fail("fit_front: bad arguments");
	FrontArgs a;
	memset(&a, 0, sizeof a);
	a.V = V, a.clockwise = clockwise, a.faces = faces;
	if (flags)
	{
		if (!ij || !edge_faces || T <= 0)
			return fail("fit_front: silhouette flags need ij, edge_faces and the number of faces");
		a.ij = ij, a.edge_faces = edge_faces, a.flags = flags, a.T = T, a.sil_x = (unsigned)fh_blocks(T);
	}
	a.shade.n = n;
	if (luminosity || colors)
	{
		if (shade_args(a.shade, posed, faces, vf_offsets, vf_corners, light, ambient, color, C, V, n, clockwise))
			return 1;
		if (colors && !color)
			return fail("fit_front: colours asked for without a colour");
		a.lum_out = luminosity, a.colors_out = colors, a.shade_x = (unsigned)fh_blocks((long long)V * GATHER_LANES);
	}
	if (gradient)
	{
		if (!vertices || !vertices_ref || !m_offsets || !m_cols || !m_vals || !energy)
			return fail("fit_front: the rigid energy needs vertices, reference, the CSR of L^T L and energy[2]");
		const Scratch sc = {scratch, scratch_bytes};
		if (!sc.holds(fit_scratch_need_rigid(V)))
			return fail("fit_front: scratch too small (deodr_hip_fit_scratch_bytes)");
		a.rigid = RigidArgs{vertices, vertices_ref, m_offsets, m_cols, m_vals, cregu, gradient, energy, nullptr, 0.0, sc.doubles(), sc.counter(FC_RIGID), V};
		a.rigid_blocks = (unsigned)fh_blocks((long long)V * GATHER_LANES);
	}
	const unsigned blocks = a.rigid_blocks + (a.shade_x + a.sil_x) * (unsigned)n;
	if (!blocks)
		return fail("fit_front: nothing to do");
	hipLaunchKernelGGL(fit_front_kernel, dim3(blocks), dim3(FH_BLOCK), 0, (hipStream_t)stream, a);
	return check_hip(hipGetLastError(), "fit_front launch");
}

static int l2_loss_impl(const void *image, const void *obs, int pixel_dtype, size_t count, double *out, void *scratch, size_t scratch_bytes, void *stream,
					   int clamp, double clamp_lo, double clamp_hi, const void *weights, int nb_colors)
{ // weights != NULL: one weight per pixel of nb_colors channels (count = pixels * nb_colors)
	if (!image || !obs || !out || count == 0 || !elem_bytes(pixel_dtype))
		return fail("l2_loss: bad arguments");
	const Scratch sc = {scratch, scratch_bytes};
	if (!sc.holds(fit_scratch_need_l2()))
		return fail("l2_loss: scratch too small (deodr_hip_fit_scratch_bytes)");
	if (((uintptr_t)image | (uintptr_t)obs) & 31)
		return fail("l2_loss: image and obs must be 32-byte aligned");
	const dim3 grid(capped_blocks(count, FH_BLOCK * 32, L2_BLOCKS));
	double *partials = sc.doubles();
	unsigned *counter = sc.counter(FC_L2);
	with_pixel_type(pixel_dtype == DEODR_HIP_F64, [&](auto pix) {
		using PixT = decltype(pix);
		if (weights)
			hipLaunchKernelGGL(l2_loss_weighted_kernel<PixT>, grid, dim3(FH_BLOCK), 0, (hipStream_t)stream, (const PixT *)image, (const PixT *)obs,
							   (const PixT *)weights, nb_colors, count, out, partials, counter, clamp, clamp_lo, clamp_hi);
		else
			hipLaunchKernelGGL(l2_loss_kernel<PixT>, grid, dim3(FH_BLOCK), 0, (hipStream_t)stream, (const PixT *)image, (const PixT *)obs, count, out, partials,
							   counter, clamp, clamp_lo, clamp_hi);
	});
	return check_hip(hipGetLastError(), "l2_loss launch");
}

int deodr_hip_l2_loss(const void *image, const void *obs, int pixel_dtype, size_t count, double *out, void *scratch, size_t scratch_bytes, void *stream)
{
	return l2_loss_impl(image, obs, pixel_dtype, count, out, scratch, scratch_bytes, stream, 0, 0.0, 0.0);
}

int deodr_hip_depth_residual(const void *image, int pixel_dtype, const double *obs, double max_depth, size_t count, double *depth, double *diff, void *image_b,
							 double *loss, void *scratch, size_t scratch_bytes, void *stream)
{
	if (!image || !obs || !depth || !diff || !image_b || !loss || count == 0 || !elem_bytes(pixel_dtype))
		return fail("depth_residual: bad arguments");
	const Scratch sc = {scratch, scratch_bytes};
	if (!sc.holds(fit_scratch_need_l2()))
		return fail("depth_residual: scratch too small (deodr_hip_fit_scratch_bytes)");
	const dim3 grid(capped_blocks(count, FH_BLOCK * 4, L2_BLOCKS));
	double *partials = sc.doubles();
	unsigned *counter = sc.counter(FC_L2);
	with_pixel_type(pixel_dtype == DEODR_HIP_F64, [&](auto pix) {
		using PixT = decltype(pix);
		hipLaunchKernelGGL(depth_residual_kernel<PixT>, grid, dim3(FH_BLOCK), 0, (hipStream_t)stream, (const PixT *)image, obs, max_depth, count, depth, diff,
						   (PixT *)image_b, loss, partials, counter);
	});
	return check_hip(hipGetLastError(), "depth_residual launch");
}

// ---- texture estimation (include/deodr_hip_texture.h, kernels in dr_texfit.h)

int deodr_hip_texture_abi_version(void) { return DEODR_HIP_TEXTURE_ABI_VERSION; }

static const char *texture_dims(int Ht, int Wt, int C, int pixel_dtype)
{ // -> NULL (the texture has Ht * Wt * C <= 2^30 elements), or why not
	if (Ht < 2 || Wt < 2)
		return "texture must be at least 2 x 2";
	if (C < 1 || C > DEODR_HIP_MAX_COLORS)
		return "nb_colors out of range";
	if (!elem_bytes(pixel_dtype))
		return "unknown dtype tag";
	if ((unsigned long long)Ht * (unsigned long long)Wt * (unsigned long long)C > (1ull << 30))
		return "texture larger than 2^30 elements";
	return NULL;
}

size_t deodr_hip_texture_scratch_bytes(int Ht, int Wt, int C) { return texture_dims(Ht, Wt, C, DEODR_HIP_F32) ? 0 : scratch_need(TEX_SMOOTH_BLOCKS); }

int deodr_hip_texture_smoothness(const void *texture, int Ht, int Wt, int C, int pixel_dtype, double weight, void *gradient, double *energy, void *scratch,
								 size_t scratch_bytes, void *stream)
{
	if (!texture || !gradient || !energy)
		return fail("texture_smoothness: texture, gradient or energy == NULL");
	if (const char *why = texture_dims(Ht, Wt, C, pixel_dtype))
		return fail(why);
	const Scratch sc = {scratch, scratch_bytes};
	if (!sc.holds(deodr_hip_texture_scratch_bytes(Ht, Wt, C)))
		return fail("texture_smoothness: scratch too small (deodr_hip_texture_scratch_bytes)");
	const int N = Ht * Wt * C;
	const size_t elem = elem_bytes(pixel_dtype);
	if (ranges_overlap(texture, (size_t)N * elem, gradient, (size_t)N * elem))
		return fail("texture_smoothness: gradient must not overlap texture");
	if ((((uintptr_t)texture | (uintptr_t)gradient) & (elem - 1)) || ((uintptr_t)scratch & 7))
		return fail("texture_smoothness: misaligned pointer");
	TexSmoothArgs a;
	a.texture = texture, a.gradient = gradient, a.energy = energy;
	a.counter = sc.counter(0), a.partials = sc.doubles();
	a.weight = weight, a.Ht = Ht, a.R = Wt * C, a.C = C, a.N = N;
	const dim3 grid(capped_blocks(N / (16 / elem), FH_BLOCK, TEX_SMOOTH_BLOCKS)); // (16-byte pieces)
	with_dtype(pixel_dtype, [&](auto pix) { hipLaunchKernelGGL(texture_smoothness_kernel<decltype(pix)>, grid, dim3(FH_BLOCK), 0, (hipStream_t)stream, a); });
	return check_hip(hipGetLastError(), "texture_smoothness launch");
}

int deodr_hip_texture_step(void *texture, void *speed, const void *gradient, int Ht, int Wt, int C, int pixel_dtype, double factor, double step_max,
						   double inertia, double damping, int clamp, double clamp_lo, double clamp_hi, void *stream)
{
	if (!texture || !speed || !gradient)
		return fail("texture_step: texture, speed or gradient == NULL");
	if (const char *why = texture_dims(Ht, Wt, C, pixel_dtype))
		return fail(why);
	const int N = Ht * Wt * C;
	const size_t elem = elem_bytes(pixel_dtype), bytes = (size_t)N * elem;
	if (ranges_overlap(texture, bytes, gradient, bytes))
		return fail("texture_step: gradient must not overlap texture");
	if (ranges_overlap(texture, bytes, speed, bytes) || ranges_overlap(speed, bytes, gradient, bytes))
		return fail("texture_step: speed must not overlap texture or gradient");
	if (((uintptr_t)texture | (uintptr_t)speed | (uintptr_t)gradient) & (elem - 1))
		return fail("texture_step: misaligned pointer");
	if (clamp && !(clamp_lo <= clamp_hi))
		return fail("texture_step: clamp_lo > clamp_hi");
	TexStepArgs a;
	a.texture = texture, a.speed = speed, a.gradient = gradient;
	a.factor = factor, a.step_max = step_max, a.inertia = inertia, a.damping = damping, a.clamp_lo = clamp_lo, a.clamp_hi = clamp_hi;
	a.clamp = clamp != 0, a.N = N;
	const dim3 grid(capped_blocks(N / (16 / elem), FH_BLOCK, TEX_STEP_BLOCKS)); // (16-byte pieces)
	with_dtype(pixel_dtype, [&](auto pix) { hipLaunchKernelGGL(texture_step_kernel<decltype(pix)>, grid, dim3(FH_BLOCK), 0, (hipStream_t)stream, a); });
	return check_hip(hipGetLastError(), "texture_step launch");
}

// ---- Loop subdivision (include/deodr_hip_subdiv.h, kernel in dr_subdiv.h)

int deodr_hip_subdiv_abi_version(void) { return DEODR_HIP_SUBDIV_ABI_VERSION; }

int deodr_hip_subdiv_lanes(int n_rows, uint32_t nnz) { return n_rows > 0 ? subdiv_lanes(n_rows, nnz) : 0; }

int deodr_hip_subdiv_apply(const uint32_t *offsets, const uint32_t *cols, const double *vals, int n_rows, int n_cols, uint32_t nnz, const void *x, void *y,
						   int batch, int D, int dtype, int accumulate, void *stream)
{
	if (!offsets || !cols || !vals || !x || !y)
		return fail("subdiv_apply: offsets, cols, vals, x or y == NULL");
	if (n_rows <= 0 || n_cols <= 0 || nnz == 0)
		return fail("subdiv_apply: n_rows, n_cols and nnz must be positive");
	if (batch <= 0 || batch > 65535)
		return fail("subdiv_apply: batch must be in 1 .. 65535");
	if (D < 1 || D > DEODR_HIP_MAX_COLORS)
		return fail("subdiv_apply: D out of range");
	const size_t elem = elem_bytes(dtype);
	if (!elem)
		return fail("unknown dtype tag");
	if (ranges_overlap(x, (size_t)batch * (size_t)n_cols * (size_t)D * elem, y, (size_t)batch * (size_t)n_rows * (size_t)D * elem))
		return fail("subdiv_apply: y must not overlap x");
	if ((((uintptr_t)x | (uintptr_t)y) & (elem - 1)) || ((uintptr_t)offsets & 3) || ((uintptr_t)cols & 3) || ((uintptr_t)vals & 7))
		return fail("subdiv_apply: misaligned pointer");
	const int lanes = subdiv_lanes(n_rows, nnz);
	// (n_rows < 2^31 with 8 lanes, n_rows <= nnz / 32 < 2^27 with 64: at most 2^26 workgroups)
	const unsigned long long blocks = ((unsigned long long)n_rows * (unsigned)lanes + FH_BLOCK - 1) / FH_BLOCK;
	SubdivArgs a;
	a.offsets = offsets, a.cols = cols, a.vals = vals, a.x = x, a.y = y;
	a.n_rows = n_rows, a.n_cols = n_cols, a.D = D, a.accumulate = accumulate != 0;
	const dim3 grid((unsigned)blocks, (unsigned)batch);
	with_constant<SUBDIV_LANES_SHORT, SUBDIV_LANES_LONG>(lanes == SUBDIV_LANES_LONG, [&](auto row_lanes) {
		with_dtype(dtype, [&](auto elem_type) { subdiv_launch_d<decltype(elem_type), decltype(row_lanes)::value>(a, grid, (hipStream_t)stream); });
	});
	return check_hip(hipGetLastError(), "subdiv_apply launch");
}

// ---- linear bases (include/deodr_hip_basis.h, kernels in dr_basis.h)

int deodr_hip_basis_abi_version(void) { return DEODR_HIP_BASIS_ABI_VERSION; }

static const char *basis_dims(int K, int N, int batch)
{ // -> NULL, or which limit of the header the dimensions break
	if (K < 1 || K > BASIS_MAX_K)
		return "K must be in 1 .. 1024";
	if (batch < 1 || batch > BASIS_MAX_BATCH)
		return "batch must be in 1 .. 64";
	if (N < 1 || N > BASIS_MAX_N)
		return "N must be in 1 .. 2^30";
	if ((unsigned long long)K * (unsigned long long)N > 0x7fffffffull)
		return "K * N must not exceed 2^31 - 1";
	return NULL;
}

int deodr_hip_basis_segments(int K, int N) { return basis_dims(K, N, 1) ? 0 : basis_segments(K, N); }

static size_t basis_counter_bytes(int K, int batch) { return (4 * (size_t)basis_chunks(batch) * (size_t)basis_row_tiles(K) + 63) / 64 * 64; }

size_t deodr_hip_basis_scratch_bytes(int K, int N, int batch)
{
	if (basis_dims(K, N, batch))
		return 0;
	return basis_counter_bytes(K, batch) +
		   sizeof(double) * (size_t)basis_chunks(batch) * (size_t)basis_row_tiles(K) * (size_t)basis_segments(K, N) * BASIS_ROW_TILE * BASIS_CHUNK;
}

int deodr_hip_basis_apply(const void *basis, const void *mean, const double *coeffs, int K, int N, int batch, int basis_dtype, void *y, int y_dtype,
						  void *stream)
{
	const char *what = "basis_apply";
	if (!basis || !coeffs || !y)
		return fail(what, "basis, coeffs or y == NULL");
	if (const char *why = basis_dims(K, N, batch))
		return fail(what, why);
	const size_t be = elem_bytes(basis_dtype), ye = elem_bytes(y_dtype);
	if (!be || !ye)
		return fail("unknown dtype tag");
	if ((((uintptr_t)basis | (uintptr_t)mean) & (be - 1)) || ((uintptr_t)y & (ye - 1)) || ((uintptr_t)coeffs & 7))
		return fail(what, "misaligned pointer");
	const size_t y_bytes = (size_t)batch * (size_t)N * ye;
	if (ranges_overlap(y, y_bytes, basis, (size_t)K * (size_t)N * be) || ranges_overlap(y, y_bytes, mean, (size_t)N * be) ||
		ranges_overlap(y, y_bytes, coeffs, (size_t)batch * (size_t)K * 8))
		return fail(what, "y must not overlap basis, mean or coeffs");
	BasisArgs a = {};
	a.basis = basis, a.mean = mean, a.coeffs = coeffs, a.y = y, a.K = K, a.N = N, a.batch = batch;
	const int pieces = N / (int)(16 / be), blocks = (pieces + FH_BLOCK - 1) / FH_BLOCK;
	const dim3 grid((unsigned)(blocks < 1 ? 1 : blocks), (unsigned)basis_chunks(batch)), block(FH_BLOCK);
	const hipStream_t st = (hipStream_t)stream;
	with_constant<1, BASIS_CHUNK>(batch > 1, [&](auto chunk) {
		with_dtype(basis_dtype, [&](auto b) {
			with_dtype(y_dtype, [&](auto out) { hipLaunchKernelGGL((basis_apply_kernel<decltype(b), decltype(out), decltype(chunk)::value>), grid, block, 0, st, a); });
		});
	});
	return check_hip(hipGetLastError(), "basis_apply launch");
}

int deodr_hip_basis_apply_b(const void *basis, const void *g, int g_dtype, int K, int N, int batch, int basis_dtype, double *coeffs_b, int accumulate,
							void *scratch, size_t scratch_bytes, void *stream)
{
	const char *what = "basis_apply_b";
	if (!basis || !g || !coeffs_b || !scratch)
		return fail(what, "basis, g, coeffs_b or scratch == NULL");
	if (const char *why = basis_dims(K, N, batch))
		return fail(what, why);
	const size_t be = elem_bytes(basis_dtype), ge = elem_bytes(g_dtype);
	if (!be || !ge)
		return fail("unknown dtype tag");
	if (((uintptr_t)basis & (be - 1)) || ((uintptr_t)g & (ge - 1)) || (((uintptr_t)coeffs_b | (uintptr_t)scratch) & 7))
		return fail(what, "misaligned pointer");
	const size_t c_bytes = (size_t)batch * (size_t)K * 8;
	if (ranges_overlap(coeffs_b, c_bytes, basis, (size_t)K * (size_t)N * be) || ranges_overlap(coeffs_b, c_bytes, g, (size_t)batch * (size_t)N * ge))
		return fail(what, "coeffs_b must not overlap basis or g");
	if (scratch_bytes < deodr_hip_basis_scratch_bytes(K, N, batch))
		return fail(what, "scratch too small (deodr_hip_basis_scratch_bytes)");
	BasisArgs a = {};
	a.basis = basis, a.g = g, a.coeffs_b = coeffs_b, a.K = K, a.N = N, a.batch = batch, a.S = basis_segments(K, N), a.accumulate = accumulate != 0;
	a.counters = (unsigned *)scratch, a.partials = (double *)((char *)scratch + basis_counter_bytes(K, batch));
	const dim3 grid((unsigned)a.S, (unsigned)basis_row_tiles(K), (unsigned)basis_chunks(batch)), block(FH_BLOCK);
	const hipStream_t st = (hipStream_t)stream;
	with_constant<1, BASIS_CHUNK>(batch > 1, [&](auto chunk) {
		with_dtype(basis_dtype, [&](auto b) {
			with_dtype(g_dtype, [&](auto grad) { hipLaunchKernelGGL((basis_apply_b_kernel<decltype(b), decltype(grad), decltype(chunk)::value>), grid, block, 0, st, a); });
		});
	});
	return check_hip(hipGetLastError(), "basis_apply_b launch");
}

// ---- camera calibration (include/deodr_hip_camera.h, kernels in dr_camera.h)

int deodr_hip_camera_abi_version(void) { return DEODR_HIP_CAMERA_ABI_VERSION; }

static const char *camera_dims(int V, int n)
{ // -> NULL, or which limit of the header the dimensions break
	if (n < 1 || n > FIT_MAX_VIEWS)
		return "n must be in 1 .. 64";
	if (V < 1 || V > CAMERA_MAX_VERTICES)
		return "V must be in 1 .. 2^24";
	return NULL;
}

int deodr_hip_camera_blocks(int V, int n) { return camera_dims(V, n) ? 0 : camera_blocks(V, n); }

static size_t camera_counter_bytes(int n) { return (2 * 4 * (size_t)n + 63) / 64 * 64; } // two counter words per view

size_t deodr_hip_camera_scratch_bytes(int V, int n)
{
	if (camera_dims(V, n))
		return 0;
	return camera_counter_bytes(n) + sizeof(double) * (size_t)n * (size_t)camera_blocks(V, n) * CAMERA_SUMS;
}

int deodr_hip_camera_project_b(const double *points, const double *extrinsic, const double *intrinsic, const double *distortion, const double *ij_b,
							   const double *depths_b, double *points_b, double *extrinsic_b, double *intrinsic_b, double *distortion_b, int V, int n,
							   int accumulate, void *scratch, size_t scratch_bytes, void *stream)
{
	const char *what = "camera_project_b";
	if (!points || !extrinsic || !intrinsic || !ij_b || !extrinsic_b || !intrinsic_b || !scratch)
		return fail(what, "points, extrinsic, intrinsic, ij_b, extrinsic_b, intrinsic_b or scratch == NULL");
	if ((distortion == nullptr) != (distortion_b == nullptr))
		return fail(what, "distortion and distortion_b go together");
	if (const char *why = camera_dims(V, n))
		return fail(what, why);
	const void *const all[] = {points, extrinsic, intrinsic, distortion, ij_b, depths_b, points_b, extrinsic_b, intrinsic_b, distortion_b, scratch};
	if (any_misaligned(all, 8))
		return fail(what, "misaligned pointer");
	if (scratch_bytes < deodr_hip_camera_scratch_bytes(V, n))
		return fail(what, "scratch too small (deodr_hip_camera_scratch_bytes)");
	const size_t nv = (size_t)n * (size_t)V * 8, nb = (size_t)n * 8;
	const Range outputs[] = {{points_b, 3 * nv}, {extrinsic_b, 12 * nb}, {intrinsic_b, 9 * nb}, {distortion_b, 5 * nb}};
	const Range inputs[] = {{points, 3 * nv}, {extrinsic, 12 * nb}, {intrinsic, 9 * nb}, {distortion, 5 * nb}, {ij_b, 2 * nv}, {depths_b, nv}};
	if (any_overlap(outputs, inputs))
		return fail(what, "an output must not overlap an input");
	CameraProjectBArgs a = {};
	a.points = points, a.extrinsic = extrinsic, a.intrinsic = intrinsic, a.distortion = distortion, a.ij_b = ij_b, a.depths_b = depths_b;
	a.points_b = points_b, a.extrinsic_b = extrinsic_b, a.intrinsic_b = intrinsic_b, a.distortion_b = distortion_b;
	a.counters = (unsigned *)scratch, a.partials = (double *)((char *)scratch + camera_counter_bytes(n));
	a.V = V, a.accumulate = accumulate != 0;
	hipLaunchKernelGGL(camera_project_b_kernel, dim3((unsigned)camera_blocks(V, n), (unsigned)n), dim3(FH_BLOCK), 0, (hipStream_t)stream, a);
	return check_hip(hipGetLastError(), "camera_project_b launch");
}

int deodr_hip_camera_assemble(const double *quaternions, const double *translations, const double *focal, const double *center,
							  const double *distortion_in, int shared, double *extrinsic, double *intrinsic, double *distortion_out, int n, void *stream)
{
	const char *what = "camera_assemble";
	if (!quaternions || !translations || !focal || !center || !extrinsic || !intrinsic)
		return fail(what, "quaternions, translations, focal, center, extrinsic or intrinsic == NULL");
	if ((distortion_in == nullptr) != (distortion_out == nullptr))
		return fail(what, "distortion_in and distortion_out go together");
	if (const char *why = camera_dims(1, n))
		return fail(what, why);
	const void *const all[] = {quaternions, translations, focal, center, distortion_in, extrinsic, intrinsic, distortion_out};
	if (any_misaligned(all, 8))
		return fail(what, "misaligned pointer");
	const size_t nb = (size_t)n * 8, ni = shared ? 8 : nb;
	const Range outputs[] = {{extrinsic, 12 * nb}, {intrinsic, 9 * nb}, {distortion_out, 5 * nb}};
	const Range inputs[] = {{quaternions, 4 * nb}, {translations, 3 * nb}, {focal, 2 * ni}, {center, 2 * ni}, {distortion_in, 5 * ni}};
	if (any_overlap(outputs, inputs))
		return fail(what, "an output must not overlap an input");
	CameraAssembleArgs a = {};
	a.quaternions = quaternions, a.translations = translations, a.focal = focal, a.center = center, a.distortion_in = distortion_in;
	a.extrinsic = extrinsic, a.intrinsic = intrinsic, a.distortion_out = distortion_out, a.shared = shared != 0, a.n = n;
	hipLaunchKernelGGL(camera_assemble_kernel, dim3(1), dim3(FIT_MAX_VIEWS), 0, (hipStream_t)stream, a);
	return check_hip(hipGetLastError(), "camera_assemble launch");
}

int deodr_hip_camera_assemble_b(const double *quaternions, const double *extrinsic_b, const double *intrinsic_b, const double *distortion_b, int shared,
								double *quaternions_b, double *translations_b, double *focal_b, double *center_b, double *distortion_in_b, int n,
								void *stream)
{
	const char *what = "camera_assemble_b";
	if (!quaternions || !extrinsic_b || !intrinsic_b || !quaternions_b || !translations_b || !focal_b || !center_b)
		return fail(what, "quaternions, extrinsic_b, intrinsic_b, quaternions_b, translations_b, focal_b or center_b == NULL");
	if ((distortion_b == nullptr) != (distortion_in_b == nullptr))
		return fail(what, "distortion_b and distortion_in_b go together");
	if (const char *why = camera_dims(1, n))
		return fail(what, why);
	const void *const all[] = {quaternions, extrinsic_b, intrinsic_b, distortion_b, quaternions_b, translations_b, focal_b, center_b, distortion_in_b};
	if (any_misaligned(all, 8))
		return fail(what, "misaligned pointer");
	const size_t nb = (size_t)n * 8, ni = shared ? 8 : nb;
	const Range outputs[] = {{quaternions_b, 4 * nb}, {translations_b, 3 * nb}, {focal_b, 2 * ni}, {center_b, 2 * ni}, {distortion_in_b, 5 * ni}};
	const Range inputs[] = {{quaternions, 4 * nb}, {extrinsic_b, 12 * nb}, {intrinsic_b, 9 * nb}, {distortion_b, 5 * nb}};
	if (any_overlap(outputs, inputs))
		return fail(what, "an output must not overlap an input");
	CameraAssembleBArgs a = {};
	a.quaternions = quaternions, a.extrinsic_b = extrinsic_b, a.intrinsic_b = intrinsic_b, a.distortion_b = distortion_b;
	a.quaternions_b = quaternions_b, a.translations_b = translations_b, a.focal_b = focal_b, a.center_b = center_b, a.distortion_in_b = distortion_in_b;
	a.shared = shared != 0, a.n = n;
	hipLaunchKernelGGL(camera_assemble_b_kernel, dim3(1), dim3(FIT_MAX_VIEWS), 0, (hipStream_t)stream, a);
	return check_hip(hipGetLastError(), "camera_assemble_b launch");
}

// ---- spherical-harmonic lighting (include/deodr_hip_lighting.h, kernels in dr_lighting.h)

int deodr_hip_lighting_abi_version(void) { return DEODR_HIP_LIGHTING_ABI_VERSION; }

static const char *sh_dims(int V, int n, int C, int S)
{ // -> NULL, or which limit of the header the dimensions break
	if (n < 1 || n > FIT_MAX_VIEWS)
		return "n must be in 1 .. 64";
	if (V < 1 || V > SH_MAX_VERTICES)
		return "V must be in 1 .. 2^24";
	if (C < 1 || C > 3)
		return "C must be in 1 .. 3";
	if (S != 1 && S != C)
		return "S must be 1 or C";
	return NULL;
}

int deodr_hip_sh_blocks(int V, int n) { return sh_dims(V, n, 1, 1) ? 0 : sh_blocks(V, n); }

size_t deodr_hip_sh_scratch_bytes(int V, int n, int C)
{
	if (sh_dims(V, n, C, 1))
		return 0;
	return scratch_need((size_t)n * V * (3 + (size_t)C) + (size_t)sh_blocks(V, n) * SH_SUMS);
}

// what the two entry points ask of their common arguments -> 0 and `a`, or the refusal
static int sh_args(const char *what, SHArgs &a, const double *posed, const uint32_t *faces, const uint32_t *vf_offsets, const uint32_t *vf_corners,
				   const double *sh, int S, const double *albedo, int albedo_per_vertex, int C, const void *lum, const void *colors, int V, int n, int clockwise)
{
	if (!posed || !faces || !vf_offsets || !vf_corners || !sh)
		return fail(what, "posed, faces, vf_offsets, vf_corners or sh == NULL");
	if (const char *why = sh_dims(V, n, C, S))
		return fail(what, why);
	if (!lum && !colors)
		return fail(what, "no output requested: neither luminosity nor colors (forward), neither of their adjoints (backward)");
	if ((albedo == nullptr) != (colors == nullptr))
		return fail(what, "albedo and colors go together");
	if (lum && S != 1)
		return fail(what, "luminosity needs S = 1");
	a.mesh = ShadeArgs{posed, faces, vf_offsets, vf_corners, nullptr, nullptr, nullptr, albedo ? C : 0, V, n, clockwise ? -1.0 : 1.0};
	a.sh = sh, a.albedo = albedo, a.S = S, a.per_vertex = albedo_per_vertex != 0;
	return 0;
}

int deodr_hip_sh_shade(const double *posed, const uint32_t *faces, const uint32_t *vf_offsets, const uint32_t *vf_corners, const double *sh, int S,
					   const double *albedo, int albedo_per_vertex, int C, double *luminosity, double *colors, int V, int n, int clockwise, void *stream)
{
	const char *what = "sh_shade";
	SHArgs a;
	if (sh_args(what, a, posed, faces, vf_offsets, vf_corners, sh, S, albedo, albedo_per_vertex, C, luminosity, colors, V, n, clockwise))
		return 1;
	const void *const doubles[] = {posed, sh, albedo, luminosity, colors};
	const void *const words[] = {faces, vf_offsets, vf_corners};
	if (any_misaligned(doubles, 8) || any_misaligned(words, 4))
		return fail(what, "misaligned pointer");
	const size_t nv = (size_t)n * (size_t)V * 8;
	const Range outputs[] = {{luminosity, nv}, {colors, nv * C}};
	const Range inputs[] = {{posed, 3 * nv}, {faces, 12}, {vf_offsets, 4 * ((size_t)V + 1)}, {vf_corners, 12}, {sh, 72 * (size_t)S},
							{albedo, 8 * (size_t)C * (a.per_vertex ? (size_t)V : 1)}};
	if (any_overlap(outputs, inputs) || any_overlap(outputs))
		return fail(what, "an output must not overlap an input or the other output");
	hipLaunchKernelGGL(sh_shade_kernel, dim3(fh_blocks((long long)V * GATHER_LANES), n), dim3(FH_BLOCK), 0, (hipStream_t)stream, a, luminosity, colors);
	return check_hip(hipGetLastError(), "sh_shade launch");
}

int deodr_hip_sh_shade_b(const double *posed, const uint32_t *faces, const uint32_t *vf_offsets, const uint32_t *vf_corners, const double *sh, int S,
						 const double *albedo, int albedo_per_vertex, int C, const double *luminosity_b, const double *colors_b, double *posed_b,
						 double *sh_b, double *albedo_b, int accumulate, void *scratch, size_t scratch_bytes, int V, int n, int clockwise, void *stream)
{
	const char *what = "sh_shade_b";
	SHArgs a;
	if (sh_args(what, a, posed, faces, vf_offsets, vf_corners, sh, S, albedo, albedo_per_vertex, C, luminosity_b, colors_b, V, n, clockwise))
		return 1;
	if (!scratch)
		return fail(what, "scratch == NULL");
	if (!posed_b && !sh_b && !albedo_b)
		return fail(what, "no output requested (posed_b, sh_b, albedo_b)");
	if (albedo_b && !albedo)
		return fail(what, "albedo_b without albedo");
	const void *const doubles[] = {posed, sh, albedo, luminosity_b, colors_b, posed_b, sh_b, albedo_b, scratch};
	const void *const words[] = {faces, vf_offsets, vf_corners};
	if (any_misaligned(doubles, 8) || any_misaligned(words, 4))
		return fail(what, "misaligned pointer");
	const Scratch sc = {scratch, scratch_bytes};
	if (!sc.holds(deodr_hip_sh_scratch_bytes(V, n, C)))
		return fail(what, "scratch too small (deodr_hip_sh_scratch_bytes)");
	const size_t nv = (size_t)n * (size_t)V * 8, alb = 8 * (size_t)C * (a.per_vertex ? (size_t)V : 1);
	const Range outputs[] = {{posed_b, 3 * nv}, {sh_b, 72 * (size_t)S}, {albedo_b, alb}, {scratch, scratch_bytes}};
	const Range inputs[] = {{posed, 3 * nv}, {faces, 12}, {vf_offsets, 4 * ((size_t)V + 1)}, {vf_corners, 12}, {sh, 72 * (size_t)S}, {albedo, alb},
							{luminosity_b, nv}, {colors_b, nv * C}};
	if (any_overlap(outputs, inputs) || any_overlap(outputs))
		return fail(what, "an output must not overlap an input, the scratch or another output");
	hipStream_t st = (hipStream_t)stream;
	const unsigned blocks = (unsigned)sh_blocks(V, n);
	SHBackArgs o = {};
	o.lum_b = luminosity_b, o.colors_b = colors_b, o.accumulate = accumulate != 0;
	o.acc_b = sc.doubles();
	double *products = o.acc_b + 3 * (size_t)n * V;
	o.partials = products + (size_t)n * V * C;
	o.counters = sc.counter(0);
	o.sh_b = sh_b;
	const bool vertex_albedo_b = a.per_vertex && albedo_b;
	o.albedo_b = a.per_vertex ? nullptr : albedo_b;
	// (several views of a per-vertex albedo: the products colors_b E are left in the scratch whether or not albedo_b is asked for -- the header's
	// "scratch after the call" -- so that a caller with a sum over the views of its own in a later launch needs no launch for it here)
	o.products = a.per_vertex && colors_b && n > 1 ? products : nullptr;
	o.albedo_direct = vertex_albedo_b && n == 1 ? albedo_b : nullptr;
	hipLaunchKernelGGL(sh_shade_b1_kernel, dim3(blocks), dim3(FH_BLOCK), 0, st, a, o);
	if (o.products && albedo_b)
		hipLaunchKernelGGL(sh_albedo_sum_kernel, dim3(fh_blocks((long long)V * C)), dim3(FH_BLOCK), 0, st, (const double *)products, albedo_b, (size_t)V * C, n,
						   o.accumulate);
	if (posed_b)
		hipLaunchKernelGGL(vertex_shade_b2_kernel, dim3(fh_blocks((long long)V * GATHER_LANES), n), dim3(FH_BLOCK), 0, st, a.mesh, (const double *)o.acc_b, posed_b);
	return check_hip(hipGetLastError(), "sh_shade_b launch");
}

// ---- linear blend skinning (include/deodr_hip_skinning.h, kernels in dr_skinning.h)

int deodr_hip_skinning_abi_version(void) { return DEODR_HIP_SKINNING_ABI_VERSION; }

static const char *skin_dims(int V, int J, int K, int n)
{ // -> NULL, or which limit of the header the dimensions break
	if (n < 1 || n > FIT_MAX_VIEWS)
		return "n must be in 1 .. 64";
	if (J < 1 || J > SKIN_MAX_JOINTS)
		return "J must be in 1 .. 256";
	if (K < 1 || K > SKIN_MAX_INFLUENCES)
		return "K must be in 1 .. 8";
	if (V < 1 || V > SKIN_MAX_VERTICES)
		return "V must be in 1 .. 2^24";
	return NULL;
}

size_t deodr_hip_skin_scratch_bytes(int V, int J, int K, int n) { return skin_dims(V, J, K, n) ? 0 : scratch_need((size_t)n * J * SKIN_CHAIN_B); }

int deodr_hip_skin_apply(const double *vertices, const double *joints, const uint32_t *parents, const double *quaternions, const uint32_t *indices,
						 const double *weights, double *world, double *posed, int V, int J, int K, int n, void *stream)
{
	const char *what = "skin_apply";
	if (!vertices || !joints || !parents || !quaternions || !indices || !weights || !world || !posed)
		return fail(what, "vertices, joints, parents, quaternions, indices, weights, world or posed == NULL");
	if (const char *why = skin_dims(V, J, K, n))
		return fail(what, why);
	const void *const doubles[] = {vertices, joints, quaternions, weights, world, posed};
	const void *const words[] = {parents, indices};
	if (any_misaligned(doubles, 8) || any_misaligned(words, 4))
		return fail(what, "misaligned pointer");
	const size_t v3 = 24 * (size_t)V, nj = (size_t)n * J, vk = (size_t)V * K;
	const Range outputs[] = {{world, 8 * SKIN_WORLD * nj}, {posed, n * v3}};
	const Range inputs[] = {{vertices, v3}, {joints, 24 * (size_t)J}, {parents, 4 * (size_t)J}, {quaternions, 32 * nj}, {indices, 4 * vk}, {weights, 8 * vk}};
	if (any_overlap(outputs, inputs) || any_overlap(outputs))
		return fail(what, "an output must not overlap an input or the other output");
	const SkinArgs a = {vertices, joints, quaternions, parents, indices, weights, V, J, K, n};
	const hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(skin_chain_kernel, dim3(1), dim3(FIT_MAX_VIEWS), 0, st, a, world);
	hipLaunchKernelGGL(skin_apply_kernel, dim3(fh_blocks((long long)V * GATHER_LANES), n), dim3(FH_BLOCK), 0, st, a, (const double *)world, posed);
	return check_hip(hipGetLastError(), "skin_apply launch");
}

int deodr_hip_skin_apply_b(const double *vertices, const double *joints, const uint32_t *parents, const double *quaternions, const uint32_t *indices,
						   const double *weights, const double *world, const double *posed_b, const uint32_t *joint_offsets,
						   const uint32_t *joint_slots, int nnz, double *vertices_b, double *quaternions_b, double *joints_b, void *scratch,
						   size_t scratch_bytes, int V, int J, int K, int n, void *stream)
{
	const char *what = "skin_apply_b";
	if (!vertices || !joints || !parents || !quaternions || !indices || !weights || !world || !posed_b || !joint_offsets || !joint_slots || !scratch)
		return fail(what, "vertices, joints, parents, quaternions, indices, weights, world, posed_b, joint_offsets, joint_slots or scratch == NULL");
	if (!vertices_b && !quaternions_b && !joints_b)
		return fail(what, "no output requested (vertices_b, quaternions_b, joints_b)");
	if (const char *why = skin_dims(V, J, K, n))
		return fail(what, why);
	if (nnz < 0 || (long long)nnz > (long long)V * K)
		return fail(what, "nnz must be in 0 .. V K");
	const void *const doubles[] = {vertices, joints, quaternions, weights, world, posed_b, vertices_b, quaternions_b, joints_b, scratch};
	const void *const words[] = {parents, indices, joint_offsets, joint_slots};
	if (any_misaligned(doubles, 8) || any_misaligned(words, 4))
		return fail(what, "misaligned pointer");
	const Scratch sc = {scratch, scratch_bytes};
	if (!sc.holds(deodr_hip_skin_scratch_bytes(V, J, K, n)))
		return fail(what, "scratch too small (deodr_hip_skin_scratch_bytes)");
	const size_t v3 = 24 * (size_t)V, nj = (size_t)n * J, vk = (size_t)V * K;
	const Range outputs[] = {{vertices_b, v3}, {quaternions_b, 32 * nj}, {joints_b, 24 * (size_t)J}, {scratch, scratch_bytes}};
	const Range inputs[] = {{vertices, v3}, {joints, 24 * (size_t)J}, {parents, 4 * (size_t)J}, {quaternions, 32 * nj}, {indices, 4 * vk}, {weights, 8 * vk},
							{world, 8 * SKIN_WORLD * nj}, {posed_b, n * v3}, {joint_offsets, 4 * ((size_t)J + 1)}, {joint_slots, 4 * (size_t)nnz}};
	if (any_overlap(outputs, inputs) || any_overlap(outputs))
		return fail(what, "an output must not overlap an input, the scratch or another output");
	const SkinArgs a = {vertices, joints, quaternions, parents, indices, weights, V, J, K, n};
	const hipStream_t st = (hipStream_t)stream;
	if (vertices_b)
		hipLaunchKernelGGL(skin_apply_b_kernel, dim3(fh_blocks((long long)V * GATHER_LANES)), dim3(FH_BLOCK), 0, st, a, world, posed_b, vertices_b);
	if (quaternions_b || joints_b)
	{
		hipLaunchKernelGGL(skin_joint_b_kernel, dim3(J, n), dim3(FH_BLOCK), 0, st, a, world, posed_b, joint_offsets, joint_slots, (uint32_t)nnz, sc.doubles());
		hipLaunchKernelGGL(skin_chain_b_kernel, dim3(1), dim3(FH_BLOCK), 0, st, a, world, sc.doubles(), quaternions_b, joints_b);
	}
	return check_hip(hipGetLastError(), "skin_apply_b launch");
}

// ---- the multi-scale L2 data term (include/deodr_hip_pyramid.h, kernels in dr_pyramid.h)

int deodr_hip_pyramid_abi_version(void) { return DEODR_HIP_PYRAMID_ABI_VERSION; }

namespace
{
const char *image_term_size(int n, int H, int W, int C) { return (double)n * H * W * C >= 1099511627776.0 ? "n H W C must be below 2^40" : NULL; }

// What deodr_hip_pyramid_l2 and deodr_hip_ssim_l2 (below) check alike, in the order their messages are documented in: the arrays that must be given
// (`param`: level_weights / mix, `param_bytes` long), `dims` and then `own` (the operator's own refusals, NULL: none), the dtype tag, the alignment,
// the scratch against `need` (`need_fn` states it), the outputs against the inputs and each other.  -> 1 with the message set, or 0.
int image_term_refused(const char *what, const void *image, const void *obs, const void *weights, const void *image_b, const double *param,
					   const char *param_name, size_t param_bytes, const double *terms, size_t terms_bytes, const double *loss, void *scratch,
					   size_t scratch_bytes, size_t need, const char *need_fn, const char *dims, const char *own, int n, int H, int W, int C, int pixel_dtype)
{
	char why[96];
	if (!image || !obs || !param || !terms || !scratch)
		return snprintf(why, sizeof why, "image, obs, %s, terms or scratch == NULL", param_name), fail(what, why);
	if (dims || own)
		return fail(what, dims ? dims : own);
	const size_t elem = elem_bytes(pixel_dtype);
	if (!elem)
		return fail(what, "pixel_dtype must be DEODR_HIP_F32 or DEODR_HIP_F64");
	const void *const pixels[] = {image, obs, weights, image_b};
	const void *const doubles[] = {param, terms, loss, scratch};
	if (any_misaligned(pixels, elem) || any_misaligned(doubles, 8))
		return fail(what, "misaligned pointer");
	if (!Scratch{scratch, scratch_bytes}.holds(need))
		return snprintf(why, sizeof why, "scratch too small (%s)", need_fn), fail(what, why);
	const size_t frame = (size_t)n * H * W * elem;
	const Range outputs[] = {{terms, terms_bytes}, {loss, 8}, {image_b, frame * C}, {scratch, scratch_bytes}};
	const Range inputs[] = {{image, frame * C}, {obs, frame * C}, {weights, frame}, {param, param_bytes}};
	if (any_overlap(outputs, inputs) || any_overlap(outputs))
		return fail(what, "an output must not overlap an input, the scratch or another output");
	return 0;
}

struct PyramidLayout
{ // the scratch after its counter words, in doubles
	size_t tiles, regions, partials_tile, partials_coarse, tile_w, tile_q, gamma, doubles;
	int TH, TW, RH, RW;
};
const char *pyramid_dims(int n, int H, int W, int C, int levels)
{ // -> NULL, or which limit of the header the dimensions break
	if (levels < 1 || levels > PYR_MAX_LEVELS)
		return "levels must be in 1 .. 8";
	if (C < 1)
		return "C must be >= 1";
	if (n < 1 || H < 1 || W < 1)
		return "n, H and W must be >= 1";
	return image_term_size(n, H, W, C);
}
PyramidLayout pyramid_layout(int n, int H, int W, int C, int levels)
{
	PyramidLayout l = {};
	l.TH = (H + PYR_TILE - 1) / PYR_TILE, l.TW = (W + PYR_TILE - 1) / PYR_TILE;
	l.RH = (l.TH + PYR_REGION - 1) / PYR_REGION, l.RW = (l.TW + PYR_REGION - 1) / PYR_REGION;
	l.tiles = (size_t)n * l.TH * l.TW, l.regions = (size_t)n * l.RH * l.RW;
	const bool above = levels > PYR_TILE_LEVELS;
	l.partials_tile = 0;
	l.partials_coarse = l.partials_tile + (size_t)PYR_BLOCKS * (PYR_TILE_LEVELS + 1);
	l.tile_w = l.partials_coarse + (above ? l.regions * PYR_COARSE_LEVELS : 0);
	l.tile_q = l.tile_w + (above ? l.tiles : 0);
	l.gamma = l.tile_q + (above ? l.tiles * C : 0);
	l.doubles = l.gamma + (above ? l.tiles * C : 0);
	return l;
}
} // namespace

size_t deodr_hip_pyramid_scratch_bytes(int n, int H, int W, int C, int levels)
{
	return pyramid_dims(n, H, W, C, levels) ? 0 : scratch_need(pyramid_layout(n, H, W, C, levels).doubles);
}

int deodr_hip_pyramid_l2(const void *image, const void *obs, const void *weights, int n, int H, int W, int C, int pixel_dtype, int levels,
						 const double *level_weights, double *terms, double *loss, void *image_b, void *scratch, size_t scratch_bytes, void *stream)
{
	const size_t lam = 8 * ((size_t)levels + 1);
	if (image_term_refused("pyramid_l2", image, obs, weights, image_b, level_weights, "level_weights", lam, terms, lam, loss, scratch, scratch_bytes,
						   deodr_hip_pyramid_scratch_bytes(n, H, W, C, levels), "deodr_hip_pyramid_scratch_bytes", pyramid_dims(n, H, W, C, levels), NULL, n, H, W,
						   C, pixel_dtype))
		return 1;
	const Scratch sc = {scratch, scratch_bytes};
	const PyramidLayout l = pyramid_layout(n, H, W, C, levels);
	double *const d = sc.doubles();
	const PyramidArgs a = {image, obs, weights, image_b, level_weights, terms, loss, d + l.partials_tile, d + l.partials_coarse, d + l.tile_w,
						   d + l.tile_q, d + l.gamma, sc.counter(0), n, H, W, C, levels, l.TH, l.TW, l.RH, l.RW};
	const hipStream_t st = (hipStream_t)stream;
	if (check_hip(hipMemsetAsync(scratch, 0, SCRATCH_COUNTER_BYTES, st), "pyramid_l2 counters"))
		return 1;
	const dim3 grid(capped_blocks(l.tiles, PYR_WAVES, PYR_BLOCKS)), block(FH_BLOCK);
	const bool above = levels > PYR_TILE_LEVELS;
	with_pixel_type(pixel_dtype == DEODR_HIP_F64, [&](auto pix) {
		using PixT = decltype(pix);
		if (!above && image_b)
			hipLaunchKernelGGL((pyramid_tile_kernel<PixT, PYR_REDUCE | PYR_ADJOINT>), grid, block, 0, st, a);
		else
			hipLaunchKernelGGL((pyramid_tile_kernel<PixT, PYR_REDUCE>), grid, block, 0, st, a);
		if (above)
			hipLaunchKernelGGL(pyramid_coarse_kernel, dim3((unsigned)l.regions), block, 0, st, a);
		if (above && image_b)
			hipLaunchKernelGGL((pyramid_tile_kernel<PixT, PYR_ADJOINT>), grid, block, 0, st, a);
		return 0;
	});
	return check_hip(hipGetLastError(), "pyramid_l2 launch");
}

// ---- the structural (SSIM) data term (include/deodr_hip_ssim.h, kernels in dr_ssim.h)

int deodr_hip_ssim_abi_version(void) { return DEODR_HIP_SSIM_ABI_VERSION; }

namespace
{
const char *ssim_dims(int n, int H, int W, int C)
{ // -> NULL, or which limit of the header the dimensions break
	if (n < 1 || H < 1 || W < 1 || C < 1)
		return "n, H, W and C must be >= 1";
	return image_term_size(n, H, W, C);
}
} // namespace

size_t deodr_hip_ssim_scratch_bytes(int n, int H, int W, int C)
{ // the partials of the stats kernel, then the three maps
	return ssim_dims(n, H, W, C) ? 0 : scratch_need((size_t)SSIM_BLOCKS * 2 + 3 * ((size_t)n * H * W * C));
}

int deodr_hip_ssim_l2(const void *image, const void *obs, const void *weights, int n, int H, int W, int C, int pixel_dtype, double data_range,
					  const double *mix, double *terms, double *loss, void *image_b, void *scratch, size_t scratch_bytes, void *stream)
{
	const char *const range = data_range > 0 && __builtin_isfinite(data_range) ? NULL : "data_range must be finite and > 0";
	if (image_term_refused("ssim_l2", image, obs, weights, image_b, mix, "mix", 16, terms, 16, loss, scratch, scratch_bytes, deodr_hip_ssim_scratch_bytes(n, H, W, C),
						   "deodr_hip_ssim_scratch_bytes", ssim_dims(n, H, W, C), range, n, H, W, C, pixel_dtype))
		return 1;
	const Scratch sc = {scratch, scratch_bytes};
	double *const d = sc.doubles();
	const int TY = (H + SSIM_TH - 1) / SSIM_TH, TX = (W + SSIM_TW - 1) / SSIM_TW;
	const double c1 = 0.01 * data_range, c2 = 0.03 * data_range;
	const SsimArgs a = {image, obs, weights, image_b, mix, terms, loss, d, d + (size_t)SSIM_BLOCKS * 2, sc.counter(0), c1 * c1, c2 * c2, n, H, W, C, TY, TX};
	const hipStream_t st = (hipStream_t)stream;
	if (check_hip(hipMemsetAsync(scratch, 0, SCRATCH_COUNTER_BYTES, st), "ssim_l2 counters"))
		return 1;
	const dim3 grid(capped_blocks((size_t)n * TY * TX, 1, SSIM_BLOCKS)), block(FH_BLOCK);
	with_pixel_type(pixel_dtype == DEODR_HIP_F64, [&](auto pix) {
		using PixT = decltype(pix);
		if (image_b)
		{
			hipLaunchKernelGGL((ssim_stats_kernel<PixT, true>), grid, block, 0, st, a);
			hipLaunchKernelGGL(ssim_adjoint_kernel<PixT>, grid, block, 0, st, a);
		}
		else
			hipLaunchKernelGGL((ssim_stats_kernel<PixT, false>), grid, block, 0, st, a);
		return 0;
	});
	return check_hip(hipGetLastError(), "ssim_l2 launch");
}

// ---- sparse symmetric positive definite solve (include/deodr_hip_solve.h, kernels in dr_solve.h)

int deodr_hip_solve_abi_version(void) { return DEODR_HIP_SOLVE_ABI_VERSION; }

namespace
{
const char *solve_dims(int n, uint32_t nnz, int D, int iterations)
{ // -> NULL, or which limit of the header the arguments break
	if (n <= 0)
		return "n must be positive";
	if (nnz < (uint32_t)n)
		return "nnz must be >= n (the diagonal is stored)";
	if (D < 1 || D > SOLVE_MAX_D)
		return "D must be in 1 .. 4";
	if (iterations < 1)
		return "iterations must be >= 1";
	return NULL;
}
} // namespace

size_t deodr_hip_spd_solve_scratch_bytes(int n, int D) { return solve_dims(n, (uint32_t)(n > 0 ? n : 0), D, 1) ? 0 : scratch_need(solve_scratch_doubles(n, D)); }

int deodr_hip_spd_solve_launches(int n, uint32_t nnz, int D, int iterations)
{
	return solve_dims(n, nnz, D, iterations) ? 0 : solve_small(n) ? 1 : 2 + 2 * iterations;
}

int deodr_hip_spd_solve(const uint32_t *offsets, const uint32_t *cols, const double *vals, int n, uint32_t nnz, const double *b, double *x, int D,
						int iterations, double rel_tol, double *residual, void *scratch, size_t scratch_bytes, void *stream)
{
	const char *what = "spd_solve";
	if (!offsets || !cols || !vals || !b || !x || !residual || !scratch)
		return fail(what, "offsets, cols, vals, b, x, residual or scratch == NULL");
	if (const char *why = solve_dims(n, nnz, D, iterations))
		return fail(what, why);
	if (!(rel_tol >= 0)) // (a NaN is refused as well)
		return fail(what, "rel_tol must be >= 0");
	const void *const words[] = {offsets, cols};
	const void *const doubles[] = {vals, b, x, residual, scratch};
	if (any_misaligned(words, 4) || any_misaligned(doubles, 8))
		return fail(what, "misaligned pointer");
	const Scratch sc = {scratch, scratch_bytes};
	if (!sc.holds(deodr_hip_spd_solve_scratch_bytes(n, D)))
		return fail(what, "scratch too small (deodr_hip_spd_solve_scratch_bytes)");
	const size_t nd = 8 * (size_t)n * (size_t)D;
	if (ranges_overlap(x, nd, b, nd))
		return fail(what, "x must not overlap b");
	const Range outputs[] = {{x, nd}, {residual, 8 * (size_t)D}, {scratch, scratch_bytes}};
	const Range inputs[] = {{offsets, 4 * ((size_t)n + 1)}, {cols, 4 * (size_t)nnz}, {vals, 8 * (size_t)nnz}, {b, nd}};
	if (any_overlap(outputs, inputs) || any_overlap(outputs))
		return fail(what, "an output must not overlap an input, the scratch or another output");
	double *const d = sc.doubles(), *const arrays = d + SOLVE_SCALARS + (size_t)SOLVE_BLOCKS * SOLVE_MAX_D;
	const size_t cells = (size_t)n * (size_t)D;
	const SolveArgs a = {offsets, cols, vals, b, x, residual, d, d + SOLVE_SCALARS, arrays, arrays + 3 * cells, sc.counter(0), rel_tol * rel_tol, n, D, iterations};
	const hipStream_t st = (hipStream_t)stream;
	if (solve_small(n))
		hipLaunchKernelGGL(solve_small_kernel, dim3(D), dim3(SOLVE_SMALL_THREADS), 0, st, a);
	else
	{
		double *const p0 = arrays + cells, *const p1 = arrays + 2 * cells;
		switch (D)
		{
		case 1: solve_launch_large<1>(a, p0, p1, st); break;
		case 2: solve_launch_large<2>(a, p0, p1, st); break;
		case 3: solve_launch_large<3>(a, p0, p1, st); break;
		default: solve_launch_large<4>(a, p0, p1, st); break;
		}
	}
	return check_hip(hipGetLastError(), "spd_solve launch");
}

// ---- as-rigid-as-possible energy (include/deodr_hip_arap.h, kernels in dr_arap.h)

int deodr_hip_arap_abi_version(void) { return DEODR_HIP_ARAP_ABI_VERSION; }

namespace
{
const char *arap_dims(int V, int n)
{ // -> NULL, or which limit of the header the arguments break
	if (V <= 0)
		return "V must be positive";
	if (n <= 0 || n > ARAP_MAX_POSES)
		return "n must be in 1 .. 65535";
	return NULL;
}
} // namespace

size_t deodr_hip_arap_scratch_bytes(int V, int n) { return arap_dims(V, n) ? 0 : scratch_need(arap_scratch_doubles(V, n)); }

int deodr_hip_arap_blocks(int V) { return V <= 0 ? 0 : (int)arap_blocks(V); }

int deodr_hip_arap_launches(int V, uint32_t nnz, int n)
{
	(void)nnz;
	return arap_dims(V, n) ? 0 : 2;
}

int deodr_hip_arap_energy(const uint32_t *offsets, const uint32_t *cols, const double *weights, int V, uint32_t nnz, const double *vertices_ref,
						  const double *vertices, int n, double cregu, double *energy, double *gradient, double *rotations, void *scratch,
						  size_t scratch_bytes, void *stream)
{
	const char *what = "arap_energy";
	if (!offsets || !vertices_ref || !vertices || !energy || !gradient || !scratch || (nnz && (!cols || !weights)))
		return fail(what, "offsets, cols, weights, vertices_ref, vertices, energy, gradient or scratch == NULL");
	if (const char *why = arap_dims(V, n))
		return fail(what, why);
	if (!(cregu >= 0)) // (a NaN is refused as well)
		return fail(what, "cregu must be >= 0");
	const void *const words[] = {offsets, cols};
	const void *const doubles[] = {weights, vertices_ref, vertices, energy, gradient, rotations, scratch};
	if (any_misaligned(words, 4) || any_misaligned(doubles, 8))
		return fail(what, "misaligned pointer");
	const Scratch sc = {scratch, scratch_bytes};
	if (!sc.holds(deodr_hip_arap_scratch_bytes(V, n)))
		return fail(what, "scratch too small (deodr_hip_arap_scratch_bytes)");
	const size_t cells = (size_t)n * (size_t)V;
	const Range outputs[] = {{energy, 8 * (size_t)n}, {gradient, 24 * cells}, {rotations, 32 * cells}, {scratch, scratch_bytes}};
	const Range inputs[] = {{offsets, 4 * ((size_t)V + 1)}, {cols, 4 * (size_t)nnz}, {weights, 8 * (size_t)nnz}, {vertices_ref, 24 * (size_t)V}, {vertices, 24 * cells}};
	if (any_overlap(outputs, inputs) || any_overlap(outputs))
		return fail(what, "an output must not overlap an input, the scratch or another output");
	double *const d = sc.doubles();
	double *const partials = d + 5 * cells;
	const ArapArgs a = {offsets, cols, weights, vertices_ref, vertices, energy, gradient, rotations, d, d + 4 * cells, partials,
						(unsigned *)(partials + (size_t)ARAP_MAX_BLOCKS * (size_t)n), cregu, V, n};
	const hipStream_t st = (hipStream_t)stream;
	const dim3 grid(arap_blocks(V), (unsigned)n), block(ARAP_BLOCK);
	hipLaunchKernelGGL(arap_rotations_kernel, grid, block, 0, st, a);
	hipLaunchKernelGGL(arap_gradient_kernel, grid, block, 0, st, a);
	return check_hip(hipGetLastError(), "arap_energy launch");
}

// ---- closest-point (Chamfer) energy (include/deodr_hip_chamfer.h, kernels in dr_chamfer.h)

int deodr_hip_chamfer_abi_version(void) { return DEODR_HIP_CHAMFER_ABI_VERSION; }

namespace
{
const char *chamfer_poses(int n) { return n <= 0 || n > CHAMFER_MAX_POSES ? "n must be in 1 .. 65535" : NULL; } // (of the three closest-point operators)
const char *chamfer_dims(int V, int P, int n)
{ // -> NULL, or which limit of the header the arguments break
	if (V <= 0)
		return "V must be positive";
	if (P <= 0)
		return "P must be positive";
	if (const char *why = chamfer_poses(n))
		return why;
	if ((unsigned long long)V * (unsigned long long)P > DEODR_HIP_CHAMFER_MAX_PAIRS)
		return "V * P is above DEODR_HIP_CHAMFER_MAX_PAIRS (the search is brute force)";
	return NULL;
}
bool chamfer_directions(int directions) { return directions >= 1 && directions <= 3; }

// What deodr_hip_chamfer, deodr_hip_surface_distance and deodr_hip_chamfer_grid check alike once their own NULL sentence and dims have passed, in
// the order their messages are documented in: the directions, `own` (the operator's own refusal, NULL: none), `misaligned` (any of its arrays),
// the scratch against `need`, `clash` (an output overlaps an input or another output).  -> 1 with the message set, or 0.
int closest_point_refused(const char *what, int directions, const char *own, bool misaligned, void *scratch, size_t scratch_bytes, size_t need,
						  const char *too_small, bool clash)
{
	if (!chamfer_directions(directions))
		return fail(what, "directions must be in 1 .. 3");
	if (own)
		return fail(what, own);
	if (misaligned)
		return fail(what, "misaligned pointer");
	if (!Scratch{scratch, scratch_bytes}.holds(need))
		return fail(what, too_small);
	if (clash)
		return fail(what, "an output must not overlap an input, the scratch or another output");
	return 0;
}
} // namespace

size_t deodr_hip_chamfer_scratch_bytes(int V, int P, int n)
{
	ChamferArgs a;
	return chamfer_dims(V, P, n) ? 0 : chamfer_carve(a, V, P, n, NULL);
}

int deodr_hip_chamfer_segments(int queries, int references) { return chamfer_segments(queries, references); }

int deodr_hip_chamfer_launches(int V, int P, int n, int directions)
{
	return chamfer_dims(V, P, n) || !chamfer_directions(directions) ? 0 : directions & DEODR_HIP_CHAMFER_POINTS_TO_MESH ? 4 : 2;
}

int deodr_hip_chamfer(const double *vertices, int V, const double *points, int P, const double *point_weights, const double *vertex_weights,
					  const double *params, int n, int directions, double *terms, double *loss, double *vertices_b, uint32_t *nearest_vertex,
					  uint32_t *nearest_point, void *scratch, size_t scratch_bytes, void *stream)
{
	const char *what = "chamfer";
	if (!vertices || !points || !params || !terms || !loss || !vertices_b || !scratch)
		return fail(what, "vertices, points, params, terms, loss, vertices_b or scratch == NULL");
	if (const char *why = chamfer_dims(V, P, n))
		return fail(what, why);
	const void *const words[] = {nearest_vertex, nearest_point};
	const void *const doubles[] = {vertices, points, point_weights, vertex_weights, params, terms, loss, vertices_b, scratch};
	const size_t N = (size_t)n, nv = N * (size_t)V, np = N * (size_t)P;
	const Range outputs[] = {{terms, 16 * N}, {loss, 8 * N}, {vertices_b, 24 * nv}, {nearest_vertex, 4 * np}, {nearest_point, 4 * nv}, {scratch, scratch_bytes}};
	const Range inputs[] = {{vertices, 24 * nv}, {points, 24 * np}, {point_weights, 8 * np}, {vertex_weights, 8 * (size_t)V}, {params, 24}};
	ChamferArgs a = {vertices, points, point_weights, vertex_weights, params, terms, loss, vertices_b, nearest_vertex, nearest_point};
	if (closest_point_refused(what, directions, NULL, any_misaligned(words, 4) || any_misaligned(doubles, 8), scratch, scratch_bytes, chamfer_carve(a, V, P, n, NULL),
							  "scratch too small (deodr_hip_chamfer_scratch_bytes)", any_overlap(outputs, inputs) || any_overlap(outputs)))
		return 1;
	chamfer_carve(a, V, P, n, scratch);
	a.directions = directions, a.clear_tickets = 1;
	const hipStream_t st = (hipStream_t)stream;
	const dim3 block(CHAMFER_BLOCK), walk_v(((unsigned)V - 1) / CHAMFER_BLOCK + 1, (unsigned)a.Sv, (unsigned)n);
	if (directions & DEODR_HIP_CHAMFER_POINTS_TO_MESH)
	{
		hipLaunchKernelGGL((chamfer_walk_kernel<true, false>), dim3(((unsigned)P - 1) / CHAMFER_BLOCK + 1, (unsigned)a.Sp, (unsigned)n), block, 0, st, a, 1);
		a.clear_tickets = 0;
		hipLaunchKernelGGL(chamfer_points_kernel, dim3(chamfer_blocks(P), (unsigned)n), block, 0, st, a);
		if (directions & DEODR_HIP_CHAMFER_MESH_TO_POINTS)
			hipLaunchKernelGGL((chamfer_walk_kernel<true, true>), walk_v, block, 0, st, a, 0);
		else
			hipLaunchKernelGGL((chamfer_walk_kernel<false, true>), walk_v, block, 0, st, a, 0);
	}
	else
		hipLaunchKernelGGL((chamfer_walk_kernel<true, false>), walk_v, block, 0, st, a, 0);
	hipLaunchKernelGGL(chamfer_vertices_kernel, dim3(chamfer_blocks(V), (unsigned)n), block, 0, st, a);
	return check_hip(hipGetLastError(), "chamfer launch");
}

// ---- point-to-surface distance (include/deodr_hip_surface.h, kernels in dr_surface.h)

int deodr_hip_surface_abi_version(void) { return DEODR_HIP_SURFACE_ABI_VERSION; }

namespace
{
const char *surface_dims(int V, int F, int P, int n)
{ // -> NULL, or which limit of the header the arguments break whatever the directions
	if (V <= 0)
		return "V must be positive";
	if (F <= 0 || F > SURFACE_MAX_FACES)
		return "F must be in 1 .. 715827882";
	if (P <= 0)
		return "P must be positive";
	if (const char *why = chamfer_poses(n))
		return why;
	if ((unsigned long long)F * (unsigned long long)P > DEODR_HIP_SURFACE_MAX_PAIRS)
		return "F * P is above DEODR_HIP_SURFACE_MAX_PAIRS (the search is brute force)";
	return NULL;
}
const char *surface_vertex_pairs(int V, int P, int directions)
{
	if ((directions & DEODR_HIP_CHAMFER_MESH_TO_POINTS) && (unsigned long long)V * (unsigned long long)P > DEODR_HIP_CHAMFER_MAX_PAIRS)
		return "V * P is above DEODR_HIP_CHAMFER_MAX_PAIRS with mesh -> points on (the search is brute force)";
	return NULL;
}
} // namespace

size_t deodr_hip_surface_distance_scratch_bytes(int V, int F, int P, int n)
{
	SurfaceArgs a;
	return surface_dims(V, F, P, n) ? 0 : surface_carve(a, V, F, P, n, NULL);
}

int deodr_hip_surface_distance_launches(int V, int F, int P, int n, int directions)
{
	if (surface_dims(V, F, P, n) || !chamfer_directions(directions) || surface_vertex_pairs(V, P, directions))
		return 0;
	return directions == 3 ? 6 : directions == 1 ? 5 : 2;
}

int deodr_hip_surface_distance(const double *vertices, int V, const int32_t *faces, int F, const int32_t *corner_offsets, const int32_t *corners,
							   const double *points, int P, const double *point_weights, const double *vertex_weights, const double *params, int n,
							   int directions, double *terms, double *loss, double *vertices_b, uint32_t *nearest_face, double *barycentric,
							   uint32_t *nearest_point, void *scratch, size_t scratch_bytes, void *stream)
{
	const char *what = "surface_distance";
	if (!vertices || !faces || !corner_offsets || !corners || !points || !params || !terms || !loss || !vertices_b || !scratch)
		return fail(what, "vertices, faces, corner_offsets, corners, points, params, terms, loss, vertices_b or scratch == NULL");
	if (const char *why = surface_dims(V, F, P, n))
		return fail(what, why);
	const void *const words[] = {faces, corner_offsets, corners, nearest_face, nearest_point};
	const void *const doubles[] = {vertices, points, point_weights, vertex_weights, params, terms, loss, vertices_b, barycentric, scratch};
	const size_t N = (size_t)n, nv = N * (size_t)V, np = N * (size_t)P;
	const Range outputs[] = {{terms, 16 * N}, {loss, 8 * N}, {vertices_b, 24 * nv}, {nearest_face, 4 * np}, {barycentric, 24 * np}, {nearest_point, 4 * nv}, {scratch, scratch_bytes}};
	const Range inputs[] = {{vertices, 24 * nv}, {faces, 12 * (size_t)F}, {corner_offsets, 4 * ((size_t)V + 1)}, {corners, 12 * (size_t)F}, {points, 24 * np},
							{point_weights, 8 * np}, {vertex_weights, 8 * (size_t)V}, {params, 24}};
	SurfaceArgs a = {vertices, faces, corner_offsets, corners, points, point_weights, vertex_weights, params, terms, loss, vertices_b, nearest_face, barycentric, nearest_point};
	if (closest_point_refused(what, directions, surface_vertex_pairs(V, P, directions), any_misaligned(words, 4) || any_misaligned(doubles, 8), scratch, scratch_bytes,
							  surface_carve(a, V, F, P, n, NULL), "scratch too small (deodr_hip_surface_distance_scratch_bytes)", any_overlap(outputs, inputs) || any_overlap(outputs)))
		return 1;
	surface_carve(a, V, F, P, n, scratch);
	a.directions = directions;
	const hipStream_t st = (hipStream_t)stream;
	const dim3 block(CHAMFER_BLOCK);
	if (directions & DEODR_HIP_CHAMFER_POINTS_TO_MESH)
	{
		hipLaunchKernelGGL(surface_prep_kernel, dim3(chamfer_blocks(F), (unsigned)n), block, 0, st, a);
		hipLaunchKernelGGL(surface_search_kernel, dim3(((unsigned)P - 1) / CHAMFER_BLOCK + 1, (unsigned)a.Sp, (unsigned)n), block, 0, st, a);
		hipLaunchKernelGGL(surface_points_kernel, dim3(chamfer_blocks(P), (unsigned)n), block, 0, st, a);
		hipLaunchKernelGGL(surface_gather_kernel, dim3(((unsigned)F - 1) / CHAMFER_BLOCK + 1, (unsigned)a.Sg, (unsigned)n), block, 0, st, a);
	}
	if (directions & DEODR_HIP_CHAMFER_MESH_TO_POINTS)
	{ // the vertex-major search of the Chamfer operator itself, into this call's scratch; alone, it is the first launch and clears the tickets
		ChamferArgs c = {};
		c.vertices = vertices, c.points = points, c.vd2 = a.vd2, c.vidx = a.vidx, c.tickets = a.tickets;
		c.V = V, c.P = P, c.n = n, c.Sv = a.Sv, c.directions = directions, c.clear_tickets = !(directions & DEODR_HIP_CHAMFER_POINTS_TO_MESH);
		hipLaunchKernelGGL((chamfer_walk_kernel<true, false>), dim3(((unsigned)V - 1) / CHAMFER_BLOCK + 1, (unsigned)a.Sv, (unsigned)n), block, 0, st, c, 0);
	}
	hipLaunchKernelGGL(surface_vertices_kernel, dim3(chamfer_blocks(V), (unsigned)n), block, 0, st, a);
	return check_hip(hipGetLastError(), "surface_distance launch");
}

// ---- stable sort by key, closest-point energy over a uniform grid (include/deodr_hip_chamfer_grid.h, kernels in dr_sort.h and dr_chamfer_grid.h)

int deodr_hip_chamfer_grid_abi_version(void) { return DEODR_HIP_CHAMFER_GRID_ABI_VERSION; }

size_t deodr_hip_sort_keys_scratch_bytes(int N, int n, int bits) { return sort_dims(N, n, bits) ? 0 : 4 * sort_scratch_words(N, n); }

int deodr_hip_sort_keys_launches(int N, int n, int bits) { return sort_dims(N, n, bits) ? 0 : 3 * sort_passes(bits); }

int deodr_hip_sort_keys(const uint32_t *keys, int N, int n, int bits, uint32_t *sorted_keys, uint32_t *order, void *scratch, size_t scratch_bytes,
						void *stream)
{
	const char *what = "sort_keys";
	if (!keys || !order || !scratch)
		return fail(what, "keys, order or scratch == NULL");
	if (const char *why = sort_dims(N, n, bits))
		return fail(what, why);
	const void *const words[] = {keys, sorted_keys, order, scratch};
	if (any_misaligned(words, 4))
		return fail(what, "misaligned pointer");
	if (scratch_bytes < deodr_hip_sort_keys_scratch_bytes(N, n, bits))
		return fail(what, "scratch too small (deodr_hip_sort_keys_scratch_bytes)");
	const size_t row_bytes = 4 * (size_t)n * (size_t)N;
	const Range buffers[] = {{keys, row_bytes}, {sorted_keys, row_bytes}, {order, row_bytes}, {scratch, scratch_bytes}};
	if (any_overlap(buffers))
		return fail(what, "keys, sorted_keys, order and scratch must not overlap");
	sort_launch(keys, N, n, bits, sorted_keys, order, (uint32_t *)scratch, (hipStream_t)stream);
	return check_hip(hipGetLastError(), "sort_keys launch");
}

namespace
{
const char *chamfer_grid_dims(int V, int P, int n)
{ // -> NULL, or which limit of the header the arguments break
	if (V <= 0 || V > CG_MAX_ITEMS)
		return "V must be in 1 .. DEODR_HIP_CHAMFER_GRID_MAX_ITEMS";
	if (P <= 0 || P > CG_MAX_ITEMS)
		return "P must be in 1 .. DEODR_HIP_CHAMFER_GRID_MAX_ITEMS";
	return chamfer_poses(n);
}
} // namespace

int deodr_hip_chamfer_grid_table_bits(int references) { return chamfer_grid_table_bits(references); }

size_t deodr_hip_chamfer_grid_scratch_bytes(int V, int P, int n)
{
	ChamferGridCall c;
	return chamfer_grid_dims(V, P, n) ? 0 : chamfer_grid_carve(c, V, P, n, NULL);
}

int deodr_hip_chamfer_grid_launches(int V, int P, int n, int directions)
{
	if (chamfer_grid_dims(V, P, n) || !chamfer_directions(directions))
		return 0;
	int launches = 1; // the vertices' combine step
	if (directions & DEODR_HIP_CHAMFER_POINTS_TO_MESH) // keys, sort, build of the vertices; search, combine, sort of the assignment, gather
		launches += 2 + 3 * sort_passes(chamfer_grid_table_bits(V)) + 3 + 3 * sort_passes(chamfer_grid_assign_bits(V));
	if (directions & DEODR_HIP_CHAMFER_MESH_TO_POINTS) // keys, sort, build of the points; search
		launches += 2 + 3 * sort_passes(chamfer_grid_table_bits(P)) + 1;
	return launches;
}

int deodr_hip_chamfer_grid(const double *vertices, int V, const double *points, int P, const double *point_weights, const double *vertex_weights,
						   const double *params, double cell_size, int n, int directions, double *terms, double *loss, double *vertices_b,
						   uint32_t *nearest_vertex, uint32_t *nearest_point, void *scratch, size_t scratch_bytes, void *stream)
{
	const char *what = "chamfer_grid";
	if (!vertices || !points || !params || !terms || !loss || !vertices_b || !scratch)
		return fail(what, "vertices, points, params, terms, loss, vertices_b or scratch == NULL");
	if (const char *why = chamfer_grid_dims(V, P, n))
		return fail(what, why);
	const void *const words[] = {nearest_vertex, nearest_point};
	const void *const doubles[] = {vertices, points, point_weights, vertex_weights, params, terms, loss, vertices_b, scratch};
	const size_t N = (size_t)n, nv = N * (size_t)V, np = N * (size_t)P;
	const Range outputs[] = {{terms, 16 * N}, {loss, 8 * N}, {vertices_b, 24 * nv}, {nearest_vertex, 4 * np}, {nearest_point, 4 * nv}, {scratch, scratch_bytes}};
	const Range inputs[] = {{vertices, 24 * nv}, {points, 24 * np}, {point_weights, 8 * np}, {vertex_weights, 8 * (size_t)V}, {params, 24}};
	ChamferGridCall call = {{}, {vertices, points, point_weights, vertex_weights, params, terms, loss, vertices_b, nearest_vertex, nearest_point}};
	if (closest_point_refused(what, directions, cell_size > 0 && cell_size < __builtin_inf() ? NULL : "cell_size must be finite and > 0", any_misaligned(words, 4) || any_misaligned(doubles, 8), scratch,
							  scratch_bytes, chamfer_grid_carve(call, V, P, n, NULL), "scratch too small (deodr_hip_chamfer_grid_scratch_bytes)", any_overlap(outputs, inputs) || any_overlap(outputs)))
		return 1;
	chamfer_grid_carve(call, V, P, n, scratch);
	ChamferGridArgs &g = call.g;
	g.set[0].coords = vertices, g.set[1].coords = points, g.params = params, g.point_weights = point_weights, g.cell_size = cell_size, g.clear_tickets = 1;
	ChamferArgs &a = call.a; // the combine steps of dr_chamfer.h, with one segment per search
	a.directions = directions;
	uint32_t *const sort_words = call.sort_words;
	const hipStream_t st = (hipStream_t)stream;
	const dim3 block(CHAMFER_BLOCK);
	const bool to_mesh = directions & DEODR_HIP_CHAMFER_POINTS_TO_MESH, to_points = directions & DEODR_HIP_CHAMFER_MESH_TO_POINTS;
	for (int which = 0; which < 2; which++)
		if (which == 0 ? to_mesh : to_points)
		{
			const ChamferGridSet &s = g.set[which];
			const size_t T = (size_t)1 << s.table_bits;
			hipLaunchKernelGGL(chamfer_grid_keys_kernel, dim3(chamfer_blocks(T > (size_t)s.R ? (int)T : s.R), (unsigned)n), block, 0, st, g, which);
			g.clear_tickets = 0;
			sort_launch(s.keys, s.R, n, s.table_bits, s.sorted_keys, s.order, sort_words, st);
			hipLaunchKernelGGL(chamfer_grid_build_kernel, dim3(chamfer_blocks(s.R), (unsigned)n), block, 0, st, g, which);
		}
	if (to_mesh)
	{
		hipLaunchKernelGGL(chamfer_grid_search_kernel, dim3(((unsigned)P - 1) / CHAMFER_BLOCK + 1, (unsigned)n), block, 0, st, g, 1, (int)to_points);
		hipLaunchKernelGGL(chamfer_points_kernel, dim3(chamfer_blocks(P), (unsigned)n), block, 0, st, a);
		sort_launch(a.assign, P, n, chamfer_grid_assign_bits(V), g.sorted_assign, g.assign_order, sort_words, st);
		hipLaunchKernelGGL(chamfer_grid_gather_kernel, dim3(((unsigned)V - 1) / CG_GATHER_VERTICES + 1, (unsigned)n), block, 0, st, g);
	}
	if (to_points)
		hipLaunchKernelGGL(chamfer_grid_search_kernel, dim3(((unsigned)V - 1) / CHAMFER_BLOCK + 1, (unsigned)n), block, 0, st, g, 0, (int)to_mesh);
	hipLaunchKernelGGL(chamfer_vertices_kernel, dim3(chamfer_blocks(V), (unsigned)n), block, 0, st, a);
	return check_hip(hipGetLastError(), "chamfer_grid launch");
}

// ---- point-to-surface distance over a uniform grid of triangles (include_staged/deodr_hip_surface_grid.h, kernels in dr_surface_grid.h)

int deodr_hip_surface_grid_abi_version(void) { return DEODR_HIP_SURFACE_GRID_ABI_VERSION; }

namespace
{
const char *surface_grid_dims(int V, int F, int P, int n)
{ // -> NULL, or which limit of the header the arguments break
	if (V <= 0 || V > CG_MAX_ITEMS)
		return "V must be in 1 .. DEODR_HIP_CHAMFER_GRID_MAX_ITEMS";
	if (F <= 0 || F > CG_MAX_ITEMS)
		return "F must be in 1 .. DEODR_HIP_CHAMFER_GRID_MAX_ITEMS";
	if (P <= 0 || P > CG_MAX_ITEMS)
		return "P must be in 1 .. DEODR_HIP_CHAMFER_GRID_MAX_ITEMS";
	return chamfer_poses(n);
}
} // namespace

size_t deodr_hip_surface_grid_scratch_bytes(int V, int F, int P, int n)
{
	SurfaceGridCall c;
	return surface_grid_dims(V, F, P, n) ? 0 : surface_grid_carve(c, V, F, P, n, NULL);
}

int deodr_hip_surface_grid_launches(int V, int F, int P, int n, int directions)
{
	if (surface_grid_dims(V, F, P, n) || !chamfer_directions(directions))
		return 0;
	int launches = 1; // the vertices' combine step
	if (directions & DEODR_HIP_CHAMFER_POINTS_TO_MESH) // prep, keys, sort, build of the faces; search, combine, sort of the assignment, gather
		launches += 3 + 3 * sort_passes(chamfer_grid_table_bits(F)) + 3 + 3 * sort_passes(chamfer_grid_assign_bits(F));
	if (directions & DEODR_HIP_CHAMFER_MESH_TO_POINTS) // keys, sort, build of the points; search of the vertices
		launches += 2 + 3 * sort_passes(chamfer_grid_table_bits(P)) + 1;
	return launches;
}

int deodr_hip_surface_grid(const double *vertices, int V, const int32_t *faces, int F, const int32_t *corner_offsets, const int32_t *corners,
						   const double *points, int P, const double *point_weights, const double *vertex_weights, const double *params, double cell_size,
						   int n, int directions, double *terms, double *loss, double *vertices_b, uint32_t *nearest_face, double *barycentric,
						   uint32_t *nearest_point, void *scratch, size_t scratch_bytes, void *stream)
{
	const char *what = "surface_grid";
	if (!vertices || !faces || !corner_offsets || !corners || !points || !params || !terms || !loss || !vertices_b || !scratch)
		return fail(what, "vertices, faces, corner_offsets, corners, points, params, terms, loss, vertices_b or scratch == NULL");
	if (const char *why = surface_grid_dims(V, F, P, n))
		return fail(what, why);
	const void *const words[] = {faces, corner_offsets, corners, nearest_face, nearest_point};
	const void *const doubles[] = {vertices, points, point_weights, vertex_weights, params, terms, loss, vertices_b, barycentric, scratch};
	const size_t N = (size_t)n, nv = N * (size_t)V, np = N * (size_t)P;
	const Range outputs[] = {{terms, 16 * N}, {loss, 8 * N}, {vertices_b, 24 * nv}, {nearest_face, 4 * np}, {barycentric, 24 * np}, {nearest_point, 4 * nv}, {scratch, scratch_bytes}};
	const Range inputs[] = {{vertices, 24 * nv}, {faces, 12 * (size_t)F}, {corner_offsets, 4 * ((size_t)V + 1)}, {corners, 12 * (size_t)F}, {points, 24 * np},
							{point_weights, 8 * np}, {vertex_weights, 8 * (size_t)V}, {params, 24}};
	SurfaceGridCall call = {{vertices, faces, corner_offsets, corners, points, point_weights, vertex_weights, params, terms, loss, vertices_b, nearest_face, barycentric, nearest_point}};
	if (closest_point_refused(what, directions, cell_size > 0 && cell_size < __builtin_inf() ? NULL : "cell_size must be finite and > 0", any_misaligned(words, 4) || any_misaligned(doubles, 8), scratch,
							  scratch_bytes, surface_grid_carve(call, V, F, P, n, NULL), "scratch too small (deodr_hip_surface_grid_scratch_bytes)", any_overlap(outputs, inputs) || any_overlap(outputs)))
		return 1;
	surface_grid_carve(call, V, F, P, n, scratch);
	const bool to_mesh = directions & DEODR_HIP_CHAMFER_POINTS_TO_MESH, to_points = directions & DEODR_HIP_CHAMFER_MESH_TO_POINTS;
	SurfaceArgs &a = call.a; // the records, surface_closest() and the combine steps of dr_surface.h, with one segment per search and gather
	a.directions = directions;
	SurfaceGridArgs &f = call.f; // the face grid
	f.points = points, f.params = params, f.cell_size = cell_size;
	ChamferGridArgs &g = call.g; // the points' grid and the search of the vertices over it (dr_chamfer_grid.h)
	g.set[0].coords = vertices, g.set[1].coords = points, g.params = params, g.point_weights = point_weights, g.cell_size = cell_size, g.clear_tickets = !to_mesh;
	f.point_order = to_points ? g.set[1].order : nullptr;
	uint32_t *const sort_words = call.sort_words;
	const hipStream_t st = (hipStream_t)stream;
	const dim3 block(CHAMFER_BLOCK);
	if (to_mesh)
	{
		const size_t T = (size_t)1 << f.table_bits;
		hipLaunchKernelGGL(surface_grid_prep_kernel, dim3(chamfer_blocks(F), (unsigned)n), block, 0, st, a, f);
		hipLaunchKernelGGL(surface_grid_keys_kernel, dim3(chamfer_blocks(T > (size_t)F ? (int)T : F), (unsigned)n), block, 0, st, a, f);
		sort_launch(f.keys, F, n, f.table_bits, f.sorted_keys, f.order, sort_words, st);
		hipLaunchKernelGGL(surface_grid_build_kernel, dim3(chamfer_blocks(F), (unsigned)n), block, 0, st, a, f);
	}
	if (to_points)
	{
		const ChamferGridSet &s = g.set[1];
		const size_t T = (size_t)1 << s.table_bits;
		hipLaunchKernelGGL(chamfer_grid_keys_kernel, dim3(chamfer_blocks(T > (size_t)P ? (int)T : P), (unsigned)n), block, 0, st, g, 1);
		sort_launch(s.keys, P, n, s.table_bits, s.sorted_keys, s.order, sort_words, st);
		hipLaunchKernelGGL(chamfer_grid_build_kernel, dim3(chamfer_blocks(P), (unsigned)n), block, 0, st, g, 1);
	}
	if (to_mesh)
	{
		hipLaunchKernelGGL(surface_grid_search_kernel, dim3(((unsigned)P - 1) / CHAMFER_BLOCK + 1, (unsigned)n), block, 0, st, a, f);
		hipLaunchKernelGGL(surface_points_kernel, dim3(chamfer_blocks(P), (unsigned)n), block, 0, st, a);
		sort_launch(a.assign, P, n, chamfer_grid_assign_bits(F), f.sorted_assign, f.assign_order, sort_words, st);
		hipLaunchKernelGGL(surface_grid_gather_kernel, dim3(((unsigned)F - 1) / SG_GATHER_FACES + 1, (unsigned)n), block, 0, st, a, f);
	}
	if (to_points)
		hipLaunchKernelGGL(chamfer_grid_search_kernel, dim3(((unsigned)V - 1) / CHAMFER_BLOCK + 1, (unsigned)n), block, 0, st, g, 0, 0);
	hipLaunchKernelGGL(surface_vertices_kernel, dim3(chamfer_blocks(V), (unsigned)n), block, 0, st, a);
	return check_hip(hipGetLastError(), "surface_grid launch");
}

#ifdef DR_WAVE_TRACE
int deodr_hip_debug_wave_phase(void *dst, size_t bytes) // tools/wave_trace.py
{
	return check_hip(hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_wave_phase), bytes < sizeof(g_wave_phase) ? bytes : sizeof(g_wave_phase)), "wave phase");
}
int deodr_hip_debug_wave_hw(void *dst, size_t bytes) // tools/wave_trace.py --slots
{
	return check_hip(hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_wave_hw), bytes < sizeof(g_wave_hw) ? bytes : sizeof(g_wave_hw)), "wave hw ids");
}
int deodr_hip_debug_wave_trace(void *dst, size_t bytes) // tools/wave_trace.py
{
	return check_hip(hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_wave_trace), bytes < sizeof(g_wave_trace) ? bytes : sizeof(g_wave_trace)), "wave trace");
}
#endif

int deodr_hip_workspace_status(const DeodrHipScene *sc, void *workspace, size_t workspace_bytes, void *stream, int *overflowed,
							   unsigned long long *needed_pairs, int *scene_errors)
{
	KParams p;
	if (fill_params(sc, 1.0, workspace, workspace_bytes, p, false))
		return 1;
	if (check_hip(hipStreamSynchronize((hipStream_t)stream), "status sync"))
		return 1;
	unsigned long long worst = 0;
	unsigned errors = 0;
	for (int v = 0; v < sc->n_views; v++)
	{
		WsHeader h;
		if (check_hip(hipMemcpy(&h, (char *)workspace + (size_t)v * p.L.view_bytes + p.L.hdr, sizeof h, hipMemcpyDeviceToHost), "status copy"))
			return 1;
		if (h.needed_max > worst)
			worst = h.needed_max;
		errors |= h.scene_errors;
	}
	if (needed_pairs)
		*needed_pairs = worst;
	if (overflowed)
		*overflowed = worst > (p.L.tri_pool_cap < p.L.edge_pool_cap ? p.L.tri_pool_cap : p.L.edge_pool_cap);
	if (scene_errors)
		*scene_errors = (int)errors;
	return 0;
}

int deodr_hip_workspace_census(const DeodrHipScene *sc, void *workspace, size_t workspace_bytes, void *stream,
								unsigned long long *nonempty_tiles, unsigned long long *edge_tiles)
{ // measurement hook: how many tiles of the last forward held a primitive / a silhouette edge (all views)
	KParams p;
	if (fill_params(sc, 1.0, workspace, workspace_bytes, p, false))
		return 1;
	if (check_hip(hipStreamSynchronize((hipStream_t)stream), "census sync"))
		return 1;
	unsigned long long filled = 0, edged = 0;
	std::vector<uint32_t> bits(p.L.nwords), saved(p.L.ntiles);
	for (int v = 0; v < sc->n_views; v++)
	{
		const char *base = (const char *)workspace + (size_t)v * p.L.view_bytes;
		WsHeader h;
		if (check_hip(hipMemcpy(&h, base + p.L.hdr, sizeof h, hipMemcpyDeviceToHost), "census copy") ||
			// (the bitmap of the last forward's parity)
			check_hip(hipMemcpy(bits.data(), base + p.L.tile_bits + sizeof(uint32_t) * p.L.nwords * (h.cur & 1u), sizeof(uint32_t) * p.L.nwords, hipMemcpyDeviceToHost), "census copy") ||
			check_hip(hipMemcpy(saved.data(), base + p.L.edge_saved, sizeof(uint32_t) * p.L.ntiles, hipMemcpyDeviceToHost), "census copy"))
			return 1;
		for (int t = 0; t < p.L.ntiles; t++)
			if ((bits[t >> 5] >> (t & 31)) & 1u)
			{
				filled++;
				edged += (saved[t] & ~SWEEP_SAVED) != 0;
			}
	}
	if (nonempty_tiles)
		*nonempty_tiles = filled;
	if (edge_tiles)
		*edge_tiles = edged;
	return 0;
}

int deodr_hip_workspace_pool_pairs(const DeodrHipScene *sc, size_t workspace_bytes, unsigned long long *pool_pairs)
{ // capacity (in pairs) of the spill pools of a workspace of this size: what the polled `all_needed_max` is compared with
	if (!sc || sc->n_views <= 0)
		return fail("scene == NULL");
	char dummy;
	KParams p;
	if (fill_params(sc, 1.0, &dummy, workspace_bytes, p, false))
		return 1;
	if (pool_pairs)
		*pool_pairs = p.L.tri_pool_cap < p.L.edge_pool_cap ? p.L.tri_pool_cap : p.L.edge_pool_cap;
	return 0;
}

} // extern "C"
