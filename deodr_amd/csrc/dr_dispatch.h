// deodr_amd/csrc/dr_dispatch.h -- which template instance of a kernel a call runs: the rule (pure functions of a few facts about the call)
// and, per kernel, the table of the instances that exist.  Host only, plain C++17, nothing of HIP in it: dr_kernels.hip instantiates and launches
// from the tables (launch_from), tests/sim/dispatch_sim.cpp compiles the same header for the CPU and tests/test_dispatch.py pins the instance of
// every call the project cares about -- all instances of a kernel compute the same result, so no parity test can see a call that fell into a
// slower one.  What the template parameters mean: dr_forward.h (raster_fwd_fast_kernel), dr_backward.h, dr_finalize.h, dr_setup.h.
#pragma once

namespace dr::dispatch
{

// (dr_kernels.hip asserts that these are the kernels' own CH, TEX_TWO_KERNELS and 8 * WORK_CHUNK)
constexpr int STAGED_CHANNELS = 4;	// colour channels the staged kernels keep in registers
constexpr int TWO_KERNEL_VIEWS = 8; // views per launch from which a textured fit step runs its forward raster as two kernels
constexpr int WALKER_UNIT = 512;	// workgroups: eight XCDs times one chunk of the work list

// ---- raster_fwd_fast_kernel<PixT, FUSED, TEX, CLAMP, NC, COMMON, TEXE, VAR>

// What the choice reads.  f64: the pixel buffers are float64.  fused: the one-call fit step (the forward back-propagates sum (image - obs)^2).  tex: the
// scene has a texture.  fuse_edges: KParams::fuse_edges, the fit step's forward also runs the adjoint of the tiles with silhouette edges.  clamp: clamped
// residual (the depth fitter).  weights: fit_weights(p) != NULL, per-pixel weights.  aa_err: antialiase_error.  C: channels.  common: strict_edge and both
// sides of the frame multiples of the tile.  capturing: the stream is being captured into a graph.
struct FwdCall
{
	bool f64, fused, tex, fuse_edges, clamp, weights, aa_err, common, capturing;
	int C, n_views, tile_blocks, heavy_share;
};

struct FwdInst
{
	bool fused, tex, clamp;
	int nc;
	bool common;
	int texe, var;
};
constexpr bool operator==(const FwdInst &a, const FwdInst &b)
{
	return a.fused == b.fused && a.tex == b.tex && a.clamp == b.clamp && a.nc == b.nc && a.common == b.common && a.texe == b.texe && a.var == b.var;
}

// The channel counts that occur get instances with the count at compile time: RGB and RGB + depth; a textured scene is RGB.
constexpr int nc_rgb_or_rgbd(int C) { return C == 3 || C == 4 ? C : 0; }
constexpr int nc_rgb(int C) { return C == 3 ? 3 : 0; }

// TEXE = 2 in the answer says "the two-kernel form": that instance for the head walkers on the side stream, its TEXE = 3 twin for everybody else.
inline FwdInst select_forward(const FwdCall &c)
{
	// A textured fit step with sigma > 0 takes the instances with the edge adjoint (TEXE != 0).  From TWO_KERNEL_VIEWS views per launch on they run as two
	// kernels on two streams -- unless the residual is clamped or weighted (those instances exist in the one-kernel form only), unless the stream is being
	// captured, and only where the split point falls between two groups of eight workgroups (a walker's list and XCD follow from its index in the
	// one-kernel grid, KParams::block_base: true for the shares heavy_share_for returns, checked all the same).
	const bool edge_fit = c.fused && c.tex && c.fuse_edges;
	const bool two = edge_fit && !c.clamp && !c.weights && c.n_views >= TWO_KERNEL_VIEWS && c.tile_blocks % WALKER_UNIT == 0 &&
					 c.tile_blocks % c.heavy_share == 0 && (c.tile_blocks / c.heavy_share) % 8 == 0 && !c.capturing;
	const int nc = c.tex ? nc_rgb(c.C) : nc_rgb_or_rgbd(c.C);
	FwdInst k{c.fused, c.tex, false, 0, false, 0, 0};
	if (two)
		k.nc = nc, k.texe = 2;
	else if (c.C > STAGED_CHANNELS)
		// more than STAGED_CHANNELS channels: only forward-only frames without edges and without texture come here (staged_forward in dr_kernels.hip)
		k = FwdInst{false, false, false, 0, false, 0, 2};
	else if (!c.fused) // (antialiase_error: the edges blend the error buffer, the image stays un-antialiased; run-time channel count)
		k.var = c.aa_err ? 1 : 0, k.nc = c.aa_err ? 0 : nc;
	else
	{
		// A weighted fit step takes the clamp-capable VAR = 3 instances (KParams::clamp decides at run time, as in the clamped ones); weighted and clamped
		// textured steps take the one-kernel form at any number of views.  Clamped or weighted: a compile-time channel count only for the depth image
		// (C = 1, untextured).  Otherwise the count as for a forward-only call, and the untextured step with a known count also the "common frame".
		k.clamp = c.clamp || c.weights;
		k.var = c.weights ? 3 : 0;
		k.texe = edge_fit ? 1 : 0;
		k.nc = !k.clamp ? nc : !c.tex && c.C == 1 ? 1 : 0;
		k.common = !k.clamp && !c.tex && nc != 0 && c.common;
	}
	// The compile-time channel count and frame flag are for float32 pixel buffers, the storage of the fit loops; with float64 buffers (the 1e-9 parity
	// path, the NumPy drop-ins of the reference's entry points) every call takes the run-time-C instance: 28 raster instances fewer to compile (the
	// library builds in ~3.5 minutes instead of ~4.7; their step is a few per cent longer).
	if (c.f64)
		k.nc = 0, k.common = false;
	return k;
}

// Every instance of the kernel for float32 pixels; float64 pixels have the ones with NC = 0 and COMMON = false (fwd_exists).
//                                   FUSED  TEX    CLAMP  NC COMMON TEXE VAR
constexpr FwdInst FWD_INSTANCES[] = {
	{false, false, false, 0, false, 0, 0}, {false, false, false, 3, false, 0, 0}, {false, false, false, 4, false, 0, 0}, // forward only
	{false, true, false, 0, false, 0, 0}, {false, true, false, 3, false, 0, 0},
	{false, false, false, 0, false, 0, 1}, {false, true, false, 0, false, 0, 1}, // antialiase_error
	{false, false, false, 0, false, 0, 2},										  // more than STAGED_CHANNELS channels
	{true, false, false, 0, false, 0, 0}, {true, false, false, 3, false, 0, 0}, {true, false, false, 4, false, 0, 0}, // fit step, untextured
	{true, false, false, 3, true, 0, 0}, {true, false, false, 4, true, 0, 0}, // ... the common frame (C = 4: the benchmark's headline step)
	{true, true, false, 0, false, 0, 0}, {true, true, false, 3, false, 0, 0}, // fit step, textured, sigma = 0
	{true, true, false, 0, false, 1, 0}, {true, true, false, 3, false, 1, 0}, // ... sigma > 0, one kernel
	{true, true, false, 0, false, 2, 0}, {true, true, false, 3, false, 2, 0}, // ... two kernels: the head walkers
	{true, true, false, 0, false, 3, 0}, {true, true, false, 3, false, 3, 0}, // ... two kernels: everybody else
	{true, false, true, 0, false, 0, 0}, {true, false, true, 1, false, 0, 0}, {true, true, true, 0, false, 0, 0}, {true, true, true, 0, false, 1, 0}, // clamped
	{true, false, true, 0, false, 0, 3}, {true, false, true, 1, false, 0, 3}, {true, true, true, 0, false, 0, 3}, {true, true, true, 0, false, 1, 3}, // weighted
};
constexpr bool fwd_exists(const FwdInst &k, bool f64) { return !f64 || (k.nc == 0 && !k.common); }

// ---- raster_bwd_fast_kernel / raster_bwd_edge_kernel<PixT, TEX, NC> (the two-call path)
// The kernels are compiled twice: a scene without texture (no KIND_TEXTURED primitive can exist: the set-up kernel drops textured triangles of
// such a scene and raises DEODR_HIP_ERR_NO_TEXTURE) runs the instances without any texture code.  Channel count: as in the forward.

struct BwdInst
{
	bool tex;
	int nc;
};
constexpr bool operator==(const BwdInst &a, const BwdInst &b) { return a.tex == b.tex && a.nc == b.nc; }
constexpr BwdInst select_adjoint_raster(bool f64, bool tex, int C) { return BwdInst{tex, f64 ? 0 : tex ? nc_rgb(C) : nc_rgb_or_rgbd(C)}; }
constexpr BwdInst BWD_INSTANCES[] = {{false, 0}, {false, 3}, {false, 4}, {true, 0}, {true, 3}};
constexpr bool bwd_exists(const BwdInst &k, bool f64) { return !f64 || k.nc == 0; }

// ---- setup_bin_kernel<VTX64, NC>, finalize_kernel<VTX64, NC, DET, TABLE>: the dtype of the vertex arrays, the channel counts that occur

struct PrimInst
{
	bool vtx_f64;
	int nc;
	bool det, table; // (finalize only)
};
constexpr bool operator==(const PrimInst &a, const PrimInst &b) { return a.vtx_f64 == b.vtx_f64 && a.nc == b.nc && a.det == b.det && a.table == b.table; }
constexpr PrimInst select_setup(bool vtx_f64, int C) { return PrimInst{vtx_f64, nc_rgb_or_rgbd(C), false, false}; }
// The deterministic mode has run-time-C instances of its own; KParams::prim_tables (many primitives per launch) takes the instances with the
// per-workgroup vertex table, which exist for the channel counts of the staged kernels.
constexpr PrimInst select_finalize(bool v64, int C, bool det, bool tables) { return det ? PrimInst{v64, 0, true, false} : PrimInst{v64, nc_rgb_or_rgbd(C), false, tables && C <= STAGED_CHANNELS}; }
constexpr PrimInst SETUP_INSTANCES[] = {{false, 0}, {false, 3}, {false, 4}, {true, 0}, {true, 3}, {true, 4}};
constexpr PrimInst FINALIZE_INSTANCES[] = {{false, 0}, {false, 3}, {false, 4}, {true, 0}, {true, 3}, {true, 4}, {false, 0, true}, {true, 0, true}, // plain; deterministic
										   {false, 0, false, true}, {false, 3, false, true}, {false, 4, false, true}, {true, 0, false, true}, {true, 3, false, true}, {true, 4, false, true}};

} // namespace dr::dispatch
