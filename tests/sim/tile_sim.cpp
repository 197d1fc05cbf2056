// tests/sim/tile_sim.cpp -- TEST / ANALYSIS TOOL, never part of the product.
//
// Host instantiation of the per-primitive code the HIP kernels run (deodr_amd/csrc/dr_math.h, dr_prims.h, dr_binning.h are
// `__host__ __device__`): set-up of every triangle and silhouette edge of a view and the binning decisions of
// setup_bin_kernel (the rule of dr_binning.h, walked block by block), executed sequentially.  Used (a) to study tile-list
// statistics of a scene without a GPU and (b) by tests/test_sim.py to check the device set-up arithmetic (stencils, spans, planes) against the CPU oracle.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../deodr_amd/csrc/dr_prims.h"

#ifndef DR_SIM_TILE
#error "compile with -DDR_SIM_TILE=<TILE of deodr_amd/csrc/dr_workspace.h> (tests/sim_util.py reads it from there)"
#endif
namespace
{
constexpr int TILE = DR_SIM_TILE;
}
#include "../../deodr_amd/csrc/dr_binning.h"

using namespace dr;

extern "C" {

struct SimScene
{
	const uint32_t *faces, *faces_uv;
	const uint8_t *textured, *shaded, *edgeflags;
	const double *depths, *ij, *shade, *colors, *uv;
	int T, V, Vuv, H, W, C, tex_h, tex_w;
	int clockwise, culling, strict, persp, integer_pixel_centers;
	double sigma;
};

static SceneView view_of(const SimScene *s)
{
	SceneView v;
	v.faces = s->faces;
	v.faces_uv = s->faces_uv;
	v.textured = s->textured;
	v.shaded = s->shaded;
	v.edgeflags = s->edgeflags;
	v.depths = s->depths;
	v.ij = s->ij;
	v.shade = s->shade;
	v.colors = s->colors;
	v.uv = s->uv;
	v.T = s->T;
	v.V = s->V;
	v.Vuv = s->Vuv;
	v.H = s->H;
	v.W = s->W;
	v.C = s->C;
	v.P = planes_per_prim(s->C);
	v.tex_h = s->tex_h;
	v.tex_w = s->tex_w;
	v.has_texture = s->tex_h > 0 && s->tex_w > 0;
	v.clockwise = s->clockwise;
	v.culling = s->culling;
	v.strict = s->strict;
	v.persp = s->persp;
	v.vtx_f64 = true;
	v.offset = s->integer_pixel_centers ? 0.0 : 0.5;
	v.sigma = s->sigma;
	return v;
}

// ---------------------------------------------------------------------------------------------------------- binning
// The rejection is the kernel's own (dr_binning.h); what is restated here is the walk: a box of tiles block by block.  The kernel
// bins block 0 of a triangle in the triangle's own thread and deals the others over the wavefront (bin_rest); an edge band has all its
// blocks dealt.  Which lane serves a block does not change which tiles are requested.

static int g_fault = 0; // TEST ONLY (sim_set_fault): of the non-strict fill rule, 1 = the kept column is dropped, 2 = the kept rows are

void sim_set_fault(int fault) { g_fault = fault; }
int sim_tile(void) { return TILE; }

// The index arithmetic of setup_bin_kernel, restated (the kernel keeps it written out in bin_rest and in the first block of a triangle):
// a box of ntx x nty tiles is walked in 3 x 3 blocks, row by row; block blk starts at tile (bx, by) of the box.
static int bin_blocks(int ntx, int nty) { return ((ntx + 2) / 3) * ((nty + 2) / 3); }
static void bin_block_origin(int blk, int ntx, int &bx, int &by)
{
	const int nbx = (ntx + 2) / 3;
	bx = (blk % nbx) * 3;
	by = (blk / nbx) * 3;
}
// Tile c = 3 dy + dx of the block at (bx, by) is requested when it lies in the box and the rejection keeps it -- or when it is in column
// keep_dx of the box (-1: none) or, with keep_rows, in the box's first or last row of tiles, which the rejection must not drop (the
// non-strict fill rule: setup_bin_kernel).
static bool bin_tile_requested(uint32_t outside, int c, int bx, int by, int ntx, int nty, int keep_dx, bool keep_rows)
{
	const int dx = bx + c % 3, dy = by + c / 3;
	return dx < ntx && dy < nty && (!((outside >> c) & 1u) || dx == keep_dx || (keep_rows && (dy == 0 || dy == nty - 1)));
}

struct Box
{
	int drawn, on_screen, tx0, ty0, ntx, nty; // (six int32: the rows sim_prim_boxes writes)
};

static Box tri_box(const SceneView &v, const TriRec &rec)
{ // as the triangle branch of setup_bin_kernel
	Box b = {rec.kind != KIND_NONE, 0, 0, 0, 0, 0};
	if (!b.drawn)
		return b;
	const int x0 = rec.x_min < 0 ? 0 : rec.x_min, x1 = rec.x_max > v.W - 1 ? v.W - 1 : rec.x_max;
	const int y0 = rec.y_begin[0] < 0 ? 0 : rec.y_begin[0], y1 = rec.y_end[1] > v.H - 1 ? v.H - 1 : rec.y_end[1];
	b.on_screen = !(x0 > x1 || y0 > y1);
	if (b.on_screen)
		b.tx0 = x0 / TILE, b.ty0 = y0 / TILE, b.ntx = x1 / TILE - b.tx0 + 1, b.nty = y1 / TILE - b.ty0 + 1;
	return b;
}

static Box edge_box(const EdgeRec &e)
{ // as edge_round of setup_bin_kernel
	Box b = {e.kind != KIND_NONE, 0, 0, 0, 0, 0};
	if (!b.drawn)
		return b;
	b.on_screen = !(e.x_begin > e.x_end || e.y_begin > e.y_end);
	if (b.on_screen)
		b.tx0 = e.x_begin / TILE, b.ty0 = e.y_begin / TILE, b.ntx = e.x_end / TILE - b.tx0 + 1, b.nty = e.y_end / TILE - b.ty0 + 1;
	return b;
}

extern "C++" template <int N>
void bin_box(const Box &b, const double *hp, int keep_dx, bool keep_rows, bool exact, int tiles_x, uint32_t *cnt)
{
	for (int blk = 0; blk < bin_blocks(b.ntx, b.nty); blk++)
	{
		int bx, by;
		bin_block_origin(blk, b.ntx, bx, by);
		const uint32_t outside = exact ? tiles3x3_outside_halfplanes<N>(hp, b.tx0 + bx, b.ty0 + by) : 0u;
		for (int c = 0; c < 9; c++)
			if (bin_tile_requested(outside, c, bx, by, b.ntx, b.nty, keep_dx, keep_rows))
				cnt[(b.ty0 + by + c / 3) * tiles_x + b.tx0 + bx + c % 3]++;
	}
}

// per-tile triangle / edge counts exactly as setup_bin_kernel bins them (exact = with the half-plane rejection); tile: must be TILE
// -> 0, or -1 for another tile size (nothing is written)
int sim_bin_counts(const SimScene *s, int tile, int exact, uint32_t *tri_cnt, uint32_t *edge_cnt)
{
	if (tile != TILE)
		return -1;
	SceneView v = view_of(s);
	const int tiles_x = (v.W + TILE - 1) / TILE, tiles_y = (v.H + TILE - 1) / TILE;
	memset(tri_cnt, 0, sizeof(uint32_t) * tiles_x * tiles_y);
	memset(edge_cnt, 0, sizeof(uint32_t) * tiles_x * tiles_y);
	std::vector<double> planes(3 * v.P), eplanes(9 * v.P);
	for (int k = 0; k < v.T; k++)
	{
		TriRec rec;
		EdgeRec erec[3];
		setup_triangle(v, k, rec, planes.data(), erec, eplanes.data());
		const Box b = tri_box(v, rec);
		if (b.on_screen)
		{
			const double eq[9] = {rec.eq[0][0], rec.eq[0][1], rec.eq[0][2], rec.eq[1][0], rec.eq[1][1], rec.eq[1][2], rec.eq[2][0], rec.eq[2][1], rec.eq[2][2]};
			const int keep_dx = (v.strict || g_fault == 1) ? -1 : b.ntx - 1; // (the column of x_max under the non-strict rule: see setup_bin_kernel)
			const bool keep_rows = !v.strict && g_fault != 2 && (eq[0] == 0 || eq[3] == 0 || eq[6] == 0); // (the row of a horizontal edge)
			bin_box<3>(b, eq, keep_dx, keep_rows, exact != 0, tiles_x, tri_cnt);
		}
		for (int n = 0; n < 3; n++)
		{
			const EdgeRec &e = erec[n];
			const Box eb = edge_box(e);
			if (!eb.on_screen)
				continue;
			const double band[12] = {e.x2b[0], e.x2b[1], e.x2b[2], e.x2b[3], e.x2b[4], e.x2b[5], e.x2t[0], e.x2t[1], e.x2t[2], -e.x2t[0], -e.x2t[1], 1 - e.x2t[2]};
			bin_box<4>(eb, band, -1, false, exact != 0, tiles_x, edge_cnt);
		}
	}
	return 0;
}

// What the dealing of setup_bin_kernel needs of every primitive: rows (drawn, on_screen, tx0, ty0, ntx, nty) of int32 for triangle k
// (tri[6 k ...]) and for edge slot 3 k + n (edge[6 (3 k + n) ...]; drawn: the slot gets a record, i.e. sigma > 0, flagged, front-facing)
void sim_prim_boxes(const SimScene *s, int32_t *tri, int32_t *edge)
{
	SceneView v = view_of(s);
	std::vector<double> planes(3 * v.P), eplanes(9 * v.P);
	for (int k = 0; k < v.T; k++)
	{
		TriRec rec;
		EdgeRec erec[3];
		setup_triangle(v, k, rec, planes.data(), erec, eplanes.data());
		const Box b = tri_box(v, rec);
		memcpy(tri + 6 * (size_t)k, &b, sizeof(Box));
		for (int n = 0; n < 3; n++)
		{
			const Box eb = edge_box(erec[n]);
			memcpy(edge + 6 * (3 * (size_t)k + n), &eb, sizeof(Box));
		}
	}
}

// coverage mask of one triangle / edge on the whole image through the span functions the kernels use
void sim_tri_coverage(const SimScene *s, int k, uint8_t *mask)
{
	SceneView v = view_of(s);
	std::vector<double> planes(3 * v.P), eplanes(9 * v.P);
	TriRec rec;
	EdgeRec erec[3];
	setup_triangle(v, k, rec, planes.data(), erec, eplanes.data());
	for (int y = 0; y < v.H; y++)
		for (int x = 0; x < v.W; x++)
			mask[y * v.W + x] = rec.kind != KIND_NONE && tri_covers(rec, x, y, v.W, v.H, v.strict);
}

void sim_edge_coverage(const SimScene *s, int k, int n, uint8_t *mask)
{
	SceneView v = view_of(s);
	std::vector<double> planes(3 * v.P), eplanes(9 * v.P);
	TriRec rec;
	EdgeRec erec[3];
	setup_triangle(v, k, rec, planes.data(), erec, eplanes.data());
	for (int y = 0; y < v.H; y++)
		for (int x = 0; x < v.W; x++)
			mask[y * v.W + x] = erec[n].kind != KIND_NONE && edge_covers(erec[n], x, y, v.W);
}
}
