// The point-to-surface distance between a point set and the triangles of a mesh, its gradient to the vertices and the correspondences
// (include/deodr_hip_surface.h has the operation, operation by operation, and the contract).  Brute force, built on dr_chamfer.h: the same split
// rule (chamfer_segments, chamfer_segment_range), the same tickets (chamfer_clear_tickets), for mesh -> points the same search kernel, and in the
// vertices' combine step the same mesh -> points half (chamfer_vertex_to_points) and tail (chamfer_write_terms).
//
// surface_prep_kernel    a thread per (pose, face): the record (a, b, c, ab, ac) of the posed triangle -> scratch; with points -> mesh on it is
//                        the first launch and clears the arrival tickets.
// surface_search_kernel  a thread per point, grid (ceil(P / BLOCK), Sp, n): the face records of segment blockIdx.y are staged in LDS SURFACE_TILE at
//                        a time, 128 bytes each, and every lane reads the same address at the same time (a broadcast).  surface_closest() is the
//                        header's sequence with the seven regions as selects (the lanes hold different points against one triangle: branches
//                        would diverge); strict < keeps the lowest face; the partial (d2, face) of (segment, point) -> scratch.
// surface_points_kernel  a thread per (pose, point): the minimum over the segments in order, surface_closest() once more on the winner (the same
//                        text, so the same bits) -> nearest_face, barycentric, assign (the face, or CHAMFER_NONE beyond tau2), the pull
//                        ((2 w) bary_0, (2 w) bary_1, (2 w) bary_2, e) of the point, term_0 through grid_sum.  A winner CHAMFER_NONE (the search
//                        over the face grid of dr_surface_grid.h found no face within tau2; this file's search never reports it) is passed on:
//                        barycentric (0, 0, 0), the constant w tau2, no gradient.
// surface_gather_kernel  a thread per face, grid (ceil(F / BLOCK), Sg, n): the compare-and-fetch walk of dr_chamfer.h over the staged assign words of
//                        a segment of the points; where assign[k] == f the pull is fetched and its nine products added, in increasing k -> scratch.
// chamfer_walk_kernel<true, false>   mesh -> points: the vertex-major search of dr_chamfer.h, unchanged.
// surface_vertices_kernel  a thread per (pose, vertex): its corners in table order, per corner the segments' sums in order, one chain; plus the
//                        mesh -> points half of dr_chamfer.h -> vertices_b, nearest_point, term_1 through grid_sum; the last workgroup of a pose
//                        writes terms and loss.
//
// No floating-point atomics.  The scratch after its 64 bytes of counter words (unused here), doubles first: rec [n][F][16], pd2 [n][Sp][P],
// pull [n][P][6], fg [n][Sg][F][9], vd2 [n][Sv][V], partials [2][n][CHAMFER_MAX_BLOCKS]; then 4-byte words: pidx [n][Sp][P], vidx [n][Sv][V],
// assign [n][P], tickets [2][n] (surface_carve).
#pragma once

namespace
{

constexpr int SURFACE_TILE = CHAMFER_TILE, SURFACE_REC = 16; // (a record: 15 doubles and one of padding, 128 bytes)
constexpr int SURFACE_MAX_FACES = 715827882;				  // 3 F + 2 is an int32
static_assert(SURFACE_TILE == CHAMFER_BLOCK, "a thread stages one record of a tile");

struct SurfaceArgs
{
	const double *vertices;
	const int32_t *faces, *corner_offsets, *corners;
	const double *points, *point_weights, *vertex_weights, *params;
	double *terms, *loss, *vertices_b;
	uint32_t *nearest_face;
	double *barycentric;
	uint32_t *nearest_point;
	double *rec, *pd2, *pull, *fg, *vd2, *partials; // the scratch
	uint32_t *pidx, *vidx, *assign;
	unsigned *tickets;
	int V, F, P, n, Sp, Sg, Sv, directions;
};

// The scratch layout of the overview, stated once: the dimensions (checked) and the splits of a call -> a, and the bytes of its scratch; with a
// base, its arrays -> a.
inline size_t surface_carve(SurfaceArgs &a, int V, int F, int P, int n, void *base)
{
	a.V = V, a.F = F, a.P = P, a.n = n, a.Sp = chamfer_segments(P, F), a.Sg = chamfer_segments(F, P), a.Sv = chamfer_segments(V, P);
	const size_t N = (size_t)n, np = N * (size_t)P, nf = N * (size_t)F, sp = (size_t)a.Sp * np, sv = (size_t)a.Sv * N * (size_t)V;
	dr::host::ScratchCarver c = {(char *)base};
	a.rec = c.take<double>((size_t)SURFACE_REC * nf), a.pd2 = c.take<double>(sp), a.pull = c.take<double>(6 * np), a.fg = c.take<double>(9 * (size_t)a.Sg * nf);
	a.vd2 = c.take<double>(sv), a.partials = c.take<double>(2 * N * (size_t)CHAMFER_MAX_BLOCKS);
	a.pidx = c.take<uint32_t>(sp), a.vidx = c.take<uint32_t>(sv), a.assign = c.take<uint32_t>(np), a.tickets = c.take<unsigned>(2 * N);
	return c.whole_doubles();
}

struct alignas(16) SurfaceRec
{
	double a[3], b[3], c[3], ab[3], ac[3], pad;
};
static_assert(sizeof(SurfaceRec) == SURFACE_REC * sizeof(double), "the record is 16 doubles");

struct SurfaceHit
{
	double v, w, ex, ey, ez, d2;
};

// the sequence of include/deodr_hip_surface.h, each operation rounded (the library is built without contraction); the regions as selects
__device__ __forceinline__ SurfaceHit surface_closest(const SurfaceRec &r, double px, double py, double pz)
{
	const double apx = px - r.a[0], apy = py - r.a[1], apz = pz - r.a[2];
	const double bpx = px - r.b[0], bpy = py - r.b[1], bpz = pz - r.b[2];
	const double cpx = px - r.c[0], cpy = py - r.c[1], cpz = pz - r.c[2];
	const double d1 = (r.ab[0] * apx + r.ab[1] * apy) + r.ab[2] * apz, d2 = (r.ac[0] * apx + r.ac[1] * apy) + r.ac[2] * apz;
	const double d3 = (r.ab[0] * bpx + r.ab[1] * bpy) + r.ab[2] * bpz, d4 = (r.ac[0] * bpx + r.ac[1] * bpy) + r.ac[2] * bpz;
	const double d5 = (r.ab[0] * cpx + r.ab[1] * cpy) + r.ab[2] * cpz, d6 = (r.ac[0] * cpx + r.ac[1] * cpy) + r.ac[2] * cpz;
	const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
	const double e_ab = d1 - d3, e_ac = d2 - d6, e_b = d4 - d3, e_c = d5 - d6, e_bc = e_b + e_c, den = (va + vb) + vc;
	const bool A = d1 <= 0 && d2 <= 0;
	const bool B = !A && d3 >= 0 && d4 <= d3;
	const bool AB = !A && !B && vc <= 0 && d1 >= 0 && d3 <= 0 && e_ab > 0;
	const bool C = !A && !B && !AB && d6 >= 0 && d5 <= d6;
	const bool AC = !A && !B && !AB && !C && vb <= 0 && d2 >= 0 && d6 <= 0 && e_ac > 0;
	const bool BC = !A && !B && !AB && !C && !AC && va <= 0 && e_b >= 0 && e_c >= 0 && e_bc > 0;
	const bool corner = A || B || C, inside = !corner && !AB && !AC && !BC, flat = inside && den == 0;
	// one numerator and one denominator per coordinate, then the two divisions every region shares (x / 1 and 0 / x are exact)
	const double v_num = B ? 1.0 : AB ? d1 : inside && !flat ? vb : 0.0, v_den = AB ? e_ab : inside && !flat ? den : 1.0;
	const double w_num = C ? 1.0 : AC ? d2 : BC ? e_b : inside && !flat ? vc : 0.0, w_den = AC ? e_ac : BC ? e_bc : inside && !flat ? den : 1.0;
	const double w = w_num / w_den, v_div = v_num / v_den, v = BC ? 1.0 - w : v_div;
	SurfaceHit h;
	h.v = v, h.w = w;
	h.ex = ((r.a[0] + v * r.ab[0]) + w * r.ac[0]) - px, h.ey = ((r.a[1] + v * r.ab[1]) + w * r.ac[1]) - py, h.ez = ((r.a[2] + v * r.ab[2]) + w * r.ac[2]) - pz;
	h.d2 = (h.ex * h.ex + h.ey * h.ey) + h.ez * h.ez;
	return h;
}

// a record of the scratch (8-byte aligned, as the scratch is) <-> one in registers or LDS
__device__ __forceinline__ void surface_copy(double *to, const double *from)
{
#pragma unroll
	for (int x = 0; x < SURFACE_REC; x++)
		to[x] = from[x];
}

__device__ __forceinline__ SurfaceRec surface_record(const double *vertices, const int32_t *face)
{
	const double *const a = vertices + 3 * (size_t)face[0], *const b = vertices + 3 * (size_t)face[1], *const c = vertices + 3 * (size_t)face[2];
	SurfaceRec r;
	for (int x = 0; x < 3; x++)
		r.a[x] = a[x], r.b[x] = b[x], r.c[x] = c[x], r.ab[x] = b[x] - a[x], r.ac[x] = c[x] - a[x];
	r.pad = 0;
	return r;
}

// grid: (chamfer_blocks(F), n)
__global__ __launch_bounds__(CHAMFER_BLOCK) void surface_prep_kernel(SurfaceArgs a)
{
	const size_t pose = blockIdx.y, F = (size_t)a.F;
	chamfer_clear_tickets(a, pose, blockIdx.x == 0);
	const double *const vertices = a.vertices + pose * (size_t)a.V * 3;
	double *const rec = a.rec + (size_t)SURFACE_REC * pose * F;
	for (size_t f = (size_t)blockIdx.x * CHAMFER_BLOCK + threadIdx.x; f < F; f += (size_t)gridDim.x * CHAMFER_BLOCK)
	{
		const SurfaceRec r = surface_record(vertices, a.faces + 3 * f);
		surface_copy(rec + (size_t)SURFACE_REC * f, (const double *)&r);
	}
}

// grid: (ceil(P / CHAMFER_BLOCK), Sp, n)
__global__ __launch_bounds__(CHAMFER_BLOCK) void surface_search_kernel(SurfaceArgs a)
{
	__shared__ SurfaceRec s_rec[SURFACE_TILE];
	const size_t pose = blockIdx.z;
	const int P = a.P, F = a.F, S = (int)gridDim.y, seg = (int)blockIdx.y;
	const double *const rec = a.rec + (size_t)SURFACE_REC * pose * (size_t)F;
	const ChamferRange range = chamfer_segment_range(seg, S, F);
	const int first = range.first, end = range.end;
	const int k = (int)blockIdx.x * CHAMFER_BLOCK + (int)threadIdx.x;
	const bool active = k < P;
	const double *const p = a.points + 3 * (pose * (size_t)P + (size_t)(active ? k : 0));
	const double px = p[0], py = p[1], pz = p[2];
	double best = __builtin_inf();
	uint32_t arg = (uint32_t)first;
	for (int base = first; base < end; base += SURFACE_TILE)
	{
		const int count = end - base < SURFACE_TILE ? end - base : SURFACE_TILE;
		__syncthreads(); // (every thread is past the tile before)
		if ((int)threadIdx.x < count)
			surface_copy((double *)&s_rec[threadIdx.x], rec + (size_t)SURFACE_REC * ((size_t)base + threadIdx.x));
		__syncthreads();
		for (int j = 0; j < count; j++)
		{
			const SurfaceHit h = surface_closest(s_rec[j], px, py, pz);
			const bool better = h.d2 < best;
			best = better ? h.d2 : best;
			arg = better ? (uint32_t)(base + j) : arg;
		}
	}
	if (!active)
		return;
	const size_t at = (pose * (size_t)S + (size_t)seg) * (size_t)P + (size_t)k;
	a.pd2[at] = best, a.pidx[at] = arg;
}

// grid: (chamfer_blocks(P), n)
__global__ __launch_bounds__(CHAMFER_BLOCK) void surface_points_kernel(SurfaceArgs a)
{
	const size_t pose = blockIdx.y, P = (size_t)a.P;
	const double tau = a.params[2], tau2 = tau * tau;
	const double *const rec = a.rec + (size_t)SURFACE_REC * pose * (size_t)a.F;
	double s[1] = {0};
	for (size_t k = (size_t)blockIdx.x * CHAMFER_BLOCK + threadIdx.x; k < P; k += (size_t)gridDim.x * CHAMFER_BLOCK)
	{
		double best;
		uint32_t arg;
		chamfer_combine(a.pd2, a.pidx, pose, a.Sp, P, k, best, arg);
		const double *const p = a.points + 3 * (pose * P + k);
		const bool found = arg != CHAMFER_NONE; // (always, after the brute-force search; the search over the face grid reports no face beyond tau2)
		SurfaceRec r;
		surface_copy((double *)&r, rec + (size_t)SURFACE_REC * (found ? arg : 0u));
		const SurfaceHit h = surface_closest(r, p[0], p[1], p[2]); // (h.d2 == best: the same text on the same values)
		const double b0 = (1.0 - h.v) - h.w;
		const bool near = found && best <= tau2;
		a.assign[pose * P + k] = near ? arg : CHAMFER_NONE;
		if (a.nearest_face)
			a.nearest_face[pose * P + k] = arg;
		if (a.barycentric)
		{
			double *const out = a.barycentric + 3 * (pose * P + k);
			out[0] = found ? b0 : 0.0, out[1] = found ? h.v : 0.0, out[2] = found ? h.w : 0.0;
		}
		const double w = a.point_weights ? a.point_weights[pose * P + k] : 1.0, w2 = 2 * w;
		double *const pull = a.pull + 6 * (pose * P + k);
		pull[0] = w2 * b0, pull[1] = w2 * h.v, pull[2] = w2 * h.w, pull[3] = h.ex, pull[4] = h.ey, pull[5] = h.ez;
		s[0] += w * (near ? best : tau2);
	}
	double total[1];
	if (grid_sum<1>(s, a.partials + pose * CHAMFER_MAX_BLOCKS, a.tickets + pose, total, blockIdx.x, gridDim.x) && threadIdx.x == 0)
		a.terms[2 * pose] = total[0];
}

// grid: (ceil(F / CHAMFER_BLOCK), Sg, n)
__global__ __launch_bounds__(CHAMFER_BLOCK) void surface_gather_kernel(SurfaceArgs a)
{
	__shared__ uint32_t s_assign[CHAMFER_TILE];
	const size_t pose = blockIdx.z;
	const int P = a.P, F = a.F, S = (int)gridDim.y, seg = (int)blockIdx.y;
	const uint32_t *const assign = a.assign + pose * (size_t)P;
	const double *const pull = a.pull + 6 * pose * (size_t)P;
	const ChamferRange range = chamfer_segment_range(seg, S, P);
	const int first = range.first, end = range.end;
	const int f = (int)blockIdx.x * CHAMFER_BLOCK + (int)threadIdx.x;
	const bool active = f < F;
	const uint32_t me = active ? (uint32_t)f : CHAMFER_NO_QUERY;
	double g[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
	for (int base = first; base < end; base += CHAMFER_TILE)
	{
		const int count = end - base < CHAMFER_TILE ? end - base : CHAMFER_TILE;
		__syncthreads(); // (every thread is past the tile before)
		if ((int)threadIdx.x < count)
			s_assign[threadIdx.x] = assign[(size_t)base + threadIdx.x];
		__syncthreads();
		for (int j = 0; j < count; j++)
			if (s_assign[j] == me)
			{
				const double *const t = pull + 6 * ((size_t)base + j);
#pragma unroll
				for (int c = 0; c < 3; c++)
					g[3 * c] += t[c] * t[3], g[3 * c + 1] += t[c] * t[4], g[3 * c + 2] += t[c] * t[5];
			}
	}
	if (!active)
		return;
	double *const out = a.fg + 9 * ((pose * (size_t)S + (size_t)seg) * (size_t)F + (size_t)f);
#pragma unroll
	for (int x = 0; x < 9; x++)
		out[x] = g[x];
}

// grid: (chamfer_blocks(V), n)
__global__ __launch_bounds__(CHAMFER_BLOCK) void surface_vertices_kernel(SurfaceArgs a)
{
	const size_t pose = blockIdx.y, V = (size_t)a.V, F = (size_t)a.F;
	const ChamferMix m = chamfer_mix(a);
	double s[1] = {0};
	for (size_t i = (size_t)blockIdx.x * CHAMFER_BLOCK + threadIdx.x; i < V; i += (size_t)gridDim.x * CHAMFER_BLOCK)
	{
		double bx = 0, by = 0, bz = 0;
		if (m.to_mesh)
		{
			double gx = 0, gy = 0, gz = 0;
			for (int32_t at = a.corner_offsets[i], stop = a.corner_offsets[i + 1]; at < stop; at++)
			{
				const int32_t corner = a.corners[at];
				const size_t f = (size_t)(corner / 3), c = (size_t)(corner % 3);
				for (int seg = 0; seg < a.Sg; seg++)
				{
					const double *const g = a.fg + 9 * ((pose * (size_t)a.Sg + (size_t)seg) * F + f) + 3 * c;
					gx += g[0], gy += g[1], gz += g[2];
				}
			}
			bx = m.mix0 * gx, by = m.mix0 * gy, bz = m.mix0 * gz;
		}
		if (m.to_points)
			chamfer_vertex_to_points(a, m, pose, i, s[0], bx, by, bz);
		double *const out = a.vertices_b + 3 * (pose * V + i);
		out[0] = bx, out[1] = by, out[2] = bz;
	}
	chamfer_write_terms(a, m, pose, s);
}

} // namespace
