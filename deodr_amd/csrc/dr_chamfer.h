// The closest-point (Chamfer) energy between the vertices of a mesh and a point set, its gradient to the vertices and the correspondences
// (include/deodr_hip_chamfer.h has the operation and the contract).  A brute-force, query-major tiled search:
//
// chamfer_walk_kernel<SEARCH, GATHER>  a thread per query, grid (ceil(Q / CHAMFER_BLOCK), S, n): the references of segment blockIdx.y -- a contiguous run of
//                         tiles, chamfer_segment_tiles -- are staged in LDS CHAMFER_TILE at a time, 32 bytes each (x, y, z, weight), and every lane
//                         reads the same address of the tile at the same time (a broadcast: no bank conflict).  SEARCH: d2 and a strict < keep
//                         the lowest index of the minimum; the partial (d2, index) of (segment, query) -> scratch.  GATHER (the queries are
//                         the vertices, the references the points): where assign[k] == i -- the nearest vertex of point k is this query and
//                         the pair is within tau2, written by chamfer_points_kernel -- the thread adds w_k (v_i - p_k), in increasing k; the
//                         partial sum of (segment, vertex) -> scratch.  The test is one integer compare per pair and the branch is wave-uniform
//                         almost always (a wavefront holds 64 of V vertices), so the time does not depend on how the points distribute.
//                         GATHER without SEARCH stages the 4-byte assignments alone and fetches a point only where it matches.
// chamfer_points_kernel   a thread per (pose, point): the minimum over the segments in order with strict <, -> assign (the index, or CHAMFER_NONE
//                         beyond tau2), nearest_vertex, and term_0 through grid_sum.
// chamfer_vertices_kernel a thread per (pose, vertex): the same minimum, the segments' gather sums added in order, -> vertices_b, nearest_point,
//                         term_1 through grid_sum; the last workgroup of a pose writes terms and loss.
//
// What the family shares -- this operator, the point-to-surface distance (dr_surface.h) and the search over a grid (dr_chamfer_grid.h) -- is here,
// once: the split of a walk (chamfer_segments, chamfer_segment_range), the ticket clear (chamfer_clear_tickets), the minimum over the segments
// (chamfer_combine), the points' combine step (chamfer_points_kernel: this operator and the grid), the mesh -> points half of a vertex
// (chamfer_vertex_to_points) and the tail that writes terms and loss (chamfer_write_terms).
//
// No floating-point atomics.  The first launch of a call clears the arrival tickets of both combine steps (the launch boundaries order them).
// The scratch after its 64 bytes of counter words (unused here), doubles first: pd2 [n][Sp][P], vd2 [n][Sv][V], vg [n][Sv][V][3],
// partials [2][n][CHAMFER_MAX_BLOCKS]; then 4-byte words: pidx [n][Sp][P], vidx [n][Sv][V], assign [n][P], tickets [2][n] (chamfer_carve).
#pragma once

namespace
{

constexpr int CHAMFER_BLOCK = DEODR_HIP_CHAMFER_BLOCK, CHAMFER_TILE = DEODR_HIP_CHAMFER_TILE, CHAMFER_MAX_BLOCKS = DEODR_HIP_CHAMFER_MAX_BLOCKS;
constexpr int CHAMFER_TARGET_BLOCKS = DEODR_HIP_CHAMFER_TARGET_BLOCKS, CHAMFER_MAX_SEGMENTS = DEODR_HIP_CHAMFER_MAX_SEGMENTS;
constexpr int CHAMFER_MAX_POSES = 65535; // (the poses are the grid's third dimension)
constexpr uint32_t CHAMFER_NONE = 0xFFFFFFFFu, CHAMFER_NO_QUERY = 0xFFFFFFFEu; // (no index reaches them: V, P < 2^31)
static_assert(CHAMFER_BLOCK == FH_BLOCK, "grid_sum adds the partials of a workgroup of FH_BLOCK threads");
static_assert(CHAMFER_TILE == CHAMFER_BLOCK, "a thread stages one reference of a tile");

// the one rule the launches, the scratch layout and deodr_hip_chamfer_segments() follow
inline int chamfer_segments(int queries, int references)
{
	if (queries <= 0 || references <= 0)
		return 0;
	const int qblocks = (queries - 1) / CHAMFER_BLOCK + 1, tiles = (references - 1) / CHAMFER_TILE + 1;
	const int fill = (CHAMFER_TARGET_BLOCKS - 1) / qblocks + 1;
	const int s = tiles < CHAMFER_MAX_SEGMENTS ? tiles : CHAMFER_MAX_SEGMENTS;
	return s < fill ? s : fill;
}
inline unsigned chamfer_blocks(int Q) { return dr::host::capped_blocks((size_t)Q, CHAMFER_BLOCK, CHAMFER_MAX_BLOCKS); }

// The references of segment seg of S, [first, end): the tiles [seg tiles / S, (seg + 1) tiles / S) of the ceil(R / CHAMFER_TILE) tiles of R
// references, cut at R.  For the tiled walks here and in dr_surface.h; the last tile may end beyond 2^31, so its end is formed in 64 bits.
struct ChamferRange
{
	int first, end;
};
constexpr ChamferRange chamfer_segment_range(int seg, int S, int R)
{
	const int tiles = (R - 1) / CHAMFER_TILE + 1;
	const int first = (int)((long long)seg * tiles / S) * CHAMFER_TILE;
	const long long last_tile = ((long long)(seg + 1) * tiles / S) * CHAMFER_TILE;
	return {first, last_tile < R ? (int)last_tile : R};
}
// with S <= tiles the ranges are whole tiles (but the end of the last), none is empty, and they are [0, R) in order: around a tile, and up to 2^31
constexpr bool chamfer_segments_partition()
{
	const int references[7] = {1, 255, 256, 257, 16129, 2147483647 - 256, 2147483647}, segments[4] = {1, 2, 63, 64};
	for (int R : references)
		for (int S : segments)
			for (int seg = 0, at = 0; seg < S && S <= (R - 1) / CHAMFER_TILE + 1; seg++)
			{
				const ChamferRange r = chamfer_segment_range(seg, S, R);
				if (r.first != at || r.end <= at || at % CHAMFER_TILE || (r.end % CHAMFER_TILE && r.end != R) || (seg + 1 == S && r.end != R))
					return false;
				at = r.end;
			}
	return true;
}
static_assert(chamfer_segments_partition(), "the segments of a walk are whole tiles, none empty, and partition the references in order");

struct ChamferArgs
{
	const double *vertices, *points, *point_weights, *vertex_weights, *params;
	double *terms, *loss, *vertices_b;
	uint32_t *nearest_vertex, *nearest_point;
	double *pd2, *vd2, *vg, *partials; // the scratch
	uint32_t *pidx, *vidx, *assign;
	unsigned *tickets;
	int V, P, n, Sp, Sv, directions, clear_tickets;
};

// The scratch layout of the overview, stated once: the dimensions (checked) and the split of a call -> a, and the bytes of its scratch; with a
// base, its arrays -> a.
inline size_t chamfer_carve(ChamferArgs &a, int V, int P, int n, void *base)
{
	a.V = V, a.P = P, a.n = n, a.Sp = chamfer_segments(P, V), a.Sv = chamfer_segments(V, P);
	const size_t N = (size_t)n, np = N * (size_t)P, sp = (size_t)a.Sp * np, sv = (size_t)a.Sv * N * (size_t)V;
	dr::host::ScratchCarver c = {(char *)base};
	a.pd2 = c.take<double>(sp), a.vd2 = c.take<double>(sv), a.vg = c.take<double>(3 * sv), a.partials = c.take<double>(2 * N * (size_t)CHAMFER_MAX_BLOCKS);
	a.pidx = c.take<uint32_t>(sp), a.vidx = c.take<uint32_t>(sv), a.assign = c.take<uint32_t>(np), a.tickets = c.take<unsigned>(2 * N);
	return c.whole_doubles();
}

// What the first launch of a call does (first_block: one workgroup per pose): the tickets the combine steps draw on; the launch boundaries order them.
template <class Args>
__device__ __forceinline__ void chamfer_clear_tickets(const Args &a, size_t pose, bool first_block)
{
	if (first_block && threadIdx.x == 0)
		a.tickets[pose] = 0, a.tickets[(size_t)a.n + pose] = 0;
}

struct alignas(16) ChamferRef
{
	double x, y, z, w;
};

// grid: (ceil(Q / CHAMFER_BLOCK), S, n).  SEARCH && !GATHER serves both directions of the search (to_vertices: the queries are the points).
template <bool SEARCH, bool GATHER>
__global__ __launch_bounds__(CHAMFER_BLOCK) void chamfer_walk_kernel(ChamferArgs a, int to_vertices)
{
	__shared__ ChamferRef s_ref[SEARCH ? CHAMFER_TILE : 1];
	__shared__ uint32_t s_assign[GATHER ? CHAMFER_TILE : 1];
	const size_t pose = blockIdx.z;
	const int Q = to_vertices ? a.P : a.V, R = to_vertices ? a.V : a.P, S = (int)gridDim.y, seg = (int)blockIdx.y;
	chamfer_clear_tickets(a, pose, a.clear_tickets && blockIdx.x == 0 && seg == 0);
	const double *const queries = (to_vertices ? a.points : a.vertices) + pose * (size_t)Q * 3;
	const double *const refs = (to_vertices ? a.vertices : a.points) + pose * (size_t)R * 3;
	const double *const ref_w = GATHER && a.point_weights ? a.point_weights + pose * (size_t)R : nullptr;
	const uint32_t *const assign = GATHER ? a.assign + pose * (size_t)R : nullptr;
	const ChamferRange range = chamfer_segment_range(seg, S, R);
	const int first = range.first, end = range.end;
	const int q = (int)blockIdx.x * CHAMFER_BLOCK + (int)threadIdx.x;
	const bool active = q < Q;
	const uint32_t me = active ? (uint32_t)q : CHAMFER_NO_QUERY;
	const double qx = active ? queries[3 * (size_t)q] : 0.0, qy = active ? queries[3 * (size_t)q + 1] : 0.0, qz = active ? queries[3 * (size_t)q + 2] : 0.0;
	double best = __builtin_inf(), gx = 0, gy = 0, gz = 0;
	uint32_t arg = (uint32_t)first;
	for (int base = first; base < end; base += CHAMFER_TILE)
	{
		const int count = end - base < CHAMFER_TILE ? end - base : CHAMFER_TILE;
		__syncthreads(); // (every thread is past the tile before)
		if ((int)threadIdx.x < count)
		{
			const size_t r = (size_t)base + threadIdx.x;
			if (SEARCH)
				s_ref[threadIdx.x] = {refs[3 * r], refs[3 * r + 1], refs[3 * r + 2], ref_w ? ref_w[r] : 1.0};
			if (GATHER)
				s_assign[threadIdx.x] = assign[r];
		}
		__syncthreads();
		for (int j = 0; j < count; j++)
		{
			if (SEARCH)
			{
				const ChamferRef r = s_ref[j];
				const double dx = qx - r.x, dy = qy - r.y, dz = qz - r.z;
				const double d2 = (dx * dx + dy * dy) + dz * dz;
				const bool better = d2 < best;
				best = better ? d2 : best;
				arg = better ? (uint32_t)(base + j) : arg;
				if (GATHER && s_assign[j] == me)
					gx += r.w * dx, gy += r.w * dy, gz += r.w * dz;
			}
			else if (s_assign[j] == me)
			{ // (gather alone: the point is fetched where it matches)
				const size_t r = (size_t)base + j;
				const double w = ref_w ? ref_w[r] : 1.0;
				gx += w * (qx - refs[3 * r]), gy += w * (qy - refs[3 * r + 1]), gz += w * (qz - refs[3 * r + 2]);
			}
		}
	}
	if (!active)
		return;
	const size_t at = (pose * (size_t)S + (size_t)seg) * (size_t)Q + (size_t)q;
	if (SEARCH)
	{
		(to_vertices ? a.pd2 : a.vd2)[at] = best;
		(to_vertices ? a.pidx : a.vidx)[at] = arg;
	}
	if (GATHER)
		a.vg[3 * at] = gx, a.vg[3 * at + 1] = gy, a.vg[3 * at + 2] = gz;
}

// the minimum of a query over the segments, in order, strict <: the lowest index wins
__device__ __forceinline__ void chamfer_combine(const double *d2, const uint32_t *idx, size_t pose, int S, size_t Q, size_t q, double &best, uint32_t &arg)
{
	best = d2[pose * (size_t)S * Q + q], arg = idx[pose * (size_t)S * Q + q];
	for (int s = 1; s < S; s++)
	{
		const size_t at = (pose * (size_t)S + (size_t)s) * Q + q;
		const double d = d2[at];
		const bool better = d < best;
		best = better ? d : best;
		arg = better ? idx[at] : arg;
	}
}

// grid: (chamfer_blocks(P), n)
__global__ __launch_bounds__(CHAMFER_BLOCK) void chamfer_points_kernel(ChamferArgs a)
{
	const size_t pose = blockIdx.y, P = (size_t)a.P;
	const double tau = a.params[2], tau2 = tau * tau;
	double s[1] = {0};
	for (size_t k = (size_t)blockIdx.x * CHAMFER_BLOCK + threadIdx.x; k < P; k += (size_t)gridDim.x * CHAMFER_BLOCK)
	{
		double best;
		uint32_t arg;
		chamfer_combine(a.pd2, a.pidx, pose, a.Sp, P, k, best, arg);
		const bool near = best <= tau2;
		a.assign[pose * P + k] = near ? arg : CHAMFER_NONE;
		if (a.nearest_vertex)
			a.nearest_vertex[pose * P + k] = arg;
		const double w = a.point_weights ? a.point_weights[pose * P + k] : 1.0;
		s[0] += w * (near ? best : tau2);
	}
	double total[1];
	if (grid_sum<1>(s, a.partials + pose * CHAMFER_MAX_BLOCKS, a.tickets + pose, total, blockIdx.x, gridDim.x) && threadIdx.x == 0)
		a.terms[2 * pose] = total[0];
}

// The two directions and the parameters of a vertices combine step (chamfer_vertices_kernel, surface_vertices_kernel)
struct ChamferMix
{
	bool to_mesh, to_points;
	double mix0, mix1, tau2;
};
template <class Args>
__device__ __forceinline__ ChamferMix chamfer_mix(const Args &a)
{
	const double tau = a.params[2];
	return {(a.directions & DEODR_HIP_CHAMFER_POINTS_TO_MESH) != 0, (a.directions & DEODR_HIP_CHAMFER_MESH_TO_POINTS) != 0, a.params[0], a.params[1], tau * tau};
}

// mesh -> points of vertex i: its minimum over the segments -> nearest_point, its share of term_1 added to `sum`, its pull added to (bx, by, bz)
template <class Args>
__device__ __forceinline__ void chamfer_vertex_to_points(const Args &a, const ChamferMix &m, size_t pose, size_t i, double &sum, double &bx, double &by, double &bz)
{
	const size_t V = (size_t)a.V, P = (size_t)a.P;
	double best;
	uint32_t arg;
	chamfer_combine(a.vd2, a.vidx, pose, a.Sv, V, i, best, arg);
	if (a.nearest_point)
		a.nearest_point[pose * V + i] = arg;
	const bool near = best <= m.tau2;
	const double u = a.vertex_weights ? a.vertex_weights[i] : 1.0;
	sum += u * (near ? best : m.tau2);
	if (near)
	{
		const double *const v = a.vertices + 3 * (pose * V + i), *const p = a.points + 3 * (pose * P + arg);
		bx += m.mix1 * ((2 * u) * (v[0] - p[0])), by += m.mix1 * ((2 * u) * (v[1] - p[1])), bz += m.mix1 * ((2 * u) * (v[2] - p[2]));
	}
}

// the tail of a vertices combine step: term_1 through grid_sum on the second ticket; the last workgroup of a pose writes terms and loss
// (term_0 is there already: the points combine step ran launches before)
template <class Args>
__device__ __forceinline__ void chamfer_write_terms(const Args &a, const ChamferMix &m, size_t pose, const double (&s)[1])
{
	double total[1];
	if (grid_sum<1>(s, a.partials + ((size_t)a.n + pose) * CHAMFER_MAX_BLOCKS, a.tickets + (size_t)a.n + pose, total, blockIdx.x, gridDim.x) && threadIdx.x == 0)
	{
		const double term0 = m.to_mesh ? a.terms[2 * pose] : 0.0, term1 = m.to_points ? total[0] : 0.0;
		a.terms[2 * pose] = term0, a.terms[2 * pose + 1] = term1;
		a.loss[pose] = (m.to_mesh ? m.mix0 * term0 : 0.0) + (m.to_points ? m.mix1 * term1 : 0.0);
	}
}

// grid: (chamfer_blocks(V), n)
__global__ __launch_bounds__(CHAMFER_BLOCK) void chamfer_vertices_kernel(ChamferArgs a)
{
	const size_t pose = blockIdx.y, V = (size_t)a.V;
	const ChamferMix m = chamfer_mix(a);
	double s[1] = {0};
	for (size_t i = (size_t)blockIdx.x * CHAMFER_BLOCK + threadIdx.x; i < V; i += (size_t)gridDim.x * CHAMFER_BLOCK)
	{
		double bx = 0, by = 0, bz = 0;
		if (m.to_mesh)
		{
			double gx = 0, gy = 0, gz = 0;
			for (int seg = 0; seg < a.Sv; seg++)
			{
				const double *const g = a.vg + 3 * ((pose * (size_t)a.Sv + (size_t)seg) * V + i);
				gx += g[0], gy += g[1], gz += g[2];
			}
			bx = m.mix0 * (2 * gx), by = m.mix0 * (2 * gy), bz = m.mix0 * (2 * gz);
		}
		if (m.to_points)
			chamfer_vertex_to_points(a, m, pose, i, s[0], bx, by, bz);
		double *const out = a.vertices_b + 3 * (pose * V + i);
		out[0] = bx, out[1] = by, out[2] = bz;
	}
	chamfer_write_terms(a, m, pose, s);
}

} // namespace
