// The closest-point (Chamfer) energy with the nearest neighbours found over a uniform grid of hashed cells (include/deodr_hip_chamfer_grid.h has
// the operation and the contract, DESIGN.md 4o the exactness argument).  On the machinery of dr_chamfer.h -- its ticket clear and its combine
// steps, with one segment -- and of dr_sort.h:
//
// chamfer_grid_keys_kernel    a thread per reference: cell = clamp(floor(x / h)) per axis -> bucket = hash(cell) & (T - 1) -> keys; the same
//                             threads clear the bucket table (start = end = 0: empty).  The first one of a call clears the arrival tickets.
// (sort_keys)                 the buckets, stably: sorted keys and the order
// chamfer_grid_build_kernel   a thread per sorted position i: the record (x, y, z, index) of reference order[i] -> records[i]; where the sorted
//                             key differs from the one before / after, the start / end of its bucket -> table.
// chamfer_grid_search_kernel  a thread per query, in the sorted order of the queries' own grid where that exists (the queries of a wavefront are
//                             neighbours in space and probe the same buckets: their loads hit the same cache lines), in index order otherwise.
//                             Ring by ring around the query's cell: every cell of the shell, its bucket's run of records, the strict
//                             lexicographic minimum of (d2, index) -- neither the visiting order nor a bucket probed twice changes it.  Stops
//                             after the last ring that can hold a pair within tau2, or earlier once every reference not yet visited is provably
//                             strictly farther than the best.  -> d2 and index (CHAMFER_NONE beyond tau2) of the query, at its ORIGINAL index.
// chamfer_points_kernel       dr_chamfer.h: term_0 in the brute-force op's order, nearest_vertex, the assignment (CHAMFER_NONE beyond tau2)
// (sort_keys)                 the assignment on ceil(log2(V + 1)) bits: the points of a vertex become a run, in increasing k; NONE sorts last
// chamfer_grid_gather_kernel  a wavefront per vertex: the bounds of its run by bisection, lane l adds w_k (v_i - p_k) over the run's elements l,
//                             l + 64, ..., then the wavefront's tree -> vg.
// chamfer_vertices_kernel     dr_chamfer.h: vertices_b, nearest_point, term_1, loss.
//
// No floating-point atomics, no integer atomics but the tickets of grid_sum.  Scratch after its 64 counter bytes (unused), doubles first:
// records_v [n][V][4], records_p [n][P][4], pd2 [n][P], vd2 [n][V], vg [n][V][3], partials [2][n][CHAMFER_MAX_BLOCKS]; then 4-byte words:
// table_v [n][Tv][2], table_p [n][Tp][2] (read as pairs: 8-byte aligned), pidx [n][P], vidx [n][V], assign [n][P], keys / sorted keys / order of
// the vertices [3][n][V] and of the points [3][n][P], the sorted assignment and its order [2][n][P], tickets [2][n]; then the scratch of the sorts
// (chamfer_grid_carve).
#pragma once

namespace
{

constexpr int CG_RINGS = DEODR_HIP_CHAMFER_GRID_RINGS, CG_MAX_ITEMS = DEODR_HIP_CHAMFER_GRID_MAX_ITEMS;
constexpr int CG_MIN_TABLE_BITS = DEODR_HIP_CHAMFER_GRID_MIN_TABLE_BITS, CG_MAX_TABLE_BITS = DEODR_HIP_CHAMFER_GRID_MAX_TABLE_BITS;
constexpr int CG_GATHER_VERTICES = DEODR_HIP_CHAMFER_GRID_GATHER_VERTICES, CG_TABLE_LOAD = DEODR_HIP_CHAMFER_GRID_TABLE_LOAD;
constexpr double CG_CELL_LIMIT = (double)DEODR_HIP_CHAMFER_GRID_CELL_LIMIT;
constexpr double CG_EXIT_MARGIN = 1.0 - 1.0 / 1048576.0; // 1 - 2^-20: what the rounding of x / h can take from a distance in cells
static_assert(DEODR_HIP_CHAMFER_GRID_NONE == CHAMFER_NONE, "one value for `no neighbour`");
static_assert(CG_GATHER_VERTICES * 64 == CHAMFER_BLOCK, "a wavefront per vertex");
static_assert(CG_MAX_ITEMS <= SORT_MAX_ITEMS && CG_MAX_TABLE_BITS <= 32 - 6, "every set can be sorted, a bucket number is a sort key");

inline int chamfer_grid_table_bits(int references)
{
	if (references <= 0 || references > CG_MAX_ITEMS)
		return 0;
	int b = CG_MIN_TABLE_BITS;
	while (b < CG_MAX_TABLE_BITS && (1LL << b) < (long long)CG_TABLE_LOAD * references)
		b++;
	return b;
}
inline int chamfer_grid_assign_bits(int V)
{ // ceil(log2(V + 1)): V + 1 values, the vertices and `none`
	int b = 1;
	while ((1LL << b) < (long long)V + 1)
		b++;
	return b;
}

struct ChamferGridSet
{ // one grid: the references of a direction
	const double *coords; // [n][R][3]
	double *records;	  // [n][R][4]: x, y, z, the index (the low word of the fourth double)
	uint32_t *keys, *sorted_keys, *order; // [n][R]
	uint32_t *table;					  // [n][T][2]: start, end of a bucket's run of records
	int R, table_bits;
};

struct ChamferGridArgs
{
	ChamferGridSet set[2]; // 0: the vertices, 1: the points
	const double *params, *point_weights;
	double *pd2, *vd2, *vg;
	uint32_t *pidx, *vidx, *sorted_assign, *assign_order;
	unsigned *tickets;
	double cell_size;
	int V, P, n, clear_tickets;
};

// What a call launches with: the grids' kernels take g, the combine steps of dr_chamfer.h a (one segment per search), the sorts sort_words
struct ChamferGridCall
{
	ChamferGridArgs g;
	ChamferArgs a;
	uint32_t *sort_words;
};

// The scratch layout of the overview, stated once: the dimensions (checked) of a call -> g and a, and the bytes of its scratch; with a base, its
// arrays -> g, a (the ones both read: the same) and sort_words.
inline size_t chamfer_grid_carve(ChamferGridCall &call, int V, int P, int n, void *base)
{
	ChamferGridArgs &g = call.g;
	ChamferArgs &a = call.a;
	g.V = a.V = V, g.P = a.P = P, g.n = a.n = n, a.Sp = a.Sv = 1;
	g.set[0].R = V, g.set[0].table_bits = chamfer_grid_table_bits(V), g.set[1].R = P, g.set[1].table_bits = chamfer_grid_table_bits(P);
	const size_t N = (size_t)n, nv = N * (size_t)V, np = N * (size_t)P;
	dr::host::ScratchCarver c = {(char *)base};
	g.set[0].records = c.take<double>(4 * nv), g.set[1].records = c.take<double>(4 * np);
	a.pd2 = g.pd2 = c.take<double>(np), a.vd2 = g.vd2 = c.take<double>(nv), a.vg = g.vg = c.take<double>(3 * nv);
	a.partials = c.take<double>(2 * N * (size_t)CHAMFER_MAX_BLOCKS);
	for (ChamferGridSet &s : g.set)
		s.table = c.take<uint32_t>(2 * N * ((size_t)1 << s.table_bits)); // (pairs: 8-byte aligned)
	a.pidx = g.pidx = c.take<uint32_t>(np), a.vidx = g.vidx = c.take<uint32_t>(nv), a.assign = c.take<uint32_t>(np);
	for (ChamferGridSet &s : g.set)
		s.keys = c.take<uint32_t>(N * (size_t)s.R), s.sorted_keys = c.take<uint32_t>(N * (size_t)s.R), s.order = c.take<uint32_t>(N * (size_t)s.R);
	g.sorted_assign = c.take<uint32_t>(np), g.assign_order = c.take<uint32_t>(np);
	a.tickets = g.tickets = c.take<unsigned>(2 * N);
	call.sort_words = c.take<uint32_t>(sort_scratch_words(V > P ? V : P, n));
	return c.used;
}

struct ChamferGridRecord
{
	double x, y, z;
	uint32_t index, unused;
};
static_assert(sizeof(ChamferGridRecord) == 32, "four doubles");

__device__ __forceinline__ double chamfer_grid_h(const double *params, double cell_size)
{
	const double least = params[2] / (double)CG_RINGS;
	return cell_size > least ? cell_size : least;
}
__device__ __forceinline__ int chamfer_grid_cell(double x, double h)
{
	const double c = floor(x / h); // (floor, not truncation: negative coordinates)
	return (int)(c < -CG_CELL_LIMIT ? -CG_CELL_LIMIT : c > CG_CELL_LIMIT ? CG_CELL_LIMIT : c);
}
__device__ __forceinline__ uint32_t chamfer_grid_hash(int x, int y, int z)
{
	uint32_t k = ((uint32_t)x * 73856093u) ^ ((uint32_t)y * 19349663u) ^ ((uint32_t)z * 83492791u);
	k ^= k >> 16, k *= 0x85EBCA6Bu, k ^= k >> 13, k *= 0xC2B2AE35u, k ^= k >> 16;
	return k;
}

// grid: (chamfer_blocks(max(R, T)), n)
__global__ __launch_bounds__(CHAMFER_BLOCK) void chamfer_grid_keys_kernel(ChamferGridArgs a, int which)
{
	const ChamferGridSet &s = a.set[which];
	const size_t pose = blockIdx.y, R = (size_t)s.R, T = (size_t)1 << s.table_bits;
	chamfer_clear_tickets(a, pose, a.clear_tickets && blockIdx.x == 0);
	const double h = chamfer_grid_h(a.params, a.cell_size);
	const uint32_t mask = (uint32_t)(T - 1);
	for (size_t i = (size_t)blockIdx.x * CHAMFER_BLOCK + threadIdx.x; i < R || i < T; i += (size_t)gridDim.x * CHAMFER_BLOCK)
	{
		if (i < R)
		{
			const double *const c = s.coords + 3 * (pose * R + i);
			s.keys[pose * R + i] = chamfer_grid_hash(chamfer_grid_cell(c[0], h), chamfer_grid_cell(c[1], h), chamfer_grid_cell(c[2], h)) & mask;
		}
		if (i < T)
			s.table[2 * (pose * T + i)] = 0, s.table[2 * (pose * T + i) + 1] = 0;
	}
}

// grid: (chamfer_blocks(R), n)
__global__ __launch_bounds__(CHAMFER_BLOCK) void chamfer_grid_build_kernel(ChamferGridArgs a, int which)
{
	const ChamferGridSet &s = a.set[which];
	const size_t pose = blockIdx.y, R = (size_t)s.R, T = (size_t)1 << s.table_bits;
	const uint32_t *const sorted = s.sorted_keys + pose * R, *const order = s.order + pose * R;
	ChamferGridRecord *const records = (ChamferGridRecord *)s.records + pose * R;
	uint32_t *const table = s.table + 2 * pose * T;
	for (size_t i = (size_t)blockIdx.x * CHAMFER_BLOCK + threadIdx.x; i < R; i += (size_t)gridDim.x * CHAMFER_BLOCK)
	{
		const uint32_t r = order[i], key = sorted[i]; // (r < R, key < T: what the sort was given)
		const double *const c = s.coords + 3 * (pose * R + r);
		records[i] = {c[0], c[1], c[2], r, 0u};
		if (i == 0 || sorted[i - 1] != key)
			table[2 * (size_t)key] = (uint32_t)i;
		if (i + 1 == R || sorted[i + 1] != key)
			table[2 * (size_t)key + 1] = (uint32_t)(i + 1);
	}
}

// the run of records of the bucket of a cell
__device__ __forceinline__ void chamfer_grid_probe(const ChamferGridRecord *records, const uint32_t *table, uint32_t mask, int cx, int cy, int cz, double qx,
												   double qy, double qz, double &best, uint32_t &arg)
{
	const uint32_t bucket = chamfer_grid_hash(cx, cy, cz) & mask;
	const uint2 run = *(const uint2 *)(table + 2 * (size_t)bucket);
	for (uint32_t i = run.x; i < run.y; i++)
	{
		const ChamferGridRecord r = records[i];
		const double dx = qx - r.x, dy = qy - r.y, dz = qz - r.z;
		const double d2 = (dx * dx + dy * dy) + dz * dz;
		const bool better = d2 < best || (d2 == best && r.index < arg);
		best = better ? d2 : best;
		arg = better ? r.index : arg;
	}
}

// grid: (ceil(Q / CHAMFER_BLOCK), n).  to_vertices: the queries are the points, the references the vertices.  in_grid_order: the queries' own grid exists
__global__ __launch_bounds__(CHAMFER_BLOCK) void chamfer_grid_search_kernel(ChamferGridArgs a, int to_vertices, int in_grid_order)
{
	const ChamferGridSet &refs = a.set[to_vertices ? 0 : 1], &own = a.set[to_vertices ? 1 : 0];
	const size_t pose = blockIdx.y, Q = (size_t)own.R, R = (size_t)refs.R, T = (size_t)1 << refs.table_bits;
	const size_t t = (size_t)blockIdx.x * CHAMFER_BLOCK + threadIdx.x;
	if (t >= Q)
		return;
	const size_t q = in_grid_order ? own.order[pose * Q + t] : t;
	const double *const c = own.coords + 3 * (pose * Q + q);
	const double qx = c[0], qy = c[1], qz = c[2];
	const double tau = a.params[2], tau2 = tau * tau, h = chamfer_grid_h(a.params, a.cell_size);
	const double reach = ceil(tau / h) + 1.0; // (one ring for the rounding of x / h; tau / h <= CG_RINGS by the choice of h)
	const int last = reach < (double)(CG_RINGS + 1) ? (int)reach : CG_RINGS + 1;
	const int cx = chamfer_grid_cell(qx, h), cy = chamfer_grid_cell(qy, h), cz = chamfer_grid_cell(qz, h);
	const ChamferGridRecord *const records = (const ChamferGridRecord *)refs.records + pose * R;
	const uint32_t *const table = refs.table + 2 * pose * T;
	const uint32_t mask = (uint32_t)(T - 1);
	double best = __builtin_inf();
	uint32_t arg = CHAMFER_NONE;
	chamfer_grid_probe(records, table, mask, cx, cy, cz, qx, qy, qz, best, arg);
	for (int s = 1; s <= last; s++)
	{
		for (int dz = -s; dz <= s; dz++)
			for (int dy = -s; dy <= s; dy++)
			{
				const bool face = dz == -s || dz == s || dy == -s || dy == s; // (the whole row is on the shell; otherwise its two ends are)
				for (int dx = -s; dx <= s; dx += face ? 1 : 2 * s)
					chamfer_grid_probe(records, table, mask, cx + dx, cy + dy, cz + dz, qx, qy, qz, best, arg);
			}
		const double clear = h * ((double)s * CG_EXIT_MARGIN);
		if (best < clear * clear) // (strictly: a reference not yet visited at exactly `best` with a lower index would have to win)
			break;
	}
	const bool near = best <= tau2;
	(to_vertices ? a.pd2 : a.vd2)[pose * Q + q] = best;
	(to_vertices ? a.pidx : a.vidx)[pose * Q + q] = near ? arg : CHAMFER_NONE;
}

// grid: (ceil(V / CG_GATHER_VERTICES), n)
__global__ __launch_bounds__(CHAMFER_BLOCK) void chamfer_grid_gather_kernel(ChamferGridArgs a)
{
	const size_t pose = blockIdx.y, V = (size_t)a.V, P = (size_t)a.P;
	const size_t i = (size_t)blockIdx.x * CG_GATHER_VERTICES + (size_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // (wave-uniform: the bisection below is scalar loads, once per wavefront)
	if (i >= V) // (the whole wavefront)
		return;
	const int lane = threadIdx.x & 63;
	const uint32_t *const sorted = a.sorted_assign + pose * P, *const order = a.assign_order + pose * P;
	size_t bound[2];
#pragma unroll
	for (int e = 0; e < 2; e++)
	{ // the first position whose assignment is >= i + e (CHAMFER_NONE is above every vertex)
		size_t lo = 0, hi = P;
		while (lo < hi)
		{
			const size_t mid = lo + (hi - lo) / 2;
			if (sorted[mid] < (uint32_t)(i + e))
				lo = mid + 1;
			else
				hi = mid;
		}
		bound[e] = lo;
	}
	const double *const v = a.set[0].coords + 3 * (pose * V + i), *const points = a.set[1].coords + 3 * pose * P;
	const double *const weights = a.point_weights ? a.point_weights + pose * P : nullptr;
	const double vx = v[0], vy = v[1], vz = v[2];
	double gx = 0, gy = 0, gz = 0;
	for (size_t at = bound[0] + lane; at < bound[1]; at += 64)
	{
		const size_t k = order[at];
		const double w = weights ? weights[k] : 1.0;
		gx += w * (vx - points[3 * k]), gy += w * (vy - points[3 * k + 1]), gz += w * (vz - points[3 * k + 2]);
	}
	gx = wave_sum(gx), gy = wave_sum(gy), gz = wave_sum(gz); // (all 64 lanes are here)
	if (lane == 0)
	{
		double *const out = a.vg + 3 * (pose * V + i);
		out[0] = gx, out[1] = gy, out[2] = gz;
	}
}

} // namespace
