// The point-to-surface distance with the closest face found over a uniform grid of hashed cells holding the posed triangles
// (include_staged/deodr_hip_surface_grid.h has the operation and the contract, DESIGN.md 4p the exactness argument).  Composed of what the tree
// has: the face records, surface_closest() and the two combine steps of dr_surface.h (with one segment), the cells, the hash, the points' grid,
// the search of the vertices and the sorted-assignment gather of dr_chamfer_grid.h, the sort of dr_sort.h.  ONE record per face: a face is keyed
// by the cell of the minimum corner of its bounding box, and the cell edge of a pose is never below the longest side of any face's box, so a face
// lies in the cells key .. key + 1 per axis and is evaluated at most once per query (but for cells that share a bucket).
//
// surface_grid_prep_kernel    a thread per (pose, face): surface_record() -> rec (what the points' combine step reads by original index), the
//                             longest side of the face's box -> a maximum per workgroup -> emax.  The first launch with points -> mesh on: it
//                             clears the arrival tickets.
// surface_grid_keys_kernel    every workgroup takes the maximum of the pose's emax (at most CHAMFER_MAX_BLOCKS values; a maximum is exact in any
//                             order, so no ticket and no last workgroup is needed: the launch boundary orders it) -> E, h_f = max(cell_size,
//                             max_distance / RINGS, E) -> hf (workgroup 0); a thread per face: the cell of the box's minimum corner -> bucket ->
//                             keys; the same threads clear the bucket table.
// (sort_keys)                 the buckets, stably
// surface_grid_build_kernel   a thread per sorted position: the 128-byte record of face order[i], its original index in the sixteenth double ->
//                             srec[i]; the bounds of the buckets -> table.  A bucket is a run of whole 128-byte lines.
// (the points' grid of dr_chamfer_grid.h when mesh -> points is on: chamfer_grid_keys_kernel, sort, chamfer_grid_build_kernel)
// surface_grid_search_kernel  a thread per point, in the sorted order of the points' own grid where that exists.  Shell s = the key cells
//                             [c - s - 1, c + s]^3 not in shell s - 1; every record of every bucket through surface_closest(); the strict
//                             lexicographic minimum of (d2, original index); stops after the last shell that can hold a face within tau2, or after
//                             shell s >= 1 once best < (h_f s (1 - 2^-20))^2.  -> pd2, pidx (CHAMFER_NONE beyond tau2) at the point's ORIGINAL index.
// surface_points_kernel       dr_surface.h with one segment: nearest_face, barycentric, assign, the pull, term_0 in the brute-force op's order.
// (sort_keys)                 the assignment on ceil(log2(F + 1)) bits: the points of a face become a run, in increasing k; NONE sorts last
// surface_grid_gather_kernel  a wavefront per face: the bounds of its run by bisection, lane l adds the nine products of G(f, .) over the run's
//                             elements l, l + 64, ..., then the wavefront's tree -> fg.
// (chamfer_grid_search_kernel the vertices over the points' grid, in index order)
// surface_vertices_kernel     dr_surface.h with one segment: vertices_b over the corner table, nearest_point, term_1, loss.
//
// No floating-point atomics, no integer atomics but the tickets of grid_sum.  Scratch after its 64 counter bytes (unused), doubles first:
// rec [n][F][16], srec [n][F][16], records_p [n][P][4], pd2 [n][P], pull [n][P][6], fg [n][F][9], vd2 [n][V], emax [n][CHAMFER_MAX_BLOCKS], hf [n],
// partials [2][n][CHAMFER_MAX_BLOCKS]; then 4-byte words: table_f [n][Tf][2], table_p [n][Tp][2] (read as pairs: 8-byte aligned), pidx [n][P],
// vidx [n][V], assign [n][P], keys / sorted keys / order of the faces [3][n][F] and of the points [3][n][P], the sorted assignment and its order
// [2][n][P], tickets [2][n]; then the scratch of the sorts (surface_grid_carve).
#pragma once

namespace
{

static_assert(DEODR_HIP_SURFACE_GRID_NONE == CHAMFER_NONE, "one value for `no face`");
static_assert(DEODR_HIP_SURFACE_GRID_GATHER_FACES * 64 == CHAMFER_BLOCK, "a wavefront per face");
constexpr int SG_GATHER_FACES = DEODR_HIP_SURFACE_GRID_GATHER_FACES;

struct SurfaceGridArgs
{
	const double *points, *params;
	double *srec, *emax, *hf; // the sorted records; the workgroups' longest box sides; the cell edge of a pose
	uint32_t *keys, *sorted_keys, *order, *table;
	const uint32_t *point_order; // the sorted order of the points' own grid, nullptr: index order
	uint32_t *sorted_assign, *assign_order;
	unsigned *tickets;
	double cell_size;
	int n, table_bits, eblocks; // eblocks: the workgroups of the prep kernel
};

// What a call launches with: dr_surface.h's kernels take a (one segment per search and gather), the face grid's a and f, the points' grid and the
// search of the vertices g (dr_chamfer_grid.h), the sorts sort_words
struct SurfaceGridCall
{
	SurfaceArgs a;
	SurfaceGridArgs f;
	ChamferGridArgs g;
	uint32_t *sort_words;
};

// The scratch layout of the overview, stated once: the dimensions (checked) of a call -> a, f and g, and the bytes of its scratch; with a base,
// its arrays.
inline size_t surface_grid_carve(SurfaceGridCall &call, int V, int F, int P, int n, void *base)
{
	SurfaceArgs &a = call.a;
	SurfaceGridArgs &f = call.f;
	ChamferGridArgs &g = call.g;
	a.V = g.V = V, a.F = F, a.P = g.P = P, a.n = f.n = g.n = n, a.Sp = a.Sg = a.Sv = 1;
	f.table_bits = chamfer_grid_table_bits(F), f.eblocks = (int)chamfer_blocks(F);
	g.set[0].R = V, g.set[0].table_bits = 0, g.set[1].R = P, g.set[1].table_bits = chamfer_grid_table_bits(P);
	const size_t N = (size_t)n, nv = N * (size_t)V, np = N * (size_t)P, nf = N * (size_t)F;
	dr::host::ScratchCarver c = {(char *)base};
	a.rec = c.take<double>((size_t)SURFACE_REC * nf), f.srec = c.take<double>((size_t)SURFACE_REC * nf);
	g.set[0].records = nullptr, g.set[1].records = c.take<double>(4 * np);
	a.pd2 = c.take<double>(np), a.pull = c.take<double>(6 * np), a.fg = c.take<double>(9 * nf), a.vd2 = g.vd2 = c.take<double>(nv);
	f.emax = c.take<double>(N * (size_t)CHAMFER_MAX_BLOCKS), f.hf = c.take<double>(N), a.partials = c.take<double>(2 * N * (size_t)CHAMFER_MAX_BLOCKS);
	f.table = c.take<uint32_t>(2 * N * ((size_t)1 << f.table_bits)), g.set[1].table = c.take<uint32_t>(2 * N * ((size_t)1 << g.set[1].table_bits)); // (pairs: 8-byte aligned)
	g.set[0].table = nullptr;
	a.pidx = c.take<uint32_t>(np), a.vidx = g.vidx = c.take<uint32_t>(nv), a.assign = c.take<uint32_t>(np);
	f.keys = c.take<uint32_t>(nf), f.sorted_keys = c.take<uint32_t>(nf), f.order = c.take<uint32_t>(nf);
	g.set[0].keys = g.set[0].sorted_keys = g.set[0].order = nullptr; // (the vertices have no grid here)
	g.set[1].keys = c.take<uint32_t>(np), g.set[1].sorted_keys = c.take<uint32_t>(np), g.set[1].order = c.take<uint32_t>(np);
	f.sorted_assign = c.take<uint32_t>(np), f.assign_order = c.take<uint32_t>(np);
	a.tickets = f.tickets = g.tickets = c.take<unsigned>(2 * N);
	g.pd2 = nullptr, g.vg = nullptr, g.pidx = nullptr, g.sorted_assign = g.assign_order = nullptr;
	call.sort_words = c.take<uint32_t>(sort_scratch_words(F > P ? F : P, n));
	return c.used;
}

__device__ __forceinline__ double surface_grid_min3(double x, double y, double z)
{
	const double m = x < y ? x : y;
	return m < z ? m : z;
}
__device__ __forceinline__ double surface_grid_max3(double x, double y, double z)
{
	const double m = x > y ? x : y;
	return m > z ? m : z;
}

// the largest value of a workgroup of CHAMFER_BLOCK threads, returned to every thread; s_max: CHAMFER_BLOCK doubles of LDS.  A maximum is exact in
// any order, so the tree's shape does not matter
__device__ __forceinline__ double surface_grid_block_max(double mine, double *s_max)
{
	s_max[threadIdx.x] = mine;
	__syncthreads();
	for (int half = CHAMFER_BLOCK / 2; half > 0; half >>= 1)
	{
		if ((int)threadIdx.x < half)
			s_max[threadIdx.x] = s_max[threadIdx.x] > s_max[threadIdx.x + half] ? s_max[threadIdx.x] : s_max[threadIdx.x + half];
		__syncthreads();
	}
	return s_max[0];
}

// the run [first, end) of the value `owner` in a sorted row of P assignments: the first position whose assignment is >= owner, and >= owner + 1
// (CHAMFER_NONE is above every owner), by bisection.  Wave-uniform arguments make it scalar loads, once per wavefront
struct SurfaceGridRun
{
	size_t first, end;
};
__device__ __forceinline__ SurfaceGridRun surface_grid_run(const uint32_t *sorted, size_t P, size_t owner)
{
	size_t bound[2];
#pragma unroll
	for (int e = 0; e < 2; e++)
	{
		size_t lo = 0, hi = P;
		while (lo < hi)
		{
			const size_t mid = lo + (hi - lo) / 2;
			if (sorted[mid] < (uint32_t)(owner + e))
				lo = mid + 1;
			else
				hi = mid;
		}
		bound[e] = lo;
	}
	return {bound[0], bound[1]};
}

// grid: (chamfer_blocks(F), n)
__global__ __launch_bounds__(CHAMFER_BLOCK) void surface_grid_prep_kernel(SurfaceArgs a, SurfaceGridArgs g)
{
	__shared__ double s_max[CHAMFER_BLOCK];
	const size_t pose = blockIdx.y, F = (size_t)a.F;
	chamfer_clear_tickets(a, pose, blockIdx.x == 0);
	const double *const vertices = a.vertices + pose * (size_t)a.V * 3;
	double *const rec = a.rec + (size_t)SURFACE_REC * pose * F;
	double longest = 0;
	for (size_t f = (size_t)blockIdx.x * CHAMFER_BLOCK + threadIdx.x; f < F; f += (size_t)gridDim.x * CHAMFER_BLOCK)
	{
		const SurfaceRec r = surface_record(vertices, a.faces + 3 * f);
		surface_copy(rec + (size_t)SURFACE_REC * f, (const double *)&r);
#pragma unroll
		for (int x = 0; x < 3; x++)
		{
			const double side = surface_grid_max3(r.a[x], r.b[x], r.c[x]) - surface_grid_min3(r.a[x], r.b[x], r.c[x]);
			longest = side > longest ? side : longest;
		}
	}
	longest = surface_grid_block_max(longest, s_max);
	if (threadIdx.x == 0)
		g.emax[pose * CHAMFER_MAX_BLOCKS + blockIdx.x] = longest;
}

// grid: (chamfer_blocks(max(F, T)), n)
__global__ __launch_bounds__(CHAMFER_BLOCK) void surface_grid_keys_kernel(SurfaceArgs a, SurfaceGridArgs g)
{
	__shared__ double s_max[CHAMFER_BLOCK];
	const size_t pose = blockIdx.y, F = (size_t)a.F, T = (size_t)1 << g.table_bits;
	double longest = 0;
	for (int b = (int)threadIdx.x; b < g.eblocks; b += CHAMFER_BLOCK) // (eblocks <= CHAMFER_MAX_BLOCKS: two values per thread at most)
	{
		const double e = g.emax[pose * CHAMFER_MAX_BLOCKS + (size_t)b];
		longest = e > longest ? e : longest;
	}
	longest = surface_grid_block_max(longest, s_max);
	const double least = chamfer_grid_h(a.params, g.cell_size), h = longest > least ? longest : least;
	if (blockIdx.x == 0 && threadIdx.x == 0)
		g.hf[pose] = h;
	const double *const rec = a.rec + (size_t)SURFACE_REC * pose * F;
	const uint32_t mask = (uint32_t)(T - 1);
	for (size_t i = (size_t)blockIdx.x * CHAMFER_BLOCK + threadIdx.x; i < F || i < T; i += (size_t)gridDim.x * CHAMFER_BLOCK)
	{
		if (i < F)
		{
			const double *const r = rec + (size_t)SURFACE_REC * i; // a, b, c: the first nine doubles
			const int cx = chamfer_grid_cell(surface_grid_min3(r[0], r[3], r[6]), h), cy = chamfer_grid_cell(surface_grid_min3(r[1], r[4], r[7]), h);
			const int cz = chamfer_grid_cell(surface_grid_min3(r[2], r[5], r[8]), h);
			g.keys[pose * F + i] = chamfer_grid_hash(cx, cy, cz) & mask;
		}
		if (i < T)
			g.table[2 * (pose * T + i)] = 0, g.table[2 * (pose * T + i) + 1] = 0;
	}
}

// grid: (chamfer_blocks(F), n)
__global__ __launch_bounds__(CHAMFER_BLOCK) void surface_grid_build_kernel(SurfaceArgs a, SurfaceGridArgs g)
{
	const size_t pose = blockIdx.y, F = (size_t)a.F, T = (size_t)1 << g.table_bits;
	const uint32_t *const sorted = g.sorted_keys + pose * F, *const order = g.order + pose * F;
	const double *const rec = a.rec + (size_t)SURFACE_REC * pose * F;
	double *const srec = g.srec + (size_t)SURFACE_REC * pose * F;
	uint32_t *const table = g.table + 2 * pose * T;
	for (size_t i = (size_t)blockIdx.x * CHAMFER_BLOCK + threadIdx.x; i < F; i += (size_t)gridDim.x * CHAMFER_BLOCK)
	{
		const uint32_t f = order[i], key = sorted[i]; // (f < F, key < T: what the sort was given)
		SurfaceRec r;
		surface_copy((double *)&r, rec + (size_t)SURFACE_REC * f);
		r.pad = (double)f; // (exact: F < 2^53)
		surface_copy(srec + (size_t)SURFACE_REC * i, (const double *)&r);
		if (i == 0 || sorted[i - 1] != key)
			table[2 * (size_t)key] = (uint32_t)i;
		if (i + 1 == F || sorted[i + 1] != key)
			table[2 * (size_t)key + 1] = (uint32_t)(i + 1);
	}
}

// the run of records of the bucket of a key cell
__device__ __forceinline__ void surface_grid_probe(const double *srec, const uint32_t *table, uint32_t mask, int cx, int cy, int cz, double px, double py,
												   double pz, double &best, uint32_t &arg)
{
	const uint32_t bucket = chamfer_grid_hash(cx, cy, cz) & mask;
	const uint2 run = *(const uint2 *)(table + 2 * (size_t)bucket);
	for (uint32_t i = run.x; i < run.y; i++)
	{
		SurfaceRec r;
		surface_copy((double *)&r, srec + (size_t)SURFACE_REC * i);
		const SurfaceHit hit = surface_closest(r, px, py, pz);
		const uint32_t f = (uint32_t)r.pad;
		const bool better = hit.d2 < best || (hit.d2 == best && f < arg);
		best = better ? hit.d2 : best;
		arg = better ? f : arg;
	}
}

// grid: (ceil(P / CHAMFER_BLOCK), n)
__global__ __launch_bounds__(CHAMFER_BLOCK) void surface_grid_search_kernel(SurfaceArgs a, SurfaceGridArgs g)
{
	const size_t pose = blockIdx.y, P = (size_t)a.P, F = (size_t)a.F, T = (size_t)1 << g.table_bits;
	const size_t t = (size_t)blockIdx.x * CHAMFER_BLOCK + threadIdx.x;
	if (t >= P)
		return;
	const size_t k = g.point_order ? g.point_order[pose * P + t] : t;
	const double *const p = g.points + 3 * (pose * P + k);
	const double px = p[0], py = p[1], pz = p[2];
	const double tau = a.params[2], tau2 = tau * tau, h = g.hf[pose];
	const double reach = ceil(tau / h) + 1.0; // (one shell for the rounding of x / h; tau / h <= CG_RINGS by the choice of h)
	const int last = reach < (double)(CG_RINGS + 1) ? (int)reach : CG_RINGS + 1;
	const int cx = chamfer_grid_cell(px, h), cy = chamfer_grid_cell(py, h), cz = chamfer_grid_cell(pz, h);
	const double *const srec = g.srec + (size_t)SURFACE_REC * pose * F;
	const uint32_t *const table = g.table + 2 * pose * T;
	const uint32_t mask = (uint32_t)(T - 1);
	double best = __builtin_inf();
	uint32_t arg = CHAMFER_NONE;
	for (int s = 0; s <= last; s++)
	{ // the key cells [-s - 1, s]^3 around the point's cell that shell s - 1 did not hold: a face keyed there reaches one cell further up
		for (int dz = -s - 1; dz <= s; dz++)
			for (int dy = -s - 1; dy <= s; dy++)
			{
				const bool face = dz == -s - 1 || dz == s || dy == -s - 1 || dy == s; // (the whole row is on the shell; otherwise its two ends are)
				for (int dx = -s - 1; dx <= s; dx += face ? 1 : 2 * s + 1)
					surface_grid_probe(srec, table, mask, cx + dx, cy + dy, cz + dz, px, py, pz, best, arg);
			}
		const double clear = h * ((double)s * CG_EXIT_MARGIN);
		if (s >= 1 && best < clear * clear) // (strictly: a face not yet visited at exactly `best` with a lower index would have to win)
			break;
	}
	const bool near = best <= tau2;
	a.pd2[pose * P + k] = best;
	a.pidx[pose * P + k] = near ? arg : CHAMFER_NONE;
}

// grid: (ceil(F / SG_GATHER_FACES), n)
__global__ __launch_bounds__(CHAMFER_BLOCK) void surface_grid_gather_kernel(SurfaceArgs a, SurfaceGridArgs g)
{
	const size_t pose = blockIdx.y, F = (size_t)a.F, P = (size_t)a.P;
	const size_t f = (size_t)blockIdx.x * SG_GATHER_FACES + (size_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // (wave-uniform: the bisection below is scalar loads, once per wavefront)
	if (f >= F) // (the whole wavefront)
		return;
	const int lane = threadIdx.x & 63;
	const uint32_t *const sorted = g.sorted_assign + pose * P, *const order = g.assign_order + pose * P;
	const SurfaceGridRun run = surface_grid_run(sorted, P, f);
	const double *const pull = a.pull + 6 * pose * P;
	double sum[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
	for (size_t at = run.first + lane; at < run.end; at += 64)
	{
		const double *const t = pull + 6 * (size_t)order[at];
#pragma unroll
		for (int c = 0; c < 3; c++)
			sum[3 * c] += t[c] * t[3], sum[3 * c + 1] += t[c] * t[4], sum[3 * c + 2] += t[c] * t[5];
	}
#pragma unroll
	for (int x = 0; x < 9; x++)
		sum[x] = wave_sum(sum[x]); // (all 64 lanes are here)
	if (lane == 0)
	{
		double *const out = a.fg + 9 * (pose * F + f);
#pragma unroll
		for (int x = 0; x < 9; x++)
			out[x] = sum[x];
	}
}

} // namespace
