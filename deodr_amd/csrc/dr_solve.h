// A sparse symmetric positive definite solve by conjugate gradients with a fixed number of steps (include/deodr_hip_solve.h): the D <= 4 columns of
// b [n, D] independently, from x = 0.  Per column:
//
//     r = b  p = r  rho = sum r^2  rho_b = rho
//     m times:  q = A p   sigma = sum p q   active = rho > tol^2 rho_b and sigma > 0   alpha = active ? rho / sigma : 0   x += alpha p   r -= alpha q
//               rho' = sum r^2   beta = active ? rho' / rho : 0   rho = active ? rho' : rho   p = r + beta p
//     residual = rho_b > 0 ? rho / rho_b : 0
//
// Two instances, chosen by solve_small() alone (deodr_hip_spd_solve_launches states the same rule):
//
// solve_small_kernel           n <= SOLVE_N_SMALL = 1024.  ONE launch, one workgroup of 1024 threads per column, a thread per row.  p in LDS (what the
//                      rows gather), the thread's x, r, q and its own p in registers; a dot is wave_sum, sixteen wave totals in LDS, one barrier, and
//                      every thread adds the sixteen in order -- so all threads hold the same sigma and rho and take the same branch.  Three barriers
//                      per step.  No workgroup waits for another.  Bounded by the 1024 threads of a workgroup (a row per thread); a row is walked
//                      by ONE thread, its entries in order: the loads of cols and vals do not depend on one another, the gathers are LDS reads.
// solve_init / _apply / _update   above.  2 + 2 m launches: solve_clear_kernel zeroes the arrival tickets -- a kernel, not a memset node: replayed in a
//                      graph, a memset node was not reliably done before these short kernels drew their tickets.
//                      solve_init_kernel: r = b, x = 0, rho.  solve_apply_kernel: eight adjacent lanes per row
//                      (dr_subdiv.h) form p_new = r + beta p for the gathered columns and for the own row ON THE FLY, write p_new to the OTHER of
//                      two p buffers (in place would race with the gathers of other workgroups), q = A p_new, sigma through grid_sum; the last
//                      workgroup writes alpha.  solve_update_kernel: a thread per row, x += alpha p, r -= alpha q, rho' through grid_sum; the last
//                      workgroup writes beta, rho and residual.  The scalars live in the scratch and pass from launch to launch there.
//
// No atomics on values.  The order of every sum: a row's entries in order (small) or lane s of the row's group the entries s, s + 8, ... and the butterfly
// of lane_group_sum (large); then the rows of a thread in order, the lanes of a wavefront, the wavefronts in order, and grid_sum over the workgroups.
// The scratch after its 64 bytes of counter words: scalars [6][4] (rho, rho_b, alpha, beta, active, spare), partials [SOLVE_BLOCKS][4], r, p0, p1,
// q [n, D] each.
#pragma once

namespace
{

constexpr int SOLVE_N_SMALL = DEODR_HIP_SOLVE_N_SMALL, SOLVE_SMALL_THREADS = 1024, SOLVE_SMALL_WAVES = SOLVE_SMALL_THREADS / 64;
constexpr int SOLVE_MAX_D = 4;
constexpr int SOLVE_LANES = 8, SOLVE_ROWS = FH_BLOCK / SOLVE_LANES; // lanes of a row's group, rows a workgroup takes per trip: 32
constexpr int SOLVE_BLOCKS = 512;									// workgroups at most (the grid strides beyond)
constexpr int SOLVE_RHO = 0, SOLVE_RHO_B = 4, SOLVE_ALPHA = 8, SOLVE_BETA = 12, SOLVE_ACTIVE = 16, SOLVE_SCALARS = 24;
static_assert(SOLVE_N_SMALL <= SOLVE_SMALL_THREADS && 64 % SOLVE_LANES == 0, "a thread per row; a group of lanes lies inside one wavefront");

// the one rule both the launch and deodr_hip_spd_solve_launches() follow
inline bool solve_small(int n) { return n <= SOLVE_N_SMALL; }
inline size_t solve_scratch_doubles(int n, int D) { return (size_t)SOLVE_SCALARS + (size_t)SOLVE_BLOCKS * SOLVE_MAX_D + 4 * ((size_t)n * (size_t)D); }

struct SolveArgs
{
	const uint32_t *offsets, *cols;
	const double *vals, *b;
	double *x, *residual;
	double *scalars, *partials, *r, *q; // the scratch
	unsigned *counters;
	double tol2; // rel_tol^2
	int n, D, iterations;
};

// The sum of v over the 1024 threads of the workgroup, the same bits in every thread.  (The barrier inside also publishes what the threads stored to
// LDS before the call; `s` is written again only after another barrier of the caller's.)
__device__ __forceinline__ double solve_block_sum(double v, double (&s)[SOLVE_SMALL_WAVES])
{
	const double w = wave_sum(v);
	if ((threadIdx.x & 63) == 0)
		s[threadIdx.x >> 6] = w;
	__syncthreads();
	double total = 0;
#pragma unroll
	for (int i = 0; i < SOLVE_SMALL_WAVES; i++)
		total += s[i];
	return total;
}

// grid: (D), one workgroup per column
__global__ __launch_bounds__(SOLVE_SMALL_THREADS) void solve_small_kernel(SolveArgs a)
{
	__shared__ double s_p[SOLVE_N_SMALL], s_sigma[SOLVE_SMALL_WAVES], s_rho[SOLVE_SMALL_WAVES];
	const int row = threadIdx.x, d = blockIdx.x;
	const bool live = row < a.n;
	const uint32_t begin = live ? a.offsets[row] : 0, end = live ? a.offsets[row + 1] : 0;
	const size_t at = (size_t)(live ? row : 0) * (size_t)a.D + (size_t)d;
	double x = 0, r = live ? a.b[at] : 0, p = r;
	s_p[row] = p;
	double rho = solve_block_sum(r * r, s_rho);
	const double rho_b = rho;
	for (int it = 0; it < a.iterations; it++)
	{
		if (!(rho > a.tol2 * rho_b)) // (the same in every thread.  rho does not change any more: every further step has alpha = 0)
			break;
		double q = 0;
		for (uint32_t k = begin; k < end; k++)
			q += a.vals[k] * s_p[a.cols[k]];
		const double sigma = solve_block_sum(p * q, s_sigma);
		const bool active = sigma > 0;
		const double alpha = active ? rho / sigma : 0;
		if (active)
			x += alpha * p, r -= alpha * q;
		const double rho_new = solve_block_sum(r * r, s_rho);
		const double beta = active ? rho_new / rho : 0;
		rho = active ? rho_new : rho;
		p = r + beta * p;
		s_p[row] = p;
		__syncthreads();
	}
	if (live)
		a.x[at] = x;
	if (row == 0)
		a.residual[d] = rho_b > 0 ? rho / rho_b : 0;
}

// the arrival tickets of the three kernels below -> 0 (the scratch need not be zeroed).  grid: (1), one wavefront
__global__ __launch_bounds__(64) void solve_clear_kernel(unsigned *counters)
{
	if (threadIdx.x < dr::host::SCRATCH_COUNTER_WORDS)
		counters[threadIdx.x] = 0;
}

// r = b, x = 0, rho = rho_b = sum b^2 per column, beta = 0.  grid: capped_blocks(n, FH_BLOCK, SOLVE_BLOCKS), a thread per row
template <int D>
__global__ __launch_bounds__(FH_BLOCK) void solve_init_kernel(SolveArgs a)
{
	double s[D];
#pragma unroll
	for (int d = 0; d < D; d++)
		s[d] = 0;
	for (long long row = (long long)blockIdx.x * FH_BLOCK + threadIdx.x; row < a.n; row += (long long)gridDim.x * FH_BLOCK)
#pragma unroll
		for (int d = 0; d < D; d++)
		{
			const double v = a.b[row * D + d];
			a.r[row * D + d] = v, a.x[row * D + d] = 0;
			s[d] += v * v;
		}
	double total[D];
	if (grid_sum<D>(s, a.partials, a.counters + 0, total) && threadIdx.x < D)
	{
		const double rho = total_of_thread<D>(total, threadIdx.x);
		a.scalars[SOLVE_RHO + threadIdx.x] = rho, a.scalars[SOLVE_RHO_B + threadIdx.x] = rho;
		a.scalars[SOLVE_BETA + threadIdx.x] = 0;
	}
}

// p_new = first ? r : r + beta p_old (own row and gathered columns alike), q = A p_new, sigma; the last workgroup: active, alpha.
// grid: capped_blocks(n, SOLVE_ROWS, SOLVE_BLOCKS); SOLVE_LANES adjacent lanes per row, the trips of a workgroup uniform (the shuffles)
template <int D>
__global__ __launch_bounds__(FH_BLOCK) void solve_apply_kernel(SolveArgs a, const double *p_old, double *p_new, int first)
{
	const int sub = threadIdx.x % SOLVE_LANES, group = threadIdx.x / SOLVE_LANES;
	double beta[D], s[D];
#pragma unroll
	for (int d = 0; d < D; d++)
		beta[d] = first ? 0 : a.scalars[SOLVE_BETA + d], s[d] = 0;
	for (long long base = (long long)blockIdx.x * SOLVE_ROWS; base < a.n; base += (long long)gridDim.x * SOLVE_ROWS)
	{
		const long long row = base + group;
		const bool live = row < a.n; // (the lanes of a group share it; dead groups still take part in the shuffles, with empty rows)
		const uint32_t begin = live ? a.offsets[row] : 0, end = live ? a.offsets[row + 1] : 0;
		double acc[D];
#pragma unroll
		for (int d = 0; d < D; d++)
			acc[d] = 0;
		for (size_t k = (size_t)begin + (size_t)sub; k < end; k += SOLVE_LANES) // (64 bits: begin + sub + 8 may pass 2^32)
		{
			const double w = a.vals[k];
			const size_t c = (size_t)a.cols[k] * D;
#pragma unroll
			for (int d = 0; d < D; d++)
				acc[d] += w * (first ? a.r[c + d] : a.r[c + d] + beta[d] * p_old[c + d]);
		}
#pragma unroll
		for (int d = 0; d < D; d++)
			acc[d] = lane_group_sum<1, SOLVE_LANES>(acc[d]); // (all lanes of the wavefront take part)
		if (live && sub == 0)
#pragma unroll
			for (int d = 0; d < D; d++)
			{
				const size_t e = (size_t)row * D + d;
				const double p = first ? a.r[e] : a.r[e] + beta[d] * p_old[e];
				p_new[e] = p, a.q[e] = acc[d];
				s[d] += p * acc[d];
			}
	}
	double total[D];
	if (grid_sum<D>(s, a.partials, a.counters + 1, total) && threadIdx.x < D)
	{
		const double sigma = total_of_thread<D>(total, threadIdx.x), rho = a.scalars[SOLVE_RHO + threadIdx.x];
		const bool active = rho > a.tol2 * a.scalars[SOLVE_RHO_B + threadIdx.x] && sigma > 0;
		a.scalars[SOLVE_ALPHA + threadIdx.x] = active ? rho / sigma : 0;
		a.scalars[SOLVE_ACTIVE + threadIdx.x] = active ? 1 : 0;
	}
}

// x += alpha p, r -= alpha q, rho' = sum r^2; the last workgroup: beta, rho, residual.  grid: capped_blocks(n, FH_BLOCK, SOLVE_BLOCKS), a thread per row
template <int D>
__global__ __launch_bounds__(FH_BLOCK) void solve_update_kernel(SolveArgs a, const double *p)
{
	double alpha[D], s[D];
	bool active[D];
#pragma unroll
	for (int d = 0; d < D; d++)
		alpha[d] = a.scalars[SOLVE_ALPHA + d], active[d] = a.scalars[SOLVE_ACTIVE + d] != 0, s[d] = 0;
	for (long long row = (long long)blockIdx.x * FH_BLOCK + threadIdx.x; row < a.n; row += (long long)gridDim.x * FH_BLOCK)
#pragma unroll
		for (int d = 0; d < D; d++)
		{
			const size_t e = (size_t)row * D + d;
			double r = a.r[e];
			if (active[d])
			{
				a.x[e] += alpha[d] * p[e];
				r -= alpha[d] * a.q[e];
				a.r[e] = r;
			}
			s[d] += r * r;
		}
	double total[D];
	if (grid_sum<D>(s, a.partials, a.counters + 2, total) && threadIdx.x < D)
	{
		const int d = threadIdx.x;
		const double rho_new = total_of_thread<D>(total, d), rho_old = a.scalars[SOLVE_RHO + d], rho_b = a.scalars[SOLVE_RHO_B + d];
		const bool on = a.scalars[SOLVE_ACTIVE + d] != 0;
		const double rho = on ? rho_new : rho_old;
		a.scalars[SOLVE_BETA + d] = on ? rho_new / rho_old : 0;
		a.scalars[SOLVE_RHO + d] = rho;
		a.residual[d] = rho_b > 0 ? rho / rho_b : 0;
	}
}

// the launches of the instance above SOLVE_N_SMALL: 2 + 2 iterations
template <int D>
void solve_launch_large(const SolveArgs &a, double *p0, double *p1, hipStream_t st)
{
	const dim3 rows(dr::host::capped_blocks((size_t)a.n, FH_BLOCK, SOLVE_BLOCKS)), groups(dr::host::capped_blocks((size_t)a.n, SOLVE_ROWS, SOLVE_BLOCKS)), block(FH_BLOCK);
	hipLaunchKernelGGL(solve_clear_kernel, dim3(1), dim3(64), 0, st, a.counters);
	hipLaunchKernelGGL(solve_init_kernel<D>, rows, block, 0, st, a);
	for (int it = 0; it < a.iterations; it++)
	{ // (p_new of a step goes to the buffer the step before read from)
		double *const p_old = it & 1 ? p1 : p0, *const p_new = it & 1 ? p0 : p1;
		hipLaunchKernelGGL(solve_apply_kernel<D>, groups, block, 0, st, a, (const double *)p_old, p_new, it == 0);
		hipLaunchKernelGGL(solve_update_kernel<D>, rows, block, 0, st, a, (const double *)p_new);
	}
}

} // namespace
