// Rows of a sparse matrix applied to a batch of small dense blocks (include/deodr_hip_subdiv.h): y[b][r][:] (= | +=) sum_k vals[k] x[b][cols[k]][:]
// over the entries k of row r.  The Loop subdivision of a control mesh is S x (many rows of 4 - 20 entries), its adjoint S^T g (few rows of
// tens to a thousand entries): one kernel, two instances that differ in the number of adjacent lanes a row is given to.
//
// One row entry is a chain of two dependent loads (column id -> the D values of that column), so a row walked by ONE lane is the kernel's
// duration (dr_fititer.h, GATHER_LANES: measured there on rows of the same length).  Lane s of a row's group takes the entries s, s + LANES, ...
// in order; the lanes' sums meet in a butterfly over the lane bits of the group (lane_group_sum, dr_fronthalf.h).  Both orders are fixed by the row alone: no atomics on values,
// results bit-identical from run to run.  LANES = 8: eight rows per wavefront, lane_group_sum<1, LANES> of dr_fronthalf.h; LANES = 64: one row per wavefront, the
// column ids and the values of a round are two coalesced loads.  Arithmetic in double, one rounding to the storage type per stored value.
#pragma once

namespace
{

struct SubdivArgs
{
	const uint32_t *offsets, *cols;
	const double *vals;
	const void *x;
	void *y;
	int n_rows, n_cols, D, accumulate;
};

constexpr int SUBDIV_LANES_SHORT = 8, SUBDIV_LANES_LONG = 64;
constexpr unsigned SUBDIV_LONG_ROW = 32; // nnz / n_rows from which a row gets a whole wavefront (below it most of its 64 lanes would load nothing)

// the one rule both the launch and deodr_hip_subdiv_lanes() follow
inline int subdiv_lanes(int n_rows, uint32_t nnz) { return nnz / (uint32_t)n_rows >= SUBDIV_LONG_ROW ? SUBDIV_LANES_LONG : SUBDIV_LANES_SHORT; }

// DC: the number of values per column at compile time (3: vertices), 0: a.D at run time, walked in pieces of 4 (the row is read again per piece)
// grid: (ceil(n_rows LANES / FH_BLOCK), batch)
template <class T, int LANES, int DC>
__global__ __launch_bounds__(FH_BLOCK) void subdiv_apply_kernel(SubdivArgs a)
{
	static_assert(64 % LANES == 0 && FH_BLOCK % 64 == 0, "a group of lanes lies inside one wavefront");
	constexpr int PIECE = DC ? DC : 4;
	const int D = DC ? DC : a.D;
	const long long th = (long long)blockIdx.x * FH_BLOCK + threadIdx.x;
	const long long row = th / LANES;
	const int sub = (int)(th % LANES);
	const bool live = row < a.n_rows; // (the lanes of a group share it; dead groups still take part in the shuffles, with empty rows)
	const uint32_t begin = live ? a.offsets[row] : 0, end = live ? a.offsets[row + 1] : 0;
	const T *x = (const T *)a.x + (size_t)blockIdx.y * (size_t)a.n_cols * (size_t)D;
	T *y = (T *)a.y + ((size_t)blockIdx.y * (size_t)a.n_rows + (size_t)(live ? row : 0)) * (size_t)D;
	for (int d0 = 0; d0 < D; d0 += PIECE)
	{
		double acc[PIECE];
#pragma unroll
		for (int c = 0; c < PIECE; c++)
			acc[c] = 0;
		for (uint32_t k = begin + (uint32_t)sub; k < end; k += LANES)
		{
			const double w = a.vals[k];
			const T *xr = x + (size_t)a.cols[k] * (size_t)D + d0;
#pragma unroll
			for (int c = 0; c < PIECE; c++)
				if (DC || d0 + c < D)
					acc[c] += w * (double)xr[c];
		}
#pragma unroll
		for (int c = 0; c < PIECE; c++)
			acc[c] = lane_group_sum<1, LANES>(acc[c]); // (all lanes of the wavefront take part)
		if (live && sub == 0)
		{
#pragma unroll
			for (int c = 0; c < PIECE; c++)
				if (DC || d0 + c < D)
					y[d0 + c] = (T)(a.accumulate ? (double)y[d0 + c] + acc[c] : acc[c]);
		}
	}
}

template <class T, int LANES>
void subdiv_launch_d(const SubdivArgs &a, dim3 grid, hipStream_t stream)
{
	if (a.D == 3)
		hipLaunchKernelGGL((subdiv_apply_kernel<T, LANES, 3>), grid, dim3(FH_BLOCK), 0, stream, a);
	else
		hipLaunchKernelGGL((subdiv_apply_kernel<T, LANES, 0>), grid, dim3(FH_BLOCK), 0, stream, a);
}

} // namespace
