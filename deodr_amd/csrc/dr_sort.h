// A stable sort by key of n independent rows of N 32-bit keys (include/deodr_hip_chamfer_grid.h has the contract): a least-significant-digit
// radix sort, SORT_DIGIT_BITS bits per pass, three launches per pass, all on a grid (ceil(N / SORT_ITEMS), n) but the scan's (1, n):
//
// sort_histogram_kernel  workgroup g counts the digits of the keys [g SORT_ITEMS, (g + 1) SORT_ITEMS) of its row (LDS integer counts: they do
//                        not depend on the order of arrival) -> hist[row][g][digit].
// sort_scan_kernel       one workgroup per row, thread d owns digit d: the total of digit d over the workgroups in order, an exclusive scan of
//                        the SORT_DIGITS totals in LDS, then hist[row][g][d] <- the first position of (digit d, workgroup g): the exclusive scan
//                        over (digit, workgroup) in that order.
// sort_scatter_kernel    workgroup g takes its keys SORT_BLOCK at a time, in order.  A lane's rank among the lanes of its wavefront with the same
//                        digit comes from SORT_DIGIT_BITS ballots (64-bit masks) and mbcnt; the lowest such lane writes the wavefront's count of
//                        the digit to LDS; position = running base of the digit + the counts of the wavefronts before + the rank: increasing
//                        index within a digit, i.e. stable.  Thread d then advances the base of digit d.
//
// No workgroup waits for another, no atomic decides a position.  Pass 0 reads the caller's keys (the index is the position), pass p writes buffer
// p & 1 of the scratch, the last pass writes `order` (and `sorted_keys` where wanted).  Scratch, 4-byte words: keys [2][n][N], indices [2][n][N],
// hist [n][G][SORT_DIGITS].
#pragma once

namespace
{

constexpr int SORT_DIGIT_BITS = DEODR_HIP_SORT_DIGIT_BITS, SORT_DIGITS = 1 << SORT_DIGIT_BITS, SORT_BLOCK = DEODR_HIP_SORT_BLOCK;
constexpr int SORT_ITEMS = DEODR_HIP_SORT_ITEMS, SORT_MAX_ITEMS = DEODR_HIP_SORT_MAX_ITEMS, SORT_MAX_ROWS = 65535;
static_assert(SORT_DIGITS == SORT_BLOCK, "thread d owns digit d");
static_assert(SORT_ITEMS % SORT_BLOCK == 0 && SORT_BLOCK % 64 == 0, "whole rounds of whole wavefronts");

inline const char *sort_dims(int N, int n, int bits)
{ // -> NULL, or which limit of the header the arguments break
	if (N <= 0 || N > SORT_MAX_ITEMS)
		return "N must be in 1 .. DEODR_HIP_SORT_MAX_ITEMS";
	if (n <= 0 || n > SORT_MAX_ROWS)
		return "n must be in 1 .. 65535";
	if (bits < 1 || bits > 32)
		return "bits must be in 1 .. 32";
	return NULL;
}
inline int sort_groups(int N) { return (N - 1) / SORT_ITEMS + 1; }
inline int sort_passes(int bits) { return (bits - 1) / SORT_DIGIT_BITS + 1; }
inline size_t sort_scratch_words(int N, int n) { return (size_t)n * (4 * (size_t)N + (size_t)SORT_DIGITS * (size_t)sort_groups(N)); }

struct SortArgs
{
	const uint32_t *keys_in, *order_in; // order_in NULL: the position
	uint32_t *keys_out, *order_out, *hist;
	uint32_t mask; // of the bits that take part
	int N, shift;
};

__device__ __forceinline__ uint32_t sort_digit(uint32_t key, const SortArgs &a) { return ((key & a.mask) >> a.shift) & (uint32_t)(SORT_DIGITS - 1); }

// grid: (G, n)
__global__ __launch_bounds__(SORT_BLOCK) void sort_histogram_kernel(SortArgs a)
{
	__shared__ unsigned s_count[SORT_DIGITS];
	const size_t row = blockIdx.y;
	const uint32_t *const keys = a.keys_in + row * (size_t)a.N;
	s_count[threadIdx.x] = 0;
	__syncthreads();
	const int base = (int)blockIdx.x * SORT_ITEMS;
	for (int r = 0; r < SORT_ITEMS / SORT_BLOCK; r++)
	{
		const int i = base + r * SORT_BLOCK + (int)threadIdx.x;
		if (i < a.N)
			atomicAdd(&s_count[sort_digit(keys[i], a)], 1u); // (a count in LDS: the same whatever the order)
	}
	__syncthreads();
	a.hist[(row * gridDim.x + blockIdx.x) * SORT_DIGITS + threadIdx.x] = s_count[threadIdx.x];
}

// grid: (1, n); G workgroups of the other two kernels
__global__ __launch_bounds__(SORT_BLOCK) void sort_scan_kernel(SortArgs a, int G)
{
	__shared__ uint32_t s_total[SORT_DIGITS];
	uint32_t *const hist = a.hist + (size_t)blockIdx.y * (size_t)G * SORT_DIGITS + threadIdx.x;
	uint32_t total = 0;
	for (int g = 0; g < G; g++)
		total += hist[(size_t)g * SORT_DIGITS];
	s_total[threadIdx.x] = total;
	__syncthreads();
	uint32_t at = 0;
	for (int d = 0; d < (int)threadIdx.x; d++) // (SORT_DIGITS broadcast reads at most: once per row and pass)
		at += s_total[d];
	for (int g = 0; g < G; g++)
	{
		const uint32_t count = hist[(size_t)g * SORT_DIGITS];
		hist[(size_t)g * SORT_DIGITS] = at;
		at += count;
	}
}

// grid: (G, n)
__global__ __launch_bounds__(SORT_BLOCK) void sort_scatter_kernel(SortArgs a)
{
	__shared__ uint32_t s_base[SORT_DIGITS];
	__shared__ uint32_t s_count[SORT_BLOCK / 64][SORT_DIGITS];
	const size_t row = blockIdx.y, at_row = row * (size_t)a.N;
	const int wave = (int)threadIdx.x >> 6;
	s_base[threadIdx.x] = a.hist[(row * gridDim.x + blockIdx.x) * SORT_DIGITS + threadIdx.x];
#pragma unroll
	for (int w = 0; w < SORT_BLOCK / 64; w++)
		s_count[w][threadIdx.x] = 0;
	__syncthreads();
	const int base = (int)blockIdx.x * SORT_ITEMS;
	for (int r = 0; r < SORT_ITEMS / SORT_BLOCK; r++)
	{
		const int i = base + r * SORT_BLOCK + (int)threadIdx.x;
		const bool valid = i < a.N;
		const uint32_t key = valid ? a.keys_in[at_row + i] : 0u;
		const uint32_t index = valid ? (a.order_in ? a.order_in[at_row + i] : (uint32_t)i) : 0u;
		const uint32_t digit = sort_digit(key, a);
		unsigned long long same = __ballot(valid); // the valid lanes of this wavefront with this lane's digit (64 bits)
#pragma unroll
		for (int b = 0; b < SORT_DIGIT_BITS; b++)
		{
			const bool bit = (digit >> b) & 1u;
			const unsigned long long set = __ballot(bit);
			same &= bit ? set : ~set;
		}
		const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0u)); // (those in lower lanes)
		if (valid && rank == 0)
			s_count[wave][digit] = (uint32_t)__popcll(same);
		__syncthreads();
		if (valid)
		{
			uint32_t to = s_base[digit] + rank;
			for (int w = 0; w < wave; w++)
				to += s_count[w][digit];
			a.keys_out[at_row + to] = key;
			a.order_out[at_row + to] = index;
		}
		__syncthreads();
		uint32_t step = 0;
#pragma unroll
		for (int w = 0; w < SORT_BLOCK / 64; w++)
			step += s_count[w][threadIdx.x], s_count[w][threadIdx.x] = 0;
		s_base[threadIdx.x] += step;
		__syncthreads();
	}
}

// the launches of a sort; the arguments were checked.  `words`: sort_scratch_words(N, n) of them
inline void sort_launch(const uint32_t *keys, int N, int n, int bits, uint32_t *sorted_keys, uint32_t *order, uint32_t *words, hipStream_t st)
{
	const size_t rows = (size_t)n * (size_t)N;
	uint32_t *const kbuf[2] = {words, words + rows}, *const obuf[2] = {words + 2 * rows, words + 3 * rows};
	const int G = sort_groups(N), passes = sort_passes(bits);
	SortArgs a = {keys, nullptr, nullptr, nullptr, words + 4 * rows, bits >= 32 ? 0xFFFFFFFFu : (1u << bits) - 1u, N, 0};
	const dim3 grid((unsigned)G, (unsigned)n), block(SORT_BLOCK);
	for (int p = 0; p < passes; p++)
	{
		const bool last = p == passes - 1;
		a.shift = p * SORT_DIGIT_BITS;
		a.keys_out = last && sorted_keys ? sorted_keys : kbuf[p & 1];
		a.order_out = last ? order : obuf[p & 1];
		hipLaunchKernelGGL(sort_histogram_kernel, grid, block, 0, st, a);
		hipLaunchKernelGGL(sort_scan_kernel, dim3(1, (unsigned)n), block, 0, st, a, G);
		hipLaunchKernelGGL(sort_scatter_kernel, grid, block, 0, st, a);
		a.keys_in = a.keys_out, a.order_in = a.order_out;
	}
}

} // namespace
