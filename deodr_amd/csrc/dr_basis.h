// A dense linear basis on the device (include/deodr_hip_basis.h): y[b][j] = mean[j] + sum_k c[b][k] B[k][j] and its adjoint
// c_b[b][k] (= | +=) sum_j B[k][j] g[b][j], B [K, N] row-major.  Both stream B once per chunk of BASIS_CHUNK coefficient vectors (batch = 1: once
// per call) and are bound by that stream: a thread moves 16 bytes of a row per load (VEC = 16 / sizeof(BT) consecutive j), the vector type
// declared with the alignment of ONE element as in dr_texfit.h (a row starts at k N elements: anywhere), the N % VEC elements behind the last
// whole piece done one by one.  Arithmetic in double, one rounding per stored value; no atomics on values: every sum is taken in an order
// fixed by (K, N, batch) alone.
//
// Forward: a thread owns one piece of j for every b of the chunk and walks k; the loads of a walk are independent, BASIS_UNROLL of them are
// in flight (a single dependent walk would be the kernel's duration: dr_fititer.h, GATHER_LANES); c[b][k] is the same in every lane.
// Adjoint: a workgroup takes BASIS_ROW_TILE rows and one segment of j (basis_segments: the one place that rule is written); a piece of g is
// loaded once and used for every row of the tile; per-thread sums -> wave_sum -> the wavefronts in order (LDS) -> one partial per (row,
// segment, b); the last workgroup to arrive for a (chunk, row tile) -- last_to_arrive of dr_fronthalf.h on that tile's OWN counter word, as
// grid_sum there -- adds the tile's partials in segment order and writes or accumulates coeffs_b.
#pragma once

namespace
{

constexpr int BASIS_CHUNK = 4;	   // coefficient vectors per pass over B (forward: 16 double accumulators per thread at VEC = 4; adjoint: 32)
constexpr int BASIS_UNROLL = 8;	   // rows of B in flight per thread in the forward walk
constexpr int BASIS_ROW_TILE = 8;  // rows of B per workgroup of the adjoint (their 8 loads of a piece are in flight together)
constexpr int BASIS_SEGMENT = 4096; // elements of j: a segment is a whole number of these (16 pieces per thread in float32, 8 in float64), but for the last
constexpr int BASIS_TARGET_BLOCKS = 1024; // workgroups from which the chip (256 CUs) is full: four per CU
constexpr int BASIS_MAX_SEGMENTS = 256;	  // (the last workgroup of a row tile adds them one after the other)
constexpr int BASIS_MAX_K = 1024, BASIS_MAX_BATCH = 64, BASIS_MAX_N = 1 << 30;

static_assert(BASIS_SEGMENT % (FH_BLOCK * 4) == 0, "a segment is a whole number of rounds of the workgroup, in either storage type");

inline int basis_row_tiles(int K) { return (K + BASIS_ROW_TILE - 1) / BASIS_ROW_TILE; }
inline int basis_chunks(int batch) { return (batch + BASIS_CHUNK - 1) / BASIS_CHUNK; }

// the one rule the launch, the scratch layout and deodr_hip_basis_segments() follow: as many segments as fill the chip together with the row
// tiles, none shorter than BASIS_SEGMENT elements but the last.  Non-decreasing in N.
inline int basis_segments(int K, int N)
{
	const int units = (N + BASIS_SEGMENT - 1) / BASIS_SEGMENT, tiles = basis_row_tiles(K);
	int want = (BASIS_TARGET_BLOCKS + tiles - 1) / tiles;
	want = want < BASIS_MAX_SEGMENTS ? want : BASIS_MAX_SEGMENTS;
	return units < want ? units : want;
}
// first element of segment s of S (s = S: N): the units of BASIS_SEGMENT elements dealt out evenly, so S = units gives segments of one unit each
__host__ __device__ inline int basis_segment_begin(int s, int S, int N)
{
	const int units = (N + BASIS_SEGMENT - 1) / BASIS_SEGMENT;
	return s >= S ? N : (int)((long long)s * units / S) * BASIS_SEGMENT;
}

template <class T, int N>
struct BasisVec
{
	typedef T aligned_type __attribute__((ext_vector_type(N)));
	typedef aligned_type type __attribute__((aligned(sizeof(T)))); // element-aligned: see above
};

struct BasisArgs
{
	const void *basis, *mean, *g;
	const double *coeffs;
	void *y;
	double *coeffs_b, *partials;
	unsigned *counters;
	int K, N, batch, S, accumulate;
};

// grid: (ceil(N / VEC / FH_BLOCK) or 1, chunks of the batch); NB = 1: batch == 1, NB = BASIS_CHUNK: the last chunk may hold fewer
template <class BT, class YT, int NB>
__global__ __launch_bounds__(FH_BLOCK) void basis_apply_kernel(BasisArgs a)
{
	constexpr int VEC = 16 / sizeof(BT);
	using VB = typename BasisVec<BT, VEC>::type;
	using VY = typename BasisVec<YT, VEC>::type;
	const BT *__restrict__ B = (const BT *)a.basis, *__restrict__ mean = (const BT *)a.mean;
	const int b0 = (int)blockIdx.y * NB, nb = a.batch - b0 < NB ? a.batch - b0 : NB;
	const double *__restrict__ c = a.coeffs + (size_t)b0 * (size_t)a.K;
	YT *y = (YT *)a.y + (size_t)b0 * (size_t)a.N;
	const size_t N = (size_t)a.N;
	const int pieces = a.N / VEC, i = (int)blockIdx.x * FH_BLOCK + (int)threadIdx.x;
	if (i < pieces)
	{
		const size_t j = (size_t)i * VEC;
		double acc[NB][VEC];
		VB m;
		if (mean)
			m = *(const VB *)(mean + j);
#pragma unroll
		for (int b = 0; b < NB; b++)
#pragma unroll
			for (int v = 0; v < VEC; v++)
				acc[b][v] = mean ? (double)m[v] : 0.0;
		int k = 0;
		for (; k + BASIS_UNROLL <= a.K; k += BASIS_UNROLL)
		{
			VB row[BASIS_UNROLL];
#pragma unroll
			for (int u = 0; u < BASIS_UNROLL; u++)
				row[u] = *(const VB *)(B + (size_t)(k + u) * N + j);
#pragma unroll
			for (int u = 0; u < BASIS_UNROLL; u++)
#pragma unroll
				for (int b = 0; b < NB; b++)
				{
					const double cb = b < nb ? c[(size_t)b * a.K + k + u] : 0.0;
#pragma unroll
					for (int v = 0; v < VEC; v++)
						acc[b][v] += cb * (double)row[u][v];
				}
		}
		for (; k < a.K; k++)
		{
			const VB row = *(const VB *)(B + (size_t)k * N + j);
#pragma unroll
			for (int b = 0; b < NB; b++)
			{
				const double cb = b < nb ? c[(size_t)b * a.K + k] : 0.0;
#pragma unroll
				for (int v = 0; v < VEC; v++)
					acc[b][v] += cb * (double)row[v];
			}
		}
#pragma unroll
		for (int b = 0; b < NB; b++)
			if (b < nb)
			{
				VY out;
#pragma unroll
				for (int v = 0; v < VEC; v++)
					out[v] = (YT)acc[b][v];
				*(VY *)(y + (size_t)b * N + j) = out;
			}
	}
	if (blockIdx.x == 0 && (int)threadIdx.x < a.N - pieces * VEC)
	{ // the elements behind the last whole piece, one thread each
		const size_t j = (size_t)pieces * VEC + threadIdx.x;
		for (int b = 0; b < nb; b++)
		{
			double s = mean ? (double)mean[j] : 0.0;
			for (int k = 0; k < a.K; k++)
				s += c[(size_t)b * a.K + k] * (double)B[(size_t)k * N + j];
			y[(size_t)b * N + j] = (YT)s;
		}
	}
}

// grid: (S segments, row tiles, chunks of the batch).  partials: [chunk][tile][segment][BASIS_ROW_TILE][BASIS_CHUNK], counters: [chunk][tile]
template <class BT, class GT, int NB>
__global__ __launch_bounds__(FH_BLOCK) void basis_apply_b_kernel(BasisArgs a)
{
	constexpr int VEC = 16 / sizeof(BT), SLOTS = BASIS_ROW_TILE * BASIS_CHUNK;
	using VB = typename BasisVec<BT, VEC>::type;
	using VG = typename BasisVec<GT, VEC>::type;
	__shared__ double s_wave[FH_BLOCK / 64][BASIS_ROW_TILE * NB];
	const BT *__restrict__ B = (const BT *)a.basis;
	const int seg = (int)blockIdx.x, tile = (int)blockIdx.y, k0 = tile * BASIS_ROW_TILE, rows = a.K - k0 < BASIS_ROW_TILE ? a.K - k0 : BASIS_ROW_TILE;
	const int b0 = (int)blockIdx.z * NB, nb = a.batch - b0 < NB ? a.batch - b0 : NB;
	const GT *__restrict__ g = (const GT *)a.g + (size_t)b0 * (size_t)a.N;
	const size_t N = (size_t)a.N;
	const int e0 = basis_segment_begin(seg, a.S, a.N), e1 = basis_segment_begin(seg + 1, a.S, a.N), pieces = (e1 - e0) / VEC;
	double acc[BASIS_ROW_TILE][NB];
#pragma unroll
	for (int r = 0; r < BASIS_ROW_TILE; r++)
#pragma unroll
		for (int b = 0; b < NB; b++)
			acc[r][b] = 0;
	for (int p = (int)threadIdx.x; p < pieces; p += FH_BLOCK)
	{
		const size_t j = (size_t)e0 + (size_t)p * VEC;
		VB row[BASIS_ROW_TILE];
#pragma unroll
		for (int r = 0; r < BASIS_ROW_TILE; r++)
			if (r < rows)
				row[r] = *(const VB *)(B + (size_t)(k0 + r) * N + j);
		double gd[NB][VEC];
#pragma unroll
		for (int b = 0; b < NB; b++)
		{
			VG gv;
			if (b < nb)
				gv = *(const VG *)(g + (size_t)b * N + j);
#pragma unroll
			for (int v = 0; v < VEC; v++)
				gd[b][v] = b < nb ? (double)gv[v] : 0.0;
		}
#pragma unroll
		for (int r = 0; r < BASIS_ROW_TILE; r++)
			if (r < rows)
#pragma unroll
				for (int b = 0; b < NB; b++)
#pragma unroll
					for (int v = 0; v < VEC; v++)
						acc[r][b] += (double)row[r][v] * gd[b][v];
	}
	if ((int)threadIdx.x < (e1 - e0) - pieces * VEC)
	{ // the elements behind the last whole piece of the last segment, one thread each
		const size_t j = (size_t)e0 + (size_t)pieces * VEC + threadIdx.x;
#pragma unroll
		for (int r = 0; r < BASIS_ROW_TILE; r++)
			if (r < rows)
#pragma unroll
				for (int b = 0; b < NB; b++)
					if (b < nb)
						acc[r][b] += (double)B[(size_t)(k0 + r) * N + j] * (double)g[(size_t)b * N + j];
	}
	// threads -> lanes -> wavefronts, every step in a fixed order (all lanes take part: rows and b beyond the tile's hold zeros)
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
	for (int r = 0; r < BASIS_ROW_TILE; r++)
#pragma unroll
		for (int b = 0; b < NB; b++)
		{
			const double s = wave_sum(acc[r][b]);
			if (lane == 0)
				s_wave[wave][r * NB + b] = s;
		}
	__syncthreads();
	const size_t group = (size_t)blockIdx.z * gridDim.y + (size_t)tile; // this (chunk, row tile)
	double *partials = a.partials + group * (size_t)a.S * SLOTS;
	if (threadIdx.x < BASIS_ROW_TILE * NB)
	{
		double s = 0;
		for (int w = 0; w < FH_BLOCK / 64; w++)
			s += s_wave[w][threadIdx.x];
		partials[(size_t)seg * SLOTS + threadIdx.x] = s;
	}
	if (!last_to_arrive(a.counters + group, (unsigned)a.S))
		return;
	if (threadIdx.x < BASIS_ROW_TILE * NB)
	{
		const int r = (int)threadIdx.x / NB, b = (int)threadIdx.x % NB;
		double s = 0;
		for (int i = 0; i < a.S; i++)
			s += partials[(size_t)i * SLOTS + threadIdx.x];
		if (r < rows && b < nb)
			store_or_add(a.coeffs_b + (size_t)(b0 + b) * a.K + (k0 + r), s, a.accumulate);
	}
	reset_arrivals(a.counters + group);
}

} // namespace
