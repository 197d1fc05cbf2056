// The multi-scale L2 data term (include/deodr_hip_pyramid.h): residuals compared after summing over 2 x 2, 4 x 4, ... cells, and the adjoint.
//
//     q_0 = w (image - obs)   q_{l+1} = sum of the children's q_l   w_{l+1} likewise   term_l = sum q_l^2 / w_l   loss = sum lambda_l term_l
//     g_L = 2 lambda_L q_L / w_L     g_l = 2 lambda_l q_l / w_l + g_{l+1}(parent)      image_b = w g_0          (1 / w_l := 0 where w_l = 0)
//
// A cell of level l is the aligned 2^l x 2^l block of pixels clipped to the frame, so levels 0 .. 3 live inside an aligned 8 x 8 tile and the
// levels above on the grid of tiles.
//
// pyramid_tile_kernel<PixT, MODE>  one wavefront per tile (a workgroup takes four, the grid strides beyond PYR_BLOCKS workgroups), lane = pixel in
//                      Morton order: the children of a level-1 cell are the four lanes of a quad, a level-2 cell is a row of 16 lanes, level 3 the
//                      wavefront; the sums are DPP moves and readlanes (pyr_tile_sums), an order fixed by the lane numbers.  (As butterflies of
//                      __shfl_xor -- twelve ds_bpermute_b32 per double -- the one-pass call on 8 x 1024^2 x 4 took 337 us instead of 294.)  The weights are
//                      reduced once per tile, the residuals channel by channel (run-time C: nothing is kept per channel).
//                      PYR_REDUCE: term_0 .. term_3 through grid_sum, the tile sums q_3 [C], w_3 to the scratch when there are levels above.
//                      PYR_ADJOINT: recomputes q_0 .. q_3, takes the tile's incoming gradient from the scratch (levels > 3) and writes image_b.
//                      Both at once when levels <= 3: the frame is read once.
// pyramid_coarse_kernel  levels 4 .. L and their adjoint.  One workgroup per region of 32 x 32 tiles (a level-8 cell, so every cell of a level <= 8
//                      lies in one region) and view; per channel the tile sums go to LDS, each level is summed from its four children in the order
//                      (0,0) (0,1) (1,0) (1,1), then the gradient walks down in place; -> gamma [tiles, C] (g_4 of the tile's parent), term_4 .. L
//                      through grid_sum, and the loss.
// No atomics on values; the arrival tickets of grid_sum (counter words 0 and 1 of the scratch) are cleared by the entry point on the stream.
#pragma once

namespace
{

constexpr int PYR_MAX_LEVELS = 8;
constexpr int PYR_TILE = 8;			// pixels per side of a tile: levels 0 .. PYR_TILE_LEVELS inside a wavefront
constexpr int PYR_TILE_LEVELS = 3;
constexpr int PYR_BLOCKS = 1024;	// workgroups of the tile kernel at most (each ends with a ticket on one counter word: L2_BLOCKS of dr_fititer.h)
constexpr int PYR_WAVES = FH_BLOCK / 64;
constexpr int PYR_CHANNELS = 4;		// channels of a pixel the tile kernel loads ahead of their reductions
constexpr int PYR_REGION = 32;		// tiles per side of a region of the coarse kernel: 2^(PYR_MAX_LEVELS - PYR_TILE_LEVELS)
constexpr int PYR_COARSE_LEVELS = PYR_MAX_LEVELS - PYR_TILE_LEVELS; // levels 4 .. 8
constexpr int PYR_LDS = 1365;		// 32^2 + 16^2 + 8^2 + 4^2 + 2^2 + 1: the cells of levels 3 .. 8 of a region
constexpr int PYR_REDUCE = 1, PYR_ADJOINT = 2;
static_assert(PYR_MAX_LEVELS == DEODR_HIP_PYRAMID_MAX_LEVELS && PYR_REGION == 1 << PYR_COARSE_LEVELS, "include/deodr_hip_pyramid.h states the limit");

struct PyramidArgs
{
	const void *image, *obs, *weights; // [n,H,W,C], [n,H,W,C], [n,H,W] | NULL in the pixel type
	void *image_b;					   // [n,H,W,C] | NULL
	const double *lambda;			   // [levels + 1], device
	double *terms, *loss;			   // [levels + 1], [1] | NULL
	double *partials_tile, *partials_coarse, *tile_w, *tile_q, *gamma; // the scratch: [PYR_BLOCKS,4], [regions,5], [tiles], [tiles,C], [tiles,C]
	unsigned *counters;
	int n, H, W, C, levels, TH, TW, RH, RW; // tiles and regions per view, down and across
};

__device__ __forceinline__ double pyr_inverse(double w) { return w > 0 ? 1.0 / w : 0.0; }
// bits 0, 2, 4 of the lane number
__device__ __forceinline__ int pyr_even_bits(int lane) { return (lane & 1) | ((lane >> 1) & 2) | ((lane >> 2) & 4); }

// The sums of v over the level-1, -2 and -3 cell of a lane's pixel, the same bits in every lane of the cell.  All 64 lanes call it.
//   level 1: the quad -- lane ^ 1, then lane ^ 2 (quad_perm);
//   level 2: the row of 16 -- the four lanes of a quad now agree, so the mirror image of a half row holds the other quad of the half
//            (row_half_mirror), then lane ^ 8 (row_ror:8);
//   level 3: the four rows, read by lane and added in row order.
struct PyrSums
{
	double l1, l2, l3;
};
__device__ __forceinline__ PyrSums pyr_tile_sums(double v)
{
	PyrSums r;
	r.l1 = v + dpp_d<0xB1>(v);
	r.l1 = r.l1 + dpp_d<0x4E>(r.l1);
	r.l2 = r.l1 + dpp_d<0x141>(r.l1);
	r.l2 = r.l2 + dpp_d<0x128>(r.l2);
	const int hi = __double2hiint(r.l2), lo = __double2loint(r.l2);
	r.l3 = __hiloint2double(__builtin_amdgcn_readlane(hi, 0), __builtin_amdgcn_readlane(lo, 0));
	r.l3 += __hiloint2double(__builtin_amdgcn_readlane(hi, 16), __builtin_amdgcn_readlane(lo, 16));
	r.l3 += __hiloint2double(__builtin_amdgcn_readlane(hi, 32), __builtin_amdgcn_readlane(lo, 32));
	r.l3 += __hiloint2double(__builtin_amdgcn_readlane(hi, 48), __builtin_amdgcn_readlane(lo, 48));
	return r;
}

template <class PixT, int MODE>
__global__ __launch_bounds__(FH_BLOCK) void pyramid_tile_kernel(PyramidArgs a)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int x_in = pyr_even_bits(lane), y_in = pyr_even_bits(lane >> 1);
	const PixT *image = (const PixT *)a.image, *obs = (const PixT *)a.obs, *weights = (const PixT *)a.weights;
	const bool above = a.levels > PYR_TILE_LEVELS;
	double c[PYR_TILE_LEVELS + 1]; // 2 lambda_l, 0 for a level this call does not have
#pragma unroll
	for (int l = 0; l <= PYR_TILE_LEVELS; l++)
		c[l] = (MODE & PYR_ADJOINT) && l <= a.levels ? 2 * a.lambda[l] : 0.0;
	double s[PYR_TILE_LEVELS + 1] = {0, 0, 0, 0};
	const long long per_view = (long long)a.TH * a.TW, tiles = per_view * a.n;
	for (long long tile = (long long)blockIdx.x * PYR_WAVES + wave; tile < tiles; tile += (long long)gridDim.x * PYR_WAVES)
	{ // (the same tile in every lane of a wavefront: the butterflies below are taken by all 64)
		const int b = (int)(tile / per_view), ty = (int)(tile % per_view / a.TW), tx = (int)(tile % a.TW);
		const int y = ty * PYR_TILE + y_in, x = tx * PYR_TILE + x_in;
		const bool in = y < a.H && x < a.W;
		const size_t pix = in ? ((size_t)b * a.H + y) * a.W + x : 0;
		const double w0 = in ? (weights ? (double)weights[pix] : 1.0) : 0.0;
		const PyrSums ws = pyr_tile_sums(w0);
		const double w1 = ws.l1, w2 = ws.l2, w3 = ws.l3;
		const double iw0 = pyr_inverse(w0), iw1 = pyr_inverse(w1), iw2 = pyr_inverse(w2), iw3 = pyr_inverse(w3);
		if ((MODE & PYR_REDUCE) && above && lane == 0)
			a.tile_w[tile] = w3;
		for (int first = 0; first < a.C; first += PYR_CHANNELS)
		{ // (the loads of PYR_CHANNELS channels are issued before the first is used: the store of image_b may alias them for all the compiler knows)
			double r[PYR_CHANNELS];
#pragma unroll
			for (int j = 0; j < PYR_CHANNELS; j++)
				r[j] = in && first + j < a.C ? (double)image[pix * a.C + first + j] - (double)obs[pix * a.C + first + j] : 0.0;
#pragma unroll
			for (int j = 0; j < PYR_CHANNELS; j++)
			{
				const int ch = first + j;
				if (ch >= a.C) // (the same in every lane)
					break;
				const size_t at = pix * a.C + ch;
				const double q0 = w0 * r[j];
				const PyrSums qs = pyr_tile_sums(q0);
				const double q1 = qs.l1, q2 = qs.l2, q3 = qs.l3;
				if (MODE & PYR_REDUCE)
				{ // one lane per cell
					s[0] += (q0 * q0) * iw0;
					s[1] += (lane & 3) == 0 ? (q1 * q1) * iw1 : 0.0;
					s[2] += (lane & 15) == 0 ? (q2 * q2) * iw2 : 0.0;
					s[3] += lane == 0 ? (q3 * q3) * iw3 : 0.0;
					if (above && lane == 0)
						a.tile_q[tile * a.C + ch] = q3;
				}
				if (MODE & PYR_ADJOINT)
				{
					const double g4 = above ? a.gamma[tile * a.C + ch] : 0.0;
					const double g3 = c[3] * q3 * iw3 + g4, g2 = c[2] * q2 * iw2 + g3, g1 = c[1] * q1 * iw1 + g2, g0 = c[0] * q0 * iw0 + g1;
					if (in)
						__builtin_nontemporal_store((PixT)(w0 * g0), (PixT *)a.image_b + at);
				}
			}
		}
	}
	if (MODE & PYR_REDUCE)
	{
		double total[PYR_TILE_LEVELS + 1];
		if (grid_sum<PYR_TILE_LEVELS + 1>(s, a.partials_tile, a.counters + 0, total) && threadIdx.x == 0)
		{
			double loss = 0;
#pragma unroll
			for (int l = 0; l <= PYR_TILE_LEVELS; l++)
				if (l <= a.levels)
				{
					a.terms[l] = total[l];
					loss += a.lambda[l] * total[l];
				}
			if (!above && a.loss)
				a.loss[0] = loss;
		}
	}
}

// where the cells of level PYR_TILE_LEVELS + k of a region start in its LDS arrays, and how many a side
__device__ __forceinline__ int pyr_level_start(int k)
{
	int at = 0;
	for (int i = 0; i < k; i++)
		at += (PYR_REGION >> i) * (PYR_REGION >> i);
	return at;
}

__global__ __launch_bounds__(FH_BLOCK) void pyramid_coarse_kernel(PyramidArgs a)
{
	__shared__ double s_w[PYR_LDS], s_q[PYR_LDS];
	const int top = a.levels - PYR_TILE_LEVELS; // 1 .. PYR_COARSE_LEVELS: the levels above the tiles
	const int per_view = a.RH * a.RW, b = blockIdx.x / per_view, ry = blockIdx.x % per_view / a.RW, rx = blockIdx.x % a.RW;
	// the tile of cell t of the region's level 3, or -1 outside the frame
	auto tile_of = [&](int t) -> long long {
		const int ty = ry * PYR_REGION + t / PYR_REGION, tx = rx * PYR_REGION + t % PYR_REGION;
		return ty < a.TH && tx < a.TW ? ((long long)b * a.TH + ty) * a.TW + tx : -1;
	};
	// level k of `v` from level k - 1: the four children in a fixed order (a child outside the frame holds 0)
	auto sum_level = [&](double *v, int k) {
		const int side = PYR_REGION >> k, from = pyr_level_start(k - 1), to = pyr_level_start(k);
		for (int t = threadIdx.x; t < side * side; t += FH_BLOCK)
		{
			const double *child = v + from + (2 * (t / side)) * (2 * side) + 2 * (t % side);
			v[to + t] = ((child[0] + child[1]) + child[2 * side]) + child[2 * side + 1];
		}
		__syncthreads();
	};
	for (int t = threadIdx.x; t < PYR_REGION * PYR_REGION; t += FH_BLOCK)
	{
		const long long tile = tile_of(t);
		s_w[t] = tile >= 0 ? a.tile_w[tile] : 0.0;
	}
	__syncthreads();
	for (int k = 1; k <= top; k++)
		sum_level(s_w, k);
	double s[PYR_COARSE_LEVELS] = {0, 0, 0, 0, 0};
	for (int ch = 0; ch < a.C; ch++)
	{
		for (int t = threadIdx.x; t < PYR_REGION * PYR_REGION; t += FH_BLOCK)
		{
			const long long tile = tile_of(t);
			s_q[t] = tile >= 0 ? a.tile_q[tile * a.C + ch] : 0.0;
		}
		__syncthreads();
		for (int k = 1; k <= top; k++)
			sum_level(s_q, k);
		// the terms, and the gradient from the top down, in place: s_q of level k becomes g of level k
#pragma unroll
		for (int k = PYR_COARSE_LEVELS; k >= 1; k--)
			if (k <= top)
			{
				const int side = PYR_REGION >> k, at = pyr_level_start(k), up = pyr_level_start(k + 1);
				const double c = 2 * a.lambda[PYR_TILE_LEVELS + k];
				for (int t = threadIdx.x; t < side * side; t += FH_BLOCK)
				{
					const double q = s_q[at + t], iw = pyr_inverse(s_w[at + t]);
					s[k - 1] += (q * q) * iw;
					const double parent = k < top ? s_q[up + (t / side / 2) * (side / 2) + t % side / 2] : 0.0;
					s_q[at + t] = c * q * iw + parent;
				}
				__syncthreads();
			}
		for (int t = threadIdx.x; t < PYR_REGION * PYR_REGION; t += FH_BLOCK)
		{
			const long long tile = tile_of(t);
			if (tile >= 0)
				a.gamma[tile * a.C + ch] = s_q[pyr_level_start(1) + (t / PYR_REGION / 2) * (PYR_REGION / 2) + t % PYR_REGION / 2];
		}
		__syncthreads();
	}
	double total[PYR_COARSE_LEVELS];
	if (grid_sum<PYR_COARSE_LEVELS>(s, a.partials_coarse, a.counters + 1, total) && threadIdx.x == 0)
	{
		double loss = 0;
		for (int l = 0; l <= PYR_TILE_LEVELS; l++)
			loss += a.lambda[l] * a.terms[l]; // (written by the tile kernel, the launch before this one)
#pragma unroll
		for (int k = 1; k <= PYR_COARSE_LEVELS; k++)
			if (k <= top)
			{
				a.terms[PYR_TILE_LEVELS + k] = total[k - 1];
				loss += a.lambda[PYR_TILE_LEVELS + k] * total[k - 1];
			}
		if (a.loss)
			a.loss[0] = loss;
	}
}

} // namespace
