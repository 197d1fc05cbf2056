// The structural data term (include/deodr_hip_ssim.h): 1 - SSIM under an 11 x 11 Gaussian window with zero padding, mixed with the pixel term, and
// the adjoint.
//
//     mx = G*x  my = G*y  sxx = G*x^2 - mx^2  syy = G*y^2 - my^2  sxy = G*xy - mx my       a1 = 2 mx my + C1  a2 = 2 sxy + C2
//     SSIM = a1 a2 / (b1 b2)                                                                  b1 = mx^2 + my^2 + C1  b2 = sxx + syy + C2
//     term_0 = sum w (x - y)^2   term_1 = sum w (1 - SSIM)   loss = alpha term_0 + beta term_1
//     A = -w S_m  B = -w S_xx  Cm = -w S_xy      image_b = 2 alpha w (x - y) + beta (G*A + 2 x (G*B) + y (G*Cm))
//
// Both kernels are stencils over the same tiling: a workgroup takes a tile of SSIM_TH x SSIM_TW = 16 x 32 pixels of one view (the grid strides
// beyond SSIM_BLOCKS workgroups: each of the first kernel's ends with a ticket on one counter word), channel by channel (run-time C).
//
// ssim_stats_kernel<PixT, MAPS>   the tile and its halo of 5 pixels of x and y -> LDS as doubles (zeros outside the frame); the window along the rows
//                      of the five quantities x, y, x^2, y^2, xy -> LDS (26 rows of 32); the window down the columns -> registers, a thread taking two
//                      adjacent rows of one column, so the twelve rows it reads serve both; SSIM, the two sums through grid_sum, and (MAPS) the
//                      three maps to the scratch as doubles, PLANAR ([3][n, C, H, W]: both kernels then read and write whole rows).
// ssim_adjoint_kernel<PixT>      the three maps with halo -> LDS (zeros outside the frame), the two passes, then image_b from x, y, w, alpha, beta.
//
// A row of 32 lanes reads 32 adjacent doubles of LDS in every pass: all 64 banks once per ds_read_b64 group, no conflicts whatever the row stride.
// Static LDS: 50 752 bytes (stats), 46 176 (adjoint), so three workgroups per CU.  No atomics on values; the order of every sum is fixed by the
// tiling: the taps in order k = -5 .. 5 along a row, then down a column (each tap one fma, written out: the library is built without
// contraction), a thread's tiles and channels in order, then grid_sum.
#pragma once

namespace
{

constexpr int SSIM_WINDOW = 11, SSIM_HALO = SSIM_WINDOW / 2;
constexpr int SSIM_TW = 32, SSIM_TH = 16;					  // pixels of a tile across and down
constexpr int SSIM_ROWS = SSIM_TH / (FH_BLOCK / SSIM_TW);	  // rows of a column one thread takes in the pass down the columns: 2
constexpr int SSIM_HW = SSIM_TW + 2 * SSIM_HALO, SSIM_HH = SSIM_TH + 2 * SSIM_HALO; // a tile with its halo: 42 across, 26 down
constexpr int SSIM_BLOCKS = 1024;							  // workgroups at most (PYR_BLOCKS of dr_pyramid.h: the ticket counter of grid_sum)
static_assert(SSIM_WINDOW == DEODR_HIP_SSIM_WINDOW && FH_BLOCK % SSIM_TW == 0 && SSIM_ROWS * (FH_BLOCK / SSIM_TW) == SSIM_TH, "the tiling of dr_ssim.h");

// g_k = exp(-k^2 / (2 1.5^2)) / sum, k = -5 .. 5, evaluated in double: the digits of deodr_amd/ssim.py's gaussian_window() (tests/test_ssim_abi.py
// compares them)
__device__ constexpr double SSIM_TAPS[SSIM_WINDOW] = {0.00102838008447911,	0.007598758135239185, 0.03600077212843083, 0.10936068950970002,
													  0.2130055377112537,	0.26601172486179436,  0.2130055377112537,  0.10936068950970002,
													  0.03600077212843083,	0.007598758135239185, 0.00102838008447911};

struct SsimArgs
{
	const void *image, *obs, *weights; // [n,H,W,C], [n,H,W,C], [n,H,W] | NULL in the pixel type
	void *image_b;					   // [n,H,W,C] | NULL
	const double *mix;				   // [2], device
	double *terms, *loss;			   // [2], [1] | NULL
	double *partials, *maps;		   // the scratch: [SSIM_BLOCKS, 2], [3][n, C, H, W]
	unsigned *counters;
	double C1, C2;
	int n, H, W, C, TY, TX; // tiles per view, down and across
};

struct SsimTile
{
	int b, y0, x0;
};
__device__ __forceinline__ SsimTile ssim_tile(const SsimArgs &a, long long tile)
{
	const long long per_view = (long long)a.TY * a.TX;
	return {(int)(tile / per_view), (int)(tile % per_view / a.TX) * SSIM_TH, (int)(tile % a.TX) * SSIM_TW};
}

// The window down the columns for the SSIM_ROWS adjacent rows of a thread: out[i] = sum_k g_k h[row + i + k][col], the taps in order for each.
template <int Q>
__device__ __forceinline__ void ssim_columns(const double (&h)[Q][SSIM_HH][SSIM_TW], int row, int col, double (&out)[SSIM_ROWS][Q])
{
#pragma unroll
	for (int i = 0; i < SSIM_ROWS; i++)
#pragma unroll
		for (int q = 0; q < Q; q++)
			out[i][q] = 0;
#pragma unroll
	for (int j = 0; j < SSIM_ROWS + SSIM_WINDOW - 1; j++)
#pragma unroll
		for (int q = 0; q < Q; q++)
		{
			const double v = h[q][row + j][col];
#pragma unroll
			for (int i = 0; i < SSIM_ROWS; i++)
				if (j - i >= 0 && j - i < SSIM_WINDOW)
					out[i][q] = fma(SSIM_TAPS[j - i], v, out[i][q]);
		}
}

template <class PixT, bool MAPS>
__global__ __launch_bounds__(FH_BLOCK) void ssim_stats_kernel(SsimArgs a)
{
	__shared__ double s_x[SSIM_HH][SSIM_HW], s_y[SSIM_HH][SSIM_HW], s_h[5][SSIM_HH][SSIM_TW];
	const PixT *image = (const PixT *)a.image, *obs = (const PixT *)a.obs, *weights = (const PixT *)a.weights;
	const int col = threadIdx.x % SSIM_TW, row = threadIdx.x / SSIM_TW * SSIM_ROWS;
	const size_t plane = (size_t)a.H * a.W, map = plane * a.C * a.n;
	const long long tiles = (long long)a.TY * a.TX * a.n;
	double s[2] = {0, 0};
	for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x)
	{
		const SsimTile t = ssim_tile(a, tile);
		double w[SSIM_ROWS];
		bool in[SSIM_ROWS];
#pragma unroll
		for (int i = 0; i < SSIM_ROWS; i++)
		{
			const int y = t.y0 + row + i, x = t.x0 + col;
			in[i] = y < a.H && x < a.W;
			w[i] = in[i] ? (weights ? (double)weights[((size_t)t.b * a.H + y) * a.W + x] : 1.0) : 0.0;
		}
		for (int ch = 0; ch < a.C; ch++)
		{
			__syncthreads(); // (the passes of the channel before are done with the LDS)
			for (int e = threadIdx.x; e < SSIM_HH * SSIM_HW; e += FH_BLOCK)
			{
				const int r = e / SSIM_HW, c = e % SSIM_HW, y = t.y0 - SSIM_HALO + r, x = t.x0 - SSIM_HALO + c;
				const bool inside = y >= 0 && y < a.H && x >= 0 && x < a.W;
				const size_t at = inside ? (((size_t)t.b * a.H + y) * a.W + x) * a.C + ch : 0;
				s_x[r][c] = inside ? (double)image[at] : 0.0;
				s_y[r][c] = inside ? (double)obs[at] : 0.0;
			}
			__syncthreads();
			for (int e = threadIdx.x; e < SSIM_HH * SSIM_TW; e += FH_BLOCK)
			{ // the window along the rows, every row of the halo
				const int r = e / SSIM_TW, c = e % SSIM_TW;
				double hx = 0, hy = 0, hxx = 0, hyy = 0, hxy = 0;
#pragma unroll
				for (int k = 0; k < SSIM_WINDOW; k++)
				{
					const double g = SSIM_TAPS[k], xv = s_x[r][c + k], yv = s_y[r][c + k];
					hx = fma(g, xv, hx), hy = fma(g, yv, hy), hxx = fma(g, xv * xv, hxx), hyy = fma(g, yv * yv, hyy), hxy = fma(g, xv * yv, hxy);
				}
				s_h[0][r][c] = hx, s_h[1][r][c] = hy, s_h[2][r][c] = hxx, s_h[3][r][c] = hyy, s_h[4][r][c] = hxy;
			}
			__syncthreads();
			double m[SSIM_ROWS][5];
			ssim_columns<5>(s_h, row, col, m);
#pragma unroll
			for (int i = 0; i < SSIM_ROWS; i++)
			{
				if (!in[i])
					continue;
				const double mx = m[i][0], my = m[i][1], sxx = m[i][2] - mx * mx, syy = m[i][3] - my * my, sxy = m[i][4] - mx * my;
				const double a1 = 2 * mx * my + a.C1, a2 = 2 * sxy + a.C2, b1 = mx * mx + my * my + a.C1, b2 = sxx + syy + a.C2;
				const double inv = 1.0 / (b1 * b2), ssim = a1 * a2 * inv;
				const double d = s_x[row + i + SSIM_HALO][col + SSIM_HALO] - s_y[row + i + SSIM_HALO][col + SSIM_HALO];
				s[0] += w[i] * (d * d);
				s[1] += w[i] * (1.0 - ssim);
				if (MAPS)
				{
					const double S_xy = 2 * a1 * inv, S_xx = -ssim / b2;
					const double S_m = 2 * my * a2 * inv - 2 * mx * ssim / b1 - 2 * mx * S_xx - my * S_xy;
					const size_t at = ((size_t)t.b * a.C + ch) * plane + (size_t)(t.y0 + row + i) * a.W + (t.x0 + col);
					a.maps[at] = -w[i] * S_m, a.maps[map + at] = -w[i] * S_xx, a.maps[2 * map + at] = -w[i] * S_xy;
				}
			}
		}
	}
	double total[2];
	if (grid_sum<2>(s, a.partials, a.counters + 0, total) && threadIdx.x == 0)
	{
		a.terms[0] = total[0], a.terms[1] = total[1];
		if (a.loss)
			a.loss[0] = a.mix[0] * total[0] + a.mix[1] * total[1];
	}
}

template <class PixT>
__global__ __launch_bounds__(FH_BLOCK) void ssim_adjoint_kernel(SsimArgs a)
{
	__shared__ double s_m[3][SSIM_HH][SSIM_HW], s_h[3][SSIM_HH][SSIM_TW];
	const PixT *image = (const PixT *)a.image, *obs = (const PixT *)a.obs, *weights = (const PixT *)a.weights;
	PixT *image_b = (PixT *)a.image_b;
	const int col = threadIdx.x % SSIM_TW, row = threadIdx.x / SSIM_TW * SSIM_ROWS;
	const size_t plane = (size_t)a.H * a.W, map = plane * a.C * a.n;
	const long long tiles = (long long)a.TY * a.TX * a.n;
	const double alpha = a.mix[0], beta = a.mix[1];
	for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x)
	{
		const SsimTile t = ssim_tile(a, tile);
		for (int ch = 0; ch < a.C; ch++)
		{
			__syncthreads();
			for (int e = threadIdx.x; e < SSIM_HH * SSIM_HW; e += FH_BLOCK)
			{
				const int r = e / SSIM_HW, c = e % SSIM_HW, y = t.y0 - SSIM_HALO + r, x = t.x0 - SSIM_HALO + c;
				const bool inside = y >= 0 && y < a.H && x >= 0 && x < a.W;
				const size_t at = inside ? ((size_t)t.b * a.C + ch) * plane + (size_t)y * a.W + x : 0;
#pragma unroll
				for (int q = 0; q < 3; q++)
					s_m[q][r][c] = inside ? a.maps[q * map + at] : 0.0;
			}
			__syncthreads();
			for (int e = threadIdx.x; e < SSIM_HH * SSIM_TW; e += FH_BLOCK)
			{
				const int r = e / SSIM_TW, c = e % SSIM_TW;
				double h[3] = {0, 0, 0};
#pragma unroll
				for (int k = 0; k < SSIM_WINDOW; k++)
#pragma unroll
					for (int q = 0; q < 3; q++)
						h[q] = fma(SSIM_TAPS[k], s_m[q][r][c + k], h[q]);
#pragma unroll
				for (int q = 0; q < 3; q++)
					s_h[q][r][c] = h[q];
			}
			__syncthreads();
			double g[SSIM_ROWS][3];
			ssim_columns<3>(s_h, row, col, g);
#pragma unroll
			for (int i = 0; i < SSIM_ROWS; i++)
			{
				const int y = t.y0 + row + i, x = t.x0 + col;
				if (y >= a.H || x >= a.W)
					continue;
				const size_t pix = ((size_t)t.b * a.H + y) * a.W + x, at = pix * a.C + ch;
				const double xv = (double)image[at], yv = (double)obs[at], w = weights ? (double)weights[pix] : 1.0;
				image_b[at] = (PixT)(2 * alpha * w * (xv - yv) + beta * (g[i][0] + 2 * xv * g[i][1] + yv * g[i][2]));
			}
		}
	}
}

} // namespace
