// deodr_amd/csrc/dr_binning.h -- the rejection rule of setup_bin_kernel's binning (dr_setup.h): which tiles of a 3 x 3 block of a primitive's
// box of tiles are clearly outside it.  `__host__ __device__`: the kernel and the host simulator (tests/sim/tile_sim.cpp) compile this one copy.
// The includer declares the compile-time tile size TILE (dr_workspace.h; the simulator takes the same number from that file).
// (The index arithmetic of the walk over a box -- block -> tiles, the kept column -- stays written out in the kernel, where the slot requests
// of a triangle's first block leave ahead of the attribute arithmetic: calling it through helpers cost the six instances 3 VGPRs each.  The
// simulator restates it.)
#pragma once

#include "dr_math.h"

namespace dr
{

// Conservative rejection for binning: a primitive covers a pixel only where every one of its N half-plane functions
// E = a x + b y + c is >= 0 (or > 0); if some E is clearly negative on the corner pixel of a tile where it is largest, no pixel of
// the tile can be covered.  The slack keeps the test safe against the rounding of the exact span arithmetic used later.
// For the 3 x 3 block of tiles whose first tile is (tx0, ty0): bit 3 dy + dx of the result is set when tile (tx0 + dx, ty0 + dy) is
// clearly outside one of the half-planes.  The corner where a half-plane function is largest is the same in every tile, so a x and
// b y + c are formed once per column / row of tiles (a test per tile costs ~20 operations per half-plane and tile, and binning was half
// of the arithmetic of the set-up kernel).  The slack uses the largest scale of the block, its far corner.
template <int N>
DR_HD uint32_t tiles3x3_outside_halfplanes(const double *eq, int tx0, int ty0)
{
	uint32_t out = 0;
	const double xmax = (tx0 + 2) * TILE + (TILE - 1), ymax = (ty0 + 2) * TILE + (TILE - 1);
#pragma unroll
	for (int k = 0; k < N; k++)
	{
		const double a = eq[3 * k], b = eq[3 * k + 1], c = eq[3 * k + 2];
		const double limit = -1e-9 * (fabs(a) * xmax + fabs(b) * ymax + fabs(c)) - 1e-12;
		const double cx = tx0 * TILE + (a > 0 ? TILE - 1 : 0), cy = ty0 * TILE + (b > 0 ? TILE - 1 : 0);
		double ax[3], by[3];
#pragma unroll
		for (int d = 0; d < 3; d++)
		{
			ax[d] = a * (cx + d * TILE);
			by[d] = b * (cy + d * TILE) + c;
		}
#pragma unroll
		for (int q = 0; q < 9; q++)
			out |= (ax[q % 3] + by[q / 3] < limit) ? (1u << q) : 0u;
	}
	return out;
}

} // namespace dr
