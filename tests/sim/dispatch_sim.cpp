// tests/sim/dispatch_sim.cpp -- TEST TOOL, never part of the product.
//
// The instance rules and the instance tables of deodr_amd/csrc/dr_dispatch.h (host-only C++, the very header dr_kernels.hip launches from) behind a C
// interface of plain ints, for tests/test_dispatch.py.
#include "../../deodr_amd/csrc/dr_dispatch.h"

using namespace dr::dispatch;

namespace
{
void put(const FwdInst &k, int *out)
{
	const int v[7] = {k.fused, k.tex, k.clamp, k.nc, k.common, k.texe, k.var};
	for (int i = 0; i < 7; i++)
		out[i] = v[i];
}
void put(const BwdInst &k, int *out) { out[0] = k.tex, out[1] = k.nc; }
void put(const PrimInst &k, int *out) { out[0] = k.vtx_f64, out[1] = k.nc, out[2] = k.det, out[3] = k.table; }

// rows of `width` ints into out (room for `cap` rows); returns the number of entries that exist for the pixel type
template <class Inst, int N, class Exists>
int table(const Inst (&t)[N], Exists exists, int width, int *out, int cap)
{
	int n = 0;
	for (const Inst &k : t)
		if (exists(k))
		{
			if (n < cap)
				put(k, out + width * n);
			n++;
		}
	return n;
}
} // namespace

extern "C" {

// in: f64, fused, tex, fuse_edges, clamp, weights, aa_err, C, common, n_views, tile_blocks, heavy_share, capturing
// out: FUSED, TEX, CLAMP, NC, COMMON, TEXE, VAR; returns 1 for the two-kernel form (out is its TEXE = 2 instance, the other one is TEXE = 3)
int dispatch_forward(const int *in, int *out)
{
	const FwdInst k = select_forward(FwdCall{in[0] != 0, in[1] != 0, in[2] != 0, in[3] != 0, in[4] != 0, in[5] != 0, in[6] != 0, in[8] != 0, in[12] != 0, in[7],
											 in[9], in[10], in[11]});
	put(k, out);
	return k.texe == 2;
}
int dispatch_forward_table(int f64, int *out, int cap)
{
	return table(FWD_INSTANCES, [&](const FwdInst &k) { return fwd_exists(k, f64 != 0); }, 7, out, cap);
}

void dispatch_adjoint_raster(int f64, int tex, int C, int *out) { put(select_adjoint_raster(f64 != 0, tex != 0, C), out); } // out: TEX, NC
int dispatch_adjoint_raster_table(int f64, int *out, int cap)
{
	return table(BWD_INSTANCES, [&](const BwdInst &k) { return bwd_exists(k, f64 != 0); }, 2, out, cap);
}

// out: VTX64, NC, DET, TABLE (set-up: the first two)
void dispatch_setup(int vtx_f64, int C, int *out) { put(select_setup(vtx_f64 != 0, C), out); }
int dispatch_setup_table(int *out, int cap)
{
	return table(SETUP_INSTANCES, [](const PrimInst &) { return true; }, 4, out, cap);
}
void dispatch_finalize(int vtx_f64, int C, int det, int prim_tables, int *out) { put(select_finalize(vtx_f64 != 0, C, det != 0, prim_tables != 0), out); }
int dispatch_finalize_table(int *out, int cap)
{
	return table(FINALIZE_INSTANCES, [](const PrimInst &) { return true; }, 4, out, cap);
}
}
