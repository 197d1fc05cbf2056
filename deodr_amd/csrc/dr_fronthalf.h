// deodr_amd/csrc/dr_fronthalf.h -- part of the single translation unit dr_kernels.hip (device code, gfx950 / wave64).
// The O(V) algebra either side of the rasterizer in a fit iteration.  At the top of THIS file and nowhere else, what the kernels
// of dr_fititer.h, dr_texfit.h, dr_subdiv.h, dr_basis.h, dr_camera.h, dr_lighting.h, dr_skinning.h, dr_pyramid.h, dr_ssim.h, dr_solve.h and dr_arap.h share with the ones here: Vec3, unit, qrot_point, CameraRow,
// project_point and their adjoints; lane_group_sum, last_to_arrive (the arrival ticket), grid_sum, total_of_thread, store_or_add.  Then the kernels:
//
//   rigid_transform_kernel (+ _b)   centred vertices -> posed vertices of every view: qrot(q, v) + t
//                                   (deodr/tools.py:8-35 qrot / qrot_backward; deodr/mesh_fitter.py:139-151)
//   project_points_kernel (+ _b)    pinhole camera with OpenCV's distortion: posed vertices -> image coordinates + depths
//                                   (Camera.project_points / project_points_backward, deodr/differentiable_renderer.py:341-438)
//   silhouette_flags_kernel         edge flags of every view: exactly one of the (at most two) faces on an edge is front-facing in
//                                   the image (TriMeshAdjacencies.edge_on_silhouette, deodr/triangulated_mesh.py:153-166)
//   momentum_update_kernel          x += s, s = (1 - damping)(inertia s + (1 - inertia) clamp(-factor g)) for all parameters of a
//                                   fitter in one launch (deodr/mesh_fitter.py:153-190)
//
// Why kernels: as torch ops one fit iteration is ~240 launches of 2 - 8 us each whatever the mesh size (profiles/README.md, round 3);
// these four groups are ~150 of them.  The arithmetic is double like the reference's NumPy; nothing here is on the rasterizer's path.
#pragma once

#include "dr_finalize.h"

using namespace dr;

namespace
{

// ---- the small algebra of pose, camera and normals (no contraction, no fast-math: an inlined function gives every caller the bits of its text)
struct Vec3
{
	double x, y, z;
};
__device__ __forceinline__ Vec3 cross3(const Vec3 &a, const Vec3 &b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ Vec3 add3(const Vec3 &a, const Vec3 &b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ Vec3 sub3(const Vec3 &a, const Vec3 &b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ Vec3 scale3(double s, const Vec3 &a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ double dot3(const Vec3 &a, const Vec3 &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ Vec3 load3(const double *p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ void store3(double *p, const Vec3 &a) { p[0] = a.x, p[1] = a.y, p[2] = a.z; }

// a / |a| with the length it was divided by, and the adjoint through it: a_b = (N_b - N (N . N_b)) / |a|
struct Unit
{
	Vec3 N;
	double len;
};
__device__ __forceinline__ Unit unit(const Vec3 &a)
{
	const double len = sqrt(dot3(a, a));
	return {{a.x / len, a.y / len, a.z / len}, len};
}
__device__ __forceinline__ Vec3 unit_b(const Vec3 &N, double len, const Vec3 &N_b)
{
	const double along = dot3(N, N_b);
	return {(N_b.x - N.x * along) / len, (N_b.y - N.y * along) / len, (N_b.z - N.z * along) / len};
}

// q = (x, y, z, w) = (u, w), unit: r = p + 2 (w a + bb), a = u x p, bb = u x a   (deodr/tools.py:8-22)
__device__ __forceinline__ Vec3 qrot_point(const Vec3 &u, double w, const Vec3 &p)
{
	const Vec3 a = cross3(u, p), bb = cross3(u, a);
	return {p.x + 2 * (w * a.x + bb.x), p.y + 2 * (w * a.y + bb.y), p.z + 2 * (w * a.z + bb.z)};
}
// its adjoint for r_b = g   (deodr/tools.py:25-35)
struct QrotB
{
	Vec3 p_b, u_b;
	double w_b;
};
__device__ __forceinline__ QrotB qrot_point_b(const Vec3 &u, double w, const Vec3 &p, const Vec3 &g)
{
	const Vec3 a = cross3(u, p);
	const double w_b = 2 * dot3(g, a);
	const Vec3 bb_b = scale3(2, g);
	const Vec3 a_b = add3(scale3(2 * w, g), cross3(bb_b, u)); // from 2 w a and from bb = u x a
	const Vec3 u_b = add3(cross3(a, bb_b), cross3(p, a_b));	  // from bb = u x a and from a = u x p
	return {add3(g, cross3(a_b, u)), u_b, w_b};
}

// projection (dr.py:341-395): pc = R p + T; (x, y) = pc.xy / pc.z; distortion (k1, k2, p1, p2, k3); ij = K[:2,:2] (xd, yd) + K[:2,2]
struct CameraRow
{
	double E[12], K[6], d[5];
	bool distort;
};
__device__ __forceinline__ CameraRow load_camera(const double *extrinsic, const double *intrinsic, const double *distortion, int b)
{
	CameraRow c;
#pragma unroll
	for (int i = 0; i < 12; i++)
		c.E[i] = extrinsic[12 * b + i];
#pragma unroll
	for (int i = 0; i < 6; i++)
		c.K[i] = intrinsic[9 * b + i]; // the first two rows of the 3 x 3 matrix
	c.distort = distortion != nullptr;
#pragma unroll
	for (int i = 0; i < 5; i++)
		c.d[i] = c.distort ? distortion[5 * b + i] : 0.0;
	return c;
}

__device__ __forceinline__ void project_point(const CameraRow &c, const Vec3 &p, double &i, double &j, double &depth)
{
	const double cx = c.E[0] * p.x + c.E[1] * p.y + c.E[2] * p.z + c.E[3], cy = c.E[4] * p.x + c.E[5] * p.y + c.E[6] * p.z + c.E[7],
				 cz = c.E[8] * p.x + c.E[9] * p.y + c.E[10] * p.z + c.E[11];
	double x = cx / cz, y = cy / cz;
	if (c.distort)
	{
		const double k1 = c.d[0], k2 = c.d[1], p1 = c.d[2], p2 = c.d[3], k3 = c.d[4];
		const double x2 = x * x, y2 = y * y, r2 = x2 + y2, r4 = r2 * r2;
		const double radial = 1 + k1 * r2 + k2 * r4 + k3 * (r2 * r4);
		const double xd = x * radial + (2 * p1 * x * y + p2 * (r2 + 2 * x2)), yd = y * radial + (p1 * (r2 + 2 * y2) + 2 * p2 * x * y);
		x = xd, y = yd;
	}
	i = c.K[0] * x + c.K[1] * y + c.K[2];
	j = c.K[3] * x + c.K[4] * y + c.K[5];
	depth = cz;
}

// adjoint of the above (Camera.project_points_backward, dr.py:397-438) for (i_b, j_b, depth_b) = (g0, g1, gd): the point's adjoint, and what the
// adjoints of the camera's own entries are made of (camera_project_b_kernel, dr_camera.h; a caller that wants point_b alone computes nothing else)
struct ProjectB
{
	Vec3 point_b, camera_b;					  // camera_b: the adjoint of pc = R p + T
	double x, y, xd_b, yd_b;				  // pc.xy / pc.z; the adjoint of the distorted point
	double r2, r4, radial, radial_b;		  // with distortion only
};
__device__ __forceinline__ ProjectB project_point_b(const CameraRow &c, const Vec3 &p, double g0, double g1, double gd)
{
	const double cx = c.E[0] * p.x + c.E[1] * p.y + c.E[2] * p.z + c.E[3], cy = c.E[4] * p.x + c.E[5] * p.y + c.E[6] * p.z + c.E[7],
				 cz = c.E[8] * p.x + c.E[9] * p.y + c.E[10] * p.z + c.E[11];
	ProjectB r;
	const double x = cx / cz, y = cy / cz;
	const double xd_b = c.K[0] * g0 + c.K[3] * g1, yd_b = c.K[1] * g0 + c.K[4] * g1;
	double x_b = xd_b, y_b = yd_b;
	r.r2 = r.r4 = r.radial_b = 0, r.radial = 1;
	if (c.distort)
	{
		const double k1 = c.d[0], k2 = c.d[1], p1 = c.d[2], p2 = c.d[3], k3 = c.d[4];
		const double r2 = x * x + y * y, r4 = r2 * r2;
		const double radial = 1 + k1 * r2 + k2 * r4 + k3 * (r2 * r4);
		const double radial_b = x * xd_b + y * yd_b;
		x_b = radial * xd_b + 2 * p1 * y * xd_b + 4 * p2 * x * xd_b + 2 * p2 * y * yd_b;
		y_b = radial * yd_b + 2 * p1 * x * xd_b + 4 * p1 * y * yd_b + 2 * p2 * x * yd_b;
		const double r2_b = p2 * xd_b + p1 * yd_b + radial_b * (k1 + 2 * k2 * r2 + 3 * k3 * r4);
		x_b += 2 * x * r2_b;
		y_b += 2 * y * r2_b;
		r.r2 = r2, r.r4 = r4, r.radial = radial, r.radial_b = radial_b;
	}
	const double cx_b = x_b / cz, cy_b = y_b / cz, cz_b = gd - (x * x_b + y * y_b) / cz;
	r.point_b = {c.E[0] * cx_b + c.E[4] * cy_b + c.E[8] * cz_b, c.E[1] * cx_b + c.E[5] * cy_b + c.E[9] * cz_b, c.E[2] * cx_b + c.E[6] * cy_b + c.E[10] * cz_b};
	r.camera_b = {cx_b, cy_b, cz_b};
	r.x = x, r.y = y, r.xd_b = xd_b, r.yd_b = yd_b;
	return r;
}

constexpr int FH_BLOCK = 256;

// ---- the sum over each group of adjacent lanes whose lane numbers differ in the bits FIRST, 2 FIRST, ... < END (powers of two), in every lane of
// the group: a butterfly, an order fixed by the lane numbers alone.  All lanes of the wavefront call it.
template <int FIRST, int END>
__device__ __forceinline__ double lane_group_sum(double v)
{
#pragma unroll
	for (int d = FIRST; d < END; d <<= 1)
		v += __shfl_xor(v, d);
	return v;
}
template <int FIRST, int END>
__device__ __forceinline__ Vec3 lane_group_sum3(const Vec3 &a)
{
	return {lane_group_sum<FIRST, END>(a.x), lane_group_sum<FIRST, END>(a.y), lane_group_sum<FIRST, END>(a.z)};
}

// ---- the arrival ticket: the one memory-ordering protocol of these headers.  Every thread of a workgroup calls it after that thread's partials
// are stored; n workgroups draw on `counter`, a word that is zero between launches.  -> true in ALL threads of the last workgroup to arrive, whose
// loads then see every workgroup's partials.  That workgroup calls reset_arrivals once it is done.
__device__ __forceinline__ bool last_to_arrive(unsigned *counter, unsigned n)
{
	__shared__ int s_last;
	__syncthreads();
	if (threadIdx.x == 0)
	{
		__threadfence(); // release (one thread, after the barrier: the workgroup's partials are visible to the device before its ticket)
		s_last = atomicAdd(counter, 1u) == n - 1;
	}
	__syncthreads();
	if (!s_last)
		return false;
	__threadfence(); // acquire: the loads that follow see every workgroup's partials
	return true;
}
__device__ __forceinline__ void reset_arrivals(unsigned *counter) { if (threadIdx.x == 0) atomicExch(counter, 0u); }

// ---- deterministic grid-wide sums without atomics on the values.  Every thread of every workgroup of a launch (blockIdx.x over the reduced
// range) brings K values; `partials` holds K doubles per workgroup, `counter` one word for last_to_arrive.  -> true in ALL threads of the last
// workgroup, whose total[] then holds the sums: the partial of workgroup i is added by thread i mod FH_BLOCK in the order i, i + FH_BLOCK, ...;
// then the lanes of a wavefront (DPP tree), then the wavefronts in order -- fixed by the launch geometry alone.
template <int K>
__device__ __forceinline__ bool grid_sum(const double (&v)[K], double *partials, unsigned *counter, double (&total)[K], unsigned block = blockIdx.x,
										 unsigned nblocks = gridDim.x)
{ // (block / nblocks: the position of this workgroup among the ones that take part, for kernels that are a part of a launch)
	__shared__ double s_wave[FH_BLOCK / 64][K];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
	for (int k = 0; k < K; k++)
	{
		const double s = wave_sum(v[k]);
		if (lane == 0)
			s_wave[wave][k] = s;
	}
	__syncthreads();
	if (threadIdx.x < K)
	{
		double s = 0;
		for (int w = 0; w < FH_BLOCK / 64; w++)
			s += s_wave[w][threadIdx.x];
		partials[(size_t)block * K + threadIdx.x] = s;
	}
	if (!last_to_arrive(counter, nblocks))
		return false;
	double mine[K];
#pragma unroll
	for (int k = 0; k < K; k++)
		mine[k] = 0;
	for (unsigned i = threadIdx.x; i < nblocks; i += FH_BLOCK)
#pragma unroll
		for (int k = 0; k < K; k++)
			mine[k] += partials[(size_t)i * K + k];
#pragma unroll
	for (int k = 0; k < K; k++)
	{
		const double s = wave_sum(mine[k]);
		if (lane == 0)
			s_wave[wave][k] = s; // (every thread is past its reads of s_wave: the barriers of last_to_arrive)
	}
	__syncthreads();
#pragma unroll
	for (int k = 0; k < K; k++)
	{
		total[k] = 0;
		for (int w = 0; w < FH_BLOCK / 64; w++)
			total[k] += s_wave[w][k];
	}
	reset_arrivals(counter);
	return true;
}

// What the last workgroup does with its totals.  Thread k's own: total[k] by a chain of compares (not an indexed register file: that is scratch);
// 0 for k >= K.
template <int K>
__device__ __forceinline__ double total_of_thread(const double (&total)[K], int k)
{
	double mine = 0;
#pragma unroll
	for (int i = 0; i < K; i++)
		mine = k == i ? total[i] : mine;
	return mine;
}
// an output that a call either writes or adds to
__device__ __forceinline__ void store_or_add(double *out, double v, int accumulate) { *out = accumulate ? *out + v : v; }

// ---- rigid transform: out[b][v] = qrot(q[b], v[v]) + t[b]   (q = (x, y, z, w), unit)
__global__ __launch_bounds__(FH_BLOCK) void rigid_transform_kernel(const double *vc, const double *q, const double *t, double *out, int V, int n)
{
	const int v = blockIdx.x * FH_BLOCK + threadIdx.x, b = blockIdx.y;
	if (v >= V)
		return;
	const Vec3 r = qrot_point(load3(q + 4 * b), q[4 * b + 3], load3(vc + 3 * v));
	double *o = out + ((size_t)b * V + v) * 3;
	o[0] = r.x + t[3 * b], o[1] = r.y + t[3 * b + 1], o[2] = r.z + t[3 * b + 2]; // (not load3(t): three values read ahead of the stores are 6 VGPRs more)
}

// adjoint: one thread per vertex walks the views (vc_b[v] = sum over views: no atomics, fixed order); the sums over the vertices --
// q_b [n,4], t_b [n,3] -- are reduced per wavefront and leave with one atomic per value, wavefront and view (zeroed by the caller)
__global__ __launch_bounds__(FH_BLOCK) void rigid_transform_b_kernel(const double *vc, const double *q, const double *out_b, double *vc_b, double *q_b,
																	  double *t_b, int V, int n)
{
	const int v = blockIdx.x * FH_BLOCK + threadIdx.x, lane = threadIdx.x & 63;
	const bool on = v < V;
	const Vec3 p = on ? load3(vc + 3 * v) : Vec3{0, 0, 0};
	Vec3 acc = {0, 0, 0};
	for (int b = 0; b < n; b++)
	{
		const Vec3 u = load3(q + 4 * b);
		const double w = q[4 * b + 3];
		const Vec3 g = on ? load3(out_b + ((size_t)b * V + v) * 3) : Vec3{0, 0, 0};
		const QrotB r = qrot_point_b(u, w, p, g);
		acc = add3(acc, r.p_b);
		const double sums[7] = {r.u_b.x, r.u_b.y, r.u_b.z, r.w_b, g.x, g.y, g.z};
#pragma unroll
		for (int i = 0; i < 7; i++)
		{
			const double s = wave_sum(sums[i]); // (every lane takes part: lanes beyond V hold zeros)
			if (lane == 0 && s != 0)
				atomic_add_f64(i < 4 ? q_b + 4 * b + i : t_b + 3 * b + (i - 4), s);
		}
	}
	if (on)
		store3(vc_b + 3 * v, acc);
}

// ---- projection: project_point and its adjoint, one thread per (view, vertex)
__global__ __launch_bounds__(FH_BLOCK) void project_points_kernel(const double *points, const double *extrinsic, const double *intrinsic,
																   const double *distortion, double *ij, double *depths, int V, int n)
{
	const int v = blockIdx.x * FH_BLOCK + threadIdx.x, b = blockIdx.y;
	if (v >= V)
		return;
	const CameraRow c = load_camera(extrinsic, intrinsic, distortion, b);
	const size_t at = (size_t)b * V + v;
	project_point(c, load3(points + at * 3), ij[2 * at], ij[2 * at + 1], depths[at]);
}

__global__ __launch_bounds__(FH_BLOCK) void project_points_b_kernel(const double *points, const double *extrinsic, const double *intrinsic,
																	 const double *distortion, const double *ij_b, const double *depths_b, double *points_b, int V,
																	 int n)
{ // depths_b may be NULL
	const int v = blockIdx.x * FH_BLOCK + threadIdx.x, b = blockIdx.y;
	if (v >= V)
		return;
	const CameraRow c = load_camera(extrinsic, intrinsic, distortion, b);
	const size_t at = (size_t)b * V + v;
	store3(points_b + at * 3, project_point_b(c, load3(points + at * 3), ij_b[2 * at], ij_b[2 * at + 1], depths_b ? depths_b[at] : 0.0).point_b);
}

// ---- silhouette flags: flag[b][f][e] = 1 when exactly one face on edge e of face f is front-facing in view b.
// edge_faces [T,3]: the face on the other side of edge (v_e, v_{e+1}) of face f, or 0xffffffff on a boundary (static per mesh).
__device__ __forceinline__ void silhouette_flags_block(const double *ij, const uint32_t *faces, const uint32_t *edge_faces, uint8_t *flags, int T, int V,
													   int clockwise, int bx, int b)
{
	const int f = bx * FH_BLOCK + threadIdx.x;
	if (f >= T)
		return;
	const double *p = ij + (size_t)b * V * 2;
	auto visible = [&](uint32_t face) {
		const uint32_t i0 = faces[3 * face], i1 = faces[3 * face + 1], i2 = faces[3 * face + 2];
		const double ux = p[2 * i1] - p[2 * i0], uy = p[2 * i1 + 1] - p[2 * i0 + 1], vx = p[2 * i2] - p[2 * i0], vy = p[2 * i2 + 1] - p[2 * i0 + 1];
		const double cr = ux * vy - uy * vx;
		return clockwise ? cr > 0 : cr < 0;
	};
	const bool mine = visible((uint32_t)f);
#pragma unroll
	for (int e = 0; e < 3; e++)
	{
		const uint32_t other = edge_faces[3 * f + e];
		const int count = (mine ? 1 : 0) + ((other != 0xffffffffu && visible(other)) ? 1 : 0);
		flags[((size_t)b * T + f) * 3 + e] = count == 1 ? 1 : 0;
	}
}
__global__ __launch_bounds__(FH_BLOCK) void silhouette_flags_kernel(const double *ij, const uint32_t *faces, const uint32_t *edge_faces, uint8_t *flags, int T,
																	 int V, int clockwise)
{
	silhouette_flags_block(ij, faces, edge_faces, flags, T, V, clockwise, blockIdx.x, blockIdx.y);
}

// ---- momentum update of up to MOMENTUM_MAX parameter tensors in one launch, IN PLACE
constexpr int MOMENTUM_MAX = 8;
struct MomentumArgs
{
	double *x[MOMENTUM_MAX], *speed[MOMENTUM_MAX];
	const double *grad[MOMENTUM_MAX], *grad2[MOMENTUM_MAX]; // the step follows -(grad_scale (grad - grad_mean) + grad2): grad2 = the rigid energy's
	const double *grad_mean[MOMENTUM_MAX];					// optional [3]: subtracted from every row of a [count/3, 3] gradient (zero-mean projection)
	double *mean_out[MOMENTUM_MAX];							// optional [3]: column mean of the updated [count/3, 3] tensor (next step's centring)
	double grad_scale[MOMENTUM_MAX], factor[MOMENTUM_MAX], step_max[MOMENTUM_MAX]; // step_max <= 0: no clamp
	int count[MOMENTUM_MAX], normalize_rows[MOMENTUM_MAX]; // normalize_rows = row length: rows of x renormalised afterwards (quaternions)
	int n;
	double inertia, damping;
	double *partials; // 3 doubles per workgroup and tensor (mean_out)
	double *energy;	  // optional [2]: energy[1] = data_weight * data_energy[0] + energy[0], what a fitter's step reports (mesh_fitter.py:147)
	const double *data_energy;
	double data_weight;
	unsigned *counters; // one word per tensor
};
__device__ __forceinline__ double momentum_step(const MomentumArgs &a, int k, int at, int column)
{
	double g = a.grad[k][at];
	if (a.grad_mean[k])
		g -= a.grad_mean[k][column];
	g = g * a.grad_scale[k] + (a.grad2[k] ? a.grad2[k][at] : 0.0);
	double step = -g * a.factor[k];
	if (a.step_max[k] > 0)
		step = fmin(fmax(step, -a.step_max[k]), a.step_max[k]);
	const double s = (1 - a.damping) * (a.speed[k][at] * a.inertia + (1 - a.inertia) * step);
	a.speed[k][at] = s;
	return s;
}
__global__ __launch_bounds__(FH_BLOCK) void momentum_update_kernel(MomentumArgs a)
{
	const int k = blockIdx.y;
	const int i = blockIdx.x * FH_BLOCK + threadIdx.x;
	const int rows = a.normalize_rows[k];
	if (a.energy && k == 0 && i == 0)
		a.energy[1] = a.data_weight * a.data_energy[0] + a.energy[0];
	if (rows > 0)
	{ // one thread per row (a handful of quaternions)
		const int nrow = a.count[k] / rows;
		if (i >= nrow)
			return;
		double norm2 = 0;
		for (int j = 0; j < rows; j++)
		{
			const int at = i * rows + j;
			const double xn = a.x[k][at] + momentum_step(a, k, at, 0);
			a.x[k][at] = xn;
			norm2 += xn * xn;
		}
		const double inv = 1 / sqrt(norm2);
		for (int j = 0; j < rows; j++)
			a.x[k][i * rows + j] *= inv;
		return;
	}
	double col[3] = {0, 0, 0};
	if (i < a.count[k])
	{
		const double xn = a.x[k][i] + momentum_step(a, k, i, i % 3);
		a.x[k][i] = xn;
		col[i % 3] = xn;
	}
	if (!a.mean_out[k])
		return; // (uniform per workgroup row)
	double total[3];
	if (grid_sum<3>(col, a.partials + (size_t)k * gridDim.x * 3, a.counters + k, total) && threadIdx.x < 3)
		a.mean_out[k][threadIdx.x] = total[threadIdx.x] / (a.count[k] / 3);
}

} // namespace
