// The camera as a differentiable input (include/deodr_hip_camera.h): the full adjoint of project_points_kernel (dr_fronthalf.h) -- the points' adjoint
// AND the 12 + 6 + 5 sums over the vertices that are the adjoints of a view's extrinsic, intrinsic and distortion --, and the map from calibration
// parameters (quaternion + translation per view; focal, centre, distortion) to the per-view matrices the kernels index, with its adjoint.
//
// camera_project_b_kernel: grid (camera_blocks(V, n), n), the view's camera row uniform per workgroup (load_camera); a thread walks the vertices
// 256 block + thread + 256 blocks i, recomputes the forward of each with project_point_b, the one copy of that adjoint (dr_fronthalf.h), keeps the
// 23 sums in registers; per view one grid_sum<12> (extrinsic) and one grid_sum<11> (intrinsic, distortion), each on its own partial range and counter
// word of that view; the last workgroup of a view to arrive at each writes (or adds to) those outputs, the second also the zero row of intrinsic_b.
// 48 - 72 bytes per vertex and view: bound by launch latency at mesh sizes, not tuned further.
#pragma once

namespace
{

constexpr int CAMERA_MAX_VERTICES = 1 << 24;
constexpr int CAMERA_SUMS = 23;			   // 12 extrinsic + 6 intrinsic (two rows) + 5 distortion
constexpr int CAMERA_SUMS_E = 12;		   // the extrinsic's, summed by a grid_sum of their own
constexpr int CAMERA_MIN_VERTICES = 1024;  // vertices below which a workgroup is not worth having: four trips of its 256 threads
constexpr int CAMERA_TARGET_BLOCKS = 1024; // workgroups from which the chip (256 CUs) is full: four per CU
constexpr int CAMERA_MAX_BLOCKS = 256;	   // per view: the last workgroup of a view reads that many partials in ONE trip of its 256 threads

static_assert(CAMERA_MAX_BLOCKS <= FH_BLOCK, "the last workgroup's pass over the partials of a view is one trip");

// the one rule the launch, the scratch layout and deodr_hip_camera_blocks() follow.  Non-decreasing in V.
inline int camera_blocks(int V, int n)
{
	const int units = (V + CAMERA_MIN_VERTICES - 1) / CAMERA_MIN_VERTICES;
	int want = (CAMERA_TARGET_BLOCKS + n - 1) / n;
	want = want < CAMERA_MAX_BLOCKS ? want : CAMERA_MAX_BLOCKS;
	return units < want ? units : want;
}

struct CameraProjectBArgs
{
	const double *points, *extrinsic, *intrinsic, *distortion, *ij_b, *depths_b;
	double *points_b, *extrinsic_b, *intrinsic_b, *distortion_b, *partials;
	unsigned *counters;
	int V, accumulate;
};

__global__ __launch_bounds__(FH_BLOCK) void camera_project_b_kernel(CameraProjectBArgs a)
{
	const int b = blockIdx.y, V = a.V;
	const CameraRow c = load_camera(a.extrinsic, a.intrinsic, a.distortion, b);
	double s[CAMERA_SUMS];
#pragma unroll
	for (int k = 0; k < CAMERA_SUMS; k++)
		s[k] = 0;
	for (int v = blockIdx.x * FH_BLOCK + threadIdx.x; v < V; v += gridDim.x * FH_BLOCK)
	{ // project_point_b (dr_fronthalf.h) gives points_b -- the bits of project_points_b_kernel, which calls it too -- and what the sums are made of
		const size_t at = (size_t)b * V + v;
		const Vec3 p = load3(a.points + at * 3);
		const double px = p.x, py = p.y, pz = p.z, g0 = a.ij_b[2 * at], g1 = a.ij_b[2 * at + 1];
		const ProjectB r = project_point_b(c, p, g0, g1, a.depths_b ? a.depths_b[at] : 0.0);
		const double x = r.x, y = r.y, xd_b = r.xd_b, yd_b = r.yd_b, cx_b = r.camera_b.x, cy_b = r.camera_b.y, cz_b = r.camera_b.z;
		double xd = x, yd = y;
		if (c.distort)
		{ // the forward's distorted point (project_point) and the adjoints of the five coefficients
			const double p1 = c.d[2], p2 = c.d[3], r2 = r.r2, r4 = r.r4, radial_b = r.radial_b;
			const double x2 = x * x, y2 = y * y;
			xd = x * r.radial + (2 * p1 * x * y + p2 * (r2 + 2 * x2)), yd = y * r.radial + (p1 * (r2 + 2 * y2) + 2 * p2 * x * y);
			s[18] += radial_b * r2;
			s[19] += radial_b * r4;
			s[20] += 2 * x * y * xd_b + (r2 + 2 * y2) * yd_b;
			s[21] += (r2 + 2 * x2) * xd_b + 2 * x * y * yd_b;
			s[22] += radial_b * (r2 * r4);
		}
		if (a.points_b)
			store3(a.points_b + at * 3, r.point_b);
		s[0] += cx_b * px, s[1] += cx_b * py, s[2] += cx_b * pz, s[3] += cx_b;
		s[4] += cy_b * px, s[5] += cy_b * py, s[6] += cy_b * pz, s[7] += cy_b;
		s[8] += cz_b * px, s[9] += cz_b * py, s[10] += cz_b * pz, s[11] += cz_b;
		s[12] += g0 * xd, s[13] += g0 * yd, s[14] += g0;
		s[15] += g1 * xd, s[16] += g1 * yd, s[17] += g1;
	}
	// two sums of fewer values, each with its own partial range and counter word: one grid_sum<23> holds three arrays of 23 doubles at its peak
	// (186 VGPRs, two waves per SIMD)
	const unsigned B = gridDim.x;
	double *partials = a.partials + (size_t)b * B * CAMERA_SUMS;
	const int k = threadIdx.x;
	{
		double part[CAMERA_SUMS_E], total[CAMERA_SUMS_E];
#pragma unroll
		for (int i = 0; i < CAMERA_SUMS_E; i++)
			part[i] = s[i];
		if (grid_sum<CAMERA_SUMS_E>(part, partials, a.counters + 2 * b, total, blockIdx.x, B))
		{ // the last workgroup of the view: thread k < 12 has value k
			const double mine = total_of_thread(total, k);
			if (k < CAMERA_SUMS_E)
				store_or_add(a.extrinsic_b + 12 * b + k, mine, a.accumulate);
		}
	}
	{
		constexpr int REST = CAMERA_SUMS - CAMERA_SUMS_E;
		double part[REST], total[REST];
#pragma unroll
		for (int i = 0; i < REST; i++)
			part[i] = s[CAMERA_SUMS_E + i];
		if (grid_sum<REST>(part, partials + (size_t)B * CAMERA_SUMS_E, a.counters + 2 * b + 1, total, blockIdx.x, B))
		{ // threads 0 .. 5: the two rows of intrinsic_b, 6 .. 10: distortion_b, 11 .. 13: the zero row of intrinsic_b
			const double mine = total_of_thread(total, k);
			double *out = k < 6 ? a.intrinsic_b + 9 * b + k : (k < REST && a.distortion_b) ? a.distortion_b + 5 * b + (k - 6) : nullptr;
			if (out)
				store_or_add(out, mine, a.accumulate);
			if (k >= REST && k < REST + 3 && !a.accumulate)
				a.intrinsic_b[9 * b + 6 + (k - REST)] = 0;
		}
	}
}

struct CameraAssembleArgs
{
	const double *quaternions, *translations, *focal, *center, *distortion_in;
	double *extrinsic, *intrinsic, *distortion_out;
	int shared, n;
};

// one thread per view (n <= FIT_MAX_VIEWS = one wavefront)
__global__ __launch_bounds__(FIT_MAX_VIEWS) void camera_assemble_kernel(CameraAssembleArgs a)
{
	const int b = threadIdx.x;
	if (b >= a.n)
		return;
	const double *q = a.quaternions + 4 * b;
	const double inv = 1 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]); // (MULTIPLIED by: load_unit_quaternion, dr_fititer.h, divides --
	const double x = q[0] * inv, y = q[1] * inv, z = q[2] * inv, w = q[3] * inv;		// other bits, so not one function)
	double *E = a.extrinsic + 12 * b, *K = a.intrinsic + 9 * b;
	// R = I + 2 w [u]x + 2 [u]x^2, u = (x, y, z): qrot(q, p) = p + 2 (w u x p + u x (u x p)) as a matrix
	E[0] = 1 - 2 * (y * y + z * z), E[1] = 2 * (x * y - w * z), E[2] = 2 * (x * z + w * y), E[3] = a.translations[3 * b];
	E[4] = 2 * (x * y + w * z), E[5] = 1 - 2 * (x * x + z * z), E[6] = 2 * (y * z - w * x), E[7] = a.translations[3 * b + 1];
	E[8] = 2 * (x * z - w * y), E[9] = 2 * (y * z + w * x), E[10] = 1 - 2 * (x * x + y * y), E[11] = a.translations[3 * b + 2];
	const int at = a.shared ? 0 : b;
	K[0] = a.focal[2 * at], K[1] = 0, K[2] = a.center[2 * at];
	K[3] = 0, K[4] = a.focal[2 * at + 1], K[5] = a.center[2 * at + 1];
	K[6] = 0, K[7] = 0, K[8] = 1;
	if (a.distortion_out)
		for (int i = 0; i < 5; i++)
			a.distortion_out[5 * b + i] = a.distortion_in[5 * at + i];
}

struct CameraAssembleBArgs
{
	const double *quaternions, *extrinsic_b, *intrinsic_b, *distortion_b;
	double *quaternions_b, *translations_b, *focal_b, *center_b, *distortion_in_b;
	int shared, n;
};

__global__ __launch_bounds__(FIT_MAX_VIEWS) void camera_assemble_b_kernel(CameraAssembleBArgs a)
{
	const int b = threadIdx.x;
	if (b >= a.n)
		return;
	const double *q = a.quaternions + 4 * b, *R = a.extrinsic_b + 12 * b; // R[4 r + c]: the adjoint of row r, column c of [R | t]
	const double inv = 1 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
	const double x = q[0] * inv, y = q[1] * inv, z = q[2] * inv, w = q[3] * inv;
	const double s01 = R[1] + R[4], s02 = R[2] + R[8], s12 = R[6] + R[9]; // symmetric parts: from 2 u u^T
	const double a01 = R[4] - R[1], a20 = R[2] - R[8], a12 = R[9] - R[6]; // antisymmetric parts: from 2 w [u]x
	const double xn_b = -4 * x * (R[5] + R[10]) + 2 * y * s01 + 2 * z * s02 + 2 * w * a12;
	const double yn_b = -4 * y * (R[0] + R[10]) + 2 * x * s01 + 2 * z * s12 + 2 * w * a20;
	const double zn_b = -4 * z * (R[0] + R[5]) + 2 * x * s02 + 2 * y * s12 + 2 * w * a01;
	const double wn_b = 2 * (x * a12 + y * a20 + z * a01);
	// through q / |q|: q_b = (qn_b - qn (qn . qn_b)) / |q|, as a product with `inv` like the forward (fit_pose_project_b_kernel divides: other bits)
	const double along = x * xn_b + y * yn_b + z * zn_b + w * wn_b;
	double *qb = a.quaternions_b + 4 * b;
	qb[0] = (xn_b - x * along) * inv, qb[1] = (yn_b - y * along) * inv, qb[2] = (zn_b - z * along) * inv, qb[3] = (wn_b - w * along) * inv;
	a.translations_b[3 * b] = R[3], a.translations_b[3 * b + 1] = R[7], a.translations_b[3 * b + 2] = R[11];
	if (!a.shared)
	{
		const double *K = a.intrinsic_b + 9 * b;
		a.focal_b[2 * b] = K[0], a.focal_b[2 * b + 1] = K[4];
		a.center_b[2 * b] = K[2], a.center_b[2 * b + 1] = K[5];
		if (a.distortion_in_b)
			for (int i = 0; i < 5; i++)
				a.distortion_in_b[5 * b + i] = a.distortion_b[5 * b + i];
	}
	else if (b == 0)
	{ // one physical camera: its adjoints are the sums over the views, in view order, by this thread
		double f0 = 0, f1 = 0, c0 = 0, c1 = 0, d[5] = {0, 0, 0, 0, 0};
		for (int v = 0; v < a.n; v++)
		{
			const double *K = a.intrinsic_b + 9 * v;
			f0 += K[0], f1 += K[4], c0 += K[2], c1 += K[5];
			if (a.distortion_in_b)
				for (int i = 0; i < 5; i++)
					d[i] += a.distortion_b[5 * v + i];
		}
		a.focal_b[0] = f0, a.focal_b[1] = f1, a.center_b[0] = c0, a.center_b[1] = c1;
		if (a.distortion_in_b)
			for (int i = 0; i < 5; i++)
				a.distortion_in_b[i] = d[i];
	}
}

} // namespace
