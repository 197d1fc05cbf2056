// The as-rigid-as-possible energy, its gradient and the per-vertex rotations (include/deodr_hip_arap.h has the operation and the contract).
//
// arap_rotations_kernel   a thread per (pose, vertex): walks the row once for S_i = sum_j w_ij e^p_ij (e^q_ij)^T, Horn's 4 x 4 matrix, ARAP_SWEEPS
//                         sweeps of cyclic Jacobi in registers (the ten entries of the upper triangle and sixteen of the eigenvectors, every index
//                         a compile-time constant), the quaternion of the largest eigenvalue -> scratch (and `rotations`), then the row a second
//                         time for the cell's energy sum_j w_ij |e^p_ij - R_i e^q_ij|^2 -> scratch.  (NOT sum w |e^p|^2 + sum w |e^q|^2
//                         - 2 tr(R^T S): that cancels near rest.)  Thread 0 of workgroup 0 of a pose clears the pose's arrival ticket.
// arap_gradient_kernel    a thread per (pose, vertex): R_i from the own quaternion, R_j from the neighbour's (32 bytes gathered per neighbour),
//                         g_i = c sum_j w_ij ((e^p_ij - R_i e^q_ij) + (e^p_ij - R_j e^q_ij)); the cell energies through grid_sum, per pose.
//
// grid of both: (arap_blocks(V), n); the threads of a pose stride over its vertices.  No atomics on values.  The order of every sum: a row's
// entries in order; the cells of a thread in order, then grid_sum (lanes, wavefronts, workgroups).  A pivot that is exactly 0 is skipped by a
// select, so vertices bit-equal to vertices_ref give R = identity and zeros exactly (S is then symmetric bit for bit: w * (e_a * e_b)).
// The scratch after its 64 bytes of counter words (unused here): quaternions [n, V, 4], cell energies [n, V], partials [n][ARAP_MAX_BLOCKS],
// tickets [n] (unsigned).
#pragma once

namespace
{

constexpr int ARAP_SWEEPS = DEODR_HIP_ARAP_SWEEPS, ARAP_BLOCK = DEODR_HIP_ARAP_BLOCK, ARAP_MAX_BLOCKS = DEODR_HIP_ARAP_MAX_BLOCKS;
constexpr int ARAP_MAX_POSES = 65535; // (the poses are the grid's second dimension)
static_assert(ARAP_BLOCK == FH_BLOCK, "grid_sum adds the partials of a workgroup of FH_BLOCK threads");

// the one rule both the launches and deodr_hip_arap_blocks() follow
inline unsigned arap_blocks(int V) { return dr::host::capped_blocks((size_t)V, ARAP_BLOCK, ARAP_MAX_BLOCKS); }
inline size_t arap_scratch_doubles(int V, int n) { return 5 * ((size_t)n * (size_t)V) + (size_t)ARAP_MAX_BLOCKS * (size_t)n + ((size_t)n + 1) / 2; }

struct ArapArgs
{
	const uint32_t *offsets, *cols;
	const double *weights, *q, *p;
	double *energy, *gradient, *rotations;
	double *quats, *cell, *partials; // the scratch
	unsigned *tickets;
	double cregu;
	int V, n;
};

// the upper triangle of a symmetric 4 x 4 matrix: entry (r, c) in either order
__device__ __forceinline__ double &arap_sym(double (&A)[4][4], int r, int c) { return r < c ? A[r][c] : A[c][r]; }

// one Jacobi rotation of the pivot (P, Q), P < Q: A <- J^T A J, E <- E J
template <int P, int Q>
__device__ __forceinline__ void arap_rotate(double (&A)[4][4], double (&E)[4][4])
{
	const double apq = A[P][Q];
	const bool skip = apq == 0;
	const double theta = (A[Q][Q] - A[P][P]) / (2 * (skip ? 1.0 : apq));
	const bool big = !(fabs(theta) <= 1e150); // (theta^2 would overflow; an infinite theta gives t = 0)
	const double th = big ? 1.0 : theta;
	double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1));
	t = big ? 1 / (2 * theta) : t;
	t = skip ? 0.0 : t;
	const double c = 1 / sqrt(t * t + 1), s = t * c;
	A[P][P] = A[P][P] - t * apq;
	A[Q][Q] = A[Q][Q] + t * apq;
	A[P][Q] = 0;
#pragma unroll
	for (int r = 0; r < 4; r++)
	{
		if (r != P && r != Q)
		{
			const double arp = arap_sym(A, r, P), arq = arap_sym(A, r, Q);
			arap_sym(A, r, P) = c * arp - s * arq;
			arap_sym(A, r, Q) = s * arp + c * arq;
		}
		const double erp = E[r][P], erq = E[r][Q];
		E[r][P] = c * erp - s * erq;
		E[r][Q] = s * erp + c * erq;
	}
}

struct ArapQuat
{
	double x, y, z, w;
};
struct ArapRot
{
	double m[3][3];
};

// S (row-major 3 x 3) -> the unit quaternion (w >= 0) of the rotation that maximises tr(R^T S)
__device__ __forceinline__ ArapQuat arap_top_quaternion(const double (&S)[3][3])
{
	double A[4][4], E[4][4]; // (of A the upper triangle only)
	A[0][0] = (S[0][0] + S[1][1]) + S[2][2];
	A[0][1] = S[2][1] - S[1][2];
	A[0][2] = S[0][2] - S[2][0];
	A[0][3] = S[1][0] - S[0][1];
	A[1][1] = (S[0][0] - S[1][1]) - S[2][2];
	A[1][2] = S[0][1] + S[1][0];
	A[1][3] = S[2][0] + S[0][2];
	A[2][2] = (S[1][1] - S[0][0]) - S[2][2];
	A[2][3] = S[1][2] + S[2][1];
	A[3][3] = (S[2][2] - S[0][0]) - S[1][1];
#pragma unroll
	for (int r = 0; r < 4; r++)
#pragma unroll
		for (int c = 0; c < 4; c++)
			E[r][c] = r == c ? 1.0 : 0.0;
#pragma unroll 1
	for (int sweep = 0; sweep < ARAP_SWEEPS; sweep++)
	{
		arap_rotate<0, 1>(A, E);
		arap_rotate<0, 2>(A, E);
		arap_rotate<0, 3>(A, E);
		arap_rotate<1, 2>(A, E);
		arap_rotate<1, 3>(A, E);
		arap_rotate<2, 3>(A, E);
	}
	double best = A[0][0], w = E[0][0], x = E[1][0], y = E[2][0], z = E[3][0];
#pragma unroll
	for (int k = 1; k < 4; k++)
	{
		const bool better = A[k][k] > best;
		best = better ? A[k][k] : best;
		w = better ? E[0][k] : w, x = better ? E[1][k] : x, y = better ? E[2][k] : y, z = better ? E[3][k] : z;
	}
	const bool flip = w < 0;
	return {flip ? -x : x, flip ? -y : y, flip ? -z : z, flip ? -w : w};
}

__device__ __forceinline__ ArapRot arap_matrix(const ArapQuat &u)
{
	const double x = u.x, y = u.y, z = u.z, w = u.w;
	return {{{1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)},
			 {2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)},
			 {2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)}}};
}
// e - R f
__device__ __forceinline__ Vec3 arap_residual(const Vec3 &e, const ArapRot &R, const Vec3 &f)
{
	return {e.x - ((R.m[0][0] * f.x + R.m[0][1] * f.y) + R.m[0][2] * f.z), e.y - ((R.m[1][0] * f.x + R.m[1][1] * f.y) + R.m[1][2] * f.z),
			e.z - ((R.m[2][0] * f.x + R.m[2][1] * f.y) + R.m[2][2] * f.z)};
}
__device__ __forceinline__ Vec3 arap_point(const double *v, size_t i) { return {v[3 * i], v[3 * i + 1], v[3 * i + 2]}; }
__device__ __forceinline__ Vec3 arap_minus(const Vec3 &a, const Vec3 &b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }

// grid: (arap_blocks(V), n)
__global__ __launch_bounds__(ARAP_BLOCK) void arap_rotations_kernel(ArapArgs a)
{
	const size_t pose = blockIdx.y, V = (size_t)a.V;
	if (blockIdx.x == 0 && threadIdx.x == 0)
		a.tickets[pose] = 0; // (what arap_gradient_kernel draws on: the launch boundary orders the two)
	const double *const p = a.p + pose * V * 3;
	for (size_t i = (size_t)blockIdx.x * ARAP_BLOCK + threadIdx.x; i < V; i += (size_t)gridDim.x * ARAP_BLOCK)
	{
		const uint32_t begin = a.offsets[i], end = a.offsets[i + 1];
		const Vec3 pi = arap_point(p, i), qi = arap_point(a.q, i);
		double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
		for (uint32_t k = begin; k < end; k++)
		{
			const size_t j = a.cols[k];
			const double w = a.weights[k];
			const Vec3 ep = arap_minus(pi, arap_point(p, j)), eq = arap_minus(qi, arap_point(a.q, j));
			S[0][0] += w * (ep.x * eq.x), S[0][1] += w * (ep.x * eq.y), S[0][2] += w * (ep.x * eq.z);
			S[1][0] += w * (ep.y * eq.x), S[1][1] += w * (ep.y * eq.y), S[1][2] += w * (ep.y * eq.z);
			S[2][0] += w * (ep.z * eq.x), S[2][1] += w * (ep.z * eq.y), S[2][2] += w * (ep.z * eq.z);
		}
		const ArapQuat u = arap_top_quaternion(S);
		const size_t at = pose * V + i;
		a.quats[4 * at] = u.x, a.quats[4 * at + 1] = u.y, a.quats[4 * at + 2] = u.z, a.quats[4 * at + 3] = u.w;
		if (a.rotations)
			a.rotations[4 * at] = u.x, a.rotations[4 * at + 1] = u.y, a.rotations[4 * at + 2] = u.z, a.rotations[4 * at + 3] = u.w;
		const ArapRot R = arap_matrix(u);
		double cell = 0;
		for (uint32_t k = begin; k < end; k++)
		{
			const size_t j = a.cols[k];
			const Vec3 d = arap_residual(arap_minus(pi, arap_point(p, j)), R, arap_minus(qi, arap_point(a.q, j)));
			cell += a.weights[k] * ((d.x * d.x + d.y * d.y) + d.z * d.z);
		}
		a.cell[at] = cell;
	}
}

// grid: (arap_blocks(V), n)
__global__ __launch_bounds__(ARAP_BLOCK) void arap_gradient_kernel(ArapArgs a)
{
	const size_t pose = blockIdx.y, V = (size_t)a.V;
	const double *const p = a.p + pose * V * 3, *const quats = a.quats + pose * V * 4;
	double s[1] = {0};
	for (size_t i = (size_t)blockIdx.x * ARAP_BLOCK + threadIdx.x; i < V; i += (size_t)gridDim.x * ARAP_BLOCK)
	{
		const uint32_t begin = a.offsets[i], end = a.offsets[i + 1];
		const Vec3 pi = arap_point(p, i), qi = arap_point(a.q, i);
		const ArapRot Ri = arap_matrix({quats[4 * i], quats[4 * i + 1], quats[4 * i + 2], quats[4 * i + 3]});
		Vec3 g = {0, 0, 0};
		for (uint32_t k = begin; k < end; k++)
		{
			const size_t j = a.cols[k];
			const double w = a.weights[k];
			const ArapRot Rj = arap_matrix({quats[4 * j], quats[4 * j + 1], quats[4 * j + 2], quats[4 * j + 3]});
			const Vec3 ep = arap_minus(pi, arap_point(p, j)), eq = arap_minus(qi, arap_point(a.q, j));
			const Vec3 d = arap_residual(ep, Ri, eq), dj = arap_residual(ep, Rj, eq);
			g.x += w * (d.x + dj.x), g.y += w * (d.y + dj.y), g.z += w * (d.z + dj.z);
		}
		double *const out = a.gradient + (pose * V + i) * 3;
		out[0] = a.cregu * g.x, out[1] = a.cregu * g.y, out[2] = a.cregu * g.z;
		s[0] += a.cell[pose * V + i];
	}
	double total[1];
	if (grid_sum<1>(s, a.partials + pose * ARAP_MAX_BLOCKS, a.tickets + pose, total, blockIdx.x, gridDim.x) && threadIdx.x == 0)
		a.energy[pose] = (a.cregu / 2) * total[0];
}

} // namespace
