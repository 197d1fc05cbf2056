// Linear blend skinning (include/deodr_hip_skinning.h): a skeleton of J joints, one quaternion per (pose, joint), at most SKIN_MAX_INFLUENCES weighted
// joints per vertex.  The world transform of a joint is carried as a composed unit quaternion Q and a translation t (world [n,J,7] = Q x y z w, t),
// so that every rotation here is qrot_point / qrot_point_b of dr_fronthalf.h:
//
//     root:  Q_j = q_j / |q_j|            t_j = joints_j                          (j = 0, or parents[j] >= j)
//     else:  Q_j = Q_p (q_j / |q_j|)      t_j = t_p + R(Q_p)(joints_j - joints_p)   (p = parents[j] < j)
//     posed[b,i] = sum_k weights[i,k] (R(Q_j)(vertices[i] - joints_j) + t_j),   j = indices[i,k]   (an index >= J: weight 0)
//
// skin_chain_kernel    one workgroup, thread b walks j = 0 .. J-1 of pose b -> world
// skin_apply_kernel    grid (V GATHER_LANES / FH_BLOCK, n): GATHER_LANES adjacent lanes per vertex, one influence each, a butterfly at the end -> posed
// skin_apply_b_kernel  grid (V GATHER_LANES / FH_BLOCK): the same lanes, each adds its influence's R^T w posed_b over the poses in order -> vertices_b
// skin_joint_b_kernel  grid (J, n): the workgroup of (joint, pose) strides the static list of the joint's (vertex, influence) slots in a fixed order,
//                      ten sums (adjoints of Q, of t, of the `- joints_j` term) threads -> lanes -> wavefronts in order -> chain_b [n,J,10]
// skin_chain_b_kernel  one workgroup: thread b walks j = J-1 .. 0 of pose b, passing the adjoints in chain_b from every joint to its parent
//                      -> quaternions_b; then joints_b[j] = the sum over the poses, in pose order, one thread per element
// No atomics, no counter words, nothing waits on another workgroup: the order of every sum is fixed by the tables and (V, J, K, n) alone.
#pragma once

namespace
{

constexpr int SKIN_MAX_VERTICES = 1 << 24;
constexpr int SKIN_MAX_JOINTS = 256;
constexpr int SKIN_MAX_INFLUENCES = GATHER_LANES;
constexpr int SKIN_WORLD = 7;	 // doubles per (pose, joint) of world: Q (x, y, z, w), t
constexpr int SKIN_CHAIN_B = 10; // doubles per (pose, joint) of the scratch: adjoints of Q (4), of t (3), of joints_j as it enters posed (3)

struct Quat
{
	Vec3 u;
	double w;
};
__device__ __forceinline__ Quat load_quat(const double *p) { return {load3(p), p[3]}; }
__device__ __forceinline__ void store_quat(double *p, const Quat &q) { store3(p, q.u), p[3] = q.w; }
__device__ __forceinline__ Quat conjugate(const Quat &q) { return {{-q.u.x, -q.u.y, -q.u.z}, q.w}; }
// the Hamilton product: R(a b) = R(a) R(b).  Linear in a and in b; as real 4-vectors the adjoints of r = a b are a_b = r_b conj(b), b_b = conj(a) r_b
__device__ __forceinline__ Quat qmul(const Quat &a, const Quat &b)
{
	const Vec3 c = cross3(a.u, b.u);
	return {{a.w * b.u.x + b.w * a.u.x + c.x, a.w * b.u.y + b.w * a.u.y + c.y, a.w * b.u.z + b.w * a.u.z + c.z}, a.w * b.w - dot3(a.u, b.u)};
}
// q / |q| with the length it was divided by (unit() of dr_fronthalf.h for four components), and the adjoint through it
__device__ __forceinline__ Quat unit_quat(const Quat &q, double &len)
{
	len = sqrt(dot3(q.u, q.u) + q.w * q.w);
	return {{q.u.x / len, q.u.y / len, q.u.z / len}, q.w / len};
}
__device__ __forceinline__ Quat unit_quat_b(const Quat &N, double len, const Quat &N_b)
{
	const double along = dot3(N.u, N_b.u) + N.w * N_b.w;
	return {{(N_b.u.x - N.u.x * along) / len, (N_b.u.y - N.u.y * along) / len, (N_b.u.z - N.u.z * along) / len}, (N_b.w - N.w * along) / len};
}

struct SkinArgs
{
	const double *vertices, *joints, *quaternions; // [V,3], [J,3], [n,J,4] (raw)
	const uint32_t *parents, *indices;			   // [J], [V,K]
	const double *weights;						   // [V,K]
	int V, J, K, n;
};
// a joint without a parent: joint 0, and any joint whose table entry does not point below it (0xffffffff among them)
__device__ __forceinline__ bool skin_is_root(const SkinArgs &a, int j, uint32_t &parent)
{
	parent = a.parents[j];
	return j == 0 || parent >= (uint32_t)j;
}

__global__ __launch_bounds__(FIT_MAX_VIEWS) void skin_chain_kernel(SkinArgs a, double *world)
{
	const int b = threadIdx.x;
	if (b >= a.n)
		return;
	double *W = world + (size_t)b * a.J * SKIN_WORLD;
	for (int j = 0; j < a.J; j++)
	{
		double len;
		const Quat q = unit_quat(load_quat(a.quaternions + ((size_t)b * a.J + j) * 4), len);
		uint32_t p;
		if (skin_is_root(a, j, p))
		{
			store_quat(W + j * SKIN_WORLD, q);
			store3(W + j * SKIN_WORLD + 4, load3(a.joints + 3 * j));
			continue;
		}
		const Quat P = load_quat(W + p * SKIN_WORLD); // (this thread's own store of an earlier trip)
		store_quat(W + j * SKIN_WORLD, qmul(P, q));
		const Vec3 d = sub3(load3(a.joints + 3 * j), load3(a.joints + 3 * p));
		store3(W + j * SKIN_WORLD + 4, add3(load3(W + p * SKIN_WORLD + 4), qrot_point(P.u, P.w, d)));
	}
}

// the influence of lane `sub` of vertex i: its joint (J: none -- beyond K, beyond V, or an index out of range) and its weight
__device__ __forceinline__ int skin_influence(const SkinArgs &a, int i, int sub, double &weight)
{
	weight = 0;
	if (i >= a.V || sub >= a.K)
		return a.J;
	const uint32_t j = a.indices[(size_t)i * a.K + sub];
	if (j >= (uint32_t)a.J)
		return a.J;
	weight = a.weights[(size_t)i * a.K + sub];
	return (int)j;
}

__global__ __launch_bounds__(FH_BLOCK) void skin_apply_kernel(SkinArgs a, const double *world, double *posed)
{
	const int t = blockIdx.x * FH_BLOCK + threadIdx.x, i = t / GATHER_LANES, sub = t % GATHER_LANES, b = blockIdx.y;
	double w;
	const int j = skin_influence(a, i, sub, w);
	Vec3 term = {0, 0, 0};
	if (j < a.J)
	{
		const double *W = world + ((size_t)b * a.J + j) * SKIN_WORLD;
		const Vec3 local = sub3(load3(a.vertices + 3 * (size_t)i), load3(a.joints + 3 * j));
		term = scale3(w, add3(qrot_point(load3(W), W[3], local), load3(W + 4)));
	}
	const Vec3 sum = lane_group_sum3<1, GATHER_LANES>(term); // (every lane of the wavefront is here)
	if (i < a.V && sub == 0)
		store3(posed + ((size_t)b * a.V + i) * 3, sum);
}

// vertices_b[i] = sum_b sum_k w R(Q_j)^T posed_b[b,i]: each lane adds its influence over the poses in order, then the butterfly of the forward
__global__ __launch_bounds__(FH_BLOCK) void skin_apply_b_kernel(SkinArgs a, const double *world, const double *posed_b, double *vertices_b)
{
	const int t = blockIdx.x * FH_BLOCK + threadIdx.x, i = t / GATHER_LANES, sub = t % GATHER_LANES;
	double w;
	const int j = skin_influence(a, i, sub, w);
	Vec3 acc = {0, 0, 0};
	if (j < a.J)
		for (int b = 0; b < a.n; b++)
		{
			const double *W = world + ((size_t)b * a.J + j) * SKIN_WORLD;
			const Vec3 g = scale3(w, load3(posed_b + ((size_t)b * a.V + i) * 3));
			acc = add3(acc, qrot_point(scale3(-1, load3(W)), W[3], g)); // the conjugate rotates back
		}
	const Vec3 sum = lane_group_sum3<1, GATHER_LANES>(acc);
	if (i < a.V && sub == 0)
		store3(vertices_b + 3 * (size_t)i, sum);
}

// chain_b[b,j] = the adjoints of world[b,j] and of joints_j as posed reads them: sums over the slots s = i K + k of the joint's list
// joint_slots[joint_offsets[j] .. joint_offsets[j+1]) (both clamped to nnz; a slot >= V K is skipped), thread t taking entries t, t + FH_BLOCK, ..
__global__ __launch_bounds__(FH_BLOCK) void skin_joint_b_kernel(SkinArgs a, const double *world, const double *posed_b, const uint32_t *joint_offsets,
																 const uint32_t *joint_slots, uint32_t nnz, double *chain_b)
{
	__shared__ double s_wave[FH_BLOCK / 64][SKIN_CHAIN_B];
	const int j = blockIdx.x, b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t last = joint_offsets[j + 1] < nnz ? joint_offsets[j + 1] : nnz;
	const uint32_t first = joint_offsets[j] < last ? joint_offsets[j] : last;
	const double *W = world + ((size_t)b * a.J + j) * SKIN_WORLD;
	const Vec3 u = load3(W), c = load3(a.joints + 3 * j);
	const double qw = W[3];
	const uint32_t slots = (uint32_t)a.V * (uint32_t)a.K;
	double s[SKIN_CHAIN_B];
#pragma unroll
	for (int k = 0; k < SKIN_CHAIN_B; k++)
		s[k] = 0;
	for (uint32_t at = first + threadIdx.x; at < last; at += FH_BLOCK)
	{
		const uint32_t slot = joint_slots[at];
		if (slot >= slots)
			continue;
		const uint32_t i = slot / (uint32_t)a.K;
		const Vec3 g = scale3(a.weights[slot], load3(posed_b + ((size_t)b * a.V + i) * 3));
		const QrotB r = qrot_point_b(u, qw, sub3(load3(a.vertices + 3 * (size_t)i), c), g);
		s[0] += r.u_b.x, s[1] += r.u_b.y, s[2] += r.u_b.z, s[3] += r.w_b;
		s[4] += g.x, s[5] += g.y, s[6] += g.z;
		s[7] -= r.p_b.x, s[8] -= r.p_b.y, s[9] -= r.p_b.z;
	}
#pragma unroll
	for (int k = 0; k < SKIN_CHAIN_B; k++)
	{
		const double sum = wave_sum(s[k]);
		if (lane == 0)
			s_wave[wave][k] = sum;
	}
	__syncthreads();
	if (threadIdx.x < SKIN_CHAIN_B)
	{
		double sum = 0;
		for (int w = 0; w < FH_BLOCK / 64; w++)
			sum += s_wave[w][threadIdx.x];
		chain_b[((size_t)b * a.J + j) * SKIN_CHAIN_B + threadIdx.x] = sum;
	}
}

// The reverse walk, in place on chain_b (each thread its own pose).  When joint j is reached every child of it has passed its adjoints on:
//     Q_j = Q_p q:  Q_p_b += Q_j_b conj(q), q_b = conj(Q_p) Q_j_b;     t_j = t_p + R(Q_p) d, d = joints_j - joints_p:  t_p_b += t_j_b, and through
// qrot_point_b to Q_p_b, to joints_j (+) and joints_p (-).  After it chain_b[b,j,7..9] is pose b's share of joints_b[j].
__global__ __launch_bounds__(FH_BLOCK) void skin_chain_b_kernel(SkinArgs a, const double *world, double *chain_b, double *quaternions_b, double *joints_b)
{
	const int b = threadIdx.x;
	if (b < a.n)
	{
		const double *W = world + (size_t)b * a.J * SKIN_WORLD;
		double *A = chain_b + (size_t)b * a.J * SKIN_CHAIN_B;
		for (int j = a.J - 1; j >= 0; j--)
		{
			double *Aj = A + j * SKIN_CHAIN_B;
			const Quat Q_b = load_quat(Aj);
			const Vec3 t_b = load3(Aj + 4);
			double len;
			const Quat q = unit_quat(load_quat(a.quaternions + ((size_t)b * a.J + j) * 4), len);
			Quat q_b = Q_b;
			uint32_t p;
			if (skin_is_root(a, j, p))
				store3(Aj + 7, add3(load3(Aj + 7), t_b)); // t_j = joints_j
			else
			{
				double *Ap = A + p * SKIN_CHAIN_B;
				const Quat P = load_quat(W + p * SKIN_WORLD);
				q_b = qmul(conjugate(P), Q_b);
				const Quat P_b = qmul(Q_b, conjugate(q));
				const QrotB r = qrot_point_b(P.u, P.w, sub3(load3(a.joints + 3 * j), load3(a.joints + 3 * p)), t_b);
				store3(Ap, add3(load3(Ap), add3(P_b.u, r.u_b)));
				Ap[3] = Ap[3] + (P_b.w + r.w_b);
				store3(Ap + 4, add3(load3(Ap + 4), t_b));
				store3(Aj + 7, add3(load3(Aj + 7), r.p_b));
				store3(Ap + 7, sub3(load3(Ap + 7), r.p_b));
			}
			if (quaternions_b)
				store_quat(quaternions_b + ((size_t)b * a.J + j) * 4, unit_quat_b(q, len, q_b));
		}
	}
	if (!joints_b)
		return; // (uniform)
	__syncthreads(); // every pose's walk is stored; one workgroup, so its threads see them
	for (int e = threadIdx.x; e < 3 * a.J; e += FH_BLOCK)
	{
		const int j = e / 3, c = e % 3;
		double sum = chain_b[(size_t)j * SKIN_CHAIN_B + 7 + c];
		for (int v = 1; v < a.n; v++)
			sum += chain_b[((size_t)v * a.J + j) * SKIN_CHAIN_B + 7 + c];
		joints_b[e] = sum;
	}
}

} // namespace
