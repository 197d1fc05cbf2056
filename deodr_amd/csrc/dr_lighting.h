// Spherical-harmonic lighting (bands 0 - 2) and per-vertex albedo (include/deodr_hip_lighting.h), beside vertex_shade_* of dr_fititer.h: the same
// vertex normal (accumulated_normal: sign * the sum of the unit normals of the faces around a vertex, GATHER_LANES lanes per vertex), normalised by unit() of dr_fronthalf.h;
//
//     E[b,v,c] = sum_k sh[k, min(c, S-1)] Y_k(N[b,v])          (not clamped)          colors[b,v,c] = albedo[v or 0, c] E[b,v,c]
//
// sh_shade_kernel      grid (V GATHER_LANES / FH_BLOCK, n) as vertex_shade_kernel -> luminosity [n,V] (S = 1) and / or colors [n,V,C]
// sh_shade_b1_kernel   sh_blocks(V, n) workgroups striding over the (view, vertex) pairs, GATHER_LANES lanes per pair: recomputes N and E, writes
//                      acc_b [n,V,3] (the adjoint of the accumulated normal, through grad Y_k and the normalisation: what vertex_shade_b2_kernel
//                      consumes), brings 9 S + 3 sums -- sh_b [9,S] and the adjoint of a single albedo [C] -- to up to three grid_sums of 12, 9, 9
//                      values, each on its own partial range and counter word; per-vertex albedo: writes the products colors_b E [n,V,C]
// sh_albedo_sum_kernel albedo_b[v,c] = the sum of those products over the views, in view order, one thread per element
// A vertex without faces or with a zero accumulated normal divides by zero exactly as vertex_shade_kernel does.
#pragma once

namespace
{

constexpr int SH_MAX_VERTICES = 1 << 24;
constexpr int SH_COEFFS = 9;
constexpr int SH_MAX_BLOCKS = 1024;		   // of sh_shade_b1_kernel: four per CU; the last one adds that many partials up in four trips of its threads
constexpr int SH_SUMS_FIRST = SH_COEFFS + 3; // first grid_sum: column 0 of sh_b, then the (at most 3) sums of a single albedo
constexpr int SH_SUMS = SH_SUMS_FIRST + 2 * SH_COEFFS; // doubles of partials per workgroup
constexpr int SH_PAIRS_PER_BLOCK = FH_BLOCK / GATHER_LANES;

// the one rule the launch of sh_shade_b1_kernel, the scratch layout and deodr_hip_sh_blocks() follow.  Non-decreasing in V and in n.
inline int sh_blocks(int V, int n)
{
	const long long want = ((long long)V * n + SH_PAIRS_PER_BLOCK - 1) / SH_PAIRS_PER_BLOCK;
	return want < SH_MAX_BLOCKS ? (int)want : SH_MAX_BLOCKS;
}

// c0 .. c4 of the real SH basis, as expressions of pi
#define DR_SH_PI 3.14159265358979323846264338327950288
#define DR_SH_C0 (1.0 / (2.0 * sqrt(DR_SH_PI)))
#define DR_SH_C1 (sqrt(3.0) / (2.0 * sqrt(DR_SH_PI)))
#define DR_SH_C2 (sqrt(15.0) / (2.0 * sqrt(DR_SH_PI)))
#define DR_SH_C3 (sqrt(5.0) / (4.0 * sqrt(DR_SH_PI)))
#define DR_SH_C4 (sqrt(15.0) / (4.0 * sqrt(DR_SH_PI)))

struct SHArgs
{
	ShadeArgs mesh;		  // posed, faces, vf_offsets, vf_corners, V, n, sign; C = channels of albedo / colors (0: none); light, ambient, color unused
	const double *sh;	  // [9,S]
	const double *albedo; // [C] or [V,C], or NULL
	int S, per_vertex;
};

__device__ __forceinline__ void sh_basis(const Vec3 &N, double (&Y)[SH_COEFFS])
{
	const double c0 = DR_SH_C0, c1 = DR_SH_C1, c2 = DR_SH_C2, c3 = DR_SH_C3, c4 = DR_SH_C4;
	Y[0] = c0, Y[1] = c1 * N.y, Y[2] = c1 * N.z, Y[3] = c1 * N.x;
	Y[4] = c2 * (N.x * N.y), Y[5] = c2 * (N.y * N.z), Y[6] = c3 * (3 * (N.z * N.z) - 1), Y[7] = c2 * (N.x * N.z), Y[8] = c4 * (N.x * N.x - N.y * N.y);
}

// sum_k a[k stride] Y_k, added in the order k = 0 .. 8
__device__ __forceinline__ double sh_dot(const double *a, int stride, const double (&Y)[SH_COEFFS])
{
	double e = a[0] * Y[0];
#pragma unroll
	for (int k = 1; k < SH_COEFFS; k++)
		e += a[k * stride] * Y[k];
	return e;
}

// sum_k a[k stride] grad Y_k(N), x, y, z taken as free variables
__device__ __forceinline__ Vec3 sh_dot_gradient(const double *a, int stride, const Vec3 &N)
{
	const double c1 = DR_SH_C1, c2 = DR_SH_C2, c3 = DR_SH_C3, c4 = DR_SH_C4;
	const double a1 = a[stride], a2 = a[2 * stride], a3 = a[3 * stride], a4 = a[4 * stride], a5 = a[5 * stride], a6 = a[6 * stride], a7 = a[7 * stride],
				 a8 = a[8 * stride];
	return {c1 * a3 + c2 * (a4 * N.y) + c2 * (a7 * N.z) + 2 * c4 * (a8 * N.x), c1 * a1 + c2 * (a4 * N.x) + c2 * (a5 * N.z) - 2 * c4 * (a8 * N.y),
			c1 * a2 + c2 * (a5 * N.y) + 6 * c3 * (a6 * N.z) + c2 * (a7 * N.x)};
}

__global__ __launch_bounds__(FH_BLOCK) void sh_shade_kernel(SHArgs a, double *lum_out, double *colors_out)
{
	const int t = blockIdx.x * FH_BLOCK + threadIdx.x, v = t / GATHER_LANES, sub = t % GATHER_LANES, b = blockIdx.y;
	const int V = a.mesh.V;
	const bool on = v < V;
	const Vec3 acc = accumulated_normal(a.mesh, a.mesh.posed + (size_t)b * V * 3, v, sub, on);
	if (!on || sub != 0)
		return;
	const Vec3 N = unit(acc).N;
	double Y[SH_COEFFS];
	sh_basis(N, Y);
	const size_t at = (size_t)b * V + v;
	const double e0 = sh_dot(a.sh, a.S, Y);
	if (lum_out)
		lum_out[at] = e0;
	if (colors_out)
	{
		const double *alb = a.albedo + (a.per_vertex ? (size_t)v * a.mesh.C : 0);
		for (int c = 0; c < a.mesh.C; c++)
			colors_out[at * a.mesh.C + c] = alb[c] * (a.S > 1 && c > 0 ? sh_dot(a.sh + c, a.S, Y) : e0);
	}
}

struct SHBackArgs
{
	const double *lum_b, *colors_b; // [n,V] or NULL, [n,V,C] or NULL
	double *acc_b;					// [n,V,3]
	double *products;				// [n,V,C] colors_b E, or NULL: no per-vertex albedo adjoint wanted through sh_albedo_sum_kernel
	double *albedo_direct;			// [V,C]: per-vertex albedo adjoint of a single view, written (or added to) here; or NULL
	double *sh_b, *albedo_b;		// [9,S], [C] (single albedo), either may be NULL
	double *partials;				// [blocks, SH_SUMS]
	unsigned *counters;				// three words
	int accumulate;
};

__global__ __launch_bounds__(FH_BLOCK) void sh_shade_b1_kernel(SHArgs a, SHBackArgs o)
{
	const int V = a.mesh.V, C = a.mesh.C, S = a.S;
	const long long pairs = (long long)a.mesh.n * V;
	const int sub = threadIdx.x % GATHER_LANES;
	double s0[SH_SUMS_FIRST], s1[SH_COEFFS], s2[SH_COEFFS];
#pragma unroll
	for (int k = 0; k < SH_SUMS_FIRST; k++)
		s0[k] = 0;
#pragma unroll
	for (int k = 0; k < SH_COEFFS; k++)
		s1[k] = 0, s2[k] = 0;
	// (the same trips for every thread of the workgroup: the lanes of a group meet in accumulated_normal)
	for (long long base = (long long)blockIdx.x * SH_PAIRS_PER_BLOCK; base < pairs; base += (long long)gridDim.x * SH_PAIRS_PER_BLOCK)
	{
		const long long at = base + threadIdx.x / GATHER_LANES;
		const bool on = at < pairs;
		const int b = on ? (int)(at / V) : 0, v = on ? (int)(at % V) : 0;
		const Vec3 acc = accumulated_normal(a.mesh, a.mesh.posed + (size_t)b * V * 3, v, sub, on);
		if (on && sub == 0)
		{ // (no `continue`: every lane is back for the next trip's shuffles)
			const Unit n = unit(acc);
			const Vec3 N = n.N;
			double Y[SH_COEFFS];
			sh_basis(N, Y);
			// E_b[c]: the adjoint of the irradiance of channel c
			double E_b[3] = {0, 0, 0};
			if (o.colors_b)
			{
				const double *alb = a.albedo + (a.per_vertex ? (size_t)v * C : 0);
				const double e0 = sh_dot(a.sh, S, Y);
#pragma unroll
				for (int c = 0; c < 3; c++)
					if (c < C)
					{
						const double g = o.colors_b[at * C + c];
						const double p = g * (S > 1 && c > 0 ? sh_dot(a.sh + c, S, Y) : e0);
						E_b[c] = g * alb[c];
						if (!a.per_vertex)
							s0[SH_COEFFS + c] += p;
						else if (o.products)
							o.products[at * C + c] = p;
						else if (o.albedo_direct)
							store_or_add(o.albedo_direct + at * C + c, p, o.accumulate); // (one view: at = v)
					}
			}
			Vec3 N_b;
			if (S == 1)
			{ // one column for all channels
				const double g = ((E_b[0] + E_b[1]) + E_b[2]) + (o.lum_b ? o.lum_b[at] : 0.0);
#pragma unroll
				for (int k = 0; k < SH_COEFFS; k++)
					s0[k] += g * Y[k];
				N_b = scale3(g, sh_dot_gradient(a.sh, 1, N));
			}
			else
			{
#pragma unroll
				for (int k = 0; k < SH_COEFFS; k++)
					s0[k] += E_b[0] * Y[k], s1[k] += E_b[1] * Y[k], s2[k] += E_b[2] * Y[k];
				N_b = scale3(E_b[0], sh_dot_gradient(a.sh, S, N));
				N_b = add3(N_b, scale3(E_b[1], sh_dot_gradient(a.sh + 1, S, N)));
				if (S > 2)
					N_b = add3(N_b, scale3(E_b[2], sh_dot_gradient(a.sh + 2, S, N)));
			}
			store3(o.acc_b + 3 * at, unit_b(N, n.len, N_b));
		}
	}
	// up to three sums of at most 12 values, each with its own partial range and counter word (one grid_sum of 30 values holds three arrays of 30
	// doubles at its peak).  Thread k of the last workgroup to arrive has value k (total_of_thread).
	const unsigned B = gridDim.x;
	const int k = threadIdx.x;
	{
		double total[SH_SUMS_FIRST];
		if (grid_sum<SH_SUMS_FIRST>(s0, o.partials, o.counters, total))
		{
			double *out = k < SH_COEFFS ? (o.sh_b ? o.sh_b + (size_t)k * S : nullptr) : (k < SH_COEFFS + C && o.albedo_b) ? o.albedo_b + (k - SH_COEFFS) : nullptr;
			if (out)
				store_or_add(out, total_of_thread(total, k), o.accumulate);
		}
	}
	if (S > 1)
	{
		double total[SH_COEFFS];
		if (grid_sum<SH_COEFFS>(s1, o.partials + (size_t)B * SH_SUMS_FIRST, o.counters + 1, total))
			if (k < SH_COEFFS && o.sh_b)
				store_or_add(o.sh_b + (size_t)k * S + 1, total_of_thread(total, k), o.accumulate);
	}
	if (S > 2)
	{
		__syncthreads(); // (the same grid_sum<9> as above, the same LDS: its last workgroup may still be reading its totals)
		double total[SH_COEFFS];
		if (grid_sum<SH_COEFFS>(s2, o.partials + (size_t)B * (SH_SUMS_FIRST + SH_COEFFS), o.counters + 2, total))
			if (k < SH_COEFFS && o.sh_b)
				store_or_add(o.sh_b + (size_t)k * S + 2, total_of_thread(total, k), o.accumulate);
	}
}

// albedo_b[i] (+)= sum over the views b = 0 .. n-1, in this order, of products[b][i]; i over the V C elements, each written once by one thread
__global__ __launch_bounds__(FH_BLOCK) void sh_albedo_sum_kernel(const double *products, double *albedo_b, size_t count, int n, int accumulate)
{
	const size_t i = (size_t)blockIdx.x * FH_BLOCK + threadIdx.x;
	if (i >= count)
		return;
	double s = products[i];
	for (int b = 1; b < n; b++)
		s += products[(size_t)b * count + i];
	store_or_add(albedo_b + i, s, accumulate);
}

} // namespace
