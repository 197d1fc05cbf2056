// Texture estimation on the device (include/deodr_hip_texture.h): the smoothness term of a texture and the momentum step that moves it.
//
// A texture is [Ht, Wt, C] contiguous in the pixel type PixT; it is walked as ONE flat array of N = Ht * R elements, R = Wt * C the length of a
// row: the x-neighbours of element e are e -+ C (inside the row), the y-neighbours e -+ R.  Both kernels are bandwidth-bound: every thread moves
// 16 bytes per array and round (VEC = 16 / sizeof(PixT) consecutive elements, vector loads and stores), in a grid-stride loop over the N / VEC
// whole pieces; the N % VEC elements behind the last piece are done one by one by the first workgroup.  The vector type is declared with the
// alignment of ONE element: R need not be a multiple of VEC (then the rows above and below a piece start anywhere), and a texture that is a
// slice of a larger buffer need not start on 16 bytes -- global_load_dwordx4 takes any dword-aligned address.  Arithmetic in double, one
// rounding to PixT per stored value.  Every element is owned by one thread: no atomics on values, bit-identical from run to run.
#pragma once

namespace
{

template <class PixT>
struct TexVec
{
	static constexpr int N = 16 / sizeof(PixT);
	typedef PixT aligned_type __attribute__((ext_vector_type(16 / sizeof(PixT))));
	typedef aligned_type type __attribute__((aligned(sizeof(PixT)))); // element-aligned: see above
};

constexpr int TEX_SMOOTH_BLOCKS = 512; // (every workgroup ends with a ticket on one counter word, one after the other: l2_loss_kernel's L2_BLOCKS)
constexpr int TEX_STEP_BLOCKS = 2048;

struct TexSmoothArgs
{
	const void *texture;
	void *gradient;
	double *energy, *partials;
	unsigned *counter;
	double weight;
	int Ht, R, C, N;
};

// One element the slow way (a division per element): the first and the last row of the texture, and the tail behind the last whole piece.
// -> its share of sum (right - centre)^2 + (below - centre)^2; gradient[e] += weight (deg t[e] - sum of the neighbours that exist)
template <class PixT>
__device__ __forceinline__ double tex_smooth_one(const PixT *t, PixT *g, const TexSmoothArgs &a, int e)
{
	const int y = e / a.R, j = e - y * a.R;
	const double c = (double)t[e];
	double deg = 0, sum = 0, energy = 0;
	if (j >= a.C)
		deg += 1, sum += (double)t[e - a.C];
	if (j + a.C < a.R)
	{
		const double r = (double)t[e + a.C];
		deg += 1, sum += r, energy += (r - c) * (r - c);
	}
	if (y > 0)
		deg += 1, sum += (double)t[e - a.R];
	if (y < a.Ht - 1)
	{
		const double d = (double)t[e + a.R];
		deg += 1, sum += d, energy += (d - c) * (d - c);
	}
	g[e] = (PixT)((double)g[e] + a.weight * (deg * c - sum));
	return energy;
}

// E = 0.5 weight sum_c [ sum_{x < Wt-1} (t[y,x+1,c] - t[y,x,c])^2 + sum_{y < Ht-1} (t[y+1,x,c] - t[y,x,c])^2 ] (free boundary) -> energy[0], the
// per-workgroup partials added in a fixed order by the last workgroup to arrive (grid_sum); dE/dt ACCUMULATED into gradient.  The texture is only read.
template <class PixT>
__global__ __launch_bounds__(FH_BLOCK) void texture_smoothness_kernel(TexSmoothArgs a)
{
	constexpr int VEC = TexVec<PixT>::N;
	using V = typename TexVec<PixT>::type;
	const PixT *t = (const PixT *)a.texture;
	PixT *g = (PixT *)a.gradient;
	const int pieces = a.N / VEC, stride = (int)gridDim.x * FH_BLOCK;
	double s[1] = {0};
	for (int i = (int)blockIdx.x * FH_BLOCK + (int)threadIdx.x; i < pieces; i += stride)
	{
		const int e0 = i * VEC;
		if (e0 >= a.R && e0 + VEC + a.R <= a.N)
		{ // the four neighbour pieces lie inside the array (an element at the end of a row reads its missing neighbour from the next row, and drops it)
			const V c = *(const V *)(t + e0), l = *(const V *)(t + e0 - a.C), r = *(const V *)(t + e0 + a.C), u = *(const V *)(t + e0 - a.R),
					d = *(const V *)(t + e0 + a.R);
			V gv = *(const V *)(g + e0);
			int j = e0 % a.R;
#pragma unroll
			for (int k = 0; k < VEC; k++)
			{ // (every element of such a piece lies in rows 1 .. Ht-2: the rows above and below exist)
				const double ck = (double)c[k], dk = (double)d[k];
				double deg = 2, sum = (double)u[k] + dk;
				s[0] += (dk - ck) * (dk - ck);
				if (j >= a.C)
					deg += 1, sum += (double)l[k];
				if (j + a.C < a.R)
				{
					const double rk = (double)r[k];
					deg += 1, sum += rk, s[0] += (rk - ck) * (rk - ck);
				}
				gv[k] = (PixT)((double)gv[k] + a.weight * (deg * ck - sum));
				if (++j == a.R)
					j = 0;
			}
			*(V *)(g + e0) = gv;
		}
		else
#pragma unroll
			for (int k = 0; k < VEC; k++)
				s[0] += tex_smooth_one(t, g, a, e0 + k);
	}
	if (blockIdx.x == 0 && (int)threadIdx.x < a.N - pieces * VEC)
		s[0] += tex_smooth_one(t, g, a, pieces * VEC + (int)threadIdx.x);
	double total[1];
	if (grid_sum<1>(s, a.partials, a.counter, total) && threadIdx.x == 0)
		a.energy[0] = 0.5 * a.weight * total[0];
}

struct TexStepArgs
{
	void *texture, *speed;
	const void *gradient;
	double factor, step_max, inertia, damping, clamp_lo, clamp_hi;
	int clamp, N;
};

// s = (1 - damping)(inertia s + (1 - inertia) clamp(-factor g, +-step_max)); t += s; with clamp: t clipped to [clamp_lo, clamp_hi], s = 0 where it clipped
template <class PixT>
__device__ __forceinline__ void tex_step_one(PixT &t, PixT &s, PixT g, const TexStepArgs &a)
{
	double step = -a.factor * (double)g;
	if (a.step_max > 0)
		step = step < -a.step_max ? -a.step_max : (step > a.step_max ? a.step_max : step);
	double sn = (1 - a.damping) * (a.inertia * (double)s + (1 - a.inertia) * step);
	double tn = (double)t + sn;
	if (a.clamp && tn < a.clamp_lo)
		tn = a.clamp_lo, sn = 0;
	if (a.clamp && tn > a.clamp_hi)
		tn = a.clamp_hi, sn = 0;
	t = (PixT)tn, s = (PixT)sn;
}

template <class PixT>
__global__ __launch_bounds__(FH_BLOCK) void texture_step_kernel(TexStepArgs a)
{
	constexpr int VEC = TexVec<PixT>::N;
	using V = typename TexVec<PixT>::type;
	PixT *t = (PixT *)a.texture, *s = (PixT *)a.speed;
	const PixT *g = (const PixT *)a.gradient;
	const int pieces = a.N / VEC, stride = (int)gridDim.x * FH_BLOCK;
	for (int i = (int)blockIdx.x * FH_BLOCK + (int)threadIdx.x; i < pieces; i += stride)
	{
		V tv = *(const V *)(t + i * VEC), sv = *(const V *)(s + i * VEC);
		const V gv = *(const V *)(g + i * VEC);
#pragma unroll
		for (int k = 0; k < VEC; k++)
		{
			PixT tk = tv[k], sk = sv[k];
			tex_step_one(tk, sk, (PixT)gv[k], a);
			tv[k] = tk, sv[k] = sk;
		}
		*(V *)(t + i * VEC) = tv, *(V *)(s + i * VEC) = sv;
	}
	if (blockIdx.x == 0 && (int)threadIdx.x < a.N - pieces * VEC)
	{
		const int e = pieces * VEC + (int)threadIdx.x;
		tex_step_one(t[e], s[e], g[e], a);
	}
}

} // namespace
