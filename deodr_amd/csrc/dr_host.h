// deodr_amd/csrc/dr_host.h -- what every entry point of the C ABI asks of its arguments before it launches: the size of a dtype tag's elements,
// whether two buffers overlap, the grid of a kernel that strides beyond a capped number of workgroups, and the layout of the scratch buffers
// (counter words, then doubles; ScratchCarver hands out the arrays of an operator in order).  Host only, plain C++17, nothing of HIP in it: dr_kernels.hip calls these from its entry points,
// tests/sim/host_sim.cpp compiles the same header for the CPU and tests/test_host_helpers.py pins the edge cases.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace dr::host
{

// Bytes per element of a dtype tag of include/deodr_hip.h (DEODR_HIP_F32 = 0, DEODR_HIP_F64 = 1; dr_kernels.hip asserts the two values); 0: no such tag.
constexpr size_t elem_bytes(int dtype_tag) { return dtype_tag == 0 ? 4 : dtype_tag == 1 ? 8 : 0; }

// Do [a, a + a_bytes) and [b, b + b_bytes) share a byte?  A NULL pointer (an optional array that was not given) and an empty range overlap nothing.
// Written with differences of addresses, so a range that ends at the top of the address space does not wrap.
inline bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
	const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
	if (!a || !b || !a_bytes || !b_bytes)
		return false;
	return x <= y ? y - x < a_bytes : x - y < b_bytes;
}

// The same for entry points with many arrays: does any of `outputs` share a byte with any of `inputs`; do any two of `ranges` share one; is any
// of `pointers` (NULL: not given) not a multiple of `alignment` (a power of two).
struct Range
{
	const void *p;
	size_t bytes;
};
template <size_t NO, size_t NI>
inline bool any_overlap(const Range (&outputs)[NO], const Range (&inputs)[NI])
{
	for (const Range &o : outputs)
		for (const Range &i : inputs)
			if (ranges_overlap(o.p, o.bytes, i.p, i.bytes))
				return true;
	return false;
}
inline bool any_overlap(const Range *ranges, size_t count)
{
	for (size_t i = 0; i < count; i++)
		for (size_t j = i + 1; j < count; j++)
			if (ranges_overlap(ranges[i].p, ranges[i].bytes, ranges[j].p, ranges[j].bytes))
				return true;
	return false;
}
template <size_t N>
inline bool any_overlap(const Range (&ranges)[N])
{
	return any_overlap(ranges, N);
}
template <size_t N>
inline bool any_misaligned(const void *const (&pointers)[N], size_t alignment)
{
	uintptr_t bits = 0;
	for (const void *p : pointers)
		bits |= (uintptr_t)p;
	return (bits & (alignment - 1)) != 0;
}

// Workgroups of a grid-stride kernel: one per `per_block` items of `count`, at least 1, at most `cap`.
constexpr unsigned capped_blocks(size_t count, size_t per_block, unsigned cap)
{
	const size_t want = count / per_block + (count % per_block != 0);
	return want < 1 ? 1u : want < cap ? (unsigned)want : cap;
}

// The scratch of the fit-iteration, data-term and texture kernels: SCRATCH_COUNTER_WORDS counter words (zero between launches: the caller allocates
// the buffer zero-filled once, every kernel leaves its counter at zero), then doubles.
constexpr int SCRATCH_COUNTER_WORDS = 16;
constexpr size_t SCRATCH_COUNTER_BYTES = 4 * SCRATCH_COUNTER_WORDS;
constexpr size_t scratch_need(size_t doubles) { return SCRATCH_COUNTER_BYTES + sizeof(double) * doubles; }

struct Scratch
{
	void *base;
	size_t bytes;
	bool holds(size_t need) const { return base && bytes >= need; }
	unsigned *counter(int word) const { return (unsigned *)base + word; }
	double *doubles() const { return (double *)((char *)base + SCRATCH_COUNTER_BYTES); }
};

// The arrays of an operator's scratch, handed out in the order they are asked for, from behind the counter bytes: the doubles first, then the 4-byte
// words, so every array is aligned as its elements are.  One layout function per operator takes its arrays from a carver: without a base
// (NULL: nothing is handed out) it states the size, with one the pointers -- the two cannot disagree.
struct ScratchCarver
{
	char *base;
	size_t used = SCRATCH_COUNTER_BYTES;
	template <class T>
	T *take(size_t count)
	{
		T *const p = base ? (T *)(base + used) : nullptr;
		used += sizeof(T) * count;
		return p;
	}
	size_t whole_doubles() const { return (used + sizeof(double) - 1) / sizeof(double) * sizeof(double); } // (an odd number of words: one more)
};

} // namespace dr::host
