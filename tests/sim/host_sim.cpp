// tests/sim/host_sim.cpp -- TEST TOOL, never part of the product.
//
// The argument checks and the scratch view of deodr_amd/csrc/dr_host.h (host-only C++, the very header the entry points of dr_kernels.hip call) behind a C
// interface of plain integers, for tests/test_host_helpers.py.  With -DHOST_SIM_MAIN: a program that walks the same edge cases, for a build with
// -fsanitize=address,undefined (addresses are passed as integers and never read, so the top of the address space can be asked about).
#include "../../deodr_amd/csrc/dr_host.h"

using namespace dr::host;

extern "C" {

size_t host_elem_bytes(int tag) { return elem_bytes(tag); }
int host_ranges_overlap(uintptr_t a, size_t a_bytes, uintptr_t b, size_t b_bytes) { return ranges_overlap((const void *)a, a_bytes, (const void *)b, b_bytes); }
unsigned host_capped_blocks(size_t count, size_t per_block, unsigned cap) { return capped_blocks(count, per_block, cap); }
size_t host_scratch_need(size_t doubles) { return scratch_need(doubles); }
int host_scratch_holds(uintptr_t base, size_t bytes, size_t need) { return Scratch{(void *)base, bytes}.holds(need); }
// offsets in bytes from the base of a scratch buffer (a real one: pointer arithmetic)
size_t host_scratch_counter(void *base, int word) { return (size_t)((char *)Scratch{base, 0}.counter(word) - (char *)base); }
size_t host_scratch_doubles(void *base) { return (size_t)((char *)Scratch{base, 0}.doubles() - (char *)base); }
// do any two of `count` ranges (at most 16) share a byte
int host_any_pair_overlaps(const uintptr_t *at, const size_t *bytes, int count)
{
	Range ranges[16];
	for (int i = 0; i < count && i < 16; i++)
		ranges[i] = {(const void *)at[i], bytes[i]};
	return any_overlap(ranges, (size_t)(count < 16 ? count : 16));
}
// a carver over `base` (0: nothing is handed out) that gives `doubles` doubles, then `words` words: the offsets of the two arrays from the base
// (SIZE_MAX: not handed out), the bytes used, and those as whole doubles
void host_carve(void *base, size_t doubles, size_t words, size_t out[4])
{
	ScratchCarver c = {(char *)base};
	const double *const d = c.take<double>(doubles);
	const uint32_t *const w = c.take<uint32_t>(words);
	out[0] = d ? (size_t)((const char *)d - (const char *)base) : SIZE_MAX, out[1] = w ? (size_t)((const char *)w - (const char *)base) : SIZE_MAX;
	out[2] = c.used, out[3] = c.whole_doubles();
}
}

#ifdef HOST_SIM_MAIN
#include <limits.h>
#include <stdio.h>

#define CHECK(x) \
	if (!(x)) \
	return printf("host_sim: %s is false (line %d)\n", #x, __LINE__), 1

int main()
{
	CHECK(elem_bytes(0) == 4 && elem_bytes(1) == 8 && elem_bytes(-1) == 0 && elem_bytes(2) == 0 && elem_bytes(INT_MAX) == 0);
	const uintptr_t at = 4096, top = UINTPTR_MAX;
	CHECK(!host_ranges_overlap(at, 64, at + 128, 64) && !host_ranges_overlap(at, 64, at + 64, 64) && !host_ranges_overlap(at + 64, 64, at, 64));
	CHECK(host_ranges_overlap(at, 64, at + 63, 64) && host_ranges_overlap(at + 63, 64, at, 64) && host_ranges_overlap(at, 64, at + 8, 8));
	CHECK(!host_ranges_overlap(0, 64, at, 64) && !host_ranges_overlap(at, 64, 0, 64) && !host_ranges_overlap(at, 0, at, 64) && !host_ranges_overlap(at, 64, at + 8, 0));
	// the last 64 bytes of the address space: the end of the range is 2^64, which no uintptr_t holds
	CHECK(!host_ranges_overlap(top - 63, 64, at, 64) && !host_ranges_overlap(at, 64, top - 63, 64) && !host_ranges_overlap(top - 127, 64, top - 63, 64));
	CHECK(host_ranges_overlap(top - 63, 64, top - 64, 64) && host_ranges_overlap(top - 64, 2, top - 63, 64) && host_ranges_overlap(top - 63, 64, top, 1));
	const size_t per = 256, counts[7] = {0, 1, per - 1, per, per + 1, 8 * per, 8 * per + 1};
	const unsigned blocks[7] = {1, 1, 1, 1, 2, 8, 8};
	for (int i = 0; i < 7; i++)
		CHECK(capped_blocks(counts[i], per, 8) == blocks[i]);
	CHECK(capped_blocks(SIZE_MAX, per, 8) == 8 && capped_blocks(SIZE_MAX, 1, UINT_MAX) == UINT_MAX);
	alignas(8) unsigned char buffer[128];
	const Scratch sc = {buffer, sizeof buffer};
	CHECK(sc.holds(sizeof buffer) && sc.holds(sizeof buffer - 1) && !sc.holds(sizeof buffer + 1) && !host_scratch_holds(0, 128, 0));
	for (int word = 0; word < SCRATCH_COUNTER_WORDS; word++)
		CHECK(host_scratch_counter(buffer, word) == 4 * (size_t)word);
	CHECK(host_scratch_doubles(buffer) == 64 && scratch_need(0) == 64 && scratch_need(3) == 88);
	*sc.counter(SCRATCH_COUNTER_WORDS - 1) = 1, *sc.doubles() = 1.0, sc.doubles()[7] = 2.0; // (the whole buffer, and not a byte more)
	const Range one[1] = {{buffer, 64}}, touching[2] = {{buffer, 64}, {buffer + 64, 64}}, sharing[2] = {{buffer, 65}, {buffer + 64, 64}};
	const Range absent[3] = {{buffer, 64}, {nullptr, SIZE_MAX}, {buffer + 64, 64}}, empty[3] = {{buffer, 64}, {buffer + 8, 0}, {buffer + 64, 64}};
	CHECK(!any_overlap(one) && !any_overlap(touching) && any_overlap(sharing) && !any_overlap(absent) && !any_overlap(empty));
	Range seven[7];
	for (int i = 0; i < 7; i++)
		seven[i] = {buffer + 16 * i, 16};
	CHECK(!any_overlap(seven));
	seven[6].p = buffer + 16 * 5 + 15; // (the last two alone)
	CHECK(any_overlap(seven));
	size_t out[4];
	host_carve(buffer, 7, 3, out); // 64 counter bytes, 7 doubles, 3 words: 132 bytes, 136 as whole doubles -- beyond this buffer, which is not touched
	CHECK(out[0] == 64 && out[1] == 120 && out[2] == 132 && out[3] == 136);
	host_carve(nullptr, 7, 3, out);
	CHECK(out[0] == SIZE_MAX && out[1] == SIZE_MAX && out[2] == 132 && out[3] == 136);
	ScratchCarver carver = {(char *)buffer};
	double *const first = carver.take<double>(7);
	uint32_t *const second = carver.take<uint32_t>(2);
	first[6] = 1.0, second[1] = 1u; // 64 + 56 + 8 = 128: the last bytes of the buffer
	CHECK(carver.used == sizeof buffer && carver.whole_doubles() == sizeof buffer);
	printf("host_sim: ok\n");
	return 0;
}
#endif
