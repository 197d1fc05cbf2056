"""What every entry point of the C ABI asks of its arguments (deodr_amd/csrc/dr_host.h, compiled for the CPU by tests/sim/host_sim.cpp): the element
size of a dtype tag, whether two buffers (or any two of a set) overlap, the capped grids and the layout of the scratch buffers, carved or not.  dr_kernels.hip calls the very same header;
the edge cases here are the ones no GPU test reaches (a buffer at the top of the address space, an unknown tag, an empty range)."""

import ctypes as C
import subprocess

import numpy as np
import pytest

import sim_util

INT_MAX, TOP = 2**31 - 1, 2**64 - 1  # (uintptr_t is 64 bits on every host of the project)
AT = 1 << 20


@pytest.fixture(scope="module")
def lib():
    return sim_util.host_lib()


def test_elem_bytes_knows_the_two_tags_and_nothing_else(lib):
    assert [lib.host_elem_bytes(tag) for tag in (0, 1)] == [4, 8]  # DEODR_HIP_F32, DEODR_HIP_F64
    assert [lib.host_elem_bytes(tag) for tag in (-1, 2, INT_MAX)] == [0, 0, 0]


@pytest.mark.parametrize(
    "a, a_bytes, b, b_bytes, overlap",
    [
        (AT, 64, AT + 128, 64, False),  # disjoint
        (AT, 64, AT + 64, 64, False),  # touching at the boundary
        (AT, 64, AT + 63, 64, True),  # ... shifted by one byte
        (AT + 1, 64, AT + 64, 64, True),
        (AT, 64, AT - 63, 64, True),  # ... the other way
        (AT, 64, AT - 64, 64, False),
        (AT, 64, AT, 64, True),
        (AT, 64, AT + 8, 8, True),  # contained
        (AT + 56, 8, AT, 64, True),
        (0, 64, 16, 64, False),  # NULL: an optional array that was not given
        (AT, 64, 0, TOP, False),
        (AT, 0, AT, 64, False),  # an empty range
        (AT, 64, AT + 8, 0, False),
        (TOP - 63, 64, AT, 64, False),  # the last bytes of the address space: a + a_bytes is 2^64
        (TOP - 127, 64, TOP - 63, 64, False),
        (TOP - 63, 64, TOP - 64, 64, True),
        (TOP - 63, 64, TOP, 1, True),
        (TOP, 1, TOP - 63, 64, True),
        (TOP - 63, 64, 8, TOP - 71, False),  # b ends where a starts
        (TOP - 63, 64, 8, TOP - 70, True),
    ],
)
def test_ranges_overlap(lib, a, a_bytes, b, b_bytes, overlap):
    assert bool(lib.host_ranges_overlap(a, a_bytes, b, b_bytes)) == overlap
    assert bool(lib.host_ranges_overlap(b, b_bytes, a, a_bytes)) == overlap


@pytest.mark.parametrize("per_block, cap", [(256, 512), (8192, 256), (1, 64), (1024, 1)])
def test_capped_blocks(lib, per_block, cap):
    counts = [0, 1, per_block - 1, per_block, per_block + 1, cap * per_block, cap * per_block + 1, TOP]
    assert [lib.host_capped_blocks(n, per_block, cap) for n in counts] == [min(max(-(-n // per_block), 1), cap) for n in counts]
    assert lib.host_capped_blocks(0, per_block, cap) == 1 and lib.host_capped_blocks(cap * per_block + 1, per_block, cap) == cap


def test_scratch_view(lib):
    buffer = np.zeros(64 + 8 * 5, np.uint8)  # the 16 counter words, then five doubles
    base, need = buffer.ctypes.data, lib.host_scratch_need(5)
    assert need == buffer.nbytes == 64 + 8 * 5 and lib.host_scratch_need(0) == 64
    assert lib.host_scratch_holds(base, need, need) and lib.host_scratch_holds(base, need, need - 1) and lib.host_scratch_holds(base, need + 1, need)
    assert not lib.host_scratch_holds(base, need - 1, need)
    assert not lib.host_scratch_holds(0, need, need) and not lib.host_scratch_holds(0, need, 0)  # NULL holds nothing
    assert [lib.host_scratch_counter(base, word) for word in range(16)] == [4 * word for word in range(16)]
    assert lib.host_scratch_doubles(base) == 64


@pytest.mark.parametrize(
    "ranges, overlap",
    [
        ([(AT, 64)], False),  # one range
        ([(AT, 64), (AT + 64, 64)], False),  # two that touch
        ([(AT, 65), (AT + 64, 64)], True),  # ... and share one byte
        ([(AT, 64), (0, TOP), (AT + 64, 64)], False),  # a NULL among three: an optional array that was not given
        ([(AT, 64), (0, TOP), (AT + 63, 64)], True),
        ([(AT, 64), (AT + 8, 0), (AT + 64, 64)], False),  # an empty range among three
        ([(AT + 16 * i, 16) for i in range(7)], False),
        ([(AT + 16 * i, 16) for i in range(6)] + [(AT + 16 * 5 + 15, 16)], True),  # a clash between the last two of seven alone
        ([(AT + 16 * i, 16) for i in range(6)] + [(AT, 1)], True),  # ... between the first and the last
    ],
)
def test_any_two_of_a_set_overlap(lib, ranges, overlap):
    array = C.c_size_t * len(ranges)
    for order in (ranges, ranges[::-1]):
        assert bool(lib.host_any_pair_overlaps(array(*(r[0] for r in order)), array(*(r[1] for r in order)), len(order))) == overlap


@pytest.mark.parametrize("doubles, words", [(0, 0), (7, 3), (7, 4), (1, 1), (0, 5), (2**40, 2**33 + 1)])
def test_scratch_carver_hands_out_doubles_then_words_and_counts_the_same_without_a_base(lib, doubles, words):
    used = 64 + 8 * doubles + 4 * words  # after the 16 counter words
    out, base = (C.c_size_t * 4)(), AT  # (the carver hands out addresses and reads nothing)
    lib.host_carve(base, doubles, words, out)
    assert list(out) == [64, 64 + 8 * doubles, used, -(-used // 8) * 8]
    lib.host_carve(None, doubles, words, out)
    assert list(out) == [TOP, TOP, used, -(-used // 8) * 8]  # nothing handed out, the same size


def test_the_scratch_sizes_of_the_closest_point_operators_are_the_restatements_of_the_tests():
    """the three layouts carved by ScratchCarver against tests/*_reference.py, over the sizes of the three ABI tests together"""
    import chamfer_grid_reference as gr
    import chamfer_reference as cr
    import surface_reference as sr
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    I = gr.SORT_ITEMS
    chamfer = [(1, 1, 1), (526, 4096, 1), (526, 40000, 8), (10002, 40000, 8), (40000, 10002, 3), (5, 5, 65535), (2**18, 2**18, 1), (65, 16129, 2), (261889, 257, 1)]
    surface = [(1, 1, 1, 1), (526, 1048, 4096, 1), (526, 1048, 40000, 8), (10002, 20000, 40000, 8), (5, 7, 9, 65535), (9, 2**16, 2**16, 1), (40, 65, 16129, 2),
               (40, 16129, 65, 2), (100, 3, 65537, 1), (50000, 65537, 3, 3)]  # fmt: skip
    sizes = (1, 2, 32, 33, 255, 256, 257, 526, I, I + 1, 10002, 65537, 2**18, 2**18 + 1, 2**24)
    grid = [(V, P, n) for V in sizes for P in sizes for n in (1, 3)]
    pairs = sorted(set(chamfer) | set(grid) | {(V, P, n) for V, _, P, n in surface})
    for V, P, n in pairs:
        if V * P <= hr.CHAMFER_MAX_PAIRS:
            assert L.deodr_hip_chamfer_scratch_bytes(V, P, n) == cr.scratch_bytes(V, P, n) > 0, (V, P, n)
        if max(V, P) <= gr.MAX_ITEMS:
            assert L.deodr_hip_chamfer_grid_scratch_bytes(V, P, n) == gr.scratch_bytes(V, P, n) > 0, (V, P, n)
    faces = sorted({F for _, F, _, _ in surface})
    for V, F, P, n in sorted(set(surface) | {(V, F, P, n) for V, P, n in chamfer for F in faces}):
        if F * P <= hr.SURFACE_MAX_PAIRS:
            assert L.deodr_hip_surface_distance_scratch_bytes(V, F, P, n) == sr.scratch_bytes(V, F, P, n) > 0, (V, F, P, n)


def test_the_same_cases_under_the_sanitizers(tmp_path):
    """the header in a program of its own (host_sim.cpp's main) with -fsanitize=address,undefined: no overflow, no read or write outside a buffer"""
    run = subprocess.run([sim_util.host_program(str(tmp_path))], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "host_sim: ok", run.stdout + run.stderr
