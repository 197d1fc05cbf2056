"""What every entry point of the C ABI asks of its arguments (deodr_amd/csrc/dr_host.h, compiled for the CPU by tests/sim/host_sim.cpp): the element
size of a dtype tag, whether two buffers overlap, the capped grids and the layout of the scratch buffers.  dr_kernels.hip calls the very same header;
the edge cases here are the ones no GPU test reaches (a buffer at the top of the address space, an unknown tag, an empty range)."""

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


def test_the_same_cases_under_the_sanitizers(tmp_path):
    """the header in a program of its own (host_sim.cpp's main) with -fsanitize=address,undefined: no overflow, no read or write outside a buffer"""
    run = subprocess.run([sim_util.host_program(str(tmp_path))], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "host_sim: ok", run.stdout + run.stderr
