"""CPU checks of the as-rigid-as-possible energy at the C ABI (include/deodr_hip_arap.h; the header itself: tests/test_companion_headers.py): the
constants of deodr_amd/csrc/dr_arap.h are the ones the case tables are built for, every bad argument of the launching entry point is refused
through its error code with a message before any launch (fake pointers, no GPU), the scratch size is 0 outside the limits, monotone inside them
and the documented formula, the launch rule is pinned at its boundaries, and the host wrapper refuses CPU tensors, wrong dtypes and wrong shapes
without reaching the library."""

import os
import re

import pytest


def test_the_constants_are_the_header_s():
    from deodr_amd import hip_renderer as hr

    assert (hr.ARAP_SWEEPS, hr.ARAP_BLOCK, hr.ARAP_MAX_BLOCKS) == (5, 256, 512)


def test_the_constants_of_the_kernels_are_the_case_table_s():
    import __graft_entry__ as g
    import arap_reference as ar
    from deodr_amd import hip_renderer as hr

    source = open(os.path.join(g.CSRC, "dr_arap.h")).read()
    assert re.search(r"ARAP_SWEEPS = DEODR_HIP_ARAP_SWEEPS, ARAP_BLOCK = DEODR_HIP_ARAP_BLOCK, ARAP_MAX_BLOCKS = DEODR_HIP_ARAP_MAX_BLOCKS", source)
    assert (hr.ARAP_SWEEPS, hr.ARAP_BLOCK, hr.ARAP_MAX_BLOCKS) == (ar.SWEEPS, ar.BLOCK, ar.MAX_BLOCKS)
    fh = open(os.path.join(g.CSRC, "dr_fronthalf.h")).read()
    assert int(re.search(r"^constexpr int FH_BLOCK = (\d+)", fh, re.M).group(1)) == ar.FH_BLOCK == ar.BLOCK
    assert ar.MAX_BLOCKS > ar.FH_BLOCK  # the last workgroup of grid_sum can add more than one partial per thread
    assert re.search(r"fabs\(theta\) <= 1e150", source) and ar.THETA_BIG == 1e150
    pivots = re.findall(r"arap_rotate<(\d), (\d)>\(A, E\);", source)
    assert tuple((int(a), int(b)) for a, b in pivots) == ar.PAIRS


def test_scratch_is_zero_outside_the_limits_monotone_inside_and_the_documented_formula():
    from deodr_amd import hip_renderer as hr

    need = hr.lib().deodr_hip_arap_scratch_bytes
    for V, n in ((0, 3), (-1, 3), (5, 0), (5, -1), (5, 65536)):
        assert need(V, n) == 0, (V, n)
    for V, n in ((1, 1), (526, 8), (10002, 1), (131073, 3), (5, 65535)):
        assert need(V, n) == 64 + 8 * (5 * n * V + 512 * n + (n + 1) // 2), (V, n)
    for sizes in ([need(V, 2) for V in (1, 2, 256, 257, 50000)], [need(526, n) for n in (1, 2, 3, 4, 8)]):
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes), sizes


def test_the_launch_rule_at_its_boundaries():
    import arap_reference as ar
    from deodr_amd import hip_renderer as hr

    B, M = hr.ARAP_BLOCK, hr.ARAP_MAX_BLOCKS
    for V, blocks in ((1, 1), (B - 1, 1), (B, 1), (B + 1, 2), (526, 3), (10002, 40), (B * B, B), (B * B + 1, B + 1), (B * M - 1, M), (B * M, M), (B * M + 1, M), (2**30, M)):
        assert hr.arap_blocks(V) == blocks == min(-(-V // B), M), V
        for n in (1, 8):
            assert hr.arap_launches(V, 6 * V, n) == 2 == hr.arap_launches(V, 0, n), (V, n)
    assert [hr.arap_blocks(V) for V in (0, -1, -(2**31))] == [0, 0, 0]
    for bad in ((0, 0, 1), (-5, 0, 1), (10, 60, 0), (10, 60, -1), (10, 60, 65536)):
        assert hr.arap_launches(*bad) == 0, bad
    assert ar.boundary_sizes(hr.arap_blocks, B, M) == [B - 1, B, B + 1, B * B + 1, B * M + 1]  # what tests/test_arap_gpu.py runs


def test_bad_arguments_are_refused_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from abi_cases import entry, misaligned, nulls, overlap_placements
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    V, nnz, n = 41, 250, 2  # (4 (V + 1) and 4 nnz multiples of 8: the overlaps below stay aligned)
    base = dict(offsets=0x10000000, cols=0x11000000, weights=0x12000000, vertices_ref=0x13000000, vertices=0x14000000, energy=0x15000000,
                gradient=0x16000000, rotations=0x17000000, scratch=0x18000000)  # fmt: skip

    call = entry(L, _abi.ARAP_HEADER, "deodr_hip_arap_energy", base, V=V, nnz=nnz, n=n, cregu=1.0,
                 scratch_bytes=lambda a: L.deodr_hip_arap_scratch_bytes(a["V"], a["n"]))  # fmt: skip
    what = "arap_energy"
    # a NULL pointer (rotations may be NULL: the call then gets past every check of this test only with real memory, not tried here)
    for bad in nulls(p for p in base if p != "rotations"):
        rc, msg = call(**bad)
        assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (bad, msg)
    for bad in (0, -1, -(2**31)):
        assert call(V=bad, scratch_bytes=1 << 20) == (1, what + ": V must be positive"), bad
    for bad in (0, -1, 65536):
        assert call(n=bad, scratch_bytes=1 << 20) == (1, what + ": n must be in 1 .. 65535"), bad
    for bad in (-1e-300, -1.0, float("-inf"), float("nan")):
        assert call(cregu=bad) == (1, what + ": cregu must be >= 0"), bad
    for bad in misaligned(base, ("offsets", "cols"), 2):
        assert call(**bad) == (1, what + ": misaligned pointer"), bad
    for bad in misaligned(base, ("weights", "vertices_ref", "vertices", "energy", "gradient", "rotations", "scratch"), 4):
        assert call(**bad) == (1, what + ": misaligned pointer"), bad
    need = L.deodr_hip_arap_scratch_bytes(V, n)
    for short in (0, 64, need - 1):
        assert call(scratch_bytes=short) == (1, what + ": scratch too small (deodr_hip_arap_scratch_bytes)"), short
    cells = n * V
    sizes = dict(offsets=4 * (V + 1), cols=4 * nnz, weights=8 * nnz, vertices_ref=24 * V, vertices=24 * cells, energy=8 * n, gradient=24 * cells,
                 rotations=32 * cells, scratch=need)  # fmt: skip
    refusal = (1, what + ": an output must not overlap an input, the scratch or another output")
    for out in ("energy", "gradient", "rotations", "scratch"):
        for other in sizes:
            if other != out:
                for at in overlap_placements(base, sizes, out, other):
                    assert call(**{out: at}) == refusal, (out, other, hex(at))


def test_host_wrapper_checks_its_tensors_before_the_library(monkeypatch):
    import torch

    from abi_cases import no_library
    from abi_cases import on_device as dev
    from deodr_amd import hip_renderer as hr

    monkeypatch.setattr(hr, "lib", no_library)
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    with pytest.raises(ValueError, match="vertices must be a ROCm tensor"):
        hr.arap_energy(i32(6), i32(9), f64(9), f64(5, 3), f64(2, 5, 3), 1.0)

    O, Cc, W, Q, P = dev(i32(6)), dev(i32(9)), dev(f64(9)), dev(f64(5, 3)), dev(f64(2, 5, 3))
    for bad in (dev(f64(5, 3)), dev(f64(2, 5, 4)), dev(f64(0, 5, 3)), dev(f64(2, 0, 3)), dev(f64(2, 5, 3, 1))):
        with pytest.raises(ValueError, match=r"vertices must have shape \[n >= 1, V >= 1, 3\]"):
            hr.arap_energy(O, Cc, W, Q, bad, 1.0)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="cregu must be >= 0"):
            hr.arap_energy(O, Cc, W, Q, P, bad)
    with pytest.raises(ValueError, match="vertices must be float64"):
        hr.arap_energy(O, Cc, W, Q, dev(f64(2, 5, 3).float()), 1.0)
    with pytest.raises(ValueError, match="vertices must be contiguous"):
        hr.arap_energy(O, Cc, W, Q, dev(f64(5, 2, 3).transpose(0, 1)), 1.0)
    with pytest.raises(ValueError, match=r"vertices_ref must have shape \[5, 3\]"):
        hr.arap_energy(O, Cc, W, dev(f64(4, 3)), P, 1.0)
    with pytest.raises(ValueError, match=r"offsets must be a 4-byte integer tensor of V \+ 1 = 6 entries"):
        hr.arap_energy(dev(i32(5)), Cc, W, Q, P, 1.0)
    with pytest.raises(ValueError, match="offsets and cols must be one-dimensional 4-byte integer tensors"):
        hr.arap_energy(O, dev(i32(9).long()), W, Q, P, 1.0)
    with pytest.raises(ValueError, match="weights must be a float64 tensor of the shape of cols"):
        hr.arap_energy(O, Cc, dev(f64(8)), Q, P, 1.0)
    with pytest.raises(ValueError, match="offsets must be a 4-byte integer tensor"):
        hr.arap_energy(i32(6), Cc, W, Q, P, 1.0)  # a CPU tensor
    with pytest.raises(ValueError, match=r"energy must have shape \[2\]"):
        hr.arap_energy(O, Cc, W, Q, P, 1.0, energy=dev(f64(3)))
    with pytest.raises(ValueError, match=r"gradient must have shape \[2, 5, 3\]"):
        hr.arap_energy(O, Cc, W, Q, P, 1.0, gradient=dev(f64(5, 3)))
    with pytest.raises(ValueError, match=r"rotations must have shape \[2, 5, 4\]"):
        hr.arap_energy(O, Cc, W, Q, P, 1.0, rotations=dev(f64(2, 5, 3)))
    with pytest.raises(ValueError, match="scratch must be uint8"):
        hr.arap_energy(O, Cc, W, Q, P, 1.0, scratch=dev(torch.zeros(64)))
