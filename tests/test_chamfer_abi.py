"""CPU checks of the closest-point energy at the C ABI (include/deodr_hip_chamfer.h; the header itself: tests/test_companion_headers.py): the
constants of deodr_amd/csrc/dr_chamfer.h are the ones the case tables are built for, every bad argument of the launching entry point is refused
through its error code with a message before any launch (fake pointers, no GPU), the scratch size is 0 outside the limits and the documented
formula inside, the split rule is swept for monotonicity and bounds, and the host wrapper refuses CPU tensors, wrong dtypes and wrong shapes
without reaching the library."""

import os
import re

import pytest


def test_the_host_side_has_the_operator_s_names():
    from deodr_amd import hip_renderer as hr

    for name in ("chamfer", "chamfer_scratch", "chamfer_launches", "chamfer_segments", "CHAMFER_ABI_VERSION"):
        assert hasattr(hr, name), name


def test_the_constants_of_the_kernels_are_the_case_table_s():
    import __graft_entry__ as g
    import chamfer_reference as cr
    from deodr_amd import hip_renderer as hr

    source = open(os.path.join(g.CSRC, "dr_chamfer.h")).read()
    assert re.search(r"CHAMFER_BLOCK = DEODR_HIP_CHAMFER_BLOCK, CHAMFER_TILE = DEODR_HIP_CHAMFER_TILE, CHAMFER_MAX_BLOCKS = DEODR_HIP_CHAMFER_MAX_BLOCKS", source)
    assert (hr.CHAMFER_BLOCK, hr.CHAMFER_TILE, hr.CHAMFER_MAX_BLOCKS, hr.CHAMFER_TARGET_BLOCKS, hr.CHAMFER_MAX_SEGMENTS) == (cr.BLOCK, cr.TILE, cr.MAX_BLOCKS, cr.TARGET_BLOCKS, cr.MAX_SEGMENTS)
    fh = open(os.path.join(g.CSRC, "dr_fronthalf.h")).read()
    assert int(re.search(r"^constexpr int FH_BLOCK = (\d+)", fh, re.M).group(1)) == cr.FH_BLOCK == cr.BLOCK
    assert cr.MAX_BLOCKS > cr.FH_BLOCK  # the last workgroup of grid_sum can add more than one partial per thread
    assert (hr.CHAMFER_POINTS_TO_MESH, hr.CHAMFER_MESH_TO_POINTS, hr.CHAMFER_MAX_PAIRS) == (1, 2, 2**36)
    assert "atomicAdd" not in source and "atomic_add" not in source  # no atomics on values (the tickets are grid_sum's, in dr_fronthalf.h)


def test_scratch_is_zero_outside_the_limits_and_the_documented_formula_inside():
    import chamfer_reference as cr
    from deodr_amd import hip_renderer as hr

    need = hr.lib().deodr_hip_chamfer_scratch_bytes
    for V, P, n in ((0, 5, 3), (-1, 5, 3), (5, 0, 3), (5, -1, 3), (5, 5, 0), (5, 5, -1), (5, 5, 65536), (2**18 + 1, 2**18, 1), (2**30, 2**30, 1)):
        assert need(V, P, n) == 0, (V, P, n)
    for V, P, n in ((1, 1, 1), (526, 4096, 1), (526, 40000, 8), (10002, 40000, 8), (40000, 10002, 3), (5, 5, 65535), (2**18, 2**18, 1), (65, 16129, 2), (261889, 257, 1)):
        Sp, Sv, M = hr.chamfer_segments(P, V), hr.chamfer_segments(V, P), hr.CHAMFER_MAX_BLOCKS
        assert need(V, P, n) == 64 + 8 * (n * (Sp * P + 4 * Sv * V + 2 * M) + (n * (Sp * P + Sv * V + P + 2) + 1) // 2) == cr.scratch_bytes(V, P, n), (V, P, n)
    sizes = [need(526, 4096, n) for n in (1, 2, 3, 4, 8)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)


def test_the_split_rule_is_monotone_and_bounded():
    import chamfer_reference as cr
    from deodr_amd import hip_renderer as hr

    S, B, T, cap = hr.chamfer_segments, hr.CHAMFER_BLOCK, hr.CHAMFER_TILE, hr.CHAMFER_MAX_SEGMENTS
    grid = [1, 2, 255, 256, 257, 511, 512, 513, 526, 4096, 10002, 16128, 16129, 16385, 40000, 65537, 131072, 131073, 261888, 261889, 262144, 262145, 10**6, 2**30, 2**31 - 1]
    for Q in grid:
        row = [S(Q, R) for R in grid]
        assert row == sorted(row) and all(1 <= s <= cap for s in row), Q  # non-decreasing in the references
        assert row == [cr.segments(Q, R) for R in grid]
        for R, s in zip(grid, row):
            assert s <= -(-R // T)  # never an empty part
            assert s == 1 or (s - 1) * -(-Q // B) < hr.CHAMFER_TARGET_BLOCKS  # never more parts than fill the device
    for R in grid:
        column = [S(Q, R) for Q in grid]
        assert column == sorted(column, reverse=True), R  # non-increasing in the queries
    dense = [S(65, R) for R in range(1, T * cap + 300)]
    assert dense == sorted(dense) and dense[0] == 1 and dense[-1] == cap and set(dense) == set(range(1, cap + 1))
    assert [S(526, 4096), S(4096, 526), S(526, 40000), S(40000, 526), S(10002, 40000), S(40000, 10002)] == [16, 3, 64, 3, 26, 7]
    for bad in ((0, 5), (5, 0), (-1, 5), (5, -(2**31))):
        assert S(*bad) == 0, bad
    for V, P, n, d, launches in ((5, 7, 1, 3, 4), (5, 7, 2, 1, 4), (5, 7, 65535, 2, 2), (2**18, 2**18, 1, 3, 4)):
        assert hr.chamfer_launches(V, P, n, d) == launches
    for bad in ((0, 7, 1, 3), (5, 0, 1, 3), (5, 7, 0, 3), (5, 7, 65536, 3), (5, 7, 1, 0), (5, 7, 1, 4), (5, 7, 1, -1), (2**18, 2**18 + 1, 1, 3)):
        assert hr.chamfer_launches(*bad) == 0, bad


def test_bad_arguments_are_refused_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from abi_cases import entry, misaligned, nulls, overlap_placements
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    V, P, n = 41, 250, 2
    base = dict(vertices=0x10000000, points=0x11000000, point_weights=0x12000000, vertex_weights=0x13000000, params=0x14000000, terms=0x15000000,
                loss=0x16000000, vertices_b=0x17000000, nearest_vertex=0x18000000, nearest_point=0x19000000, scratch=0x1A000000)  # fmt: skip
    optional = ("point_weights", "vertex_weights", "nearest_vertex", "nearest_point")

    call = entry(L, _abi.CHAMFER_HEADER, "deodr_hip_chamfer", base, V=V, P=P, n=n, directions=3,
                 scratch_bytes=lambda a: L.deodr_hip_chamfer_scratch_bytes(a["V"], a["P"], a["n"]))  # fmt: skip
    what = "chamfer"
    # a NULL required pointer (the optional ones may be NULL: such a call gets past every check only with real memory, not tried here)
    for bad in nulls(p for p in base if p not in optional):
        rc, msg = call(**bad)
        assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (bad, msg)
    for bad in (0, -1, -(2**31)):
        assert call(V=bad, scratch_bytes=1 << 20) == (1, what + ": V must be positive"), bad
        assert call(P=bad, scratch_bytes=1 << 20) == (1, what + ": P must be positive"), bad
    for bad in (0, -1, 65536):
        assert call(n=bad, scratch_bytes=1 << 20) == (1, what + ": n must be in 1 .. 65535"), bad
    for bad in (0, 4, -1, 7):
        assert call(directions=bad) == (1, what + ": directions must be in 1 .. 3"), bad
    assert call(V=2**18, P=2**18 + 1, n=1, scratch_bytes=1 << 40) == (1, what + ": V * P is above DEODR_HIP_CHAMFER_MAX_PAIRS (the search is brute force)")
    assert call(V=2**31 - 1, P=2**31 - 1, n=1, scratch_bytes=1 << 40)[1].endswith("(the search is brute force)")
    for bad in misaligned(base, ("nearest_vertex", "nearest_point"), 2):
        assert call(**bad) == (1, what + ": misaligned pointer"), bad
    for bad in misaligned(base, (p for p in base if p not in ("nearest_vertex", "nearest_point")), 4):
        assert call(**bad) == (1, what + ": misaligned pointer"), bad
    need = L.deodr_hip_chamfer_scratch_bytes(V, P, n)
    for short in (0, 64, need - 1):
        assert call(scratch_bytes=short) == (1, what + ": scratch too small (deodr_hip_chamfer_scratch_bytes)"), short
    sizes = dict(vertices=24 * n * V, points=24 * n * P, point_weights=8 * n * P, vertex_weights=8 * V, params=24, terms=16 * n, loss=8 * n,
                 vertices_b=24 * n * V, nearest_vertex=4 * n * P, nearest_point=4 * n * V, scratch=need)  # fmt: skip
    refusal = (1, what + ": an output must not overlap an input, the scratch or another output")
    for out in ("terms", "loss", "vertices_b", "nearest_vertex", "nearest_point", "scratch"):
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
        hr.chamfer(f64(2, 5, 3), f64(2, 9, 3), f64(3))

    Vt, Pt, Prm = dev(f64(2, 5, 3)), dev(f64(2, 9, 3)), dev(f64(3))
    for bad in (dev(f64(5, 3)), dev(f64(2, 5, 4)), dev(f64(0, 5, 3)), dev(f64(2, 0, 3)), dev(f64(2, 5, 3, 1))):
        with pytest.raises(ValueError, match=r"vertices must have shape \[n >= 1, V >= 1, 3\]"):
            hr.chamfer(bad, Pt, Prm)
    for bad in (dev(f64(9, 3)), dev(f64(3, 9, 3)), dev(f64(2, 0, 3)), dev(f64(2, 9, 2)), None):
        with pytest.raises(ValueError, match=r"points must have shape \[2, P >= 1, 3\]"):
            hr.chamfer(Vt, bad, Prm)
    for bad in (0, 4, -1):
        with pytest.raises(ValueError, match="directions must be in 1 .. 3"):
            hr.chamfer(Vt, Pt, Prm, directions=bad)
    with pytest.raises(ValueError, match="vertices must be float64"):
        hr.chamfer(dev(f64(2, 5, 3).float()), Pt, Prm)
    with pytest.raises(ValueError, match="vertices must be contiguous"):
        hr.chamfer(dev(f64(5, 2, 3).transpose(0, 1)), Pt, Prm)
    with pytest.raises(ValueError, match="points must be a ROCm tensor on the device of vertices"):
        hr.chamfer(Vt, f64(2, 9, 3), Prm)
    with pytest.raises(ValueError, match=r"params must have shape \[3\]"):
        hr.chamfer(Vt, Pt, dev(f64(2)))
    with pytest.raises(ValueError, match="params must be a ROCm tensor"):
        hr.chamfer(Vt, Pt, f64(3))
    with pytest.raises(ValueError, match=r"point_weights must have shape \[2, 9\]"):
        hr.chamfer(Vt, Pt, Prm, point_weights=dev(f64(9)))
    with pytest.raises(ValueError, match=r"vertex_weights must have shape \[5\]"):
        hr.chamfer(Vt, Pt, Prm, vertex_weights=dev(f64(2, 5)))
    with pytest.raises(ValueError, match=r"terms must have shape \[2, 2\]"):
        hr.chamfer(Vt, Pt, Prm, terms=dev(f64(2)))
    with pytest.raises(ValueError, match=r"loss must have shape \[2\]"):
        hr.chamfer(Vt, Pt, Prm, loss=dev(f64(1)))
    with pytest.raises(ValueError, match=r"vertices_b must have shape \[2, 5, 3\]"):
        hr.chamfer(Vt, Pt, Prm, vertices_b=dev(f64(5, 3)))
    with pytest.raises(ValueError, match="nearest_vertex must be int32 or uint32"):
        hr.chamfer(Vt, Pt, Prm, nearest_vertex=dev(i32(2, 9).long()))
    with pytest.raises(ValueError, match=r"nearest_point must have shape \[2, 5\]"):
        hr.chamfer(Vt, Pt, Prm, nearest_point=dev(i32(2, 9)))
    with pytest.raises(ValueError, match="scratch must be uint8"):
        hr.chamfer(Vt, Pt, Prm, scratch=dev(torch.zeros(64)))
