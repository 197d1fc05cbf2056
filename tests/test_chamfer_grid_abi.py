"""CPU checks of the stable sort by key and the closest-point energy over a uniform grid at the C ABI (include/deodr_hip_chamfer_grid.h; the
header itself: tests/test_companion_headers.py): its constants are the restatement's and the kernels', every bad argument of the two launching
entry points is refused through its error code with a message before any launch (fake pointers, no GPU), ``scratch_bytes`` / ``launches`` /
``table_bits`` are the restatement's at and around their change points and 0 for refused arguments, and the host wrappers refuse CPU tensors,
wrong dtypes and wrong shapes without reaching the library."""

import os
import re

import pytest

import chamfer_grid_reference as gr


def test_the_constants_are_the_restatement_s_and_the_host_side_has_the_operators_names():
    from deodr_amd import hip_renderer as hr

    assert gr.SORT_ITEMS % gr.SORT_BLOCK == 0 and 1 << gr.DIGIT_BITS == gr.SORT_BLOCK and 2 * gr.MAX_ITEMS == 1 << gr.MAX_TABLE_BITS
    for name in ("chamfer_grid", "chamfer_grid_scratch", "chamfer_grid_launches", "chamfer_grid_table_bits", "sort_keys", "sort_keys_scratch", "sort_keys_launches",
                 "CHAMFER_GRID_ABI_VERSION", "CHAMFER_GRID_NONE"):  # fmt: skip
        assert hasattr(hr, name), name
    assert hr.CHAMFER_GRID_NONE == gr.NONE and (hr.SORT_DIGIT_BITS, hr.SORT_ITEMS, hr.CHAMFER_GRID_RINGS) == (gr.DIGIT_BITS, gr.SORT_ITEMS, gr.RINGS)


def test_the_kernels_use_the_header_s_constants_and_no_atomics_on_values():
    import __graft_entry__ as g

    grid, sort = open(os.path.join(g.CSRC, "dr_chamfer_grid.h")).read(), open(os.path.join(g.CSRC, "dr_sort.h")).read()
    assert re.search(r"SORT_DIGIT_BITS = DEODR_HIP_SORT_DIGIT_BITS, SORT_DIGITS = 1 << SORT_DIGIT_BITS, SORT_BLOCK = DEODR_HIP_SORT_BLOCK", sort)
    assert re.search(r"SORT_ITEMS = DEODR_HIP_SORT_ITEMS", sort) and re.search(r"CG_RINGS = DEODR_HIP_CHAMFER_GRID_RINGS", grid)
    assert re.search(r"CG_EXIT_MARGIN = 1\.0 - 1\.0 / 1048576\.0", grid) and gr.EXIT_MARGIN == 1.0 - 1.0 / 1048576.0
    assert "atomic" not in grid.replace("floating-point atomics", "").replace("integer atomics", "")  # (the tickets are grid_sum's, in dr_fronthalf.h)
    assert sort.count("atomicAdd") == 1 and "atomicAdd(&s_count" in sort  # the LDS digit counts of the histogram alone
    assert "rocprim" not in sort.lower() and "rocprim" not in grid.lower()


def test_sizes_at_and_around_their_change_points_and_zero_for_refused_arguments():
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    I, D, M = gr.SORT_ITEMS, gr.DIGIT_BITS, gr.SORT_MAX_ITEMS
    for N in (1, 2, I - 1, I, I + 1, 2 * I, 2 * I + 1, M - 1, M):
        for n in (1, 3, 65535):
            for bits in (1, D - 1, D, D + 1, 2 * D, 2 * D + 1, 3 * D + 1, 32):
                assert L.deodr_hip_sort_keys_scratch_bytes(N, n, bits) == gr.sort_scratch_bytes(N, n, bits) > 0, (N, n, bits)
                assert hr.sort_keys_launches(N, n, bits) == gr.sort_launches(N, n, bits) == 3 * -(-bits // D), (N, n, bits)
    for bad in ((0, 1, 8), (-1, 1, 8), (M + 1, 1, 8), (5, 0, 8), (5, 65536, 8), (5, 1, 0), (5, 1, 33), (5, 1, -1)):
        assert L.deodr_hip_sort_keys_scratch_bytes(*bad) == 0 == hr.sort_keys_launches(*bad), bad
    table = hr.chamfer_grid_table_bits
    for r in (1, 2, 31, 32, 33, 63, 64, 65, 2**20, 2**20 + 1, 2**23, 2**23 + 1, 2**24 - 1, 2**24):
        assert table(r) == gr.table_bits(r) and (1 << table(r)) >= 2 * r and (table(r) == gr.MIN_TABLE_BITS or (1 << table(r)) < 4 * r), r
    assert [table(r) for r in (1, 32, 33, 2**24)] == [6, 6, 7, 25] and [table(r) for r in (0, -1, 2**24 + 1)] == [0, 0, 0]
    sizes = (1, 2, 32, 33, 255, 256, 257, 526, I, I + 1, 10002, 65537, 2**18, 2**18 + 1, 2**24)
    for V in sizes:
        for P in sizes:
            for n in (1, 3):
                assert L.deodr_hip_chamfer_grid_scratch_bytes(V, P, n) == gr.scratch_bytes(V, P, n) > 0, (V, P, n)
                for directions in (1, 2, 3):
                    assert hr.chamfer_grid_launches(V, P, n, directions) == gr.launches(V, P, n, directions) > 0
    assert hr.chamfer_grid_launches(255, 7, 1, 1) + 3 == hr.chamfer_grid_launches(256, 7, 1, 1)  # the assignment needs a ninth bit: one pass more
    assert hr.chamfer_grid_launches(7, 128, 1, 2) + 3 == hr.chamfer_grid_launches(7, 129, 1, 2)  # 2^9 buckets: one pass more
    assert [hr.chamfer_grid_launches(526, 40000, 1, d) for d in (1, 2, 3)] == [18, 13, 30]
    for bad in ((0, 5, 3), (-1, 5, 3), (5, 0, 3), (5, -1, 3), (5, 5, 0), (5, 5, 65536), (2**24 + 1, 5, 1), (5, 2**24 + 1, 1)):
        assert L.deodr_hip_chamfer_grid_scratch_bytes(*bad) == 0 == hr.chamfer_grid_launches(*bad, 3), bad
    for bad in (0, 4, -1):
        assert hr.chamfer_grid_launches(5, 7, 1, bad) == 0
    assert L.deodr_hip_chamfer_grid_scratch_bytes(2**18, 2**18 + 1, 1) > 0 and L.deodr_hip_chamfer_scratch_bytes(2**18, 2**18 + 1, 1) == 0  # no cap on V * P


def test_bad_arguments_of_the_sort_are_refused_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from abi_cases import entry, misaligned, nulls, overlap_placements
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    N, n, bits = 300, 2, 12
    base = dict(keys=0x10000000, sorted_keys=0x11000000, order=0x12000000, scratch=0x13000000)
    need = L.deodr_hip_sort_keys_scratch_bytes(N, n, bits)

    call = entry(L, _abi.CHAMFER_GRID_HEADER, "deodr_hip_sort_keys", base, N=N, n=n, bits=bits, scratch_bytes=need)
    what = "sort_keys"
    for bad in nulls(("keys", "order", "scratch")):
        rc, msg = call(**bad)
        assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (bad, msg)
    for bad in (0, -1, gr.SORT_MAX_ITEMS + 1):
        assert call(N=bad, scratch_bytes=1 << 40) == (1, what + ": N must be in 1 .. DEODR_HIP_SORT_MAX_ITEMS"), bad
    for bad in (0, -1, 65536):
        assert call(n=bad, scratch_bytes=1 << 40) == (1, what + ": n must be in 1 .. 65535"), bad
    for bad in (0, -1, 33):
        assert call(bits=bad) == (1, what + ": bits must be in 1 .. 32"), bad
    for bad in misaligned(base, base, 2):
        assert call(**bad) == (1, what + ": misaligned pointer"), bad
    for short in (0, 64, need - 1):
        assert call(scratch_bytes=short) == (1, what + ": scratch too small (deodr_hip_sort_keys_scratch_bytes)"), short
    sizes = dict(keys=4 * n * N, sorted_keys=4 * n * N, order=4 * n * N, scratch=need)
    for a in base:
        for b in base:
            if a != b:
                for at in overlap_placements(base, sizes, a, b, unit=4):
                    assert call(**{a: at}) == (1, what + ": keys, sorted_keys, order and scratch must not overlap"), (a, b, hex(at))


def test_bad_arguments_of_the_operator_are_refused_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from abi_cases import entry, misaligned, nulls, overlap_placements
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    V, P, n = 41, 250, 2
    base = dict(vertices=0x10000000, points=0x11000000, point_weights=0x12000000, vertex_weights=0x13000000, params=0x14000000, terms=0x15000000,
                loss=0x16000000, vertices_b=0x17000000, nearest_vertex=0x18000000, nearest_point=0x19000000, scratch=0x1A000000)  # fmt: skip
    optional = ("point_weights", "vertex_weights", "nearest_vertex", "nearest_point")

    call = entry(L, _abi.CHAMFER_GRID_HEADER, "deodr_hip_chamfer_grid", base, V=V, P=P, n=n, directions=3, cell_size=0.1,
                 scratch_bytes=lambda a: L.deodr_hip_chamfer_grid_scratch_bytes(a["V"], a["P"], a["n"]))  # fmt: skip
    what = "chamfer_grid"
    # a NULL required pointer (the optional ones may be NULL: such a call gets past every check only with real memory, not tried here)
    for bad in nulls(p for p in base if p not in optional):
        rc, msg = call(**bad)
        assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (bad, msg)
    for bad in (0, -1, -(2**31), gr.MAX_ITEMS + 1):
        assert call(V=bad, scratch_bytes=1 << 40) == (1, what + ": V must be in 1 .. DEODR_HIP_CHAMFER_GRID_MAX_ITEMS"), bad
        assert call(P=bad, scratch_bytes=1 << 40) == (1, what + ": P must be in 1 .. DEODR_HIP_CHAMFER_GRID_MAX_ITEMS"), bad
    for bad in (0, -1, 65536):
        assert call(n=bad, scratch_bytes=1 << 40) == (1, what + ": n must be in 1 .. 65535"), bad
    for bad in (0, 4, -1, 7):
        assert call(directions=bad) == (1, what + ": directions must be in 1 .. 3"), bad
    for bad in (0.0, -0.1, float("inf"), float("-inf"), float("nan")):
        assert call(cell_size=bad) == (1, what + ": cell_size must be finite and > 0"), bad
    for bad in misaligned(base, ("nearest_vertex", "nearest_point"), 2):
        assert call(**bad) == (1, what + ": misaligned pointer"), bad
    for bad in misaligned(base, (p for p in base if p not in ("nearest_vertex", "nearest_point")), 4):
        assert call(**bad) == (1, what + ": misaligned pointer"), bad
    need = L.deodr_hip_chamfer_grid_scratch_bytes(V, P, n)
    for short in (0, 64, need - 1):
        assert call(scratch_bytes=short) == (1, what + ": scratch too small (deodr_hip_chamfer_grid_scratch_bytes)"), short
    sizes = dict(vertices=24 * n * V, points=24 * n * P, point_weights=8 * n * P, vertex_weights=8 * V, params=24, terms=16 * n, loss=8 * n,
                 vertices_b=24 * n * V, nearest_vertex=4 * n * P, nearest_point=4 * n * V, scratch=need)  # fmt: skip
    refusal = (1, what + ": an output must not overlap an input, the scratch or another output")
    for out in ("terms", "loss", "vertices_b", "nearest_vertex", "nearest_point", "scratch"):
        for other in sizes:
            if other != out:
                for at in overlap_placements(base, sizes, out, other):
                    assert call(**{out: at}) == refusal, (out, other, hex(at))


def test_host_wrappers_check_their_tensors_before_the_library(monkeypatch):
    import torch

    from abi_cases import no_library
    from abi_cases import on_device as dev
    from deodr_amd import hip_renderer as hr

    monkeypatch.setattr(hr, "lib", no_library)
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    with pytest.raises(ValueError, match="vertices must be a ROCm tensor"):
        hr.chamfer_grid(f64(2, 5, 3), f64(2, 9, 3), f64(3), 0.1)
    with pytest.raises(ValueError, match="keys must be a ROCm tensor"):
        hr.sort_keys(i32(2, 9))

    Vt, Pt, Prm = dev(f64(2, 5, 3)), dev(f64(2, 9, 3)), dev(f64(3))
    for bad in (dev(f64(5, 3)), dev(f64(2, 5, 4)), dev(f64(0, 5, 3)), dev(f64(2, 0, 3))):
        with pytest.raises(ValueError, match=r"vertices must have shape \[n >= 1, V >= 1, 3\]"):
            hr.chamfer_grid(bad, Pt, Prm, 0.1)
    for bad in (dev(f64(9, 3)), dev(f64(3, 9, 3)), dev(f64(2, 9, 2)), None):
        with pytest.raises(ValueError, match=r"points must have shape \[2, P >= 1, 3\]"):
            hr.chamfer_grid(Vt, bad, Prm, 0.1)
    for bad in (0, 4, -1):
        with pytest.raises(ValueError, match="directions must be in 1 .. 3"):
            hr.chamfer_grid(Vt, Pt, Prm, 0.1, directions=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="cell_size must be finite and > 0"):
            hr.chamfer_grid(Vt, Pt, Prm, bad)
    with pytest.raises(ValueError, match="vertices must be float64"):
        hr.chamfer_grid(dev(f64(2, 5, 3).float()), Pt, Prm, 0.1)
    with pytest.raises(ValueError, match="points must be a ROCm tensor on the device of vertices"):
        hr.chamfer_grid(Vt, f64(2, 9, 3), Prm, 0.1)
    with pytest.raises(ValueError, match=r"params must have shape \[3\]"):
        hr.chamfer_grid(Vt, Pt, dev(f64(2)), 0.1)
    with pytest.raises(ValueError, match=r"point_weights must have shape \[2, 9\]"):
        hr.chamfer_grid(Vt, Pt, Prm, 0.1, point_weights=dev(f64(9)))
    with pytest.raises(ValueError, match=r"nearest_point must have shape \[2, 5\]"):
        hr.chamfer_grid(Vt, Pt, Prm, 0.1, nearest_point=dev(i32(2, 9)))
    with pytest.raises(ValueError, match="scratch must be uint8"):
        hr.chamfer_grid(Vt, Pt, Prm, 0.1, scratch=dev(torch.zeros(64)))
    for bad in (dev(i32(9)), dev(i32(0, 9)), dev(i32(2, 0)), dev(i32(2, 9, 1))):
        with pytest.raises(ValueError, match=r"keys must have shape \[n >= 1, N >= 1\]"):
            hr.sort_keys(bad)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="bits must be in 1 .. 32"):
            hr.sort_keys(dev(i32(2, 9)), bits=bad)
    with pytest.raises(ValueError, match="keys must be int32 or uint32"):
        hr.sort_keys(dev(i32(2, 9).long()))
    with pytest.raises(ValueError, match=r"order must have shape \[2, 9\]"):
        hr.sort_keys(dev(i32(2, 9)), order=dev(i32(9, 2)))
