"""CPU checks of the point-to-surface distance over a uniform grid of triangles at the C ABI (include_staged/deodr_hip_surface_grid.h; the header
itself: tests/test_staged_headers.py): its constants are the restatement's and the kernels', every bad argument is refused through its error
code with a message before any launch (fake pointers, no GPU), ``scratch_bytes`` / ``launches`` are the restatement's at and around their change
points and 0 for refused arguments, the kernels add no value atomically and reuse the parents' texts by calling, and the host wrappers refuse CPU
tensors, wrong dtypes and wrong shapes without reaching the library."""

import os
import re

import pytest

import chamfer_grid_reference as gr
import surface_grid_reference as sg


def test_the_constants_are_the_restatement_s_and_the_host_side_has_the_operators_names():
    from deodr_amd import hip_renderer as hr

    for name in ("surface_grid", "surface_grid_scratch", "surface_grid_launches", "SURFACE_GRID_ABI_VERSION", "SURFACE_GRID_NONE"):
        assert hasattr(hr, name), name
    assert hr.SURFACE_GRID_NONE == sg.NONE == hr.CHAMFER_GRID_NONE and hr.SURFACE_GRID_GATHER_FACES == sg.GATHER_FACES and hr.SURFACE_GRID_ABI_VERSION == 1
    assert (sg.RINGS, sg.MAX_ITEMS, sg.CELL_LIMIT) == (hr.CHAMFER_GRID_RINGS, hr.CHAMFER_GRID_MAX_ITEMS, hr.CHAMFER_GRID_CELL_LIMIT)  # by reference


def test_the_kernels_add_no_value_atomically_and_call_their_parents_texts():
    import __graft_entry__ as g

    source = open(os.path.join(g.CSRC, "dr_surface_grid.h")).read()
    assert "atomic" not in source.replace("floating-point atomics", "").replace("integer atomics", "")  # (the tickets are grid_sum's, in dr_fronthalf.h)
    assert "rocprim" not in source.lower()
    # reuse by calling: the closest-point sequence, the records, the cells, the hash, the exit margin and the table rule have one text each
    for name in ("surface_closest(", "surface_record(", "chamfer_grid_cell(", "chamfer_grid_hash(", "chamfer_grid_h(", "CG_EXIT_MARGIN", "chamfer_grid_table_bits(", "wave_sum("):
        assert name in source, name
    for text in ("SurfaceHit surface_closest", "int chamfer_grid_cell", "uint32_t chamfer_grid_hash", "CG_EXIT_MARGIN =", "__global__ __launch_bounds__(CHAMFER_BLOCK) void surface_points_kernel",
                 "void surface_vertices_kernel", "void chamfer_grid_search_kernel"):  # fmt: skip
        assert text not in source, text
    entry = open(os.path.join(g.CSRC, "dr_kernels.hip")).read().split("int deodr_hip_surface_grid(const double")[1].split("\n}\n")[0]
    for kernel in ("surface_grid_prep_kernel", "surface_grid_keys_kernel", "surface_grid_build_kernel", "surface_grid_search_kernel", "surface_points_kernel",
                   "surface_grid_gather_kernel", "surface_vertices_kernel", "chamfer_grid_keys_kernel", "chamfer_grid_build_kernel", "chamfer_grid_search_kernel"):  # fmt: skip
        assert entry.count("hipLaunchKernelGGL(" + kernel) == 1, kernel
    assert entry.count("sort_launch(") == 3 and "hipMemset" not in entry and "hipMemcpy" not in entry  # nothing but kernels, nothing read back


def test_sizes_at_and_around_their_change_points_and_zero_for_refused_arguments():
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    I = gr.SORT_ITEMS
    sizes = (1, 2, 32, 33, 128, 129, 255, 256, 257, 1048, I, I + 1, 16768, 65535, 65536, 2**18, 2**18 + 1, 2**24)
    for F in sizes:
        for P in sizes:
            for V, n in ((3, 1), (526, 3), (2**24, 1)):
                assert L.deodr_hip_surface_grid_scratch_bytes(V, F, P, n) == sg.scratch_bytes(V, F, P, n) > 0, (V, F, P, n)
                for directions in (1, 2, 3):
                    assert hr.surface_grid_launches(V, F, P, n, directions) == sg.launches(V, F, P, n, directions) > 0
    assert hr.surface_grid_launches(5, 255, 7, 1, 1) + 3 == hr.surface_grid_launches(5, 256, 7, 1, 1)  # the assignment needs a ninth bit: one pass more
    assert hr.surface_grid_launches(5, 128, 7, 1, 1) + 3 == hr.surface_grid_launches(5, 129, 7, 1, 1)  # 2^9 buckets of faces: one pass more
    assert hr.surface_grid_launches(5, 7, 128, 1, 2) + 3 == hr.surface_grid_launches(5, 7, 129, 1, 2)  # 2^9 buckets of points: one pass more
    assert hr.surface_grid_launches(5, 65535, 7, 1, 1) + 3 == hr.surface_grid_launches(5, 65536, 7, 1, 1)  # a seventeenth bit
    assert [hr.surface_grid_launches(526, 1048, 40000, 1, d) for d in (1, 2, 3)] == [19, 13, 31]
    M = gr.MAX_ITEMS
    for bad in ((0, 5, 5, 3), (-1, 5, 5, 3), (5, 0, 5, 3), (5, -1, 5, 3), (5, 5, 0, 3), (5, 5, -1, 3), (5, 5, 5, 0), (5, 5, 5, 65536), (M + 1, 5, 5, 1), (5, M + 1, 5, 1), (5, 5, M + 1, 1)):
        assert L.deodr_hip_surface_grid_scratch_bytes(*bad) == 0 == hr.surface_grid_launches(*bad, 3), bad
    for bad in (0, 4, -1):
        assert hr.surface_grid_launches(5, 7, 9, 1, bad) == 0
    # no cap on F * P and none on V * P: the VGA depth frame against the benchmark's sphere, which the brute-force operator refuses
    assert L.deodr_hip_surface_grid_scratch_bytes(10002, 20000, 307200, 1) > 0 and L.deodr_hip_surface_distance_scratch_bytes(10002, 20000, 307200, 1) == 0
    assert hr.surface_grid_launches(2**19, 2**20, 2**20, 1, 3) > 0 and hr.surface_launches(2**19, 2**20, 2**20, 1, 3) == 0


def test_bad_arguments_are_refused_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from abi_cases import entry, misaligned, nulls, overlap_placements
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    V, F, P, n = 41, 70, 250, 2
    base = dict(vertices=0x10000000, faces=0x10800000, corner_offsets=0x10900000, corners=0x10A00000, points=0x11000000, point_weights=0x12000000,
                vertex_weights=0x13000000, params=0x14000000, terms=0x15000000, loss=0x16000000, vertices_b=0x17000000, nearest_face=0x18000000,
                barycentric=0x18800000, nearest_point=0x19000000, scratch=0x1A000000)  # fmt: skip
    optional = ("point_weights", "vertex_weights", "nearest_face", "barycentric", "nearest_point")
    words = ("faces", "corner_offsets", "corners", "nearest_face", "nearest_point")

    call = entry(L, _abi.SURFACE_GRID_HEADER, "deodr_hip_surface_grid", base, V=V, F=F, P=P, n=n, directions=3, cell_size=0.1,
                 scratch_bytes=lambda a: L.deodr_hip_surface_grid_scratch_bytes(a["V"], a["F"], a["P"], a["n"]))  # fmt: skip
    what = "surface_grid"
    for bad in nulls(p for p in base if p not in optional):
        rc, msg = call(**bad)
        assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (bad, msg)
    for bad in (0, -1, -(2**31), gr.MAX_ITEMS + 1):
        for name in ("V", "F", "P"):
            assert call(**{name: bad}, scratch_bytes=1 << 40) == (1, f"{what}: {name} must be in 1 .. DEODR_HIP_CHAMFER_GRID_MAX_ITEMS"), (name, bad)
    for bad in (0, -1, 65536):
        assert call(n=bad, scratch_bytes=1 << 40) == (1, what + ": n must be in 1 .. 65535"), bad
    for bad in (0, 4, -1, 7):
        assert call(directions=bad) == (1, what + ": directions must be in 1 .. 3"), bad
    for bad in (0.0, -0.1, float("inf"), float("-inf"), float("nan")):
        assert call(cell_size=bad) == (1, what + ": cell_size must be finite and > 0"), bad
    for bad in misaligned(base, words, 2):
        assert call(**bad) == (1, what + ": misaligned pointer"), bad
    for bad in misaligned(base, (p for p in base if p not in words), 4):
        assert call(**bad) == (1, what + ": misaligned pointer"), bad
    need = L.deodr_hip_surface_grid_scratch_bytes(V, F, P, n)
    for short in (0, 64, need - 1):
        assert call(scratch_bytes=short) == (1, what + ": scratch too small (deodr_hip_surface_grid_scratch_bytes)"), short
    sizes = dict(vertices=24 * n * V, faces=12 * F, corner_offsets=4 * (V + 1), corners=12 * F, points=24 * n * P, point_weights=8 * n * P, vertex_weights=8 * V, params=24,
                 terms=16 * n, loss=8 * n, vertices_b=24 * n * V, nearest_face=4 * n * P, barycentric=24 * n * P, nearest_point=4 * n * V, scratch=need)  # fmt: skip
    refusal = (1, what + ": an output must not overlap an input, the scratch or another output")
    for out in ("terms", "loss", "vertices_b", "nearest_face", "barycentric", "nearest_point", "scratch"):
        for other in sizes:
            if other != out:
                for at in overlap_placements(base, sizes, out, other, unit=4 if out in words else 8):  # (every size here is a multiple of 8)
                    assert call(**{out: at}) == refusal, (out, other, hex(at))
    # neither pair cap of the parents: sizes they refuse pass the dimension checks here (and are then refused for their short scratch)
    assert call(F=2**20, P=2**20, V=2**19, scratch_bytes=64)[1] == what + ": scratch too small (deodr_hip_surface_grid_scratch_bytes)"


def test_host_wrappers_check_their_tensors_before_the_library(monkeypatch):
    import torch

    from abi_cases import no_library
    from abi_cases import on_device as dev
    from deodr_amd import hip_renderer as hr

    monkeypatch.setattr(hr, "lib", no_library)
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    with pytest.raises(ValueError, match="vertices must be a ROCm tensor"):
        hr.surface_grid(f64(2, 5, 3), i32(4, 3), i32(6), i32(12), f64(2, 9, 3), f64(3), 0.1)

    Vt, Ft, Ot, Ct, Pt, Prm = dev(f64(2, 5, 3)), dev(i32(4, 3)), dev(i32(6)), dev(i32(12)), dev(f64(2, 9, 3)), dev(f64(3))
    for bad in (dev(f64(5, 3)), dev(f64(2, 5, 4)), dev(f64(0, 5, 3)), dev(f64(2, 0, 3))):
        with pytest.raises(ValueError, match=r"vertices must have shape \[n >= 1, V >= 1, 3\]"):
            hr.surface_grid(bad, Ft, Ot, Ct, Pt, Prm, 0.1)
    for bad in (dev(i32(4)), dev(i32(0, 3)), dev(i32(4, 2)), None):
        with pytest.raises(ValueError, match=r"faces must have shape \[F >= 1, 3\]"):
            hr.surface_grid(Vt, bad, Ot, Ct, Pt, Prm, 0.1)
    for bad in (dev(f64(9, 3)), dev(f64(3, 9, 3)), dev(f64(2, 9, 2)), None):
        with pytest.raises(ValueError, match=r"points must have shape \[2, P >= 1, 3\]"):
            hr.surface_grid(Vt, Ft, Ot, Ct, bad, Prm, 0.1)
    for bad in (0, 4, -1):
        with pytest.raises(ValueError, match="directions must be in 1 .. 3"):
            hr.surface_grid(Vt, Ft, Ot, Ct, Pt, Prm, 0.1, directions=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="cell_size must be finite and > 0"):
            hr.surface_grid(Vt, Ft, Ot, Ct, Pt, Prm, bad)
    with pytest.raises(ValueError, match="vertices must be float64"):
        hr.surface_grid(dev(f64(2, 5, 3).float()), Ft, Ot, Ct, Pt, Prm, 0.1)
    with pytest.raises(ValueError, match="faces must be int32"):
        hr.surface_grid(Vt, dev(i32(4, 3).long()), Ot, Ct, Pt, Prm, 0.1)
    with pytest.raises(ValueError, match=r"corner_offsets must have shape \[6\]"):
        hr.surface_grid(Vt, Ft, dev(i32(5)), Ct, Pt, Prm, 0.1)
    with pytest.raises(ValueError, match=r"corners must have shape \[12\]"):
        hr.surface_grid(Vt, Ft, Ot, dev(i32(4, 3)), Pt, Prm, 0.1)
    with pytest.raises(ValueError, match="points must be a ROCm tensor on the device of vertices"):
        hr.surface_grid(Vt, Ft, Ot, Ct, f64(2, 9, 3), Prm, 0.1)
    with pytest.raises(ValueError, match=r"params must have shape \[3\]"):
        hr.surface_grid(Vt, Ft, Ot, Ct, Pt, dev(f64(2)), 0.1)
    with pytest.raises(ValueError, match=r"point_weights must have shape \[2, 9\]"):
        hr.surface_grid(Vt, Ft, Ot, Ct, Pt, Prm, 0.1, point_weights=dev(f64(9)))
    with pytest.raises(ValueError, match=r"barycentric must have shape \[2, 9, 3\]"):
        hr.surface_grid(Vt, Ft, Ot, Ct, Pt, Prm, 0.1, barycentric=dev(f64(2, 9)))
    with pytest.raises(ValueError, match=r"nearest_point must have shape \[2, 5\]"):
        hr.surface_grid(Vt, Ft, Ot, Ct, Pt, Prm, 0.1, nearest_point=dev(i32(2, 9)))
    with pytest.raises(ValueError, match="scratch must be uint8"):
        hr.surface_grid(Vt, Ft, Ot, Ct, Pt, Prm, 0.1, scratch=dev(torch.zeros(64)))
