"""CPU checks of the point-to-surface distance at the C ABI (include/deodr_hip_surface.h; the header itself: tests/test_companion_headers.py): the
header states the rule it uses and why, its kernels add no value with an atomic and reuse the one vertex search, every bad argument of the
launching entry point is refused through its error code with a message before any launch (fake pointers, no GPU), the scratch size is 0 outside
the limits and the documented formula inside, the launch counts, the host wrapper refuses CPU tensors, wrong dtypes and wrong shapes without
reaching the library, and ``corner_table`` is checked and a wrong table refused on the host."""

import os

import numpy as np
import pytest

MAX_PAIRS = 2**32


def test_the_header_states_its_rule_and_the_host_side_has_the_operator_s_names():
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    text = open(_abi.SURFACE_HEADER_PATH).read()
    assert "deodr_hip_chamfer_segments" in text and "LOWEST face index" in text and "TIES ARE THE GENERIC CASE" in text  # the rule it uses, and why
    for name in ("surface_distance", "surface_scratch", "surface_launches", "SURFACE_ABI_VERSION", "SURFACE_MAX_PAIRS"):
        assert hasattr(hr, name), name
    assert hr.SURFACE_MAX_PAIRS == MAX_PAIRS


def test_the_kernels_add_no_value_atomically_and_reuse_the_vertex_search():
    import __graft_entry__ as g

    source = open(os.path.join(g.CSRC, "dr_surface.h")).read()
    assert "atomicAdd" not in source and "atomic_add" not in source  # no atomics on values (the tickets are grid_sum's, in dr_fronthalf.h)
    assert source.count("chamfer_walk_kernel") == 1 and "chamfer_walk_kernel<true, false>" in source  # (named in the overview alone: no second copy of that search)
    assert "chamfer_walk_kernel<true, false>" in open(os.path.join(g.CSRC, "dr_kernels.hip")).read().split("deodr_hip_surface_distance(const double")[1]


def test_scratch_is_zero_outside_the_limits_and_the_documented_formula_inside():
    import surface_reference as sr
    from deodr_amd import hip_renderer as hr

    need = hr.lib().deodr_hip_surface_distance_scratch_bytes
    for V, F, P, n in ((0, 5, 5, 3), (-1, 5, 5, 3), (5, 0, 5, 3), (5, -1, 5, 3), (5, 715827883, 1, 1), (5, 5, 0, 3), (5, 5, -1, 3), (5, 5, 5, 0), (5, 5, 5, -1),
                       (5, 5, 5, 65536), (9, 2**16, 2**16 + 1, 1), (9, 2**30, 2**30, 1)):  # fmt: skip
        assert need(V, F, P, n) == 0, (V, F, P, n)
    S = hr.chamfer_segments
    for V, F, P, n in ((1, 1, 1, 1), (526, 1048, 4096, 1), (526, 1048, 40000, 8), (10002, 20000, 40000, 8), (5, 7, 9, 65535), (9, 2**16, 2**16, 1),
                       (40, 65, 16129, 2), (40, 16129, 65, 2), (100, 3, 65537, 1), (50000, 65537, 3, 3)):  # fmt: skip
        Sp, Sg, Sv, M = S(P, F), S(F, P), S(V, P), hr.CHAMFER_MAX_BLOCKS
        want = 64 + 8 * (n * (16 * F + Sp * P + 6 * P + 9 * Sg * F + Sv * V + 2 * M) + (n * (Sp * P + Sv * V + P + 2) + 1) // 2)
        assert need(V, F, P, n) == want == sr.scratch_bytes(V, F, P, n), (V, F, P, n)
    sizes = [need(526, 1048, 4096, n) for n in (1, 2, 3, 4, 8)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)


def test_launch_counts():
    from deodr_amd import hip_renderer as hr

    for V, F, P, n, d, launches in ((5, 4, 7, 1, 3, 6), (5, 4, 7, 2, 1, 5), (5, 4, 7, 65535, 2, 2), (9, 2**16, 2**16, 1, 3, 6), (2**20, 2, 2**17, 1, 1, 5)):
        assert hr.surface_launches(V, F, P, n, d) == launches, (V, F, P, n, d)
    for bad in ((0, 4, 7, 1, 3), (5, 0, 7, 1, 3), (5, 4, 0, 1, 3), (5, 4, 7, 0, 3), (5, 4, 7, 65536, 3), (5, 4, 7, 1, 0), (5, 4, 7, 1, 4), (5, 4, 7, 1, -1),
                (9, 2**16, 2**16 + 1, 1, 3), (2**20, 2, 2**17, 1, 3), (2**20, 2, 2**17, 1, 2)):  # fmt: skip
        assert hr.surface_launches(*bad) == 0, bad


def test_bad_arguments_are_refused_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from abi_cases import entry, misaligned, nulls, overlap_placements
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    V, F, P, n = 41, 78, 250, 2  # (every array a multiple of 8 bytes long, so that the overlap probes below stay aligned)
    base = dict(vertices=0x10000000, faces=0x10800000, corner_offsets=0x10900000, corners=0x10A00000, points=0x11000000, point_weights=0x12000000,
                vertex_weights=0x13000000, params=0x14000000, terms=0x15000000, loss=0x16000000, vertices_b=0x17000000, nearest_face=0x18000000,
                barycentric=0x18800000, nearest_point=0x19000000, scratch=0x1A000000)  # fmt: skip
    optional = ("point_weights", "vertex_weights", "nearest_face", "barycentric", "nearest_point")
    words = ("faces", "corner_offsets", "corners", "nearest_face", "nearest_point")

    call = entry(L, _abi.SURFACE_HEADER, "deodr_hip_surface_distance", base, V=V, F=F, P=P, n=n, directions=3,
                 scratch_bytes=lambda a: L.deodr_hip_surface_distance_scratch_bytes(a["V"], a["F"], a["P"], a["n"]))  # fmt: skip
    what = "surface_distance"
    # a NULL required pointer (the optional ones may be NULL: such a call gets past every check only with real memory, not tried here)
    for bad in nulls(p for p in base if p not in optional):
        rc, msg = call(**bad)
        assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (bad, msg)
    for bad in (0, -1, -(2**31)):
        assert call(V=bad, scratch_bytes=1 << 20) == (1, what + ": V must be positive"), bad
        assert call(F=bad, scratch_bytes=1 << 20) == (1, what + ": F must be in 1 .. 715827882"), bad
        assert call(P=bad, scratch_bytes=1 << 20) == (1, what + ": P must be positive"), bad
    assert call(F=715827883, P=1, scratch_bytes=1 << 40) == (1, what + ": F must be in 1 .. 715827882")
    for bad in (0, -1, 65536):
        assert call(n=bad, scratch_bytes=1 << 20) == (1, what + ": n must be in 1 .. 65535"), bad
    for bad in (0, 4, -1, 7):
        assert call(directions=bad) == (1, what + ": directions must be in 1 .. 3"), bad
    assert call(F=2**16, P=2**16 + 1, n=1, scratch_bytes=1 << 40) == (1, what + ": F * P is above DEODR_HIP_SURFACE_MAX_PAIRS (the search is brute force)")
    assert call(F=715827882, P=2**31 - 1, n=1, scratch_bytes=1 << 40)[1].endswith("(the search is brute force)")
    for d in (2, 3):  # V * P above the Chamfer cap counts where mesh -> points is on, and only there
        assert call(V=2**20, F=2, P=2**17, n=1, directions=d, scratch_bytes=1 << 40) == (
            1, what + ": V * P is above DEODR_HIP_CHAMFER_MAX_PAIRS with mesh -> points on (the search is brute force)")  # fmt: skip
    assert L.deodr_hip_surface_distance_launches(2**20, 2, 2**17, 1, 1) == 5
    for bad in misaligned(base, words, 2):
        assert call(**bad) == (1, what + ": misaligned pointer"), bad
    for bad in misaligned(base, (p for p in base if p not in words), 4):
        assert call(**bad) == (1, what + ": misaligned pointer"), bad
    need = L.deodr_hip_surface_distance_scratch_bytes(V, F, P, n)
    for short in (0, 64, need - 1):
        assert call(scratch_bytes=short) == (1, what + ": scratch too small (deodr_hip_surface_distance_scratch_bytes)"), short
    sizes = dict(vertices=24 * n * V, faces=12 * F, corner_offsets=4 * (V + 1), corners=12 * F, points=24 * n * P, point_weights=8 * n * P,
                 vertex_weights=8 * V, params=24, terms=16 * n, loss=8 * n, vertices_b=24 * n * V, nearest_face=4 * n * P, barycentric=24 * n * P,
                 nearest_point=4 * n * V, scratch=need)  # fmt: skip
    refusal = (1, what + ": an output must not overlap an input, the scratch or another output")
    for out in ("terms", "loss", "vertices_b", "nearest_face", "barycentric", "nearest_point", "scratch"):
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
        hr.surface_distance(f64(2, 5, 3), i32(4, 3), i32(6), i32(12), f64(2, 9, 3), f64(3))

    Vt, Ft, Ot, Ct, Pt, Prm = dev(f64(2, 5, 3)), dev(i32(4, 3)), dev(i32(6)), dev(i32(12)), dev(f64(2, 9, 3)), dev(f64(3))
    call = lambda **kw: hr.surface_distance(**dict(dict(vertices=Vt, faces=Ft, corner_offsets=Ot, corners=Ct, points=Pt, params=Prm), **kw))
    for bad in (dev(f64(5, 3)), dev(f64(2, 5, 4)), dev(f64(0, 5, 3)), dev(f64(2, 0, 3))):
        with pytest.raises(ValueError, match=r"vertices must have shape \[n >= 1, V >= 1, 3\]"):
            call(vertices=bad)
    for bad in (dev(i32(4)), dev(i32(0, 3)), dev(i32(4, 2)), None):
        with pytest.raises(ValueError, match=r"faces must have shape \[F >= 1, 3\]"):
            call(faces=bad)
    for bad in (dev(f64(9, 3)), dev(f64(3, 9, 3)), dev(f64(2, 0, 3)), dev(f64(2, 9, 2)), None):
        with pytest.raises(ValueError, match=r"points must have shape \[2, P >= 1, 3\]"):
            call(points=bad)
    for bad in (0, 4, -1):
        with pytest.raises(ValueError, match="directions must be in 1 .. 3"):
            call(directions=bad)
    with pytest.raises(ValueError, match="vertices must be float64"):
        call(vertices=dev(f64(2, 5, 3).float()))
    with pytest.raises(ValueError, match="faces must be int32"):
        call(faces=dev(i32(4, 3).long()))
    with pytest.raises(ValueError, match="faces must be a ROCm tensor on the device of vertices"):
        call(faces=i32(4, 3))
    with pytest.raises(ValueError, match=r"corner_offsets must have shape \[6\]"):
        call(corner_offsets=dev(i32(5)))
    with pytest.raises(ValueError, match=r"corners must have shape \[12\]"):
        call(corners=dev(i32(4, 3)))
    with pytest.raises(ValueError, match="corners must be int32"):
        call(corners=dev(f64(12)))
    with pytest.raises(ValueError, match=r"params must have shape \[3\]"):
        call(params=dev(f64(2)))
    with pytest.raises(ValueError, match=r"point_weights must have shape \[2, 9\]"):
        call(point_weights=dev(f64(9)))
    with pytest.raises(ValueError, match=r"vertex_weights must have shape \[5\]"):
        call(vertex_weights=dev(f64(2, 5)))
    with pytest.raises(ValueError, match=r"terms must have shape \[2, 2\]"):
        call(terms=dev(f64(2)))
    with pytest.raises(ValueError, match=r"vertices_b must have shape \[2, 5, 3\]"):
        call(vertices_b=dev(f64(5, 3)))
    with pytest.raises(ValueError, match="nearest_face must be int32 or uint32"):
        call(nearest_face=dev(i32(2, 9).long()))
    with pytest.raises(ValueError, match=r"barycentric must have shape \[2, 9, 3\]"):
        call(barycentric=dev(f64(2, 9)))
    with pytest.raises(ValueError, match=r"nearest_point must have shape \[2, 5\]"):
        call(nearest_point=dev(i32(2, 9)))
    with pytest.raises(ValueError, match="scratch must be uint8"):
        call(scratch=dev(torch.zeros(64)))


def test_corner_table_is_checked_and_a_wrong_one_refused():
    from deodr_amd.surface import PointSurfaceTerm, check_corner_table, corner_table

    faces = np.array([[0, 1, 2], [2, 1, 3], [3, 3, 0]])
    offsets, corners = corner_table(faces, 6)  # vertices 4 and 5: no face
    assert offsets.tolist() == [0, 2, 4, 6, 9, 9, 9] and corners.tolist() == [0, 8, 1, 4, 2, 3, 5, 6, 7]
    check_corner_table(faces, 6, offsets, corners)
    swapped = corners.copy()
    swapped[[0, 1]] = swapped[[1, 0]]  # the entries of vertex 0 out of order
    for bad_offsets, bad_corners in ((offsets, swapped), (offsets[:-1], corners), (np.where(np.arange(7) == 1, 3, offsets), corners), (offsets, corners[:-1])):
        with pytest.raises(ValueError, match="not the transposed table of faces"):
            check_corner_table(faces, 6, bad_offsets, bad_corners)
    for bad, V in ((faces, 3), (-faces, 6), (faces[:, :2], 6), (faces[:0], 6), (faces.astype(np.float64), 6), (faces, 0)):
        with pytest.raises(ValueError, match="corner_table:"):
            corner_table(bad, V)
    cloud = np.random.RandomState(0).rand(30, 3)
    with pytest.raises(ValueError, match=r"entries of faces must be in \[0, 3\)"):
        PointSurfaceTerm(faces, 3, cloud, device="cpu")
    term = PointSurfaceTerm(faces, 6, cloud, device="cpu")
    assert term.faces.dtype == term.corners.dtype == term.corner_offsets.dtype and str(term.faces.dtype) == "torch.int32"
    assert (term.nb_faces, term.nb_vertices, term.nb_points, term.n) == (3, 6, 30, 1)
    import torch

    with pytest.raises(ValueError, match="the faces are those of 6 vertices, not of 7"):
        term.evaluate(torch.zeros((7, 3), dtype=torch.float64))
