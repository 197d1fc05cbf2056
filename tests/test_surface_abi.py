"""CPU checks of the companion header include/deodr_hip_surface.h (the point-to-surface distance): it parses with the parser of deodr_hip.h and
shares no name with the other thirteen headers, its prototypes are type by type what the header documents, every name it declares is exported by
the cross-compiled library and bound with the declared types, its version is 1 on both sides, it is on the list that decides whether the library is
stale, every bad argument of the launching entry point is refused through its error code with a message before any launch (fake pointers, no GPU),
the scratch size is 0 outside the limits and the documented formula inside, the launch counts, the host wrapper refuses CPU tensors, wrong dtypes
and wrong shapes without reaching the library, and ``corner_table`` is checked and a wrong table refused on the host."""

import ctypes as C
import os
import re

import numpy as np
import pytest

SURFACE_FUNCTIONS = ["deodr_hip_surface_distance", "deodr_hip_surface_distance_scratch_bytes", "deodr_hip_surface_distance_launches", "deodr_hip_surface_abi_version"]
MAX_PAIRS = 2**32


def test_companion_header_parses_and_is_versioned_on_its_own():
    from deodr_amd import _abi

    h = _abi.SURFACE_HEADER
    assert sorted(h.functions) == sorted(SURFACE_FUNCTIONS)
    assert h.defines == {"DEODR_HIP_SURFACE_ABI_VERSION": 1, "DEODR_HIP_SURFACE_MAX_PAIRS": MAX_PAIRS}
    assert h.structs == {} and h.name == "include/deodr_hip_surface.h"
    others = (_abi.HEADER, _abi.TEXTURE_HEADER, _abi.SUBDIV_HEADER, _abi.RETAINED_HEADER, _abi.BASIS_HEADER, _abi.CAMERA_HEADER, _abi.LIGHTING_HEADER,
              _abi.SKINNING_HEADER, _abi.PYRAMID_HEADER, _abi.SSIM_HEADER, _abi.SOLVE_HEADER, _abi.ARAP_HEADER, _abi.CHAMFER_HEADER)  # fmt: skip
    assert len(others) == 13
    for other in others:
        assert not set(h.functions) & set(other.functions) and not set(h.defines) & set(other.defines)
    text = open(_abi.SURFACE_HEADER_PATH).read()
    assert re.search(r"#define\s+DEODR_HIP_SURFACE_ABI_VERSION\s+1\b", text)
    assert "deodr_hip_chamfer_segments" in text and "LOWEST face index" in text and "TIES ARE THE GENERIC CASE" in text  # the rule it uses, and why
    p, i, z = C.c_void_p, C.c_int, C.c_size_t
    assert h.functions["deodr_hip_surface_distance"] == (i, [p, i, p, i, p, p, p, i, p, p, p, i, i, p, p, p, p, p, p, p, z, p])  # 22 parameters
    assert h.functions["deodr_hip_surface_distance_scratch_bytes"] == (z, [i, i, i, i])
    assert h.functions["deodr_hip_surface_distance_launches"] == (i, [i, i, i, i, i])
    assert h.functions["deodr_hip_surface_abi_version"] == (i, [])


def test_library_exports_and_binds_every_name_of_the_companion_header():
    import __graft_entry__ as g
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    raw = C.CDLL(g.build_hip())
    for name in SURFACE_FUNCTIONS:
        assert hasattr(raw, name), name
    assert raw.deodr_hip_surface_abi_version() == 1 == hr.SURFACE_ABI_VERSION
    L = hr.lib()  # binds every header
    for name, (restype, argtypes) in _abi.SURFACE_HEADER.functions.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    for name in ("surface_distance", "surface_scratch", "surface_launches", "SURFACE_ABI_VERSION", "SURFACE_MAX_PAIRS"):
        assert hasattr(hr, name), name
    assert hr.SURFACE_MAX_PAIRS == MAX_PAIRS


def test_the_header_is_on_the_list_that_decides_whether_the_library_is_stale():
    import inspect

    import __graft_entry__ as g
    from deodr_amd import _abi

    assert '"deodr_hip_surface.h"' in inspect.getsource(g.build_hip)
    assert ("SURFACE_HEADER", "deodr_hip_surface.h", False) in _abi._COMPANIONS
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
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    V, F, P, n = 41, 78, 250, 2  # (every array a multiple of 8 bytes long, so that the overlap probes below stay aligned)
    base = dict(vertices=0x10000000, faces=0x10800000, corner_offsets=0x10900000, corners=0x10A00000, points=0x11000000, point_weights=0x12000000,
                vertex_weights=0x13000000, params=0x14000000, terms=0x15000000, loss=0x16000000, vertices_b=0x17000000, nearest_face=0x18000000,
                barycentric=0x18800000, nearest_point=0x19000000, scratch=0x1A000000)  # fmt: skip
    optional = ("point_weights", "vertex_weights", "nearest_face", "barycentric", "nearest_point")
    words = ("faces", "corner_offsets", "corners", "nearest_face", "nearest_point")

    def call(V=V, F=F, P=P, n=n, directions=3, scratch_bytes=None, **changed):
        a = dict(base, **changed)
        need = L.deodr_hip_surface_distance_scratch_bytes(V, F, P, n)
        rc = L.deodr_hip_surface_distance(a["vertices"], V, a["faces"], F, a["corner_offsets"], a["corners"], a["points"], P, a["point_weights"],
                                          a["vertex_weights"], a["params"], n, directions, a["terms"], a["loss"], a["vertices_b"], a["nearest_face"],
                                          a["barycentric"], a["nearest_point"], a["scratch"], need if scratch_bytes is None else scratch_bytes, None)  # fmt: skip
        return rc, L.deodr_hip_last_error().decode()

    what = "surface_distance"
    for p in base:  # a NULL required pointer (the optional ones may be NULL: such a call gets past every check only with real memory, not tried here)
        if p not in optional:
            rc, msg = call(**{p: None})
            assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (p, msg)
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
    for p in words:
        assert call(**{p: base[p] + 2}) == (1, what + ": misaligned pointer"), p
    for p in base:
        if p not in words:
            assert call(**{p: base[p] + 4}) == (1, what + ": misaligned pointer"), p
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
                for at in (base[other], base[other] + sizes[other] - 8, base[other] - sizes[out] + 8):
                    assert call(**{out: at}) == refusal, (out, other, hex(at))


def test_host_wrapper_checks_its_tensors_before_the_library(monkeypatch):
    import torch

    from deodr_amd import hip_renderer as hr

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(hr, "lib", no_library)
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    with pytest.raises(ValueError, match="vertices must be a ROCm tensor"):
        hr.surface_distance(f64(2, 5, 3), i32(4, 3), i32(6), i32(12), f64(2, 9, 3), f64(3))

    class OnDevice(torch.Tensor):
        is_cuda = property(lambda self: True)
        device = property(lambda self: torch.device("cuda", 0))

    dev = lambda x: x.as_subclass(OnDevice)
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
