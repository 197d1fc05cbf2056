"""CPU checks of the companion header include/deodr_hip_camera.h (camera calibration): it parses with the parser of deodr_hip.h and shares no name
with the other headers, its prototypes are type by type what the header documents, every name it declares is exported by the cross-compiled library
and bound with the declared types, its version is 1 on both sides, every bad argument of the three launching entry points is refused with a message
before any launch (fake pointers, no GPU), the block rule and the scratch size behave as the header says, and the host wrappers refuse CPU tensors,
wrong dtypes, wrong shapes and non-contiguous tensors without reaching the library."""

import ctypes as C
import re

import pytest

CAMERA_FUNCTIONS = ["deodr_hip_camera_project_b", "deodr_hip_camera_blocks", "deodr_hip_camera_scratch_bytes", "deodr_hip_camera_assemble",
                    "deodr_hip_camera_assemble_b", "deodr_hip_camera_abi_version"]  # fmt: skip


def test_companion_header_parses_and_is_versioned_on_its_own():
    from deodr_amd import _abi

    h = _abi.CAMERA_HEADER
    assert sorted(h.functions) == sorted(CAMERA_FUNCTIONS)
    assert h.defines == {"DEODR_HIP_CAMERA_ABI_VERSION": 1} and h.structs == {}
    assert h.name == "include/deodr_hip_camera.h"
    for other in (_abi.HEADER, _abi.TEXTURE_HEADER, _abi.SUBDIV_HEADER, _abi.RETAINED_HEADER, _abi.BASIS_HEADER):  # disjoint from the other five
        assert not set(h.functions) & set(other.functions) and not set(h.defines) & set(other.defines)
    text = open(_abi.CAMERA_HEADER_PATH).read()
    assert re.search(r"#define\s+DEODR_HIP_CAMERA_ABI_VERSION\s+1\b", text)
    p, i, z = C.c_void_p, C.c_int, C.c_size_t
    assert h.functions["deodr_hip_camera_project_b"] == (i, [p, p, p, p, p, p, p, p, p, p, i, i, i, p, z, p])
    assert h.functions["deodr_hip_camera_blocks"] == (i, [i, i])
    assert h.functions["deodr_hip_camera_scratch_bytes"] == (z, [i, i])
    assert h.functions["deodr_hip_camera_assemble"] == (i, [p, p, p, p, p, i, p, p, p, i, p])
    assert h.functions["deodr_hip_camera_assemble_b"] == (i, [p, p, p, p, i, p, p, p, p, p, i, p])
    assert h.functions["deodr_hip_camera_abi_version"] == (i, [])


def test_library_exports_and_binds_every_name_of_the_companion_header():
    import __graft_entry__ as g
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    raw = C.CDLL(g.build_hip())
    for name in CAMERA_FUNCTIONS:
        assert hasattr(raw, name), name
    assert raw.deodr_hip_camera_abi_version() == 1 == hr.CAMERA_ABI_VERSION
    L = hr.lib()  # binds every header
    for name, (restype, argtypes) in _abi.CAMERA_HEADER.functions.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    more = _abi.parse(open(_abi.CAMERA_HEADER_PATH).read().replace("int deodr_hip_camera_abi_version(void);",
                                                                   "int deodr_hip_camera_abi_version(void);\nint deodr_hip_camera_not_there(int on);"),
                      "include/deodr_hip_camera.h")  # fmt: skip
    with pytest.raises(ImportError, match=r"deodr_hip_camera_not_there, which include/deodr_hip_camera\.h declares"):
        _abi.bind(C.CDLL(g.build_hip()), more)


def test_the_header_is_on_the_list_that_decides_whether_the_library_is_stale():
    import inspect

    import __graft_entry__ as g

    assert '"deodr_hip_camera.h"' in inspect.getsource(g.build_hip)


def test_blocks_and_scratch_follow_the_header():
    import camera_reference as cr
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    constants = cr.kernel_constants()
    cap = constants["CAMERA_MAX_BLOCKS"]
    # the limits the host wrappers state are the kernel headers'
    assert hr.CAMERA_MAX_VIEWS == constants["FIT_MAX_VIEWS"] and hr.CAMERA_MAX_VERTICES == constants["CAMERA_MAX_VERTICES"]
    assert L.deodr_hip_camera_blocks(hr.CAMERA_MAX_VERTICES, hr.CAMERA_MAX_VIEWS) >= 1
    for V, n in ((0, 1), (-1, 1), (2**24 + 1, 1), (10, 0), (10, -3), (10, 65)):
        assert L.deodr_hip_camera_blocks(V, n) == 0 == hr.camera_blocks(V, n), (V, n)
        assert L.deodr_hip_camera_scratch_bytes(V, n) == 0, (V, n)
    sizes = sorted(set(list(range(1, 40000, 997)) + [2**e + d for e in range(6, 25) for d in (-1, 0, 1) if 2**e + d <= 2**24]))
    for n in (1, 2, 3, 4, 5, 9, 63, 64):
        previous, previous_bytes = 0, 0
        for V in sizes:
            B, nbytes = L.deodr_hip_camera_blocks(V, n), L.deodr_hip_camera_scratch_bytes(V, n)
            assert 1 <= B <= cap and B >= previous, (V, n, B, previous)  # at least 1, non-decreasing in V, capped
            assert nbytes >= 4 * n + 8 * 23 * n * B and nbytes >= previous_bytes and (B == previous or nbytes > previous_bytes), (V, n)  # grows with it
            previous, previous_bytes = B, nbytes
        assert L.deodr_hip_camera_blocks(1, n) == 1  # small meshes are one workgroup per view
        assert L.deodr_hip_camera_blocks(2**24, n) * n >= 256  # large ones fill the chip
    assert L.deodr_hip_camera_blocks(2**24, 1) == cap
    assert L.deodr_hip_camera_scratch_bytes(5000, 64) > L.deodr_hip_camera_scratch_bytes(5000, 4)


def test_bad_arguments_are_refused_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    V, n = 100, 2
    base = dict(points=0x10000000, extrinsic=0x11000000, intrinsic=0x12000000, distortion=0x13000000, ij_b=0x14000000, depths_b=0x15000000,
                points_b=0x16000000, extrinsic_b=0x17000000, intrinsic_b=0x18000000, distortion_b=0x19000000, scratch=0x1A000000)  # fmt: skip

    def project_b(V=V, n=n, accumulate=0, scratch_bytes=None, **changed):
        a = dict(base, **changed)
        need = L.deodr_hip_camera_scratch_bytes(V, n)
        rc = L.deodr_hip_camera_project_b(a["points"], a["extrinsic"], a["intrinsic"], a["distortion"], a["ij_b"], a["depths_b"], a["points_b"],
                                          a["extrinsic_b"], a["intrinsic_b"], a["distortion_b"], V, n, accumulate, a["scratch"],
                                          need if scratch_bytes is None else scratch_bytes, None)  # fmt: skip
        return rc, L.deodr_hip_last_error().decode()

    what = "camera_project_b"
    for p in ("points", "extrinsic", "intrinsic", "ij_b", "extrinsic_b", "intrinsic_b", "scratch"):
        rc, msg = project_b(**{p: None})
        assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (p, msg)
    for bad in (dict(distortion=None), dict(distortion_b=None)):
        assert project_b(**bad) == (1, what + ": distortion and distortion_b go together"), bad
    for bad in (dict(n=0), dict(n=-1), dict(n=65)):
        assert project_b(**bad) == (1, what + ": n must be in 1 .. 64"), bad
    for bad in (dict(V=0), dict(V=-7), dict(V=2**24 + 1)):
        assert project_b(**bad) == (1, what + ": V must be in 1 .. 2^24"), bad
    for p in base:
        assert project_b(**{p: base[p] + 4}) == (1, what + ": misaligned pointer"), p
    need = L.deodr_hip_camera_scratch_bytes(V, n)
    for short in (0, 8, need - 1):
        assert project_b(scratch_bytes=short) == (1, what + ": scratch too small (deodr_hip_camera_scratch_bytes)"), short
    # bytes: points and points_b 4800, ij_b 3200, depths_b 1600, extrinsic(_b) 192, intrinsic(_b) 144, distortion(_b) 80
    sizes = dict(points=4800, extrinsic=192, intrinsic=144, distortion=80, ij_b=3200, depths_b=1600, points_b=4800, extrinsic_b=192, intrinsic_b=144, distortion_b=80)
    for out in ("points_b", "extrinsic_b", "intrinsic_b", "distortion_b"):
        for inp in ("points", "extrinsic", "intrinsic", "distortion", "ij_b", "depths_b"):
            for at in (base[inp], base[inp] + sizes[inp] - 8, base[inp] - sizes[out] + 8):
                assert project_b(**{out: at}) == (1, what + ": an output must not overlap an input"), (out, inp, hex(at))

    # ---- assemble / assemble_b
    ab = dict(quaternions=0x20000000, translations=0x21000000, focal=0x22000000, center=0x23000000, distortion_in=0x24000000, extrinsic=0x25000000,
              intrinsic=0x26000000, distortion_out=0x27000000)  # fmt: skip

    def assemble(n=n, shared=1, **changed):
        a = dict(ab, **changed)
        rc = L.deodr_hip_camera_assemble(a["quaternions"], a["translations"], a["focal"], a["center"], a["distortion_in"], shared, a["extrinsic"],
                                         a["intrinsic"], a["distortion_out"], n, None)  # fmt: skip
        return rc, L.deodr_hip_last_error().decode()

    bb = dict(quaternions=0x30000000, extrinsic_b=0x31000000, intrinsic_b=0x32000000, distortion_b=0x33000000, quaternions_b=0x34000000,
              translations_b=0x35000000, focal_b=0x36000000, center_b=0x37000000, distortion_in_b=0x38000000)  # fmt: skip

    def assemble_b(n=n, shared=1, **changed):
        a = dict(bb, **changed)
        rc = L.deodr_hip_camera_assemble_b(a["quaternions"], a["extrinsic_b"], a["intrinsic_b"], a["distortion_b"], shared, a["quaternions_b"],
                                           a["translations_b"], a["focal_b"], a["center_b"], a["distortion_in_b"], n, None)  # fmt: skip
        return rc, L.deodr_hip_last_error().decode()

    for call, what, args, required, pair in (
        (assemble, "camera_assemble", ab, ("quaternions", "translations", "focal", "center", "extrinsic", "intrinsic"), ("distortion_in", "distortion_out")),
        (assemble_b, "camera_assemble_b", bb, ("quaternions", "extrinsic_b", "intrinsic_b", "quaternions_b", "translations_b", "focal_b", "center_b"),
         ("distortion_b", "distortion_in_b")),
    ):  # fmt: skip
        for p in required:
            rc, msg = call(**{p: None})
            assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (p, msg)
        for p in pair:
            assert call(**{p: None}) == (1, f"{what}: {pair[0]} and {pair[1]} go together"), p
        for bad in (dict(n=0), dict(n=-1), dict(n=65)):
            assert call(**bad) == (1, what + ": n must be in 1 .. 64"), bad
        for p in args:
            assert call(**{p: args[p] + 4}) == (1, what + ": misaligned pointer"), p
    # outputs against inputs (n = 2): extrinsic 192 bytes against quaternions 64, translations 48, focal / center 16 shared or 32 per view
    for shared, focal_bytes in ((1, 16), (0, 32)):
        for at in (ab["quaternions"], ab["quaternions"] + 56, ab["translations"] + 40, ab["focal"] + focal_bytes - 8, ab["center"] - 192 + 8):
            assert assemble(shared=shared, extrinsic=at) == (1, "camera_assemble: an output must not overlap an input"), (shared, hex(at))
        for at in (bb["quaternions"], bb["extrinsic_b"] + 184, bb["intrinsic_b"] - focal_bytes + 8, bb["distortion_b"] + 72):
            assert assemble_b(shared=shared, focal_b=at) == (1, "camera_assemble_b: an output must not overlap an input"), (shared, hex(at))


def test_host_wrappers_check_their_tensors_before_the_library(monkeypatch):
    import torch

    from deodr_amd import hip_renderer as hr

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(hr, "lib", no_library)
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    n, V = 2, 10
    points, E, K, D, ij_b = f64(n, V, 3), f64(n, 3, 4), f64(n, 3, 3), f64(n, 5), f64(n, V, 2)
    q, t, f, c = f64(n, 4), f64(n, 3), f64(2), f64(2)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.camera_project_b(points, E, K, D, ij_b)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.camera_assemble(q, t, f, c)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.camera_assemble_b(q, E, K)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.camera_project_b(points.numpy(), E.numpy(), K, D, ij_b)

    # the checks behind the device check, on tensors that only claim to be on the device
    class OnDevice(torch.Tensor):
        is_cuda = property(lambda self: True)
        device = property(lambda self: torch.device("cuda", 0))

    dev = lambda x: x.as_subclass(OnDevice)
    P, E_, K_, D_, G = dev(points), dev(E), dev(K), dev(D), dev(ij_b)
    with pytest.raises(ValueError, match=r"extrinsic must have shape \[1 <= n <= 64, 3, 4\]"):
        hr.camera_project_b(P, dev(f64(65, 3, 4)), K_, D_, G)
    with pytest.raises(ValueError, match=r"extrinsic must have shape"):
        hr.camera_project_b(P, dev(f64(3, 4)), K_, D_, G)
    with pytest.raises(ValueError, match=r"points must have shape \[2, 1 <= V <= 2\^24, 3\]"):
        hr.camera_project_b(dev(f64(3, V, 3)), E_, K_, D_, G)
    with pytest.raises(ValueError, match=r"points must have shape"):
        hr.camera_project_b(dev(f64(n, 0, 3)), E_, K_, D_, G)
    with pytest.raises(ValueError, match="extrinsic must be float64"):
        hr.camera_project_b(P, dev(E.float()), K_, D_, G)
    with pytest.raises(ValueError, match="points must be float64"):
        hr.camera_project_b(dev(points.float()), E_, K_, D_, G)
    with pytest.raises(ValueError, match="points must be contiguous"):
        hr.camera_project_b(dev(f64(n, 3, V).transpose(1, 2)), E_, K_, D_, G)
    with pytest.raises(ValueError, match=r"intrinsic must have shape \[2, 3, 3\]"):
        hr.camera_project_b(P, E_, dev(f64(1, 3, 3)), D_, G)
    with pytest.raises(ValueError, match=r"ij_b must have shape \[2, 10, 2\]"):
        hr.camera_project_b(P, E_, K_, D_, dev(f64(n, V, 3)))
    with pytest.raises(ValueError, match=r"distortion must have shape \[2, 5\]"):
        hr.camera_project_b(P, E_, K_, dev(f64(5)), G)
    with pytest.raises(ValueError, match=r"depths_b must have shape \[2, 10\]"):
        hr.camera_project_b(P, E_, K_, D_, G, depths_b=dev(f64(n, V, 1)))
    with pytest.raises(ValueError, match="intrinsic_b must be contiguous"):
        hr.camera_project_b(P, E_, K_, D_, G, intrinsic_b=dev(f64(3, 3, n).permute(2, 0, 1)))
    with pytest.raises(ValueError, match="distortion_b without distortion"):
        hr.camera_project_b(P, E_, K_, None, G, distortion_b=D_)
    with pytest.raises(ValueError, match="accumulate needs"):
        hr.camera_project_b(P, E_, K_, D_, G, accumulate=True)
    with pytest.raises(ValueError, match="scratch must be uint8"):
        hr.camera_project_b(P, E_, K_, D_, G, scratch=dev(torch.zeros(64)))
    Q, T, F, Cc = dev(q), dev(t), dev(f), dev(c)
    with pytest.raises(ValueError, match=r"quaternions must have shape \[1 <= n <= 64, 4\]"):
        hr.camera_assemble(dev(f64(65, 4)), T, F, Cc)
    with pytest.raises(ValueError, match=r"translations must have shape \[2, 3\]"):
        hr.camera_assemble(Q, dev(f64(3, 3)), F, Cc)
    with pytest.raises(ValueError, match=r"focal must have shape \[2, 2\]"):
        hr.camera_assemble(Q, T, F, Cc, shared=False)
    with pytest.raises(ValueError, match=r"center must have shape \[2\]"):
        hr.camera_assemble(Q, T, F, dev(f64(n, 2)), shared=True)
    with pytest.raises(ValueError, match="focal must be float64"):
        hr.camera_assemble(Q, T, dev(f.float()), Cc)
    with pytest.raises(ValueError, match=r"distortion must have shape \[5\]"):
        hr.camera_assemble(Q, T, F, Cc, dev(f64(n, 5)))
    with pytest.raises(ValueError, match="quaternions must be contiguous"):
        hr.camera_assemble(dev(f64(4, n).T), T, F, Cc)
    with pytest.raises(ValueError, match=r"extrinsic_b must have shape \[2, 3, 4\]"):
        hr.camera_assemble_b(Q, dev(f64(n, 4, 3)), K_)
    with pytest.raises(ValueError, match="intrinsic_b must be float64"):
        hr.camera_assemble_b(Q, E_, dev(K.float()))
    with pytest.raises(ValueError, match=r"distortion_b must have shape \[2, 5\]"):
        hr.camera_assemble_b(Q, E_, K_, dev(f64(5)))
    with pytest.raises(ValueError, match=r"focal_b must have shape \[2\]"):
        hr.camera_assemble_b(Q, E_, K_, out=(None, None, dev(f64(n, 2)), None, None))
