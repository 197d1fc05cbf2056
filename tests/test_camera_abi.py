"""CPU checks of camera calibration at the C ABI (include/deodr_hip_camera.h; the header itself: tests/test_companion_headers.py): a library that
lacks a declared symbol is refused by name, every bad argument of the three launching entry points is refused with a message before any launch
(fake pointers, no GPU), the block rule and the scratch size behave as the header says, and the host wrappers refuse CPU tensors, wrong dtypes,
wrong shapes and non-contiguous tensors without reaching the library."""

import ctypes as C

import pytest


def test_a_library_that_lacks_a_declared_symbol_is_refused_by_name():
    import __graft_entry__ as g
    from deodr_amd import _abi

    more = _abi.parse(open(_abi.CAMERA_HEADER_PATH).read().replace("int deodr_hip_camera_abi_version(void);",
                                                                   "int deodr_hip_camera_abi_version(void);\nint deodr_hip_camera_not_there(int on);"),
                      "include/deodr_hip_camera.h")  # fmt: skip
    with pytest.raises(ImportError, match=r"deodr_hip_camera_not_there, which include/deodr_hip_camera\.h declares"):
        _abi.bind(C.CDLL(g.build_hip()), more)


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
    from abi_cases import entry, misaligned, nulls, overlap_placements
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    V, n = 100, 2
    base = dict(points=0x10000000, extrinsic=0x11000000, intrinsic=0x12000000, distortion=0x13000000, ij_b=0x14000000, depths_b=0x15000000,
                points_b=0x16000000, extrinsic_b=0x17000000, intrinsic_b=0x18000000, distortion_b=0x19000000, scratch=0x1A000000)  # fmt: skip

    project_b = entry(L, _abi.CAMERA_HEADER, "deodr_hip_camera_project_b", base, V=V, n=n, accumulate=0,
                      scratch_bytes=lambda a: L.deodr_hip_camera_scratch_bytes(a["V"], a["n"]))  # fmt: skip
    what = "camera_project_b"
    for bad in nulls(("points", "extrinsic", "intrinsic", "ij_b", "extrinsic_b", "intrinsic_b", "scratch")):
        rc, msg = project_b(**bad)
        assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (bad, msg)
    for bad in (dict(distortion=None), dict(distortion_b=None)):
        assert project_b(**bad) == (1, what + ": distortion and distortion_b go together"), bad
    for bad in (dict(n=0), dict(n=-1), dict(n=65)):
        assert project_b(**bad) == (1, what + ": n must be in 1 .. 64"), bad
    for bad in (dict(V=0), dict(V=-7), dict(V=2**24 + 1)):
        assert project_b(**bad) == (1, what + ": V must be in 1 .. 2^24"), bad
    for bad in misaligned(base, base, 4):
        assert project_b(**bad) == (1, what + ": misaligned pointer"), bad
    need = L.deodr_hip_camera_scratch_bytes(V, n)
    for short in (0, 8, need - 1):
        assert project_b(scratch_bytes=short) == (1, what + ": scratch too small (deodr_hip_camera_scratch_bytes)"), short
    # bytes: points and points_b 4800, ij_b 3200, depths_b 1600, extrinsic(_b) 192, intrinsic(_b) 144, distortion(_b) 80
    sizes = dict(points=4800, extrinsic=192, intrinsic=144, distortion=80, ij_b=3200, depths_b=1600, points_b=4800, extrinsic_b=192, intrinsic_b=144, distortion_b=80)
    for out in ("points_b", "extrinsic_b", "intrinsic_b", "distortion_b"):
        for inp in ("points", "extrinsic", "intrinsic", "distortion", "ij_b", "depths_b"):
            for at in overlap_placements(base, sizes, out, inp):
                assert project_b(**{out: at}) == (1, what + ": an output must not overlap an input"), (out, inp, hex(at))

    # ---- assemble / assemble_b
    ab = dict(quaternions=0x20000000, translations=0x21000000, focal=0x22000000, center=0x23000000, distortion_in=0x24000000, extrinsic=0x25000000,
              intrinsic=0x26000000, distortion_out=0x27000000)  # fmt: skip

    assemble = entry(L, _abi.CAMERA_HEADER, "deodr_hip_camera_assemble", ab, n=n, shared=1)
    bb = dict(quaternions=0x30000000, extrinsic_b=0x31000000, intrinsic_b=0x32000000, distortion_b=0x33000000, quaternions_b=0x34000000,
              translations_b=0x35000000, focal_b=0x36000000, center_b=0x37000000, distortion_in_b=0x38000000)  # fmt: skip
    assemble_b = entry(L, _abi.CAMERA_HEADER, "deodr_hip_camera_assemble_b", bb, n=n, shared=1)
    for call, what, args, required, pair in (
        (assemble, "camera_assemble", ab, ("quaternions", "translations", "focal", "center", "extrinsic", "intrinsic"), ("distortion_in", "distortion_out")),
        (assemble_b, "camera_assemble_b", bb, ("quaternions", "extrinsic_b", "intrinsic_b", "quaternions_b", "translations_b", "focal_b", "center_b"),
         ("distortion_b", "distortion_in_b")),
    ):  # fmt: skip
        for bad in nulls(required):
            rc, msg = call(**bad)
            assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (bad, msg)
        for p in pair:
            assert call(**{p: None}) == (1, f"{what}: {pair[0]} and {pair[1]} go together"), p
        for bad in (dict(n=0), dict(n=-1), dict(n=65)):
            assert call(**bad) == (1, what + ": n must be in 1 .. 64"), bad
        for bad in misaligned(args, args, 4):
            assert call(**bad) == (1, what + ": misaligned pointer"), bad
    # outputs against inputs (n = 2): extrinsic 192 bytes against quaternions 64, translations 48, focal / center 16 shared or 32 per view
    for shared, focal_bytes in ((1, 16), (0, 32)):
        for at in (ab["quaternions"], ab["quaternions"] + 56, ab["translations"] + 40, ab["focal"] + focal_bytes - 8, ab["center"] - 192 + 8):
            assert assemble(shared=shared, extrinsic=at) == (1, "camera_assemble: an output must not overlap an input"), (shared, hex(at))
        for at in (bb["quaternions"], bb["extrinsic_b"] + 184, bb["intrinsic_b"] - focal_bytes + 8, bb["distortion_b"] + 72):
            assert assemble_b(shared=shared, focal_b=at) == (1, "camera_assemble_b: an output must not overlap an input"), (shared, hex(at))


def test_host_wrappers_check_their_tensors_before_the_library(monkeypatch):
    import torch

    from abi_cases import no_library
    from abi_cases import on_device as dev
    from deodr_amd import hip_renderer as hr

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
