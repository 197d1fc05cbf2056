"""CPU checks of the companion header include/deodr_hip_pyramid.h (the multi-scale L2 data term): it parses with the parser of deodr_hip.h and shares no
name with the other headers, its prototypes are type by type what the header documents, every name it declares is exported by the cross-compiled
library and bound with the declared types, its version is 1 on both sides, every bad argument of the launching entry point is refused through its
error code with a message before any launch (fake pointers, no GPU), the scratch size is 0 outside the limits and monotone inside them, and the host
wrapper refuses CPU tensors, wrong dtypes and wrong shapes without reaching the library."""

import ctypes as C
import re

import pytest

PYRAMID_FUNCTIONS = ["deodr_hip_pyramid_l2", "deodr_hip_pyramid_scratch_bytes", "deodr_hip_pyramid_abi_version"]


def test_companion_header_parses_and_is_versioned_on_its_own():
    from deodr_amd import _abi

    h = _abi.PYRAMID_HEADER
    assert sorted(h.functions) == sorted(PYRAMID_FUNCTIONS)
    assert h.defines == {"DEODR_HIP_PYRAMID_ABI_VERSION": 1, "DEODR_HIP_PYRAMID_MAX_LEVELS": 8} and h.structs == {}
    assert h.name == "include/deodr_hip_pyramid.h"
    for other in (_abi.HEADER, _abi.TEXTURE_HEADER, _abi.SUBDIV_HEADER, _abi.RETAINED_HEADER, _abi.BASIS_HEADER, _abi.CAMERA_HEADER, _abi.LIGHTING_HEADER,
                  _abi.SKINNING_HEADER):  # fmt: skip
        assert not set(h.functions) & set(other.functions) and not set(h.defines) & set(other.defines)
    assert re.search(r"#define\s+DEODR_HIP_PYRAMID_ABI_VERSION\s+1\b", open(_abi.PYRAMID_HEADER_PATH).read())
    p, i, z = C.c_void_p, C.c_int, C.c_size_t
    assert h.functions["deodr_hip_pyramid_l2"] == (i, [p, p, p, i, i, i, i, i, i, p, p, p, p, p, z, p])  # 16 parameters
    assert h.functions["deodr_hip_pyramid_scratch_bytes"] == (z, [i, i, i, i, i])
    assert h.functions["deodr_hip_pyramid_abi_version"] == (i, [])


def test_library_exports_and_binds_every_name_of_the_companion_header():
    import __graft_entry__ as g
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr
    from deodr_amd import pyramid

    raw = C.CDLL(g.build_hip())
    for name in PYRAMID_FUNCTIONS:
        assert hasattr(raw, name), name
    assert raw.deodr_hip_pyramid_abi_version() == 1 == hr.PYRAMID_ABI_VERSION
    assert hr.PYRAMID_MAX_LEVELS == pyramid.MAX_LEVELS == 8
    L = hr.lib()  # binds every header
    for name, (restype, argtypes) in _abi.PYRAMID_HEADER.functions.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name


def test_the_header_is_on_the_list_that_decides_whether_the_library_is_stale():
    import inspect

    import __graft_entry__ as g

    assert '"deodr_hip_pyramid.h"' in inspect.getsource(g.build_hip)


def test_scratch_is_zero_outside_the_limits_and_monotone_inside():
    from deodr_amd import hip_renderer as hr

    need = hr.lib().deodr_hip_pyramid_scratch_bytes
    for n, H, W, Cn, levels in ((0, 8, 8, 3, 3), (-1, 8, 8, 3, 3), (1, 0, 8, 3, 3), (1, 8, 0, 3, 3), (1, 8, -8, 3, 3), (1, 8, 8, 0, 3), (1, 8, 8, -1, 3),
                                (1, 8, 8, 3, 0), (1, 8, 8, 3, 9), (1, 8, 8, 3, -1), (64, 2**15, 2**15, 16, 3)):  # fmt: skip
        assert need(n, H, W, Cn, levels) == 0, (n, H, W, Cn, levels)
    # levels <= 3: the partials of the tile kernel alone, whatever the frame
    assert need(1, 1, 1, 1, 1) == need(8, 1024, 1024, 4, 3) == 64 + 8 * 4 * 1024
    # levels > 3: + 5 doubles per region of 32 x 32 tiles and 1 + 2 C doubles per tile
    assert need(1, 16, 16, 4, 4) == 64 + 8 * (4 * 1024 + 5 + 4 * 9)
    assert need(3, 17, 23, 4, 5) == 64 + 8 * (4 * 1024 + 3 * 5 + 3 * 9 * 9)
    assert need(1, 520, 264, 2, 8) == 64 + 8 * (4 * 1024 + 3 * 2 * 5 + 65 * 33 * 5)
    base = (2, 100, 90, 3, 3)
    for axis, values in ((0, (1, 2, 3, 7, 64)), (1, (1, 8, 9, 100, 255, 256, 257, 1000)), (2, (1, 8, 9, 90, 256, 257, 4096)), (3, (1, 2, 3, 4, 5, 17)),
                         (4, (1, 2, 3, 4, 5, 6, 7, 8))):  # fmt: skip
        for levels in (3, 4, 8):
            sizes = []
            for v in values:
                args = list(base[:4]) + [levels]
                args[axis] = v
                sizes.append(need(*args))
            assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (axis, levels, sizes)


def test_bad_arguments_are_refused_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    n, H, W, Cn, levels = 2, 20, 30, 3, 5
    base = dict(image=0x10000000, obs=0x11000000, weights=0x12000000, level_weights=0x13000000, terms=0x14000000, loss=0x15000000, image_b=0x16000000,
                scratch=0x17000000)  # fmt: skip

    def call(n=n, H=H, W=W, Cn=Cn, levels=levels, dtype=hr._F64, scratch_bytes=None, **changed):
        a = dict(base, **changed)
        need = L.deodr_hip_pyramid_scratch_bytes(n, H, W, Cn, levels)
        rc = L.deodr_hip_pyramid_l2(a["image"], a["obs"], a["weights"], n, H, W, Cn, dtype, levels, a["level_weights"], a["terms"], a["loss"], a["image_b"],
                                    a["scratch"], need if scratch_bytes is None else scratch_bytes, None)  # fmt: skip
        return rc, L.deodr_hip_last_error().decode()

    what = "pyramid_l2"
    for p in ("image", "obs", "level_weights", "terms", "scratch"):  # a NULL that is not allowed
        rc, msg = call(**{p: None})
        assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (p, msg)
    for bad in (0, -1, 9, 100):
        assert call(levels=bad) == (1, what + ": levels must be in 1 .. 8"), bad
    for bad in (0, -3):
        assert call(Cn=bad) == (1, what + ": C must be >= 1"), bad
    for bad in (dict(n=0), dict(H=0), dict(W=-1)):
        assert call(**bad) == (1, what + ": n, H and W must be >= 1"), bad
    assert call(n=64, H=2**15, W=2**15, Cn=16) == (1, what + ": n H W C must be below 2^40")
    for bad in (2, -1, 7):
        assert call(dtype=bad) == (1, what + ": pixel_dtype must be DEODR_HIP_F32 or DEODR_HIP_F64"), bad
    for p in ("image", "obs", "weights", "image_b"):  # aligned to their element
        assert call(**{p: base[p] + 4}) == (1, what + ": misaligned pointer"), p
        assert call(dtype=hr._F32, **{p: base[p] + 2}) == (1, what + ": misaligned pointer"), p
    for p in ("level_weights", "terms", "loss", "scratch"):
        assert call(**{p: base[p] + 4}) == (1, what + ": misaligned pointer"), p
    need = L.deodr_hip_pyramid_scratch_bytes(n, H, W, Cn, levels)
    for short in (0, 64, need - 1):
        assert call(scratch_bytes=short) == (1, what + ": scratch too small (deodr_hip_pyramid_scratch_bytes)"), short
    frame, pixels = 8 * n * H * W * Cn, 8 * n * H * W
    sizes = dict(image=frame, obs=frame, weights=pixels, level_weights=8 * (levels + 1), terms=8 * (levels + 1), loss=8, image_b=frame, scratch=need)
    refusal = (1, what + ": an output must not overlap an input, the scratch or another output")
    for out in ("terms", "loss", "image_b", "scratch"):
        for other in sizes:
            if other != out:
                for at in (base[other], base[other] + sizes[other] - 8, base[other] - sizes[out] + 8):
                    assert call(**{out: at}) == refusal, (out, other, hex(at))
    # two things wrong at once: the checks run in the order above, and the first one speaks
    assert call(image=None, n=0) == (1, what + ": image, obs, level_weights, terms or scratch == NULL")
    assert call(n=0, dtype=7) == (1, what + ": n, H and W must be >= 1")
    assert call(dtype=7, image=base["image"] + 4) == (1, what + ": pixel_dtype must be DEODR_HIP_F32 or DEODR_HIP_F64")
    assert call(image=base["image"] + 4, scratch_bytes=need - 1) == (1, what + ": misaligned pointer")
    assert call(scratch_bytes=need - 1, terms=base["image"]) == (1, what + ": scratch too small (deodr_hip_pyramid_scratch_bytes)")


def test_host_wrapper_checks_its_tensors_before_the_library(monkeypatch):
    import torch

    from deodr_amd import hip_renderer as hr

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(hr, "lib", no_library)
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    image, lam = f64(2, 5, 6, 3), f64(4)
    with pytest.raises(ValueError, match="image must be a ROCm tensor"):
        hr.pyramid_l2(image, image, None, 3, lam)

    class OnDevice(torch.Tensor):
        is_cuda = property(lambda self: True)
        device = property(lambda self: torch.device("cuda", 0))

    dev = lambda x: x.as_subclass(OnDevice)
    I, O, Lw = dev(image), dev(f64(2, 5, 6, 3)), dev(lam)
    with pytest.raises(ValueError, match=r"image must have shape \[n >= 1, H >= 1, W >= 1, C >= 1\]"):
        hr.pyramid_l2(dev(f64(5, 6, 3)), O, None, 3, Lw)
    for levels in (0, 9):
        with pytest.raises(ValueError, match="levels must be in 1 .. 8"):
            hr.pyramid_l2(I, O, None, levels, Lw)
    with pytest.raises(ValueError, match=r"obs must have shape \[2, 5, 6, 3\]"):
        hr.pyramid_l2(I, dev(f64(2, 5, 6, 4)), None, 3, Lw)
    with pytest.raises(ValueError, match="obs must be float64"):
        hr.pyramid_l2(I, dev(image.float()), None, 3, Lw)
    with pytest.raises(ValueError, match="image must be float32 or float64"):
        hr.pyramid_l2(dev(image.half()), O, None, 3, Lw)
    with pytest.raises(ValueError, match=r"level_weights must have shape \[4\]"):
        hr.pyramid_l2(I, O, None, 3, dev(f64(3)))
    with pytest.raises(ValueError, match="level_weights must be float64"):
        hr.pyramid_l2(I, O, None, 3, dev(lam.float()))
    with pytest.raises(ValueError, match="level_weights must be a ROCm tensor"):
        hr.pyramid_l2(I, O, None, 3, lam)
    with pytest.raises(ValueError, match=r"weights must have shape \[2, 5, 6\]"):
        hr.pyramid_l2(I, O, dev(f64(5, 6)), 3, Lw)
    with pytest.raises(ValueError, match="weights must be contiguous"):
        hr.pyramid_l2(I, O, dev(f64(2, 6, 5).transpose(1, 2)), 3, Lw)
    with pytest.raises(ValueError, match=r"terms must have shape \[4\]"):
        hr.pyramid_l2(I, O, None, 3, Lw, terms=dev(f64(5)))
    with pytest.raises(ValueError, match=r"image_b must have shape \[2, 5, 6, 3\]"):
        hr.pyramid_l2(I, O, None, 3, Lw, image_b=dev(f64(2, 5, 6)))
    with pytest.raises(ValueError, match="scratch must be uint8"):
        hr.pyramid_l2(I, O, None, 3, Lw, scratch=dev(torch.zeros(64)))
