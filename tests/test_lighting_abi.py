"""CPU checks of the companion header include/deodr_hip_lighting.h (spherical-harmonic lighting, per-vertex albedo): it parses with the parser of
deodr_hip.h and shares no name with the other headers, its prototypes are type by type what the header documents, every name it declares is exported
by the cross-compiled library and bound with the declared types, its version is 1 on both sides, every bad argument of the two launching entry
points is refused with a message before any launch (fake pointers, no GPU), the block rule and the scratch size behave as the header says, and the
host wrappers refuse CPU tensors, wrong dtypes and wrong shapes without reaching the library."""

import ctypes as C
import re

import pytest

LIGHTING_FUNCTIONS = ["deodr_hip_sh_shade", "deodr_hip_sh_shade_b", "deodr_hip_sh_scratch_bytes", "deodr_hip_sh_blocks", "deodr_hip_lighting_abi_version"]


def test_companion_header_parses_and_is_versioned_on_its_own():
    from deodr_amd import _abi

    h = _abi.LIGHTING_HEADER
    assert sorted(h.functions) == sorted(LIGHTING_FUNCTIONS)
    assert h.defines == {"DEODR_HIP_LIGHTING_ABI_VERSION": 1} and h.structs == {}
    assert h.name == "include/deodr_hip_lighting.h"
    for other in (_abi.HEADER, _abi.TEXTURE_HEADER, _abi.SUBDIV_HEADER, _abi.RETAINED_HEADER, _abi.BASIS_HEADER, _abi.CAMERA_HEADER):
        assert not set(h.functions) & set(other.functions) and not set(h.defines) & set(other.defines)
    text = open(_abi.LIGHTING_HEADER_PATH).read()
    assert re.search(r"#define\s+DEODR_HIP_LIGHTING_ABI_VERSION\s+1\b", text)
    p, i, z = C.c_void_p, C.c_int, C.c_size_t
    assert h.functions["deodr_hip_sh_shade"] == (i, [p, p, p, p, p, i, p, i, i, p, p, i, i, i, p])  # 15 parameters
    assert h.functions["deodr_hip_sh_shade_b"] == (i, [p, p, p, p, p, i, p, i, i, p, p, p, p, p, i, p, z, i, i, i, p])  # 21 parameters
    assert h.functions["deodr_hip_sh_scratch_bytes"] == (z, [i, i, i])
    assert h.functions["deodr_hip_sh_blocks"] == (i, [i, i])
    assert h.functions["deodr_hip_lighting_abi_version"] == (i, [])


def test_library_exports_and_binds_every_name_of_the_companion_header():
    import __graft_entry__ as g
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    raw = C.CDLL(g.build_hip())
    for name in LIGHTING_FUNCTIONS:
        assert hasattr(raw, name), name
    assert raw.deodr_hip_lighting_abi_version() == 1 == hr.LIGHTING_ABI_VERSION
    L = hr.lib()  # binds every header
    for name, (restype, argtypes) in _abi.LIGHTING_HEADER.functions.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name


def test_the_header_is_on_the_list_that_decides_whether_the_library_is_stale():
    import inspect

    import __graft_entry__ as g

    assert '"deodr_hip_lighting.h"' in inspect.getsource(g.build_hip)


def test_blocks_and_scratch_follow_the_header():
    import lighting_reference as lr
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    k = lr.kernel_constants()
    cap, per_block = k["SH_MAX_BLOCKS"], k["FH_BLOCK"] // k["GATHER_LANES"]
    assert hr.SH_MAX_VIEWS == k["FIT_MAX_VIEWS"] and hr.SH_MAX_VERTICES == k["SH_MAX_VERTICES"] and hr.SH_COEFFS == k["SH_COEFFS"]
    for V, n in ((0, 1), (-1, 1), (2**24 + 1, 1), (10, 0), (10, -3), (10, 65)):  # zero outside the limits
        assert L.deodr_hip_sh_blocks(V, n) == 0 == hr.sh_blocks(V, n), (V, n)
        assert L.deodr_hip_sh_scratch_bytes(V, n, 3) == 0, (V, n)
    for C_ in (0, -1, 4):
        assert L.deodr_hip_sh_scratch_bytes(10, 1, C_) == 0
    sizes = sorted(set(list(range(1, 40000, 997)) + [2**e + d for e in range(4, 25) for d in (-1, 0, 1) if 2**e + d <= 2**24]))
    for n in (1, 2, 3, 9, 63, 64):
        previous, previous_bytes = 0, 0
        for V in sizes:
            B, nbytes = L.deodr_hip_sh_blocks(V, n), L.deodr_hip_sh_scratch_bytes(V, n, 3)
            assert B == min(cap, -(-V * n // per_block)) and B >= previous, (V, n, B)  # the rule the header states; non-decreasing in V
            assert nbytes == 64 + 8 * (n * V * 6 + 30 * B) and nbytes > previous_bytes, (V, n)
            assert L.deodr_hip_sh_scratch_bytes(V, n, 1) == nbytes - 8 * 2 * n * V
            previous, previous_bytes = B, nbytes
        assert L.deodr_hip_sh_blocks(2**24, n) == cap
    for V in (1, 31, 33, 1000):  # non-decreasing in n as well
        blocks = [L.deodr_hip_sh_blocks(V, n) for n in range(1, 65)]
        assert blocks == sorted(blocks)


def test_bad_arguments_are_refused_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    V, n, C_ = 100, 2, 3
    base = dict(posed=0x10000000, faces=0x11000000, vf_offsets=0x12000000, vf_corners=0x13000000, sh=0x14000000, albedo=0x15000000,
                luminosity=None, colors=0x17000000, posed_b=0x18000000, sh_b=0x19000000, albedo_b=0x1A000000, scratch=0x1B000000)  # fmt: skip

    def shade(V=V, n=n, C=C_, S=3, per_vertex=0, **changed):
        a = dict(base, **changed)
        rc = L.deodr_hip_sh_shade(a["posed"], a["faces"], a["vf_offsets"], a["vf_corners"], a["sh"], S, a["albedo"], per_vertex, C, a["luminosity"],
                                  a["colors"], V, n, 0, None)  # fmt: skip
        return rc, L.deodr_hip_last_error().decode()

    def shade_b(V=V, n=n, C=C_, S=3, per_vertex=0, accumulate=0, scratch_bytes=None, **changed):
        a = dict(base, **changed)  # (luminosity / colors stand for luminosity_b / colors_b)
        need = L.deodr_hip_sh_scratch_bytes(V, n, C)
        rc = L.deodr_hip_sh_shade_b(a["posed"], a["faces"], a["vf_offsets"], a["vf_corners"], a["sh"], S, a["albedo"], per_vertex, C, a["luminosity"],
                                    a["colors"], a["posed_b"], a["sh_b"], a["albedo_b"], accumulate, a["scratch"],
                                    need if scratch_bytes is None else scratch_bytes, V, n, 0, None)  # fmt: skip
        return rc, L.deodr_hip_last_error().decode()

    for call, what in ((shade, "sh_shade"), (shade_b, "sh_shade_b")):
        for p in ("posed", "faces", "vf_offsets", "vf_corners", "sh"):  # a NULL among the required pointers
            rc, msg = call(**{p: None})
            assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (p, msg)
        rc, msg = call(colors=None, albedo=None)  # no output (forward) / no incoming adjoint (backward)
        assert rc == 1 and msg.startswith(what + ": no output requested"), msg
        for bad in (dict(albedo=None), dict(colors=None, luminosity=0x16000000, S=1)):  # albedo without colors, and the reverse
            assert call(**bad) == (1, what + ": albedo and colors go together"), bad
        assert call(luminosity=0x16000000) == (1, what + ": luminosity needs S = 1")  # S = 3 here
        for bad in (dict(n=0), dict(n=-1), dict(n=65)):
            assert call(**bad) == (1, what + ": n must be in 1 .. 64"), bad
        for bad in (dict(V=0), dict(V=-7), dict(V=2**24 + 1)):
            assert call(**bad) == (1, what + ": V must be in 1 .. 2^24"), bad
        for bad in (dict(C=0), dict(C=4), dict(C=-1)):
            assert call(**bad) == (1, what + ": C must be in 1 .. 3"), bad
        for bad in (dict(S=0), dict(S=2), dict(S=4), dict(S=3, C=2)):
            assert call(**bad) == (1, what + ": S must be 1 or C"), bad
        mine = ("posed", "sh", "albedo", "colors") + (("posed_b", "sh_b", "albedo_b", "scratch") if call is shade_b else ())
        for p in mine:
            assert call(**{p: base[p] + 4}) == (1, what + ": misaligned pointer"), p
        for p in ("faces", "vf_offsets", "vf_corners"):  # 4-byte aligned
            assert call(**{p: base[p] + 2}) == (1, what + ": misaligned pointer"), p
        assert call(luminosity=0x16000004, S=1) == (1, what + ": misaligned pointer")
    # the adjoint's own refusals
    what = "sh_shade_b"
    assert shade_b(scratch=None) == (1, what + ": scratch == NULL")
    assert shade_b(posed_b=None, sh_b=None, albedo_b=None) == (1, what + ": no output requested (posed_b, sh_b, albedo_b)")
    assert shade_b(albedo=None, colors=None, luminosity=0x16000000, S=1) == (1, what + ": albedo_b without albedo")
    need = L.deodr_hip_sh_scratch_bytes(V, n, C_)
    for short in (0, 8, need - 1):
        assert shade_b(scratch_bytes=short) == (1, what + ": scratch too small (deodr_hip_sh_scratch_bytes)"), short
    # an output overlapping an input.  bytes: posed(_b) 4800, colors(_b) 4800, sh(_b) 216, albedo(_b) 24 (one colour) or 2400 (per vertex), vf_offsets 404
    sizes = dict(posed=4800, vf_offsets=404, faces=12, vf_corners=12, sh=216, albedo=24, colors=4800, posed_b=4800, sh_b=216, albedo_b=24)
    refusal = (1, what + ": an output must not overlap an input, the scratch or another output")
    for out in ("posed_b", "sh_b", "albedo_b"):
        for inp in ("posed", "faces", "vf_offsets", "vf_corners", "sh", "albedo", "colors"):
            for at in (base[inp], base[inp] + (sizes[inp] - 4) // 8 * 8, base[inp] - sizes[out] + 8):
                assert shade_b(**{out: at}) == refusal, (out, inp, hex(at))
        assert shade_b(**{out: base["scratch"] + 64}) == refusal and shade_b(**{out: base["scratch"] + need - 8}) == refusal, out
    assert shade_b(per_vertex=1, albedo_b=base["albedo"] + 2392) == refusal  # (a per-vertex albedo is V C doubles)
    assert shade_b(sh_b=base["posed_b"] + 8) == refusal and shade_b(albedo_b=base["sh_b"] + 208) == refusal
    assert shade_b(scratch=base["posed"] - 64) == refusal
    refusal = (1, "sh_shade: an output must not overlap an input or the other output")
    for inp in ("posed", "faces", "vf_offsets", "vf_corners", "sh", "albedo"):
        for at in (base[inp], base[inp] + (sizes[inp] - 4) // 8 * 8, base[inp] - 4800 + 8):
            assert shade(colors=at) == refusal, (inp, hex(at))
    for inp in ("posed", "faces", "vf_offsets", "vf_corners", "sh"):  # luminosity [n,V]: 1600 bytes
        for at in (base[inp], base[inp] - 1600 + 8):
            assert shade(colors=None, albedo=None, luminosity=at, S=1) == refusal, (inp, hex(at))
    assert shade(S=1, luminosity=base["colors"] + 4792) == refusal


def test_host_wrappers_check_their_tensors_before_the_library(monkeypatch):
    import torch

    from deodr_amd import hip_renderer as hr

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(hr, "lib", no_library)
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    n, V, T = 2, 10, 7
    posed, faces, off, corners, sh, albedo = f64(n, V, 3), i32(T, 3), i32(V + 1), i32(3 * T), f64(9, 3), f64(V, 3)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.sh_shade(posed, faces, off, corners, sh, albedo)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.sh_shade_b(posed, faces, off, corners, sh, albedo, colors_b=f64(n, V, 3))

    class OnDevice(torch.Tensor):
        is_cuda = property(lambda self: True)
        device = property(lambda self: torch.device("cuda", 0))

    dev = lambda x: x.as_subclass(OnDevice)
    P, F, O, Cn, SH, A = (dev(t) for t in (posed, faces, off, corners, sh, albedo))
    with pytest.raises(ValueError, match=r"posed must have shape \[1 <= n <= 64, 1 <= V <= 2\^24, 3\]"):
        hr.sh_shade(dev(f64(65, V, 3)), F, O, Cn, SH, A)
    with pytest.raises(ValueError, match=r"sh must have shape \[9\] or \[9, S\]"):
        hr.sh_shade(P, F, O, Cn, dev(f64(8, 3)), A)
    with pytest.raises(ValueError, match=r"albedo must have shape"):
        hr.sh_shade(P, F, O, Cn, SH, dev(f64(V + 1, 3)))
    with pytest.raises(ValueError, match=r"albedo must have shape"):
        hr.sh_shade(P, F, O, Cn, SH, dev(f64(4)))
    with pytest.raises(ValueError, match="sh must have 1 column or one per channel"):
        hr.sh_shade(P, F, O, Cn, dev(f64(9, 2)), A)
    with pytest.raises(ValueError, match="posed must be float64"):
        hr.sh_shade(dev(posed.float()), F, O, Cn, SH, A)
    with pytest.raises(ValueError, match="faces must be int32"):
        hr.sh_shade(P, dev(faces.long()), O, Cn, SH, A)
    with pytest.raises(ValueError, match=r"vf_offsets must have shape \[11\]"):
        hr.sh_shade(P, F, dev(i32(V)), Cn, SH, A)
    with pytest.raises(ValueError, match=r"vf_corners must have shape \[21\]"):
        hr.sh_shade(P, F, O, dev(i32(3 * T + 1)), SH, A)
    with pytest.raises(ValueError, match="posed must be contiguous"):
        hr.sh_shade(dev(f64(n, 3, V).transpose(1, 2)), F, O, Cn, SH, A)
    with pytest.raises(ValueError, match=r"colors must have shape \[2, 10, 3\]"):
        hr.sh_shade(P, F, O, Cn, SH, A, colors=dev(f64(n, V, 1)))
    with pytest.raises(ValueError, match="colors without albedo"):
        hr.sh_shade(P, F, O, Cn, dev(f64(9)), None, colors=dev(f64(n, V, 1)))
    with pytest.raises(ValueError, match=r"sh_b must have shape \[9, 3\]"):
        hr.sh_shade_b(P, F, O, Cn, SH, A, colors_b=dev(f64(n, V, 3)), sh_b=dev(f64(9)))
    with pytest.raises(ValueError, match=r"albedo_b must have shape \[10, 3\]"):
        hr.sh_shade_b(P, F, O, Cn, SH, A, colors_b=dev(f64(n, V, 3)), albedo_b=dev(f64(3)))
    with pytest.raises(ValueError, match="albedo_b without albedo"):
        hr.sh_shade_b(P, F, O, Cn, dev(f64(9)), None, luminosity_b=dev(f64(n, V)), albedo_b=dev(f64(3)))
    with pytest.raises(ValueError, match="accumulate needs"):
        hr.sh_shade_b(P, F, O, Cn, SH, A, colors_b=dev(f64(n, V, 3)), accumulate=True)
    with pytest.raises(ValueError, match="scratch must be uint8"):
        hr.sh_shade_b(P, F, O, Cn, SH, A, colors_b=dev(f64(n, V, 3)), scratch=dev(torch.zeros(64)))
