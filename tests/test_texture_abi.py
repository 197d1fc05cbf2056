"""CPU checks of the companion header include/deodr_hip_texture.h (texture estimation): it parses with the parser of deodr_hip.h, every name it
declares is exported by the cross-compiled library and bound with the declared types, its version is 1 on both sides, and every bad argument
of the two calls is refused with a message before any launch (fake pointers, no GPU)."""

import ctypes as C
import re

import pytest

TEXTURE_FUNCTIONS = ["deodr_hip_texture_scratch_bytes", "deodr_hip_texture_smoothness", "deodr_hip_texture_step", "deodr_hip_texture_abi_version"]


def test_companion_header_parses_and_is_versioned_on_its_own():
    from deodr_amd import _abi

    h = _abi.TEXTURE_HEADER
    assert sorted(h.functions) == sorted(TEXTURE_FUNCTIONS)
    assert h.defines == {"DEODR_HIP_TEXTURE_ABI_VERSION": 1} and h.structs == {}
    assert h.name == "include/deodr_hip_texture.h"
    # nothing of it leaks into the main header's binding, which stays what the existing tests pin
    assert not set(h.functions) & set(_abi.HEADER.functions) and "DEODR_HIP_TEXTURE_ABI_VERSION" not in _abi.HEADER.defines
    # the prototypes as the header spells them, against the parsed types
    text = open(_abi.TEXTURE_HEADER_PATH).read()
    assert re.search(r"#define\s+DEODR_HIP_TEXTURE_ABI_VERSION\s+1\b", text)
    restype, argtypes = h.functions["deodr_hip_texture_smoothness"]
    assert restype is C.c_int
    assert argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    restype, argtypes = h.functions["deodr_hip_texture_step"]
    assert restype is C.c_int
    assert argtypes == [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_double] * 4 + [C.c_int, C.c_double, C.c_double, C.c_void_p]
    assert h.functions["deodr_hip_texture_scratch_bytes"] == (C.c_size_t, [C.c_int] * 3)
    assert h.functions["deodr_hip_texture_abi_version"] == (C.c_int, [])


def test_parser_errors_name_the_header_being_parsed():
    from deodr_amd import _abi

    text = open(_abi.TEXTURE_HEADER_PATH).read()
    with pytest.raises(ImportError, match=r"include/deodr_hip_texture\.h: no ctypes type for `float \*`"):
        _abi.parse(text.replace("double *energy", "float *energy"), "include/deodr_hip_texture.h")
    with pytest.raises(ImportError, match=r"include/deodr_hip\.h: "):  # the default name is the main header's
        _abi.parse(text.replace("double *energy", "float *energy"))


def test_library_exports_and_binds_every_name_of_the_companion_header():
    import __graft_entry__ as g
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    raw = C.CDLL(g.build_hip())
    for name in TEXTURE_FUNCTIONS:
        assert hasattr(raw, name), name
    assert raw.deodr_hip_texture_abi_version() == 1 == hr.TEXTURE_ABI_VERSION
    L = hr.lib()  # binds both headers
    for name, (restype, argtypes) in _abi.TEXTURE_HEADER.functions.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    # a library that lacks a declared symbol is refused by name, and the message names the companion header
    more = _abi.parse(open(_abi.TEXTURE_HEADER_PATH).read().replace("int deodr_hip_texture_abi_version(void);",
                                                                    "int deodr_hip_texture_abi_version(void);\nint deodr_hip_texture_not_there(int on);"),
                      "include/deodr_hip_texture.h")  # fmt: skip
    with pytest.raises(ImportError, match=r"deodr_hip_texture_not_there, which include/deodr_hip_texture\.h declares"):
        _abi.bind(C.CDLL(g.build_hip()), more)


def test_texture_calls_reject_bad_arguments_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    F32, F64, MAXC = _abi.HEADER.defines["DEODR_HIP_F32"], _abi.HEADER.defines["DEODR_HIP_F64"], _abi.HEADER.defines["DEODR_HIP_MAX_COLORS"]
    tex, grad, speed, energy, scratch = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
    need = L.deodr_hip_texture_scratch_bytes(64, 64, 3)
    assert need > 0 and need % 8 == 0

    def smooth(texture=tex, Ht=64, Wt=64, Cc=3, dtype=F32, gradient=grad, energy=energy, scratch=scratch, nbytes=need):
        rc = L.deodr_hip_texture_smoothness(texture, Ht, Wt, Cc, dtype, 1.0, gradient, energy, scratch, nbytes, None)
        return rc, L.deodr_hip_last_error().decode()

    def step(texture=tex, speed=speed, gradient=grad, Ht=64, Wt=64, Cc=3, dtype=F32, clamp=0, lo=0.0, hi=1.0):
        rc = L.deodr_hip_texture_step(texture, speed, gradient, Ht, Wt, Cc, dtype, 0.1, 0.0, 0.9, 0.05, clamp, lo, hi, None)
        return rc, L.deodr_hip_last_error().decode()

    for call, pointers in ((smooth, ("texture", "gradient", "energy")), (step, ("texture", "speed", "gradient"))):
        for p in pointers:
            rc, msg = call(**{p: None})
            assert rc == 1 and "== NULL" in msg, (call.__name__, p, msg)
        for bad in (dict(Ht=1), dict(Wt=1), dict(Ht=0), dict(Wt=-5)):
            assert call(**bad) == (1, "texture must be at least 2 x 2"), bad
        for bad in (dict(Cc=0), dict(Cc=MAXC + 1), dict(Cc=-1)):
            assert call(**bad) == (1, "nb_colors out of range"), bad
        for bad in (dict(dtype=2), dict(dtype=-1), dict(dtype=7)):
            assert call(**bad) == (1, "unknown dtype tag"), bad
        assert call(Ht=1 << 15, Wt=1 << 15, Cc=2)[1] == "texture larger than 2^30 elements"
        # gradient aliasing the texture: the same address, and a partial overlap (64 x 64 x 3 float32 = 49 152 bytes; F64 twice that)
        for g_at, dtype in ((tex, F32), (tex + 49152 - 4, F32), (tex - 49152 + 4, F32), (tex + 49152, F64)):
            rc, msg = call(gradient=g_at, dtype=dtype)
            assert rc == 1 and "gradient must not overlap texture" in msg, (g_at, msg)
        rc, msg = call(texture=tex + 2)
        assert rc == 1 and "misaligned" in msg
    assert smooth(scratch=None)[1].startswith("texture_smoothness: scratch too small")
    assert smooth(nbytes=need - 1)[1].startswith("texture_smoothness: scratch too small")
    assert step(speed=tex + 8)[1] == "texture_step: speed must not overlap texture or gradient"
    assert step(clamp=1, lo=1.0, hi=0.0)[1] == "texture_step: clamp_lo > clamp_hi"
    # the scratch size: 0 for dimensions no call takes
    for bad in ((1, 64, 3), (64, 1, 3), (64, 64, 0), (64, 64, MAXC + 1)):
        assert L.deodr_hip_texture_scratch_bytes(*bad) == 0, bad


def test_host_wrappers_check_their_tensors_before_the_library(monkeypatch):
    import torch

    from deodr_amd import hip_renderer as hr

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(hr, "lib", no_library)
    t = torch.zeros(8, 8, 3)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.texture_smoothness(t, torch.zeros_like(t), 1.0)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.texture_step(t, torch.zeros_like(t), torch.zeros_like(t), 0.1)
