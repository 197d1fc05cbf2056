"""CPU checks of texture estimation at the C ABI (include/deodr_hip_texture.h; the header itself: tests/test_companion_headers.py): the parser's
errors name the header being parsed, a library that lacks a declared symbol is refused by name, and every bad argument of the two calls is refused
with a message before any launch (fake pointers, no GPU)."""

import ctypes as C

import pytest


def test_parser_errors_name_the_header_being_parsed():
    from deodr_amd import _abi

    text = open(_abi.TEXTURE_HEADER_PATH).read()
    with pytest.raises(ImportError, match=r"include/deodr_hip_texture\.h: no ctypes type for `float \*`"):
        _abi.parse(text.replace("double *energy", "float *energy"), "include/deodr_hip_texture.h")
    with pytest.raises(ImportError, match=r"include/deodr_hip\.h: "):  # the default name is the main header's
        _abi.parse(text.replace("double *energy", "float *energy"))


def test_a_library_that_lacks_a_declared_symbol_is_refused_by_name():
    import __graft_entry__ as g
    from deodr_amd import _abi

    # a library that lacks a declared symbol is refused by name, and the message names the companion header
    more = _abi.parse(open(_abi.TEXTURE_HEADER_PATH).read().replace("int deodr_hip_texture_abi_version(void);",
                                                                    "int deodr_hip_texture_abi_version(void);\nint deodr_hip_texture_not_there(int on);"),
                      "include/deodr_hip_texture.h")  # fmt: skip
    with pytest.raises(ImportError, match=r"deodr_hip_texture_not_there, which include/deodr_hip_texture\.h declares"):
        _abi.bind(C.CDLL(g.build_hip()), more)


def test_texture_calls_reject_bad_arguments_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from abi_cases import entry, nulls
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    F32, F64, MAXC = _abi.HEADER.defines["DEODR_HIP_F32"], _abi.HEADER.defines["DEODR_HIP_F64"], _abi.HEADER.defines["DEODR_HIP_MAX_COLORS"]
    tex, grad, speed, energy, scratch = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
    need = L.deodr_hip_texture_scratch_bytes(64, 64, 3)
    assert need > 0 and need % 8 == 0

    base = dict(texture=tex, gradient=grad, speed=speed, energy=energy, scratch=scratch)
    smooth = entry(L, _abi.TEXTURE_HEADER, "deodr_hip_texture_smoothness", base, Ht=64, Wt=64, C=3, pixel_dtype=F32, weight=1.0, scratch_bytes=need)
    step = entry(L, _abi.TEXTURE_HEADER, "deodr_hip_texture_step", base, Ht=64, Wt=64, C=3, pixel_dtype=F32, factor=0.1, step_max=0.0, inertia=0.9,
                 damping=0.05, clamp=0, clamp_lo=0.0, clamp_hi=1.0)  # fmt: skip

    for call, pointers in ((smooth, ("texture", "gradient", "energy")), (step, ("texture", "speed", "gradient"))):
        for bad in nulls(pointers):
            rc, msg = call(**bad)
            assert rc == 1 and "== NULL" in msg, (bad, msg)
        for bad in (dict(Ht=1), dict(Wt=1), dict(Ht=0), dict(Wt=-5)):
            assert call(**bad) == (1, "texture must be at least 2 x 2"), bad
        for bad in (dict(C=0), dict(C=MAXC + 1), dict(C=-1)):
            assert call(**bad) == (1, "nb_colors out of range"), bad
        for bad in (dict(pixel_dtype=2), dict(pixel_dtype=-1), dict(pixel_dtype=7)):
            assert call(**bad) == (1, "unknown dtype tag"), bad
        assert call(Ht=1 << 15, Wt=1 << 15, C=2)[1] == "texture larger than 2^30 elements"
        # gradient aliasing the texture: the same address, and a partial overlap (64 x 64 x 3 float32 = 49 152 bytes; F64 twice that)
        for g_at, dtype in ((tex, F32), (tex + 49152 - 4, F32), (tex - 49152 + 4, F32), (tex + 49152, F64)):
            rc, msg = call(gradient=g_at, pixel_dtype=dtype)
            assert rc == 1 and "gradient must not overlap texture" in msg, (g_at, msg)
        rc, msg = call(texture=tex + 2)
        assert rc == 1 and "misaligned" in msg
    assert smooth(scratch=None)[1].startswith("texture_smoothness: scratch too small")
    assert smooth(scratch_bytes=need - 1)[1].startswith("texture_smoothness: scratch too small")
    assert step(speed=tex + 8)[1] == "texture_step: speed must not overlap texture or gradient"
    assert step(clamp=1, clamp_lo=1.0, clamp_hi=0.0)[1] == "texture_step: clamp_lo > clamp_hi"
    # the scratch size: 0 for dimensions no call takes
    for bad in ((1, 64, 3), (64, 1, 3), (64, 64, 0), (64, 64, MAXC + 1)):
        assert L.deodr_hip_texture_scratch_bytes(*bad) == 0, bad


def test_host_wrappers_check_their_tensors_before_the_library(monkeypatch):
    import torch

    from abi_cases import no_library
    from deodr_amd import hip_renderer as hr

    monkeypatch.setattr(hr, "lib", no_library)
    t = torch.zeros(8, 8, 3)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.texture_smoothness(t, torch.zeros_like(t), 1.0)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.texture_step(t, torch.zeros_like(t), torch.zeros_like(t), 0.1)
