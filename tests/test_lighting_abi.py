"""CPU checks of spherical-harmonic lighting and per-vertex albedo at the C ABI (include/deodr_hip_lighting.h; the header itself:
tests/test_companion_headers.py): every bad argument of the two launching entry points is refused with a message before any launch (fake pointers,
no GPU), the block rule and the scratch size behave as the header says, and the host wrappers refuse CPU tensors, wrong dtypes and wrong shapes
without reaching the library."""

import pytest


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
    from abi_cases import entry, misaligned, nulls
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    V, n, C_ = 100, 2, 3
    base = dict(posed=0x10000000, faces=0x11000000, vf_offsets=0x12000000, vf_corners=0x13000000, sh=0x14000000, albedo=0x15000000,
                luminosity=None, luminosity_b=None, colors=0x17000000, colors_b=0x17000000, posed_b=0x18000000, sh_b=0x19000000, albedo_b=0x1A000000,
                scratch=0x1B000000)  # fmt: skip
    shade = entry(L, _abi.LIGHTING_HEADER, "deodr_hip_sh_shade", base, V=V, n=n, C=C_, S=3, albedo_per_vertex=0, clockwise=0)
    shade_b = entry(L, _abi.LIGHTING_HEADER, "deodr_hip_sh_shade_b", base, V=V, n=n, C=C_, S=3, albedo_per_vertex=0, clockwise=0, accumulate=0,
                    scratch_bytes=lambda a: L.deodr_hip_sh_scratch_bytes(a["V"], a["n"], a["C"]))  # fmt: skip

    for call, what, luminosity, colors in ((shade, "sh_shade", "luminosity", "colors"), (shade_b, "sh_shade_b", "luminosity_b", "colors_b")):
        for bad in nulls(("posed", "faces", "vf_offsets", "vf_corners", "sh")):  # a NULL among the required pointers
            rc, msg = call(**bad)
            assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (bad, msg)
        rc, msg = call(**{colors: None, "albedo": None})  # no output (forward) / no incoming adjoint (backward)
        assert rc == 1 and msg.startswith(what + ": no output requested"), msg
        for bad in (dict(albedo=None), {colors: None, luminosity: 0x16000000, "S": 1}):  # albedo without colors, and the reverse
            assert call(**bad) == (1, what + ": albedo and colors go together"), bad
        assert call(**{luminosity: 0x16000000}) == (1, what + ": luminosity needs S = 1")  # S = 3 here
        for bad in (dict(n=0), dict(n=-1), dict(n=65)):
            assert call(**bad) == (1, what + ": n must be in 1 .. 64"), bad
        for bad in (dict(V=0), dict(V=-7), dict(V=2**24 + 1)):
            assert call(**bad) == (1, what + ": V must be in 1 .. 2^24"), bad
        for bad in (dict(C=0), dict(C=4), dict(C=-1)):
            assert call(**bad) == (1, what + ": C must be in 1 .. 3"), bad
        for bad in (dict(S=0), dict(S=2), dict(S=4), dict(S=3, C=2)):
            assert call(**bad) == (1, what + ": S must be 1 or C"), bad
        mine = ("posed", "sh", "albedo", colors) + (("posed_b", "sh_b", "albedo_b", "scratch") if call is shade_b else ())
        for bad in misaligned(base, mine, 4):
            assert call(**bad) == (1, what + ": misaligned pointer"), bad
        for bad in misaligned(base, ("faces", "vf_offsets", "vf_corners"), 2):  # 4-byte aligned
            assert call(**bad) == (1, what + ": misaligned pointer"), bad
        assert call(**{luminosity: 0x16000004, "S": 1}) == (1, what + ": misaligned pointer")
    # the adjoint's own refusals
    what = "sh_shade_b"
    assert shade_b(scratch=None) == (1, what + ": scratch == NULL")
    assert shade_b(posed_b=None, sh_b=None, albedo_b=None) == (1, what + ": no output requested (posed_b, sh_b, albedo_b)")
    assert shade_b(albedo=None, colors_b=None, luminosity_b=0x16000000, S=1) == (1, what + ": albedo_b without albedo")
    need = L.deodr_hip_sh_scratch_bytes(V, n, C_)
    for short in (0, 8, need - 1):
        assert shade_b(scratch_bytes=short) == (1, what + ": scratch too small (deodr_hip_sh_scratch_bytes)"), short
    # an output overlapping an input.  bytes: posed(_b) 4800, colors(_b) 4800, sh(_b) 216, albedo(_b) 24 (one colour) or 2400 (per vertex), vf_offsets 404
    sizes = dict(posed=4800, vf_offsets=404, faces=12, vf_corners=12, sh=216, albedo=24, colors=4800, colors_b=4800, posed_b=4800, sh_b=216, albedo_b=24)
    refusal = (1, what + ": an output must not overlap an input, the scratch or another output")
    for out in ("posed_b", "sh_b", "albedo_b"):
        for inp in ("posed", "faces", "vf_offsets", "vf_corners", "sh", "albedo", "colors_b"):
            for at in (base[inp], base[inp] + (sizes[inp] - 4) // 8 * 8, base[inp] - sizes[out] + 8):
                assert shade_b(**{out: at}) == refusal, (out, inp, hex(at))
        assert shade_b(**{out: base["scratch"] + 64}) == refusal and shade_b(**{out: base["scratch"] + need - 8}) == refusal, out
    assert shade_b(albedo_per_vertex=1, albedo_b=base["albedo"] + 2392) == refusal  # (a per-vertex albedo is V C doubles)
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

    from abi_cases import no_library
    from abi_cases import on_device as dev
    from deodr_amd import hip_renderer as hr

    monkeypatch.setattr(hr, "lib", no_library)
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    n, V, T = 2, 10, 7
    posed, faces, off, corners, sh, albedo = f64(n, V, 3), i32(T, 3), i32(V + 1), i32(3 * T), f64(9, 3), f64(V, 3)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.sh_shade(posed, faces, off, corners, sh, albedo)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.sh_shade_b(posed, faces, off, corners, sh, albedo, colors_b=f64(n, V, 3))

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
