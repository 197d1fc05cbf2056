"""CPU checks of the companion header include/deodr_hip_arap.h (the as-rigid-as-possible energy): it parses with the parser of deodr_hip.h and shares
no name with the other eleven headers, its prototypes are type by type what the header documents, every name it declares is exported by the
cross-compiled library and bound with the declared types, its version is 1 on both sides, the constants of deodr_amd/csrc/dr_arap.h are the ones the
case tables are built for, every bad argument of the launching entry point is refused through its error code with a message before any launch (fake
pointers, no GPU), the scratch size is 0 outside the limits, monotone inside them and the documented formula, the launch rule is pinned at its
boundaries, and the host wrapper refuses CPU tensors, wrong dtypes and wrong shapes without reaching the library."""

import ctypes as C
import os
import re

import pytest

ARAP_FUNCTIONS = ["deodr_hip_arap_energy", "deodr_hip_arap_scratch_bytes", "deodr_hip_arap_launches", "deodr_hip_arap_blocks", "deodr_hip_arap_abi_version"]


def test_companion_header_parses_and_is_versioned_on_its_own():
    from deodr_amd import _abi

    h = _abi.ARAP_HEADER
    assert sorted(h.functions) == sorted(ARAP_FUNCTIONS)
    assert h.defines == {"DEODR_HIP_ARAP_ABI_VERSION": 1, "DEODR_HIP_ARAP_SWEEPS": 5, "DEODR_HIP_ARAP_BLOCK": 256, "DEODR_HIP_ARAP_MAX_BLOCKS": 512}
    assert h.structs == {} and h.name == "include/deodr_hip_arap.h"
    others = (_abi.HEADER, _abi.TEXTURE_HEADER, _abi.SUBDIV_HEADER, _abi.RETAINED_HEADER, _abi.BASIS_HEADER, _abi.CAMERA_HEADER, _abi.LIGHTING_HEADER,
              _abi.SKINNING_HEADER, _abi.PYRAMID_HEADER, _abi.SSIM_HEADER, _abi.SOLVE_HEADER)  # fmt: skip
    assert len(others) == 11
    for other in others:
        assert not set(h.functions) & set(other.functions) and not set(h.defines) & set(other.defines)
    assert re.search(r"#define\s+DEODR_HIP_ARAP_ABI_VERSION\s+1\b", open(_abi.ARAP_HEADER_PATH).read())
    p, i, z, d, u = C.c_void_p, C.c_int, C.c_size_t, C.c_double, C.c_uint32
    assert h.functions["deodr_hip_arap_energy"] == (i, [p, p, p, i, u, p, p, i, d, p, p, p, p, z, p])  # 15 parameters
    assert h.functions["deodr_hip_arap_scratch_bytes"] == (z, [i, i])
    assert h.functions["deodr_hip_arap_launches"] == (i, [i, u, i])
    assert h.functions["deodr_hip_arap_blocks"] == (i, [i])
    assert h.functions["deodr_hip_arap_abi_version"] == (i, [])


def test_library_exports_and_binds_every_name_of_the_companion_header():
    import __graft_entry__ as g
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    raw = C.CDLL(g.build_hip())
    for name in ARAP_FUNCTIONS:
        assert hasattr(raw, name), name
    assert raw.deodr_hip_arap_abi_version() == 1 == hr.ARAP_ABI_VERSION
    assert (hr.ARAP_SWEEPS, hr.ARAP_BLOCK, hr.ARAP_MAX_BLOCKS) == (5, 256, 512)
    L = hr.lib()  # binds every header
    for name, (restype, argtypes) in _abi.ARAP_HEADER.functions.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name


def test_the_header_is_on_the_list_that_decides_whether_the_library_is_stale():
    import inspect

    import __graft_entry__ as g

    assert '"deodr_hip_arap.h"' in inspect.getsource(g.build_hip)


def test_the_constants_of_the_kernels_are_the_case_table_s():
    import __graft_entry__ as g
    import arap_reference as ar
    from deodr_amd import hip_renderer as hr

    source = open(os.path.join(g.CSRC, "dr_arap.h")).read()
    assert re.search(r"ARAP_SWEEPS = DEODR_HIP_ARAP_SWEEPS, ARAP_BLOCK = DEODR_HIP_ARAP_BLOCK, ARAP_MAX_BLOCKS = DEODR_HIP_ARAP_MAX_BLOCKS", source)
    assert (hr.ARAP_SWEEPS, hr.ARAP_BLOCK, hr.ARAP_MAX_BLOCKS) == (ar.SWEEPS, ar.BLOCK, ar.MAX_BLOCKS)
    fh = open(os.path.join(g.CSRC, "dr_fronthalf.h")).read()
    assert int(re.search(r"^constexpr int FH_BLOCK = (\d+)", fh, re.M).group(1)) == ar.FH_BLOCK == ar.BLOCK
    assert ar.MAX_BLOCKS > ar.FH_BLOCK  # the last workgroup of grid_sum can add more than one partial per thread
    assert re.search(r"fabs\(theta\) <= 1e150", source) and ar.THETA_BIG == 1e150
    pivots = re.findall(r"arap_rotate<(\d), (\d)>\(A, E\);", source)
    assert tuple((int(a), int(b)) for a, b in pivots) == ar.PAIRS


def test_scratch_is_zero_outside_the_limits_monotone_inside_and_the_documented_formula():
    from deodr_amd import hip_renderer as hr

    need = hr.lib().deodr_hip_arap_scratch_bytes
    for V, n in ((0, 3), (-1, 3), (5, 0), (5, -1), (5, 65536)):
        assert need(V, n) == 0, (V, n)
    for V, n in ((1, 1), (526, 8), (10002, 1), (131073, 3), (5, 65535)):
        assert need(V, n) == 64 + 8 * (5 * n * V + 512 * n + (n + 1) // 2), (V, n)
    for sizes in ([need(V, 2) for V in (1, 2, 256, 257, 50000)], [need(526, n) for n in (1, 2, 3, 4, 8)]):
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes), sizes


def test_the_launch_rule_at_its_boundaries():
    import arap_reference as ar
    from deodr_amd import hip_renderer as hr

    B, M = hr.ARAP_BLOCK, hr.ARAP_MAX_BLOCKS
    for V, blocks in ((1, 1), (B - 1, 1), (B, 1), (B + 1, 2), (526, 3), (10002, 40), (B * B, B), (B * B + 1, B + 1), (B * M - 1, M), (B * M, M), (B * M + 1, M), (2**30, M)):
        assert hr.arap_blocks(V) == blocks == min(-(-V // B), M), V
        for n in (1, 8):
            assert hr.arap_launches(V, 6 * V, n) == 2 == hr.arap_launches(V, 0, n), (V, n)
    assert [hr.arap_blocks(V) for V in (0, -1, -(2**31))] == [0, 0, 0]
    for bad in ((0, 0, 1), (-5, 0, 1), (10, 60, 0), (10, 60, -1), (10, 60, 65536)):
        assert hr.arap_launches(*bad) == 0, bad
    assert ar.boundary_sizes(hr.arap_blocks, B, M) == [B - 1, B, B + 1, B * B + 1, B * M + 1]  # what tests/test_arap_gpu.py runs


def test_bad_arguments_are_refused_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    V, nnz, n = 41, 250, 2  # (4 (V + 1) and 4 nnz multiples of 8: the overlaps below stay aligned)
    base = dict(offsets=0x10000000, cols=0x11000000, weights=0x12000000, vertices_ref=0x13000000, vertices=0x14000000, energy=0x15000000,
                gradient=0x16000000, rotations=0x17000000, scratch=0x18000000)  # fmt: skip

    def call(V=V, nnz=nnz, n=n, cregu=1.0, scratch_bytes=None, **changed):
        a = dict(base, **changed)
        need = L.deodr_hip_arap_scratch_bytes(V, n)
        rc = L.deodr_hip_arap_energy(a["offsets"], a["cols"], a["weights"], V, nnz, a["vertices_ref"], a["vertices"], n, cregu, a["energy"], a["gradient"],
                                     a["rotations"], a["scratch"], need if scratch_bytes is None else scratch_bytes, None)  # fmt: skip
        return rc, L.deodr_hip_last_error().decode()

    what = "arap_energy"
    for p in base:  # a NULL pointer (rotations may be NULL: the call then gets past every check of this test only with real memory, not tried here)
        if p != "rotations":
            rc, msg = call(**{p: None})
            assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (p, msg)
    for bad in (0, -1, -(2**31)):
        assert call(V=bad, scratch_bytes=1 << 20) == (1, what + ": V must be positive"), bad
    for bad in (0, -1, 65536):
        assert call(n=bad, scratch_bytes=1 << 20) == (1, what + ": n must be in 1 .. 65535"), bad
    for bad in (-1e-300, -1.0, float("-inf"), float("nan")):
        assert call(cregu=bad) == (1, what + ": cregu must be >= 0"), bad
    for p in ("offsets", "cols"):
        assert call(**{p: base[p] + 2}) == (1, what + ": misaligned pointer"), p
    for p in ("weights", "vertices_ref", "vertices", "energy", "gradient", "rotations", "scratch"):
        assert call(**{p: base[p] + 4}) == (1, what + ": misaligned pointer"), p
    need = L.deodr_hip_arap_scratch_bytes(V, n)
    for short in (0, 64, need - 1):
        assert call(scratch_bytes=short) == (1, what + ": scratch too small (deodr_hip_arap_scratch_bytes)"), short
    cells = n * V
    sizes = dict(offsets=4 * (V + 1), cols=4 * nnz, weights=8 * nnz, vertices_ref=24 * V, vertices=24 * cells, energy=8 * n, gradient=24 * cells,
                 rotations=32 * cells, scratch=need)  # fmt: skip
    refusal = (1, what + ": an output must not overlap an input, the scratch or another output")
    for out in ("energy", "gradient", "rotations", "scratch"):
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
        hr.arap_energy(i32(6), i32(9), f64(9), f64(5, 3), f64(2, 5, 3), 1.0)

    class OnDevice(torch.Tensor):
        is_cuda = property(lambda self: True)
        device = property(lambda self: torch.device("cuda", 0))

    dev = lambda x: x.as_subclass(OnDevice)
    O, Cc, W, Q, P = dev(i32(6)), dev(i32(9)), dev(f64(9)), dev(f64(5, 3)), dev(f64(2, 5, 3))
    for bad in (dev(f64(5, 3)), dev(f64(2, 5, 4)), dev(f64(0, 5, 3)), dev(f64(2, 0, 3)), dev(f64(2, 5, 3, 1))):
        with pytest.raises(ValueError, match=r"vertices must have shape \[n >= 1, V >= 1, 3\]"):
            hr.arap_energy(O, Cc, W, Q, bad, 1.0)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="cregu must be >= 0"):
            hr.arap_energy(O, Cc, W, Q, P, bad)
    with pytest.raises(ValueError, match="vertices must be float64"):
        hr.arap_energy(O, Cc, W, Q, dev(f64(2, 5, 3).float()), 1.0)
    with pytest.raises(ValueError, match="vertices must be contiguous"):
        hr.arap_energy(O, Cc, W, Q, dev(f64(5, 2, 3).transpose(0, 1)), 1.0)
    with pytest.raises(ValueError, match=r"vertices_ref must have shape \[5, 3\]"):
        hr.arap_energy(O, Cc, W, dev(f64(4, 3)), P, 1.0)
    with pytest.raises(ValueError, match=r"offsets must be a 4-byte integer tensor of V \+ 1 = 6 entries"):
        hr.arap_energy(dev(i32(5)), Cc, W, Q, P, 1.0)
    with pytest.raises(ValueError, match="offsets and cols must be one-dimensional 4-byte integer tensors"):
        hr.arap_energy(O, dev(i32(9).long()), W, Q, P, 1.0)
    with pytest.raises(ValueError, match="weights must be a float64 tensor of the shape of cols"):
        hr.arap_energy(O, Cc, dev(f64(8)), Q, P, 1.0)
    with pytest.raises(ValueError, match="offsets must be a 4-byte integer tensor"):
        hr.arap_energy(i32(6), Cc, W, Q, P, 1.0)  # a CPU tensor
    with pytest.raises(ValueError, match=r"energy must have shape \[2\]"):
        hr.arap_energy(O, Cc, W, Q, P, 1.0, energy=dev(f64(3)))
    with pytest.raises(ValueError, match=r"gradient must have shape \[2, 5, 3\]"):
        hr.arap_energy(O, Cc, W, Q, P, 1.0, gradient=dev(f64(5, 3)))
    with pytest.raises(ValueError, match=r"rotations must have shape \[2, 5, 4\]"):
        hr.arap_energy(O, Cc, W, Q, P, 1.0, rotations=dev(f64(2, 5, 3)))
    with pytest.raises(ValueError, match="scratch must be uint8"):
        hr.arap_energy(O, Cc, W, Q, P, 1.0, scratch=dev(torch.zeros(64)))
