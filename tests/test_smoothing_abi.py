"""CPU checks of the companion header include/deodr_hip_solve.h (the sparse symmetric positive definite solve): it parses with the parser of deodr_hip.h
and shares no name with the other ten headers, its prototypes are type by type what the header documents, every name it declares is exported by the
cross-compiled library and bound with the declared types, its version is 1 on both sides, the constants of deodr_amd/csrc/dr_solve.h are the ones the
case table is built for, every bad argument of the launching entry point is refused through its error code with a message before any launch (fake
pointers, no GPU), the scratch size is 0 outside the limits, monotone inside them and the documented formula, the launch rule is the documented one
either side of N_SMALL, and the host wrapper refuses CPU tensors, wrong dtypes and wrong shapes without reaching the library."""

import ctypes as C
import os
import re

import pytest

SOLVE_FUNCTIONS = ["deodr_hip_spd_solve", "deodr_hip_spd_solve_scratch_bytes", "deodr_hip_spd_solve_launches", "deodr_hip_solve_abi_version"]


def test_companion_header_parses_and_is_versioned_on_its_own():
    from deodr_amd import _abi

    h = _abi.SOLVE_HEADER
    assert sorted(h.functions) == sorted(SOLVE_FUNCTIONS)
    assert h.defines == {"DEODR_HIP_SOLVE_ABI_VERSION": 1, "DEODR_HIP_SOLVE_N_SMALL": 1024} and h.structs == {}
    assert h.name == "include/deodr_hip_solve.h"
    others = (_abi.HEADER, _abi.TEXTURE_HEADER, _abi.SUBDIV_HEADER, _abi.RETAINED_HEADER, _abi.BASIS_HEADER, _abi.CAMERA_HEADER, _abi.LIGHTING_HEADER,
              _abi.SKINNING_HEADER, _abi.PYRAMID_HEADER, _abi.SSIM_HEADER)  # fmt: skip
    assert len(others) == 10
    for other in others:
        assert not set(h.functions) & set(other.functions) and not set(h.defines) & set(other.defines)
    assert re.search(r"#define\s+DEODR_HIP_SOLVE_ABI_VERSION\s+1\b", open(_abi.SOLVE_HEADER_PATH).read())
    p, i, z, d, u = C.c_void_p, C.c_int, C.c_size_t, C.c_double, C.c_uint32
    assert h.functions["deodr_hip_spd_solve"] == (i, [p, p, p, i, u, p, p, i, i, d, p, p, z, p])  # 14 parameters
    assert h.functions["deodr_hip_spd_solve_scratch_bytes"] == (z, [i, i])
    assert h.functions["deodr_hip_spd_solve_launches"] == (i, [i, u, i, i])
    assert h.functions["deodr_hip_solve_abi_version"] == (i, [])


def test_library_exports_and_binds_every_name_of_the_companion_header():
    import __graft_entry__ as g
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    raw = C.CDLL(g.build_hip())
    for name in SOLVE_FUNCTIONS:
        assert hasattr(raw, name), name
    assert raw.deodr_hip_solve_abi_version() == 1 == hr.SOLVE_ABI_VERSION
    assert hr.SOLVE_N_SMALL == 1024 and hr.SOLVE_MAX_D == 4
    L = hr.lib()  # binds every header
    for name, (restype, argtypes) in _abi.SOLVE_HEADER.functions.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name


def test_the_header_is_on_the_list_that_decides_whether_the_library_is_stale():
    import inspect

    import __graft_entry__ as g

    assert '"deodr_hip_solve.h"' in inspect.getsource(g.build_hip)


def test_the_constants_of_the_kernels_are_the_case_table_s():
    import __graft_entry__ as g
    import smoothing_reference as sr
    from deodr_amd import hip_renderer as hr

    source = open(os.path.join(g.CSRC, "dr_solve.h")).read()
    constant = lambda name, text=source: int(re.search(rf"^constexpr int [^;]*\b{name} = (\d+)", text, re.M).group(1))
    assert constant("SOLVE_BLOCKS") == sr.BLOCKS and constant("SOLVE_LANES") == sr.LANES and constant("SOLVE_SMALL_THREADS") == sr.N_SMALL
    assert constant("FH_BLOCK", open(os.path.join(g.CSRC, "dr_fronthalf.h")).read()) == sr.FH_BLOCK and sr.ROWS == sr.FH_BLOCK // sr.LANES
    assert re.search(r"SOLVE_N_SMALL = DEODR_HIP_SOLVE_N_SMALL", source) and hr.SOLVE_N_SMALL == sr.N_SMALL
    sizes = {sr.reference(name)[0]["n"] for name in sr.CASES if name.startswith("hubs")}
    for n in (sr.N_SMALL - 1, sr.N_SMALL, sr.N_SMALL + 1, sr.N_SMALL + sr.ROWS, sr.N_SMALL + sr.FH_BLOCK, sr.BLOCKS * sr.ROWS + 1, sr.BLOCKS * sr.FH_BLOCK + 1):
        assert n in sizes, n
    assert sr.BLOCKS > sr.FH_BLOCK  # the last workgroup of grid_sum adds more than one partial per thread
    lengths = set(sr.row_lengths(sr.reference(f"hubs n={sr.N_SMALL + 1} lam=4 D=3 m=16")[0]["offsets"]))
    assert {sr.LANES - 1, sr.LANES, sr.LANES + 1, 2 * sr.LANES + 1} <= lengths  # one trip of the lane group short of full, full, two trips, three


def test_scratch_is_zero_outside_the_limits_monotone_inside_and_the_documented_formula():
    from deodr_amd import hip_renderer as hr

    need = hr.lib().deodr_hip_spd_solve_scratch_bytes
    for n, D in ((0, 3), (-1, 3), (5, 0), (5, 5), (5, -1)):
        assert need(n, D) == 0, (n, D)
    for n, D in ((1, 1), (526, 3), (1025, 4), (10002, 3)):
        assert need(n, D) == 64 + 8 * (24 + 4 * 512 + 4 * n * D), (n, D)
    for sizes in ([need(n, 3) for n in (1, 2, 1024, 1025, 50000)], [need(526, D) for D in (1, 2, 3, 4)]):
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes), sizes


def test_the_launch_rule_either_side_of_n_small():
    from deodr_amd import hip_renderer as hr

    N = hr.SOLVE_N_SMALL
    for n in (1, 2, 526, N - 1, N):
        for m in (1, 16, 64):
            assert hr.spd_launches(n, 7 * n, 3, m) == 1, (n, m)
    for n in (N + 1, N + 2, 10002, 2**20):
        for m in (1, 2, 16, 64):
            assert hr.spd_launches(n, 7 * n, 3, m) == 2 + 2 * m, (n, m)
    assert hr.spd_launches(N + 1, 7 * N, 1, 5) == hr.spd_launches(N + 1, 100 * N, 4, 5) == 12  # nnz and D do not enter the rule
    for bad in ((0, 1, 3, 4), (-5, 1, 3, 4), (10, 9, 3, 4), (10, 70, 0, 4), (10, 70, 5, 4), (10, 70, 3, 0), (10, 70, 3, -1)):
        assert hr.spd_launches(*bad) == 0, bad


def test_bad_arguments_are_refused_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    n, nnz, D = 41, 250, 3  # (4 (n + 1) and 4 nnz multiples of 8: the overlaps below stay aligned)
    base = dict(offsets=0x10000000, cols=0x11000000, vals=0x12000000, b=0x13000000, x=0x14000000, residual=0x15000000, scratch=0x16000000)

    def call(n=n, nnz=nnz, D=D, iterations=8, rel_tol=0.0, scratch_bytes=None, **changed):
        a = dict(base, **changed)
        need = L.deodr_hip_spd_solve_scratch_bytes(n, D)
        rc = L.deodr_hip_spd_solve(a["offsets"], a["cols"], a["vals"], n, nnz, a["b"], a["x"], D, iterations, rel_tol, a["residual"], a["scratch"],
                                   need if scratch_bytes is None else scratch_bytes, None)  # fmt: skip
        return rc, L.deodr_hip_last_error().decode()

    what = "spd_solve"
    for p in base:  # a NULL pointer
        rc, msg = call(**{p: None})
        assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (p, msg)
    for bad in (0, -1, -(2**31)):
        assert call(n=bad, scratch_bytes=1 << 20) == (1, what + ": n must be positive"), bad
    assert call(nnz=n - 1) == (1, what + ": nnz must be >= n (the diagonal is stored)")
    for bad in (0, 5, -1, 16):
        assert call(D=bad, scratch_bytes=1 << 20) == (1, what + ": D must be in 1 .. 4"), bad
    for bad in (0, -1):
        assert call(iterations=bad) == (1, what + ": iterations must be >= 1"), bad
    for bad in (-1e-300, -1.0, float("-inf"), float("nan")):
        assert call(rel_tol=bad) == (1, what + ": rel_tol must be >= 0"), bad
    for p in ("offsets", "cols"):
        assert call(**{p: base[p] + 2}) == (1, what + ": misaligned pointer"), p
    for p in ("vals", "b", "x", "residual", "scratch"):
        assert call(**{p: base[p] + 4}) == (1, what + ": misaligned pointer"), p
    need = L.deodr_hip_spd_solve_scratch_bytes(n, D)
    for short in (0, 64, need - 1):
        assert call(scratch_bytes=short) == (1, what + ": scratch too small (deodr_hip_spd_solve_scratch_bytes)"), short
    nd = 8 * n * D
    for at in (base["b"], base["b"] + nd - 8, base["b"] - nd + 8):  # x overlapping b: in place, and by one element either side
        assert call(x=at) == (1, what + ": x must not overlap b"), hex(at)
    sizes = dict(offsets=4 * (n + 1), cols=4 * nnz, vals=8 * nnz, b=nd, x=nd, residual=8 * D, scratch=need)
    refusal = (1, what + ": an output must not overlap an input, the scratch or another output")
    for out in ("x", "residual", "scratch"):
        for other in sizes:
            if other != out and (out, other) != ("x", "b"):
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
    with pytest.raises(ValueError, match="b must be a ROCm tensor"):
        hr.spd_solve(i32(6), i32(9), f64(9), f64(5, 3), 4)

    class OnDevice(torch.Tensor):
        is_cuda = property(lambda self: True)
        device = property(lambda self: torch.device("cuda", 0))

    dev = lambda x: x.as_subclass(OnDevice)
    O, Cc, V, B = dev(i32(6)), dev(i32(9)), dev(f64(9)), dev(f64(5, 3))
    for bad in (dev(f64(5)), dev(f64(5, 5)), dev(f64(0, 3)), dev(f64(5, 3, 1))):
        with pytest.raises(ValueError, match=r"b must have shape \[n >= 1, 1 <= D <= 4\]"):
            hr.spd_solve(O, Cc, V, bad, 4)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="iterations must be >= 1"):
            hr.spd_solve(O, Cc, V, B, bad)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="rel_tol must be >= 0"):
            hr.spd_solve(O, Cc, V, B, 4, rel_tol=bad)
    with pytest.raises(ValueError, match="b must be float64"):
        hr.spd_solve(O, Cc, V, dev(f64(5, 3).float()), 4)
    with pytest.raises(ValueError, match="b must be contiguous"):
        hr.spd_solve(O, Cc, V, dev(f64(3, 5).t()), 4)
    with pytest.raises(ValueError, match=r"offsets must be a 4-byte integer tensor of n \+ 1 = 6 entries"):
        hr.spd_solve(dev(i32(5)), Cc, V, B, 4)
    with pytest.raises(ValueError, match="offsets must be a 4-byte integer tensor"):
        hr.spd_solve(dev(i32(6).long()), Cc, V, B, 4)
    with pytest.raises(ValueError, match="offsets and cols must be one-dimensional 4-byte integer tensors"):
        hr.spd_solve(O, dev(i32(9).long()), V, B, 4)
    with pytest.raises(ValueError, match="vals must be a float64 tensor of the shape of cols"):
        hr.spd_solve(O, Cc, dev(f64(8)), B, 4)
    with pytest.raises(ValueError, match="vals must be a float64 tensor of the shape of cols"):
        hr.spd_solve(O, Cc, dev(f64(9).float()), B, 4)
    with pytest.raises(ValueError, match="offsets must be a 4-byte integer tensor"):
        hr.spd_solve(i32(6), Cc, V, B, 4)  # a CPU tensor
    with pytest.raises(ValueError, match=r"x must have shape \[5, 3\]"):
        hr.spd_solve(O, Cc, V, B, 4, x=dev(f64(5, 4)))
    with pytest.raises(ValueError, match=r"residual must have shape \[3\]"):
        hr.spd_solve(O, Cc, V, B, 4, residual=dev(f64(4)))
    with pytest.raises(ValueError, match="scratch must be uint8"):
        hr.spd_solve(O, Cc, V, B, 4, scratch=dev(torch.zeros(64)))
    with pytest.raises(ValueError, match="the matrix has 4 entries for 5 rows"):
        hr.spd_solve(O, dev(i32(4)), dev(f64(4)), B, 4)
