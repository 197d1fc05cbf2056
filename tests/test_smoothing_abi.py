"""CPU checks of the sparse symmetric positive definite solve at the C ABI (include/deodr_hip_solve.h; the header itself:
tests/test_companion_headers.py): the constants of deodr_amd/csrc/dr_solve.h are the ones the case table is built for, every bad argument of the
launching entry point is refused through its error code with a message before any launch (fake pointers, no GPU), the scratch size is 0 outside
the limits, monotone inside them and the documented formula, the launch rule is the documented one either side of N_SMALL, and the host wrapper
refuses CPU tensors, wrong dtypes and wrong shapes without reaching the library."""

import os
import re

import pytest


def test_the_limits_are_the_header_s():
    from deodr_amd import hip_renderer as hr

    assert hr.SOLVE_N_SMALL == 1024 and hr.SOLVE_MAX_D == 4


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
    from abi_cases import entry, misaligned, nulls, overlap_placements
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    n, nnz, D = 41, 250, 3  # (4 (n + 1) and 4 nnz multiples of 8: the overlaps below stay aligned)
    base = dict(offsets=0x10000000, cols=0x11000000, vals=0x12000000, b=0x13000000, x=0x14000000, residual=0x15000000, scratch=0x16000000)

    call = entry(L, _abi.SOLVE_HEADER, "deodr_hip_spd_solve", base, n=n, nnz=nnz, D=D, iterations=8, rel_tol=0.0,
                 scratch_bytes=lambda a: L.deodr_hip_spd_solve_scratch_bytes(a["n"], a["D"]))  # fmt: skip
    what = "spd_solve"
    for bad in nulls(base):  # a NULL pointer
        rc, msg = call(**bad)
        assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (bad, msg)
    for bad in (0, -1, -(2**31)):
        assert call(n=bad, scratch_bytes=1 << 20) == (1, what + ": n must be positive"), bad
    assert call(nnz=n - 1) == (1, what + ": nnz must be >= n (the diagonal is stored)")
    for bad in (0, 5, -1, 16):
        assert call(D=bad, scratch_bytes=1 << 20) == (1, what + ": D must be in 1 .. 4"), bad
    for bad in (0, -1):
        assert call(iterations=bad) == (1, what + ": iterations must be >= 1"), bad
    for bad in (-1e-300, -1.0, float("-inf"), float("nan")):
        assert call(rel_tol=bad) == (1, what + ": rel_tol must be >= 0"), bad
    for bad in misaligned(base, ("offsets", "cols"), 2):
        assert call(**bad) == (1, what + ": misaligned pointer"), bad
    for bad in misaligned(base, ("vals", "b", "x", "residual", "scratch"), 4):
        assert call(**bad) == (1, what + ": misaligned pointer"), bad
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
                for at in overlap_placements(base, sizes, out, other):
                    assert call(**{out: at}) == refusal, (out, other, hex(at))


def test_host_wrapper_checks_its_tensors_before_the_library(monkeypatch):
    import torch

    from abi_cases import no_library
    from abi_cases import on_device as dev
    from deodr_amd import hip_renderer as hr

    monkeypatch.setattr(hr, "lib", no_library)
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    with pytest.raises(ValueError, match="b must be a ROCm tensor"):
        hr.spd_solve(i32(6), i32(9), f64(9), f64(5, 3), 4)

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
