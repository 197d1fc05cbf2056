"""CPU checks of the linear bases at the C ABI (include/deodr_hip_basis.h; the header itself: tests/test_companion_headers.py): a library that lacks
a declared symbol is refused by name, every bad argument of the two entry points is refused with a message before any launch (fake pointers, no
GPU), the segment rule and the scratch size behave as the header says, and the host wrappers refuse CPU tensors, wrong dtypes and wrong shapes
without reaching the library."""

import ctypes as C

import pytest


def test_a_library_that_lacks_a_declared_symbol_is_refused_by_name():
    import __graft_entry__ as g
    from deodr_amd import _abi

    more = _abi.parse(open(_abi.BASIS_HEADER_PATH).read().replace("int deodr_hip_basis_abi_version(void);",
                                                                  "int deodr_hip_basis_abi_version(void);\nint deodr_hip_basis_not_there(int on);"),
                      "include/deodr_hip_basis.h")  # fmt: skip
    with pytest.raises(ImportError, match=r"deodr_hip_basis_not_there, which include/deodr_hip_basis\.h declares"):
        _abi.bind(C.CDLL(g.build_hip()), more)


INVALID = [(0, 10), (-1, 10), (1025, 10), (4, 0), (4, -5), (4, 2**30 + 1), (1024, 2**21), (3, 2**30)]  # (K, N): a range, or K N > 2^31 - 1


def test_segments_and_scratch_follow_the_header():
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    for K, N in INVALID:
        assert L.deodr_hip_basis_segments(K, N) == 0 == hr.basis_segments(K, N), (K, N)
        assert L.deodr_hip_basis_scratch_bytes(K, N, 1) == 0, (K, N)
    for batch in (0, -1, 65):
        assert L.deodr_hip_basis_scratch_bytes(4, 100, batch) == 0
    assert L.deodr_hip_basis_segments(1023, 2**21) >= 1 and L.deodr_hip_basis_segments(1, 2**30) >= 1 and L.deodr_hip_basis_segments(2, 2**30 - 1) >= 1
    for K in (1, 4, 8, 9, 150, 199, 1024):
        previous, previous_bytes = 0, 0
        top = min(2**30, (2**31 - 1) // K)
        sizes = sorted(set(list(range(1, 40000, 997)) + [2**e + d for e in range(12, 31) for d in (-1, 0, 1)] + [top - 1, top]))
        for N in (n for n in sizes if 1 <= n <= top):
            S, nbytes = L.deodr_hip_basis_segments(K, N), L.deodr_hip_basis_scratch_bytes(K, N, 1)
            assert S >= 1 and S >= previous, (K, N, S, previous)  # at least 1, non-decreasing in N
            assert nbytes >= 8 * S and nbytes >= previous_bytes and (S == previous or nbytes > previous_bytes), (K, N)  # the scratch grows with it
            assert L.deodr_hip_basis_scratch_bytes(K, N, 64) > L.deodr_hip_basis_scratch_bytes(K, N, 4) >= nbytes
            previous, previous_bytes = S, nbytes
        assert L.deodr_hip_basis_segments(K, 1) == 1  # small problems are one segment
    assert L.deodr_hip_basis_segments(199, 160470) > 8  # a face model fills the chip


def test_bad_arguments_are_refused_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from abi_cases import entry, nulls
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    F32, F64 = _abi.HEADER.defines["DEODR_HIP_F32"], _abi.HEADER.defines["DEODR_HIP_F64"]
    basis, mean, coeffs, y, g, c_b, scratch = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000, 0x70000000
    base = dict(basis=basis, mean=mean, coeffs=coeffs, y=y, g=g, coeffs_b=c_b, scratch=scratch)
    apply = entry(L, _abi.BASIS_HEADER, "deodr_hip_basis_apply", base, K=4, N=100, batch=2, basis_dtype=F32, y_dtype=F64)
    apply_b = entry(L, _abi.BASIS_HEADER, "deodr_hip_basis_apply_b", base, g_dtype=F32, K=4, N=100, batch=2, basis_dtype=F32, accumulate=0,
                    scratch_bytes=lambda a: L.deodr_hip_basis_scratch_bytes(a["K"], a["N"], a["batch"]))  # fmt: skip

    for call, what, required in ((apply, "basis_apply", ("basis", "coeffs", "y")), (apply_b, "basis_apply_b", ("basis", "g", "coeffs_b", "scratch"))):
        for bad in nulls(required):
            rc, msg = call(**bad)
            assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (bad, msg)
        for bad in (dict(K=0), dict(K=-1), dict(K=1025)):
            assert call(**bad) == (1, what + ": K must be in 1 .. 1024"), bad
        for bad in (dict(batch=0), dict(batch=-1), dict(batch=65)):
            assert call(**bad) == (1, what + ": batch must be in 1 .. 64"), bad
        for bad in (dict(N=0), dict(N=-7), dict(N=2**30 + 1)):
            assert call(**bad) == (1, what + ": N must be in 1 .. 2^30"), bad
        for bad in (dict(K=2, N=2**30), dict(K=1024, N=2**21), dict(K=3, N=715827883)):
            assert call(**bad) == (1, what + ": K * N must not exceed 2^31 - 1"), bad
        for bad in (dict(basis_dtype=2), dict(basis_dtype=-1)):
            assert call(**bad) == (1, "unknown dtype tag"), bad
    for bad in (dict(y_dtype=2), dict(y_dtype=-1)):
        assert apply(**bad) == (1, "unknown dtype tag"), bad
    for bad in (dict(g_dtype=2), dict(g_dtype=7)):
        assert apply_b(**bad) == (1, "unknown dtype tag"), bad
    for bad in (dict(basis=basis + 2), dict(basis=basis + 4, basis_dtype=F64), dict(mean=mean + 1), dict(mean=mean + 4, basis_dtype=F64), dict(coeffs=coeffs + 4),
                dict(y=y + 4), dict(y=y + 2, y_dtype=F32)):  # fmt: skip
        assert apply(**bad) == (1, "basis_apply: misaligned pointer"), bad
    for bad in (dict(basis=basis + 2), dict(basis=basis + 4, basis_dtype=F64), dict(g=g + 3), dict(g=g + 4, g_dtype=F64), dict(coeffs_b=c_b + 4), dict(scratch=scratch + 4)):
        assert apply_b(**bad) == (1, "basis_apply_b: misaligned pointer"), bad
    # y [2, 100] float64 = 1600 bytes against basis [4, 100] float32 = 1600 bytes, mean 400 bytes, coeffs [2, 4] = 64 bytes
    for y_at in (basis, basis + 1600 - 8, basis - 1600 + 8, mean, mean + 400 - 8, mean - 1600 + 8, coeffs, coeffs + 64 - 8, coeffs - 1600 + 8):
        assert apply(y=y_at) == (1, "basis_apply: y must not overlap basis, mean or coeffs"), hex(y_at)
    # coeffs_b [2, 4] = 64 bytes against basis 1600 bytes and g [2, 100] float32 = 800 bytes
    for at in (basis, basis + 1600 - 8, basis - 64 + 8, g, g + 800 - 8, g - 64 + 8):
        assert apply_b(coeffs_b=at) == (1, "basis_apply_b: coeffs_b must not overlap basis or g"), hex(at)
    need = L.deodr_hip_basis_scratch_bytes(4, 100, 2)
    for short in (0, 8, need - 1):
        assert apply_b(scratch_bytes=short) == (1, "basis_apply_b: scratch too small (deodr_hip_basis_scratch_bytes)"), short


def test_host_wrappers_check_their_tensors_before_the_library(monkeypatch):
    import torch

    from abi_cases import no_library
    from abi_cases import on_device as dev
    from deodr_amd import hip_renderer as hr

    monkeypatch.setattr(hr, "lib", no_library)
    basis, mean, coeffs, g = torch.zeros(4, 10), torch.zeros(10), torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, 10)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.basis_apply(basis, mean, coeffs)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.basis_apply_b(basis, g)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.basis_apply_b(basis, g, out=torch.zeros(2, 4, dtype=torch.float64), accumulate=True)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.basis_apply(basis.numpy(), None, coeffs)

    B, m, c, gd = dev(basis), dev(mean), dev(coeffs), dev(g)
    with pytest.raises(ValueError, match="basis must be float32 or float64"):
        hr.basis_apply(dev(basis.to(torch.float16)), None, c)
    with pytest.raises(ValueError, match=r"basis must have shape"):
        hr.basis_apply(dev(torch.zeros(4, 10, 1)), None, c)
    with pytest.raises(ValueError, match=r"basis must have shape"):
        hr.basis_apply_b(dev(torch.zeros(1025, 2)), dev(torch.zeros(1, 2)))
    with pytest.raises(ValueError, match="basis must be contiguous"):
        hr.basis_apply(dev(torch.zeros(10, 4).T), None, c)
    with pytest.raises(ValueError, match="coeffs must be float64"):
        hr.basis_apply(B, m, dev(coeffs.float()))
    with pytest.raises(ValueError, match=r"coeffs must have shape \[batch, 4\]"):
        hr.basis_apply(B, m, dev(torch.zeros(2, 5, dtype=torch.float64)))
    with pytest.raises(ValueError, match=r"coeffs must have shape \[batch, 4\]"):
        hr.basis_apply(B, m, dev(torch.zeros(4, dtype=torch.float64)))
    with pytest.raises(ValueError, match="coeffs must be contiguous"):
        hr.basis_apply(B, m, dev(torch.zeros(4, 2, dtype=torch.float64).T))
    with pytest.raises(ValueError, match="mean must be float32"):
        hr.basis_apply(B, dev(mean.double()), c)
    with pytest.raises(ValueError, match=r"mean must have shape \[10\]"):
        hr.basis_apply(B, dev(torch.zeros(11)), c)
    with pytest.raises(ValueError, match=r"out must have shape \[batch, 10\]"):
        hr.basis_apply(B, m, c, out=dev(torch.zeros(2, 9)))
    with pytest.raises(ValueError, match=r"out must have shape \[2, 10\]"):
        hr.basis_apply(B, m, c, out=dev(torch.zeros(3, 10)))
    with pytest.raises(ValueError, match="out must be float32 or float64"):
        hr.basis_apply(B, m, c, out=dev(torch.zeros(2, 10, dtype=torch.int32)))
    with pytest.raises(ValueError, match="batch must be in 1 .. 64"):
        hr.basis_apply(B, m, dev(torch.zeros(65, 4, dtype=torch.float64)))
    with pytest.raises(ValueError, match="g must be float32 or float64"):
        hr.basis_apply_b(B, dev(g.to(torch.int32)))
    with pytest.raises(ValueError, match=r"g must have shape \[batch, 10\]"):
        hr.basis_apply_b(B, dev(torch.zeros(2, 11)))
    with pytest.raises(ValueError, match="g must be contiguous"):
        hr.basis_apply_b(B, dev(torch.zeros(10, 2).T))
    with pytest.raises(ValueError, match="out must be float64"):
        hr.basis_apply_b(B, gd, out=dev(torch.zeros(2, 4)))
    with pytest.raises(ValueError, match=r"out must have shape \[2, 4\]"):
        hr.basis_apply_b(B, gd, out=dev(torch.zeros(3, 4, dtype=torch.float64)))
    with pytest.raises(ValueError, match="scratch must be uint8"):
        hr.basis_apply_b(B, gd, scratch=dev(torch.zeros(64)))
    with pytest.raises(ValueError, match="batch must be in 1 .. 64"):
        hr.basis_apply_b(B, dev(torch.zeros(65, 10)))
