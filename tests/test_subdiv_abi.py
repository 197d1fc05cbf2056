"""CPU checks of Loop subdivision at the C ABI (include/deodr_hip_subdiv.h; the header itself: tests/test_companion_headers.py): a library that
lacks a declared symbol is refused by name, the instance rule, every bad argument of deodr_hip_subdiv_apply is refused with a message before any
launch (fake pointers, no GPU), and the host wrapper refuses CPU tensors without reaching the library."""

import ctypes as C

import pytest


def test_a_library_that_lacks_a_declared_symbol_is_refused_by_name():
    import __graft_entry__ as g
    from deodr_amd import _abi

    more = _abi.parse(open(_abi.SUBDIV_HEADER_PATH).read().replace("int deodr_hip_subdiv_abi_version(void);",
                                                                   "int deodr_hip_subdiv_abi_version(void);\nint deodr_hip_subdiv_not_there(int on);"),
                      "include/deodr_hip_subdiv.h")  # fmt: skip
    with pytest.raises(ImportError, match=r"deodr_hip_subdiv_not_there, which include/deodr_hip_subdiv\.h declares"):
        _abi.bind(C.CDLL(g.build_hip()), more)


def test_instance_rule():
    """8 adjacent lanes per row below 32 entries per row on average, a wavefront per row from there on: the matrices of the hand"""
    from deodr_amd import hip_renderer as hr

    assert hr.sparse_rows_lanes(2098, 9958) == 8 and hr.sparse_rows_lanes(526, 9958) == 8  # one level: S, S^T
    assert hr.sparse_rows_lanes(8386, 67930) == 8 and hr.sparse_rows_lanes(526, 67930) == 64  # two levels
    assert hr.sparse_rows_lanes(33538, 340306) == 8 and hr.sparse_rows_lanes(526, 340306) == 64  # three levels
    assert hr.sparse_rows_lanes(10, 319) == 8 and hr.sparse_rows_lanes(10, 320) == 64
    assert hr.sparse_rows_lanes(0, 5) == 0 and hr.sparse_rows_lanes(-1, 5) == 0


def test_subdiv_apply_rejects_bad_arguments_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from abi_cases import entry, nulls
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    F32, F64, MAXC = _abi.HEADER.defines["DEODR_HIP_F32"], _abi.HEADER.defines["DEODR_HIP_F64"], _abi.HEADER.defines["DEODR_HIP_MAX_COLORS"]
    offsets, cols, vals, x, y = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000

    base = dict(offsets=offsets, cols=cols, vals=vals, x=x, y=y)
    apply = entry(L, _abi.SUBDIV_HEADER, "deodr_hip_subdiv_apply", base, n_rows=100, n_cols=50, nnz=400, batch=2, D=3, dtype=F64, accumulate=0)

    for bad in nulls(base):
        rc, msg = apply(**bad)
        assert rc == 1 and "== NULL" in msg, (bad, msg)
    for bad in (dict(n_rows=0), dict(n_rows=-3), dict(n_cols=0), dict(n_cols=-1), dict(nnz=0)):
        assert apply(**bad) == (1, "subdiv_apply: n_rows, n_cols and nnz must be positive"), bad
    for bad in (dict(batch=0), dict(batch=-1), dict(batch=65536)):
        assert apply(**bad) == (1, "subdiv_apply: batch must be in 1 .. 65535"), bad
    for bad in (dict(D=0), dict(D=-1), dict(D=MAXC + 1)):
        assert apply(**bad) == (1, "subdiv_apply: D out of range"), bad
    for bad in (dict(dtype=2), dict(dtype=-1), dict(dtype=7)):
        assert apply(**bad) == (1, "unknown dtype tag"), bad
    # y aliasing x: x is 2 x 50 x 3 doubles = 2 400 bytes, y 2 x 100 x 3 doubles = 4 800 bytes (float32: half of each)
    for y_at, dtype in ((x, F64), (x + 2400 - 8, F64), (x - 4800 + 8, F64), (x + 1200 - 4, F32), (x - 2400 + 4, F32)):
        rc, msg = apply(y=y_at, dtype=dtype)
        assert rc == 1 and msg == "subdiv_apply: y must not overlap x", (y_at, msg)
    for bad in (dict(x=x + 4), dict(y=y + 2, dtype=F32), dict(offsets=offsets + 2), dict(cols=cols + 1), dict(vals=vals + 4)):
        rc, msg = apply(**bad)
        assert rc == 1 and "misaligned" in msg, bad


def test_host_wrapper_checks_its_tensors_before_the_library(monkeypatch):
    import torch

    from abi_cases import no_library
    from deodr_amd import hip_renderer as hr

    monkeypatch.setattr(hr, "lib", no_library)
    offsets, cols = torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32)
    vals, x = torch.ones(2, dtype=torch.float64), torch.zeros(1, 2, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.sparse_rows_apply(offsets, cols, vals, x)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.sparse_rows_apply(offsets, cols, vals, x, out=torch.zeros(1, 2, 3, dtype=torch.float64), accumulate=True)
