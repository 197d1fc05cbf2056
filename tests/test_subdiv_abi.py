"""CPU checks of the companion header include/deodr_hip_subdiv.h (Loop subdivision): it parses with the parser of deodr_hip.h and shares no name
with the other two headers, every name it declares is exported by the cross-compiled library and bound with the declared types, its version is 1 on
both sides, every bad argument of deodr_hip_subdiv_apply is refused with a message before any launch (fake pointers, no GPU), and the host
wrapper refuses CPU tensors without reaching the library."""

import ctypes as C
import re

import pytest

SUBDIV_FUNCTIONS = ["deodr_hip_subdiv_apply", "deodr_hip_subdiv_lanes", "deodr_hip_subdiv_abi_version"]


def test_companion_header_parses_and_is_versioned_on_its_own():
    from deodr_amd import _abi

    h = _abi.SUBDIV_HEADER
    assert sorted(h.functions) == sorted(SUBDIV_FUNCTIONS)
    assert h.defines == {"DEODR_HIP_SUBDIV_ABI_VERSION": 1} and h.structs == {}
    assert h.name == "include/deodr_hip_subdiv.h"
    for other in (_abi.HEADER, _abi.TEXTURE_HEADER):  # disjoint from the other two headers
        assert not set(h.functions) & set(other.functions) and not set(h.defines) & set(other.defines)
    text = open(_abi.SUBDIV_HEADER_PATH).read()
    assert re.search(r"#define\s+DEODR_HIP_SUBDIV_ABI_VERSION\s+1\b", text)
    restype, argtypes = h.functions["deodr_hip_subdiv_apply"]
    assert restype is C.c_int
    assert argtypes == [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]
    assert h.functions["deodr_hip_subdiv_lanes"] == (C.c_int, [C.c_int, C.c_uint32])
    assert h.functions["deodr_hip_subdiv_abi_version"] == (C.c_int, [])


def test_library_exports_and_binds_every_name_of_the_companion_header():
    import __graft_entry__ as g
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    raw = C.CDLL(g.build_hip())
    for name in SUBDIV_FUNCTIONS:
        assert hasattr(raw, name), name
    assert raw.deodr_hip_subdiv_abi_version() == 1 == hr.SUBDIV_ABI_VERSION
    L = hr.lib()  # binds the three headers
    for name, (restype, argtypes) in _abi.SUBDIV_HEADER.functions.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
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
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    F32, F64, MAXC = _abi.HEADER.defines["DEODR_HIP_F32"], _abi.HEADER.defines["DEODR_HIP_F64"], _abi.HEADER.defines["DEODR_HIP_MAX_COLORS"]
    offsets, cols, vals, x, y = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000

    def apply(offsets=offsets, cols=cols, vals=vals, n_rows=100, n_cols=50, nnz=400, x=x, y=y, batch=2, D=3, dtype=F64, accumulate=0):
        rc = L.deodr_hip_subdiv_apply(offsets, cols, vals, n_rows, n_cols, nnz, x, y, batch, D, dtype, accumulate, None)
        return rc, L.deodr_hip_last_error().decode()

    for p in ("offsets", "cols", "vals", "x", "y"):
        rc, msg = apply(**{p: None})
        assert rc == 1 and "== NULL" in msg, (p, msg)
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

    from deodr_amd import hip_renderer as hr

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(hr, "lib", no_library)
    offsets, cols = torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32)
    vals, x = torch.ones(2, dtype=torch.float64), torch.zeros(1, 2, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.sparse_rows_apply(offsets, cols, vals, x)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.sparse_rows_apply(offsets, cols, vals, x, out=torch.zeros(1, 2, 3, dtype=torch.float64), accumulate=True)
