"""CPU checks of every STAGED companion header include_staged/deodr_hip_{key}.h, one test id per row of ``_abi.STAGED`` -- every check
tests/test_companion_headers.py gives a companion: the header parses with the parser of deodr_hip.h and is versioned on its own, its functions, its
defines and every prototype are what ``PINNED`` spells out, it shares no name with the main header, with any companion or with any other staged
header, the cross-compiled library exports every name and binds it with the declared types, its version is the same on both sides, it is among the
files that decide whether the library is stale, and include_staged/ holds no orphan file."""

import ctypes as C
import glob
import os
import re

import pytest

import __graft_entry__ as g
import surface_grid_reference as sg
from deodr_amd import _abi

p, i, z, d = C.c_void_p, C.c_int, C.c_size_t, C.c_double

# key -> (defines, {function: (restype, [argtypes])})
PINNED = {
    "surface_grid": ({"DEODR_HIP_SURFACE_GRID_NONE": sg.NONE, "DEODR_HIP_SURFACE_GRID_GATHER_FACES": sg.GATHER_FACES, "DEODR_HIP_SURFACE_GRID_ABI_VERSION": 1}, {
        "deodr_hip_surface_grid": (i, [p, i, p, i, p, p, p, i, p, p, p, d, i, i, p, p, p, p, p, p, p, z, p]),  # deodr_hip_surface_distance's and cell_size: 23 parameters
        "deodr_hip_surface_grid_scratch_bytes": (z, [i, i, i, i]),
        "deodr_hip_surface_grid_launches": (i, [i, i, i, i, i]),
        "deodr_hip_surface_grid_abi_version": (i, []),
    }),
}  # fmt: skip


@pytest.mark.parametrize("row", _abi.STAGED, ids=lambda row: row.key)
def test_staged_header_is_pinned_disjoint_exported_bound_and_a_source(row):
    from deodr_amd import hip_renderer as hr

    KEY = row.key.upper()
    h, path = getattr(_abi, KEY + "_HEADER"), getattr(_abi, KEY + "_HEADER_PATH")
    defines, functions = PINNED[row.key]
    version = defines[f"DEODR_HIP_{KEY}_ABI_VERSION"]
    # it parses, and is what the pins say
    assert h.name == f"include_staged/deodr_hip_{row.key}.h" and path == os.path.join(g.ROOT, "include_staged", f"deodr_hip_{row.key}.h")
    assert sorted(h.functions) == sorted(functions)
    assert h.defines == defines and h.structs == {}
    assert re.search(rf"#define\s+DEODR_HIP_{KEY}_ABI_VERSION\s+{version}\b", open(path).read())
    for name, pinned in functions.items():
        assert h.functions[name] == pinned, name
        assert len(h.parameters[name]) == len(pinned[1]) and all(h.parameters[name]), name
    # no name of it is the main header's, a companion's or any other staged header's
    for other in [_abi.HEADER] + [getattr(_abi, c.key.upper() + "_HEADER") for c in _abi.COMPANIONS + _abi.STAGED if c is not row]:
        assert not set(h.functions) & set(other.functions) and not set(h.defines) & set(other.defines), other.name
    # the library exports every name, and is of the header's version
    raw = C.CDLL(g.build_hip())
    for name in functions:
        assert hasattr(raw, name), name
    assert getattr(raw, f"deodr_hip_{row.key}_abi_version")() == version == getattr(hr, KEY + "_ABI_VERSION") == _abi.companion(row)[1]
    L = hr.lib()  # binds every header
    for name, (restype, argtypes) in h.functions.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    # a change of the header rebuilds the library
    assert path in g.hip_sources()


def test_the_staged_table_is_the_headers_on_disk_and_shares_no_key_with_the_companions():
    on_disk = sorted(glob.glob(os.path.join(g.ROOT, "include_staged", "deodr_hip_*.h")))
    assert on_disk == sorted(getattr(_abi, c.key.upper() + "_HEADER_PATH") for c in _abi.STAGED)  # no orphan header, no dangling or doubled row
    assert sorted(PINNED) == sorted(c.key for c in _abi.STAGED)
    assert sorted(os.listdir(os.path.join(g.ROOT, "include_staged"))) == sorted(os.path.basename(f) for f in on_disk)  # no orphan file
    assert not {c.key for c in _abi.STAGED} & {c.key for c in _abi.COMPANIONS}
    assert not any(os.path.exists(os.path.join(g.ROOT, "include", os.path.basename(f))) for f in on_disk)  # staged, or a companion: not both


def test_the_surface_grid_header_builds_on_its_two_parents_and_redefines_none_of_their_constants():
    text = open(_abi.SURFACE_GRID_HEADER_PATH).read()
    assert '#include "../include/deodr_hip_surface.h"' in text and '#include "../include/deodr_hip_chamfer_grid.h"' in text  # (by path: no flag of the build is needed)
    for name in ("RINGS", "CELL_LIMIT", "MAX_ITEMS"):
        assert f"#define DEODR_HIP_CHAMFER_GRID_{name}" not in text and f"DEODR_HIP_SURFACE_GRID_{name}" not in text
    assert not any(flag.startswith("-I") for flag in g.HIPCC_FLAGS)  # every tool that compiles dr_kernels.hip with its own flags still builds
