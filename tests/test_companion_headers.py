"""CPU checks of every companion header include/deodr_hip_{key}.h, one test id per row of ``_abi.COMPANIONS``: the header parses with the parser of
deodr_hip.h and is versioned on its own, its functions, its defines and every prototype are what ``PINNED`` spells out, it shares no name with the
main header or with any other companion, the cross-compiled library exports every name and binds it with the declared types, its version is the
same on both sides, and it is among the files that decide whether the library is stale.  What only one family checks is in that family's file."""

import ctypes as C
import glob
import os
import re

import pytest

import __graft_entry__ as g
import chamfer_grid_reference as gr
from deodr_amd import _abi

p, i, z, d, u = C.c_void_p, C.c_int, C.c_size_t, C.c_double, C.c_uint32
scene, options = C.POINTER(_abi.HEADER.structs["DeodrHipScene"]), C.POINTER(_abi.HEADER.structs["DeodrHipFitOptions"])
MAX_PAIRS = 2**32
DEFINES = {"ABI_VERSION": 1, "POINTS_TO_MESH": 1, "MESH_TO_POINTS": 2, "BLOCK": 256, "TILE": 256, "MAX_BLOCKS": 512, "TARGET_BLOCKS": 1024, "MAX_SEGMENTS": 64,
           "MAX_PAIRS": 2**36}  # fmt: skip

# key -> (defines, {function: (restype, [argtypes])}), each literal as the family's own test file pinned it
PINNED = {
    "texture": ({"DEODR_HIP_TEXTURE_ABI_VERSION": 1}, {
        "deodr_hip_texture_smoothness": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
        "deodr_hip_texture_step": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_double] * 4 + [C.c_int, C.c_double, C.c_double, C.c_void_p]),
        "deodr_hip_texture_scratch_bytes": (C.c_size_t, [C.c_int] * 3),
        "deodr_hip_texture_abi_version": (C.c_int, []),
    }),
    "subdiv": ({"DEODR_HIP_SUBDIV_ABI_VERSION": 1}, {
        "deodr_hip_subdiv_apply": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]),
        "deodr_hip_subdiv_lanes": (C.c_int, [C.c_int, C.c_uint32]),
        "deodr_hip_subdiv_abi_version": (C.c_int, []),
    }),
    "retained": ({"DEODR_HIP_RETAINED_ABI_VERSION": 1}, {
        "deodr_hip_render_scene_fit_retained": (C.c_int, [scene, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int, options, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
        "deodr_hip_retained_abi_version": (C.c_int, []),
    }),
    "basis": ({"DEODR_HIP_BASIS_ABI_VERSION": 1}, {
        "deodr_hip_basis_apply": (i, [p, p, p, i, i, i, i, p, i, p]),
        "deodr_hip_basis_apply_b": (i, [p, p, i, i, i, i, i, p, i, p, C.c_size_t, p]),
        "deodr_hip_basis_scratch_bytes": (C.c_size_t, [i, i, i]),
        "deodr_hip_basis_segments": (i, [i, i]),
        "deodr_hip_basis_abi_version": (i, []),
    }),
    "camera": ({"DEODR_HIP_CAMERA_ABI_VERSION": 1}, {
        "deodr_hip_camera_project_b": (i, [p, p, p, p, p, p, p, p, p, p, i, i, i, p, z, p]),
        "deodr_hip_camera_blocks": (i, [i, i]),
        "deodr_hip_camera_scratch_bytes": (z, [i, i]),
        "deodr_hip_camera_assemble": (i, [p, p, p, p, p, i, p, p, p, i, p]),
        "deodr_hip_camera_assemble_b": (i, [p, p, p, p, i, p, p, p, p, p, i, p]),
        "deodr_hip_camera_abi_version": (i, []),
    }),
    "lighting": ({"DEODR_HIP_LIGHTING_ABI_VERSION": 1}, {
        "deodr_hip_sh_shade": (i, [p, p, p, p, p, i, p, i, i, p, p, i, i, i, p]),  # 15 parameters
        "deodr_hip_sh_shade_b": (i, [p, p, p, p, p, i, p, i, i, p, p, p, p, p, i, p, z, i, i, i, p]),  # 21 parameters
        "deodr_hip_sh_scratch_bytes": (z, [i, i, i]),
        "deodr_hip_sh_blocks": (i, [i, i]),
        "deodr_hip_lighting_abi_version": (i, []),
    }),
    "skinning": ({"DEODR_HIP_SKINNING_ABI_VERSION": 1}, {
        "deodr_hip_skin_apply": (i, [p, p, p, p, p, p, p, p, i, i, i, i, p]),  # 13 parameters
        "deodr_hip_skin_apply_b": (i, [p, p, p, p, p, p, p, p, p, p, i, p, p, p, p, z, i, i, i, i, p]),  # 21 parameters
        "deodr_hip_skin_scratch_bytes": (z, [i, i, i, i]),
        "deodr_hip_skinning_abi_version": (i, []),
    }),
    "pyramid": ({"DEODR_HIP_PYRAMID_ABI_VERSION": 1, "DEODR_HIP_PYRAMID_MAX_LEVELS": 8}, {
        "deodr_hip_pyramid_l2": (i, [p, p, p, i, i, i, i, i, i, p, p, p, p, p, z, p]),  # 16 parameters
        "deodr_hip_pyramid_scratch_bytes": (z, [i, i, i, i, i]),
        "deodr_hip_pyramid_abi_version": (i, []),
    }),
    "ssim": ({"DEODR_HIP_SSIM_ABI_VERSION": 1, "DEODR_HIP_SSIM_WINDOW": 11}, {
        "deodr_hip_ssim_l2": (i, [p, p, p, i, i, i, i, i, d, p, p, p, p, p, z, p]),  # 16 parameters
        "deodr_hip_ssim_scratch_bytes": (z, [i, i, i, i]),
        "deodr_hip_ssim_abi_version": (i, []),
    }),
    "solve": ({"DEODR_HIP_SOLVE_ABI_VERSION": 1, "DEODR_HIP_SOLVE_N_SMALL": 1024}, {
        "deodr_hip_spd_solve": (i, [p, p, p, i, u, p, p, i, i, d, p, p, z, p]),  # 14 parameters
        "deodr_hip_spd_solve_scratch_bytes": (z, [i, i]),
        "deodr_hip_spd_solve_launches": (i, [i, u, i, i]),
        "deodr_hip_solve_abi_version": (i, []),
    }),
    "arap": ({"DEODR_HIP_ARAP_ABI_VERSION": 1, "DEODR_HIP_ARAP_SWEEPS": 5, "DEODR_HIP_ARAP_BLOCK": 256, "DEODR_HIP_ARAP_MAX_BLOCKS": 512}, {
        "deodr_hip_arap_energy": (i, [p, p, p, i, u, p, p, i, d, p, p, p, p, z, p]),  # 15 parameters
        "deodr_hip_arap_scratch_bytes": (z, [i, i]),
        "deodr_hip_arap_launches": (i, [i, u, i]),
        "deodr_hip_arap_blocks": (i, [i]),
        "deodr_hip_arap_abi_version": (i, []),
    }),
    "chamfer": ({"DEODR_HIP_CHAMFER_" + k: v for k, v in DEFINES.items()}, {
        "deodr_hip_chamfer": (i, [p, i, p, i, p, p, p, i, i, p, p, p, p, p, p, z, p]),  # 17 parameters
        "deodr_hip_chamfer_scratch_bytes": (z, [i, i, i]),
        "deodr_hip_chamfer_launches": (i, [i, i, i, i]),
        "deodr_hip_chamfer_segments": (i, [i, i]),
        "deodr_hip_chamfer_abi_version": (i, []),
    }),
    "surface": ({"DEODR_HIP_SURFACE_ABI_VERSION": 1, "DEODR_HIP_SURFACE_MAX_PAIRS": MAX_PAIRS}, {
        "deodr_hip_surface_distance": (i, [p, i, p, i, p, p, p, i, p, p, p, i, i, p, p, p, p, p, p, p, z, p]),  # 22 parameters
        "deodr_hip_surface_distance_scratch_bytes": (z, [i, i, i, i]),
        "deodr_hip_surface_distance_launches": (i, [i, i, i, i, i]),
        "deodr_hip_surface_abi_version": (i, []),
    }),
    "chamfer_grid": ({"DEODR_HIP_SORT_DIGIT_BITS": gr.DIGIT_BITS, "DEODR_HIP_SORT_BLOCK": gr.SORT_BLOCK, "DEODR_HIP_SORT_ITEMS": gr.SORT_ITEMS,
                      "DEODR_HIP_SORT_MAX_ITEMS": gr.SORT_MAX_ITEMS, "DEODR_HIP_CHAMFER_GRID_NONE": 0xFFFFFFFF, "DEODR_HIP_CHAMFER_GRID_RINGS": gr.RINGS, "DEODR_HIP_CHAMFER_GRID_TABLE_LOAD": gr.TABLE_LOAD,
                      "DEODR_HIP_CHAMFER_GRID_CELL_LIMIT": gr.CELL_LIMIT, "DEODR_HIP_CHAMFER_GRID_MAX_ITEMS": gr.MAX_ITEMS, "DEODR_HIP_CHAMFER_GRID_MIN_TABLE_BITS": gr.MIN_TABLE_BITS,
                      "DEODR_HIP_CHAMFER_GRID_MAX_TABLE_BITS": gr.MAX_TABLE_BITS, "DEODR_HIP_CHAMFER_GRID_GATHER_VERTICES": gr.GATHER_VERTICES,
                      "DEODR_HIP_CHAMFER_GRID_ABI_VERSION": 1}, {
        "deodr_hip_sort_keys": (i, [p, i, i, i, p, p, p, z, p]),
        "deodr_hip_sort_keys_scratch_bytes": (z, [i, i, i]),
        "deodr_hip_sort_keys_launches": (i, [i, i, i]),
        "deodr_hip_chamfer_grid": (i, [p, i, p, i, p, p, p, d, i, i, p, p, p, p, p, p, z, p]),  # deodr_hip_chamfer's and cell_size
        "deodr_hip_chamfer_grid_scratch_bytes": (z, [i, i, i]),
        "deodr_hip_chamfer_grid_launches": (i, [i, i, i, i]),
        "deodr_hip_chamfer_grid_table_bits": (i, [i]),
        "deodr_hip_chamfer_grid_abi_version": (i, []),
    }),
}  # fmt: skip


@pytest.mark.parametrize("row", _abi.COMPANIONS, ids=lambda row: row.key)
def test_companion_header_is_pinned_disjoint_exported_bound_and_a_source(row):
    from deodr_amd import hip_renderer as hr

    KEY = row.key.upper()
    h, path = getattr(_abi, KEY + "_HEADER"), getattr(_abi, KEY + "_HEADER_PATH")
    defines, functions = PINNED[row.key]
    version = defines[f"DEODR_HIP_{KEY}_ABI_VERSION"]
    # it parses, and is what the pins say
    assert h.name == f"include/deodr_hip_{row.key}.h" and path == os.path.join(g.ROOT, "include", f"deodr_hip_{row.key}.h")
    assert sorted(h.functions) == sorted(functions)
    assert h.defines == defines and h.structs == {}
    assert re.search(rf"#define\s+DEODR_HIP_{KEY}_ABI_VERSION\s+{version}\b", open(path).read())
    for name, pinned in functions.items():
        assert h.functions[name] == pinned, name
        assert len(h.parameters[name]) == len(pinned[1]) and all(h.parameters[name]), name
    # no name of it is the main header's or any other companion's
    for other in [_abi.HEADER] + [getattr(_abi, c.key.upper() + "_HEADER") for c in _abi.COMPANIONS if c is not row]:
        assert not set(h.functions) & set(other.functions) and not set(h.defines) & set(other.defines), other.name
    # the library exports every name, and is of the header's version
    raw = C.CDLL(g.build_hip())
    for name in functions:
        assert hasattr(raw, name), name
    assert getattr(raw, f"deodr_hip_{row.key}_abi_version")() == version == getattr(hr, KEY + "_ABI_VERSION")
    L = hr.lib()  # binds every header
    for name, (restype, argtypes) in h.functions.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    # a change of the header rebuilds the library
    assert path in g.hip_sources()


def test_the_table_is_the_headers_on_disk_and_the_main_header_is_a_source():
    on_disk = sorted(glob.glob(os.path.join(g.ROOT, "include", "deodr_hip_*.h")))
    assert on_disk == sorted(getattr(_abi, c.key.upper() + "_HEADER_PATH") for c in _abi.COMPANIONS)  # no orphan header, no dangling or doubled row
    assert sorted(PINNED) == sorted(c.key for c in _abi.COMPANIONS)
    assert sorted(os.listdir(os.path.join(g.ROOT, "include"))) == sorted(["deodr_hip.h"] + [os.path.basename(f) for f in on_disk])
    assert _abi.HEADER_PATH in g.hip_sources() and _abi.HEADER_PATH == os.path.join(g.ROOT, "include", "deodr_hip.h")
