"""ctypes front-end of tests/sim/libtile_sim.so (host instantiation of the kernels' per-primitive code), libdispatch_sim.so and libhost_sim.so; tests only."""

import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sim", "tile_sim.cpp")
LIB = os.path.join(HERE, "sim", "libtile_sim.so")


class SimScene(C.Structure):
    _fields_ = (
        [(n, C.c_void_p) for n in ("faces", "faces_uv", "textured", "shaded", "edgeflags", "depths", "ij", "shade", "colors", "uv")]
        + [(n, C.c_int) for n in ("T", "V", "Vuv", "H", "W", "C", "tex_h", "tex_w", "clockwise", "culling", "strict", "persp", "ipc")]
        + [("sigma", C.c_double)]
    )


def _built(src, out, headers, defines=()):
    deps = [src] + [os.path.join(HERE, "..", "deodr_amd", "csrc", h) for h in headers]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", *defines, "-o", out, src], check=True)
    return C.CDLL(out)


def kernel_tile():
    """TILE of deodr_amd/csrc/dr_workspace.h: the simulator is compiled for the kernels' tile size"""
    with open(os.path.join(HERE, "..", "deodr_amd", "csrc", "dr_workspace.h")) as f:
        return int(re.search(r"constexpr\s+int\s+TILE\s*=\s*(\d+)\s*;", f.read()).group(1))


def lib():
    L = _built(SRC, LIB, ("dr_math.h", "dr_prims.h", "dr_binning.h", "dr_workspace.h"), (f"-DDR_SIM_TILE={kernel_tile()}",))
    L.sim_bin_counts.argtypes = [C.POINTER(SimScene), C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.sim_bin_counts.restype = C.c_int
    L.sim_prim_boxes.argtypes = [C.POINTER(SimScene), C.c_void_p, C.c_void_p]
    L.sim_set_fault.argtypes = [C.c_int]
    L.sim_tile.restype = C.c_int
    L.sim_tri_coverage.argtypes = [C.POINTER(SimScene), C.c_int, C.c_void_p]
    L.sim_edge_coverage.argtypes = [C.POINTER(SimScene), C.c_int, C.c_int, C.c_void_p]
    return L


def dispatch_lib():
    """tests/sim/libdispatch_sim.so: the instance rules and tables of deodr_amd/csrc/dr_dispatch.h (tests/sim/dispatch_sim.cpp)."""
    return _built(os.path.join(HERE, "sim", "dispatch_sim.cpp"), os.path.join(HERE, "sim", "libdispatch_sim.so"), ("dr_dispatch.h",))


def host_lib():
    """tests/sim/libhost_sim.so: the argument checks and the scratch view of deodr_amd/csrc/dr_host.h (tests/sim/host_sim.cpp)."""
    L = _built(os.path.join(HERE, "sim", "host_sim.cpp"), os.path.join(HERE, "sim", "libhost_sim.so"), ("dr_host.h",))
    for name, restype, argtypes in (
        ("host_elem_bytes", C.c_size_t, [C.c_int]), ("host_ranges_overlap", C.c_int, [C.c_size_t] * 4),
        ("host_capped_blocks", C.c_uint, [C.c_size_t, C.c_size_t, C.c_uint]), ("host_scratch_need", C.c_size_t, [C.c_size_t]),
        ("host_scratch_holds", C.c_int, [C.c_size_t] * 3), ("host_scratch_counter", C.c_size_t, [C.c_void_p, C.c_int]),
        ("host_scratch_doubles", C.c_size_t, [C.c_void_p]), ("host_any_pair_overlaps", C.c_int, [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_int]),
        ("host_carve", None, [C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t)]),
    ):  # fmt: skip
        getattr(L, name).restype, getattr(L, name).argtypes = restype, argtypes
    return L


def host_program(directory):
    """tests/sim/host_sim.cpp as a program of its own (its main walks the edge cases) with the address and undefined-behaviour sanitizers; -> its path"""
    out = os.path.join(directory, "host_sim")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DHOST_SIM_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                    os.path.join(HERE, "sim", "host_sim.cpp")], check=True)  # fmt: skip
    return out


def declared_symbols():
    """the deodr_hip_* names include/deodr_hip.h declares, found with one regular expression (not with deodr_amd/_abi.py)"""
    text = open(os.path.join(HERE, "..", "include", "deodr_hip.h")).read()
    return sorted(set(re.findall(r"\b(deodr_hip_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))


def struct_layout(struct, fields):
    """(sizeof, [(offsetof, sizeof) of every field]) of a struct of include/deodr_hip.h as the host C compiler lays it out: a few
    generated lines of C that include the header -- the judge of the ctypes mirrors that does not go through deodr_amd/_abi.py"""
    lines = "".join(f'\tprintf("%zu %zu\\n", offsetof({struct}, {f}), sizeof((({struct} *)0)->{f}));\n' for f in fields)
    source = f'#include <stdio.h>\n#include "deodr_hip.h"\nint main(void)\n{{\n\tprintf("%zu\\n", sizeof({struct}));\n{lines}\treturn 0;\n}}\n'
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "layout.c"), "w") as f:
            f.write(source)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(HERE, "..", "include"), "-o", os.path.join(tmp, "layout"),
                        os.path.join(tmp, "layout.c")], check=True)  # fmt: skip
        out = subprocess.run([os.path.join(tmp, "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    return int(out[0]), [tuple(map(int, line.split())) for line in out[1 : 1 + len(fields)]]


def assert_layout_is_the_compilers(mirror, struct, fields):
    """`mirror` (a ctypes.Structure that deodr_amd/_abi.py derived from the header) has the fields `fields` = [(name, ctypes type)], and
    its size and every field's offset and size are those the C compiler gives `struct` -- the reader that does not share _abi's parser"""
    assert [n for n, _ in fields] == [f[0] for f in mirror._fields_]
    size, layout = struct_layout(struct, [n for n, _ in fields])
    assert size == C.sizeof(mirror)
    for (name, expected), (offset, field_size) in zip(fields, layout):
        field = getattr(mirror, name)
        assert (field.offset, field.size) == (offset, field_size), name
        assert C.sizeof(expected) == field_size, name


def sim_scene(s, sigma=1.0):
    keep = dict(
        faces=np.ascontiguousarray(s.faces, np.uint32), faces_uv=np.ascontiguousarray(s.faces_uv, np.uint32),
        textured=np.ascontiguousarray(s.textured, np.uint8), shaded=np.ascontiguousarray(s.shaded, np.uint8),
        edgeflags=np.ascontiguousarray(s.edgeflags, np.uint8), depths=np.ascontiguousarray(s.depths, np.float64),
        ij=np.ascontiguousarray(s.ij, np.float64), shade=np.ascontiguousarray(s.shade, np.float64),
        colors=np.ascontiguousarray(s.colors, np.float64), uv=np.ascontiguousarray(s.uv, np.float64),
    )  # fmt: skip
    c = SimScene()
    for k, v in keep.items():
        setattr(c, k, v.ctypes.data)
    c.T, c.V, c.Vuv = len(keep["faces"]), len(keep["depths"]), len(keep["uv"])
    c.H, c.W, c.C = s.height, s.width, keep["colors"].shape[1]
    c.tex_h, c.tex_w = s.texture.shape[:2] if np.size(s.texture) else (0, 0)
    c.clockwise, c.culling, c.strict = int(s.clockwise), int(s.backface_culling), int(s.strict_edge)
    c.persp, c.ipc, c.sigma = int(s.perspective_correct), int(s.integer_pixel_centers), sigma
    return c, keep


def bin_counts(s, sigma=1.0, tile=8, exact=True):
    c, keep = sim_scene(s, sigma)
    nt = ((s.width + tile - 1) // tile) * ((s.height + tile - 1) // tile)
    tc, ec = np.zeros(nt, np.uint32), np.zeros(nt, np.uint32)
    if lib().sim_bin_counts(C.byref(c), tile, int(exact), tc.ctypes.data, ec.ctypes.data) != 0:
        raise ValueError(f"the simulator bins into the kernels' tiles of {lib().sim_tile()} pixels, not {tile}")
    return tc, ec


def prim_boxes(s, sigma=1.0):
    """-> (tri [T, 6], edge [T, 3, 6]) int32 rows (drawn, on_screen, tx0, ty0, ntx, nty): the box of tiles setup_bin_kernel walks for every
    triangle and for the band of every edge slot (drawn: the slot gets a record)"""
    c, keep = sim_scene(s, sigma)
    tri, edge = np.zeros((c.T, 6), np.int32), np.zeros((c.T, 3, 6), np.int32)
    lib().sim_prim_boxes(C.byref(c), tri.ctypes.data, edge.ctypes.data)
    return tri, edge
