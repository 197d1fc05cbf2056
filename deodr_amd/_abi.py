"""The Python side of the C ABI, derived from ``include/deodr_hip.h``: the ctypes mirrors of its two structs, its integer ``#define``s and
``restype`` / ``argtypes`` of every ``deodr_hip_*`` function it declares.  Nothing about the boundary is written out a second time.

A few regular expressions over a header the project owns, not a C parser: it takes the declarations that header contains (``typedef
struct``, prototypes, integer ``#define``s) and raises ``ImportError``, quoting the declaration, on anything else."""

import ctypes as C
import os
import re
import types

_INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER_PATH = os.path.join(_INCLUDE, "deodr_hip.h")
# The companion headers, each versioned on its own and bound onto the same library: (the parsed header's name here -- its path is that name + _PATH --,
# the file, whether its prototypes may point to the structs of deodr_hip.h)
_COMPANIONS = (
    ("TEXTURE_HEADER", "deodr_hip_texture.h", False),  # texture estimation
    ("SUBDIV_HEADER", "deodr_hip_subdiv.h", False),  # Loop subdivision
    ("RETAINED_HEADER", "deodr_hip_retained.h", True),  # fit step into retained frames
    ("BASIS_HEADER", "deodr_hip_basis.h", False),  # linear bases: morphable models
    ("CAMERA_HEADER", "deodr_hip_camera.h", False),  # camera calibration
    ("LIGHTING_HEADER", "deodr_hip_lighting.h", False),  # spherical-harmonic lighting, per-vertex albedo
    ("SKINNING_HEADER", "deodr_hip_skinning.h", False),  # linear blend skinning
    ("PYRAMID_HEADER", "deodr_hip_pyramid.h", False),  # multi-scale L2 data term
    ("SSIM_HEADER", "deodr_hip_ssim.h", False),  # structural (SSIM) data term
    ("SOLVE_HEADER", "deodr_hip_solve.h", False),  # sparse SPD solve: smoothed vertex steps
    ("ARAP_HEADER", "deodr_hip_arap.h", False),  # as-rigid-as-possible energy
    ("CHAMFER_HEADER", "deodr_hip_chamfer.h", False),  # closest-point (Chamfer) data term
    ("SURFACE_HEADER", "deodr_hip_surface.h", False),  # point-to-surface distance
    ("CHAMFER_GRID_HEADER", "deodr_hip_chamfer_grid.h", False),  # closest-point term over a uniform grid, stable sort by key
)

# C type (without `const`, without spaces around the stars) -> ctypes.  Data pointers are c_void_p: callers pass device addresses (Python
# ints, c_void_p), None, byref(...) and small ctypes arrays, and c_void_p takes all of them.  int and unsigned long long are only ever
# pointed to in HOST memory (out-parameters, the per-tensor arrays of the momentum update), where a wrong width would corrupt the
# caller: those are typed.  Pointers to the header's own structs are added as the structs are met.
_CTYPES = {
    "int": C.c_int, "double": C.c_double, "size_t": C.c_size_t, "uint32_t": C.c_uint32, "char*": C.c_char_p,
    "void*": C.c_void_p, "double*": C.c_void_p, "uint32_t*": C.c_void_p, "int32_t*": C.c_void_p, "uint8_t*": C.c_void_p, "double**": C.c_void_p,
    "int*": C.POINTER(C.c_int), "unsigned long long*": C.POINTER(C.c_ulonglong),
}  # fmt: skip


_parsing = "include/deodr_hip.h"  # the header parse() is working on, for its error texts


def _refuse(what, declaration):
    raise ImportError(f"{_parsing}: {what}: `{' '.join(declaration.split())}`")


def _ctype(c_type, ctypes_of, declaration):
    key = " ".join(re.sub(r"\bconst\b", " ", c_type).split()).replace(" *", "*").replace("* ", "*")
    if key not in ctypes_of:
        _refuse(f"no ctypes type for `{c_type.strip()}`", declaration)
    return ctypes_of[key]


def _typed_name(text, ctypes_of, declaration):
    """`const void *obs` / `double ms_sum[4]` -> (ctypes type, name); an array parameter is a pointer"""
    c_type, name, array = re.fullmatch(r"(.*?)(\w*)\s*(\[\d*\])?\s*", text, re.S).groups()
    return _ctype(c_type + ("*" if array else ""), ctypes_of, declaration), name


def parse(text, name="include/deodr_hip.h", structs=None):
    """-> namespace(name, defines {name: int}, structs {name: ctypes.Structure}, functions {name: (restype, [argtypes])}) of a header text;
    ``name``: what the header is called in error texts; ``structs``: those of a header this one includes, which its prototypes may point to"""
    global _parsing
    _parsing = name
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)  # (the extern "C" braces)
    defines = {name: int(value) for name, value in re.findall(r"^[ \t]*#define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    ctypes_of, included, structs, functions = dict(_CTYPES), structs or {}, {}, {}
    ctypes_of.update({n + "*": C.POINTER(s) for n, s in included.items()})

    def struct(m):
        fields = []
        for decl in filter(str.strip, m.group(2).split(";")):
            first, *others = decl.split(",")  # `int height, width, nb_colors`: the type of the first for all
            c_type, name = _typed_name(first, ctypes_of, decl)
            if not all(re.fullmatch(r"\s*\w+\s*", other) for other in others):
                _refuse("cannot parse", decl)
            fields += [(n.strip(), c_type) for n in [name] + others]
        structs[m.group(1)] = type(m.group(1), (C.Structure,), {"_fields_": fields, "__doc__": f"{name}::{m.group(1)}"})
        ctypes_of[m.group(1) + "*"] = C.POINTER(structs[m.group(1)])
        return " "

    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", struct, text, flags=re.S)
    for decl in filter(str.strip, text.split(";")):
        m = re.fullmatch(r"(.*?)\b(deodr_hip_\w+)\s*\((.*)\)\s*", decl, re.S)
        if not m:
            _refuse("cannot parse", decl)
        restype = None if m.group(1).split() == ["void"] else _ctype(m.group(1), ctypes_of, decl)
        params = [] if m.group(3).split() == ["void"] else m.group(3).split(",")
        functions[m.group(2)] = (restype, [_typed_name(p, ctypes_of, decl)[0] for p in params])
    return types.SimpleNamespace(name=name, defines=defines, structs=structs, functions=functions)


def bind(library, header=None):
    """Set restype / argtypes of every function the header declares on a loaded ``ctypes.CDLL``; -> the library."""
    header = header or HEADER
    for name, (restype, argtypes) in header.functions.items():
        if not hasattr(library, name):
            raise ImportError(f"{library._name} does not export {name}, which {getattr(header, 'name', 'include/deodr_hip.h')} declares; rebuild it")
        function = getattr(library, name)
        function.restype, function.argtypes = restype, argtypes
    return library


def _parse_file(path, structs=None):
    with open(path) as f:
        return parse(f.read(), "include/" + os.path.basename(path), structs)


HEADER = _parse_file(HEADER_PATH)
for _name, _file, _sees_structs in _COMPANIONS:
    globals()[_name + "_PATH"] = os.path.join(_INCLUDE, _file)
    globals()[_name] = _parse_file(globals()[_name + "_PATH"], HEADER.structs if _sees_structs else None)
