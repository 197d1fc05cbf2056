"""The Python side of the C ABI, derived from ``include/deodr_hip.h``: the ctypes mirrors of its two structs, its integer ``#define``s and
``restype`` / ``argtypes`` of every ``deodr_hip_*`` function it declares.  Nothing about the boundary is written out a second time.

A few regular expressions over a header the project owns, not a C parser: it takes the declarations that header contains (``typedef
struct``, prototypes, integer ``#define``s) and raises ``ImportError``, quoting the declaration, on anything else."""

import collections
import ctypes as C
import os
import re
import types

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_INCLUDE, _INCLUDE_STAGED = os.path.join(_ROOT, "include"), os.path.join(_ROOT, "include_staged")
HEADER_PATH = os.path.join(_INCLUDE, "deodr_hip.h")
# The companion headers, each versioned on its own and bound onto the same library; the only list of them.  Everything else follows from `key`: the
# file include/deodr_hip_{key}.h, the parsed header {KEY}_HEADER here and its path {KEY}_HEADER_PATH, DEODR_HIP_{KEY}_ABI_VERSION and
# deodr_hip_{key}_abi_version().  sees_structs: whether its prototypes may point to the structs of deodr_hip.h; words: what a version mismatch is called
Companion = collections.namedtuple("Companion", "key sees_structs words")
COMPANIONS = (
    Companion("texture", False, "texture"),  # texture estimation
    Companion("subdiv", False, "subdivision"),  # Loop subdivision
    Companion("retained", True, "retained-frames"),  # fit step into retained frames
    Companion("basis", False, "linear-basis"),  # linear bases: morphable models
    Companion("camera", False, "camera"),  # camera calibration
    Companion("lighting", False, "lighting"),  # spherical-harmonic lighting, per-vertex albedo
    Companion("skinning", False, "skinning"),  # linear blend skinning
    Companion("pyramid", False, "pyramid-loss"),  # multi-scale L2 data term
    Companion("ssim", False, "ssim-loss"),  # structural (SSIM) data term
    Companion("solve", False, "sparse-solve"),  # sparse SPD solve: smoothed vertex steps
    Companion("arap", False, "arap-energy"),  # as-rigid-as-possible energy
    Companion("chamfer", False, "chamfer-term"),  # closest-point (Chamfer) data term
    Companion("surface", False, "surface-distance"),  # point-to-surface distance
    Companion("chamfer_grid", False, "chamfer-grid"),  # closest-point term over a uniform grid, stable sort by key
)
# The STAGED companions: the same rows, the same derived names, bound and version-checked by hip_renderer.lib() like the others, but their headers
# live in include_staged/.  A family waits here while the table above cannot change; the next change of that table moves the header into include/
# and the row into COMPANIONS ("Adding an operator family").
STAGED = (
    Companion("surface_grid", False, "surface-grid"),  # point-to-surface distance over a uniform grid of triangles
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
    """-> namespace(name, defines {name: int}, structs {name: ctypes.Structure}, functions {name: (restype, [argtypes])}, parameters {name: [names]})
    of a header text;
    ``name``: what the header is called in error texts; ``structs``: those of a header this one includes, which its prototypes may point to"""
    global _parsing
    _parsing = name
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)  # (the extern "C" braces)
    defines = {name: int(value) for name, value in re.findall(r"^[ \t]*#define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    ctypes_of, included, structs, functions, parameters = dict(_CTYPES), structs or {}, {}, {}, {}
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
        typed = [_typed_name(p, ctypes_of, decl) for p in params]
        functions[m.group(2)], parameters[m.group(2)] = (restype, [c_type for c_type, _ in typed]), [name for _, name in typed]
    return types.SimpleNamespace(name=name, defines=defines, structs=structs, functions=functions, parameters=parameters)


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
        return parse(f.read(), os.path.basename(os.path.dirname(path)) + "/" + os.path.basename(path), structs)


HEADER = _parse_file(HEADER_PATH)
for _c in COMPANIONS + STAGED:
    _path = os.path.join(_INCLUDE if _c in COMPANIONS else _INCLUDE_STAGED, f"deodr_hip_{_c.key}.h")
    globals()[_c.key.upper() + "_HEADER_PATH"], globals()[_c.key.upper() + "_HEADER"] = _path, _parse_file(_path, HEADER.structs if _c.sees_structs else None)


def companion(c):
    """-> (parsed header, its DEODR_HIP_{KEY}_ABI_VERSION) of a row of COMPANIONS or STAGED"""
    header = globals()[c.key.upper() + "_HEADER"]
    return header, header.defines[f"DEODR_HIP_{c.key.upper()}_ABI_VERSION"]
