"""What the Python wrappers of the closest-point operators and of the sort refuse, and with which words (no GPU needed):
    python tools/closest_point_refusals.py [root of a tree of this project]
hip_renderer.chamfer, chamfer_grid, surface_distance and sort_keys of that tree (default: this one) with good, bad and doubly-bad arguments: CPU tensors
that claim to be on a device (the subclass of the ABI tests), the library replaced by one that knows the sizes only (0 bytes, 0 launches above 10^6
items).  One line per call: the exception, or how far a call that passes every check gets without a GPU.  Two trees refuse alike when their
outputs are equal byte for byte (profiles/closest_point_refactor_refusals.txt)."""
import os
import sys

ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from deodr_amd import hip_renderer as hr


class SizesOnly:
    def __getattr__(self, name):
        if name.endswith(("_scratch_bytes", "_launches")):
            return lambda *dims: 0 if max(dims) > 10**6 else 4096
        raise AssertionError(f"the library was reached ({name})")


hr.lib = SizesOnly


class OnDevice(torch.Tensor):
    is_cuda = property(lambda self: True)
    device = property(lambda self: torch.device("cuda", 0))


dev = lambda x: x.as_subclass(OnDevice)
f64 = lambda *shape: dev(torch.zeros(*shape, dtype=torch.float64))
i32 = lambda *shape: dev(torch.zeros(*shape, dtype=torch.int32))
cpu = lambda *shape: torch.zeros(*shape, dtype=torch.float64)


def show(label, function, *args, **kwargs):
    try:
        function(*args, **kwargs)
        print(f"{label}: ok")
    except Exception as e:  # (every kind: the point is what the caller sees)
        print(f"{label}: {type(e).__name__}: {str(e).splitlines()[0] if str(e) else ''}")


n, V, P, F = 2, 5, 9, 4
v, p, prm = f64(n, V, 3), f64(n, P, 3), f64(3)
faces, offsets, corners = i32(F, 3), i32(V + 1), i32(3 * F)
operators = (
    ("chamfer", lambda v=v, p=p, prm=prm, **kw: hr.chamfer(v, p, prm, **kw), "nearest_vertex"),
    ("chamfer_grid", lambda v=v, p=p, prm=prm, cell_size=0.5, **kw: hr.chamfer_grid(v, p, prm, cell_size, **kw), "nearest_vertex"),
    ("surface_distance", lambda v=v, p=p, prm=prm, faces=faces, offsets=offsets, corners=corners, **kw: hr.surface_distance(v, faces, offsets, corners, p, prm, **kw), "nearest_face"),
)  # fmt: skip
for name, call, found in operators:
    show(f"{name} good", call)
    show(f"{name} good, every optional array", call, point_weights=f64(n, P), vertex_weights=f64(V), terms=f64(n, 2), loss=f64(n), vertices_b=f64(n, V, 3),
         nearest_point=i32(n, V), scratch=dev(torch.zeros(64, dtype=torch.uint8)), want_nearest=True, **{found: i32(n, P)})  # fmt: skip
    show(f"{name} vertices cpu", call, v=cpu(n, V, 3))
    show(f"{name} vertices none", call, v=None)
    show(f"{name} vertices cpu + shape", call, v=cpu(V, 3))
    for shape in ((V, 3), (n, V, 4), (0, V, 3), (n, 0, 3), (n, V, 3, 1)):
        show(f"{name} vertices {list(shape)}", call, v=f64(*shape))
    show(f"{name} vertices shape + points shape", call, v=f64(V, 3), p=f64(P, 3))
    show(f"{name} vertices float32", call, v=dev(torch.zeros(n, V, 3)))
    show(f"{name} vertices float32 + points cpu", call, v=dev(torch.zeros(n, V, 3)), p=cpu(n, P, 3))
    show(f"{name} vertices not contiguous", call, v=f64(V, n, 3).transpose(0, 1))
    for shape in ((P, 3), (3, P, 3), (n, 0, 3), (n, P, 2)):
        show(f"{name} points {list(shape)}", call, p=f64(*shape))
    show(f"{name} points none", call, p=None)
    show(f"{name} points shape + directions", call, p=f64(P, 3), directions=0)
    show(f"{name} points cpu", call, p=cpu(n, P, 3))
    show(f"{name} points float32", call, p=dev(torch.zeros(n, P, 3)))
    show(f"{name} points cpu + params shape", call, p=cpu(n, P, 3), prm=f64(2))
    for bad in (0, 4, -1, "3", None):
        show(f"{name} directions {bad!r}", call, directions=bad)
    show(f"{name} directions + params cpu", call, directions=7, prm=cpu(3))
    show(f"{name} params [2]", call, prm=f64(2))
    show(f"{name} params cpu", call, prm=cpu(3))
    show(f"{name} params none", call, prm=None)
    show(f"{name} point_weights [P]", call, point_weights=f64(P))
    show(f"{name} point_weights + vertex_weights", call, point_weights=f64(P), vertex_weights=f64(n, V))
    show(f"{name} vertex_weights [n, V]", call, vertex_weights=f64(n, V))
    show(f"{name} vertex_weights float32", call, vertex_weights=dev(torch.zeros(V)))
    show(f"{name} terms [n]", call, terms=f64(n))
    show(f"{name} loss [1]", call, loss=f64(1))
    show(f"{name} loss cpu", call, loss=cpu(n))
    show(f"{name} vertices_b [V, 3]", call, vertices_b=f64(V, 3))
    show(f"{name} vertices_b + scratch", call, vertices_b=f64(V, 3), scratch=dev(torch.zeros(64)))
    show(f"{name} {found} int64", call, **{found: i32(n, P).long()})
    show(f"{name} {found} [n, V]", call, **{found: i32(n, V)})
    show(f"{name} {found} + nearest_point", call, nearest_point=i32(n, P), **{found: i32(n, V)})
    show(f"{name} nearest_point [n, P]", call, nearest_point=i32(n, P))
    show(f"{name} scratch float32", call, scratch=dev(torch.zeros(64)))
    show(f"{name} scratch cpu", call, scratch=torch.zeros(64, dtype=torch.uint8))
    table = (lambda V: dict(offsets=i32(V + 1))) if name == "surface_distance" else (lambda V: {})
    show(f"{name} outside the limits", call, v=f64(1, 10**6 + 1, 3), p=f64(1, 3, 3), **table(10**6 + 1))
    show(f"{name} outside the limits + scratch float32", call, v=f64(1, 10**6 + 1, 3), p=f64(1, 3, 3), scratch=dev(torch.zeros(64)), **table(10**6 + 1))
    show(f"{name} outside the limits, points", call, v=f64(1, 3, 3), p=f64(1, 10**6 + 1, 3), **table(3))
for bad in (0.0, -1.0, float("inf"), float("nan"), "x", None):
    show(f"chamfer_grid cell_size {bad!r}", operators[1][1], cell_size=bad)
show("chamfer_grid cell_size + directions", operators[1][1], cell_size=0.0, directions=0)
show("chamfer_grid cell_size + points shape", operators[1][1], cell_size=0.0, p=f64(P, 3))
show("chamfer_grid cell_size + params shape", operators[1][1], cell_size=-2.0, prm=f64(2))
surface = operators[2][1]
for shape in ((F,), (F, 4), (0, 3), (F, 3, 1)):
    show(f"surface_distance faces {list(shape)}", surface, faces=i32(*shape))
show("surface_distance faces none", surface, faces=None)
show("surface_distance faces shape + vertices shape", surface, faces=i32(F), v=f64(V, 3))
show("surface_distance faces shape + points shape", surface, faces=i32(F), p=f64(P, 3))
show("surface_distance faces int64", surface, faces=i32(F, 3).long())
show("surface_distance faces cpu", surface, faces=torch.zeros(F, 3, dtype=torch.int32))
show("surface_distance corner_offsets [V]", surface, offsets=i32(V))
show("surface_distance corner_offsets + corners", surface, offsets=i32(V), corners=i32(F))
show("surface_distance corners [F]", surface, corners=i32(F))
show("surface_distance corners float64", surface, corners=f64(3 * F))
show("surface_distance corners + points cpu", surface, corners=i32(F), p=cpu(n, P, 3))
show("surface_distance barycentric [n, P]", surface, barycentric=f64(n, P))
show("surface_distance barycentric float32", surface, barycentric=dev(torch.zeros(n, P, 3)))
show("surface_distance barycentric + nearest_face", surface, barycentric=f64(n, P), nearest_face=i32(n, V))
show("surface_distance outside the limits, faces", surface, faces=i32(10**6 + 1, 3), corners=i32(3 * (10**6 + 1)))
for label, function, dims in (("chamfer_scratch", hr.chamfer_scratch, (V, P, n)), ("chamfer_grid_scratch", hr.chamfer_grid_scratch, (V, P, n)),
                              ("surface_scratch", hr.surface_scratch, (V, F, P, n)), ("sort_keys_scratch", hr.sort_keys_scratch, (300, n, 12))):  # fmt: skip
    show(f"{label} good", function, *dims, "cuda")
    show(f"{label} outside the limits", function, 10**6 + 1, *dims[1:], "cuda")
    show(f"{label} a dimension that is no number", function, "many", *dims[1:], "cuda")
keys = i32(n, 300)
sort = lambda keys=keys, **kw: hr.sort_keys(keys, **kw)
show("sort_keys good", sort)
show("sort_keys good, every optional array", sort, bits=12, sorted_keys=i32(n, 300), order=i32(n, 300), scratch=dev(torch.zeros(64, dtype=torch.uint8)))
show("sort_keys keys cpu", sort, keys=torch.zeros(n, 300, dtype=torch.int32))
for shape in ((300,), (0, 300), (n, 0), (n, 300, 1)):
    show(f"sort_keys keys {list(shape)}", sort, keys=i32(*shape))
show("sort_keys keys shape + bits", sort, keys=i32(300), bits=0)
show("sort_keys keys float64", sort, keys=f64(n, 300))
show("sort_keys keys float64 + bits", sort, keys=f64(n, 300), bits=40)
for bad in (0, 33, -1, None):
    show(f"sort_keys bits {bad!r}", sort, bits=bad)
show("sort_keys sorted_keys [n, 299]", sort, sorted_keys=i32(n, 299))
show("sort_keys sorted_keys + order", sort, sorted_keys=i32(n, 299), order=i32(300))
show("sort_keys order int64", sort, order=i32(n, 300).long())
show("sort_keys scratch float32", sort, scratch=dev(torch.zeros(64)))
show("sort_keys outside the limits", sort, keys=i32(1, 10**6 + 1))
show("sort_keys outside the limits + order shape", sort, keys=i32(1, 10**6 + 1), order=i32(3))
