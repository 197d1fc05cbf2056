"""What the Python wrappers of the library's operators refuse, and with which words (no GPU needed):
    python tools/wrapper_refusals.py [--family closest_point|image_terms] [root of a tree of this project]
The wrappers of that tree (default: this one) with good, bad and doubly-bad arguments: CPU tensors that claim to be on a device (the subclass of the
ABI tests), the library replaced by one that knows the sizes only (0 bytes, 0 launches above 10^6 items).  One line per call: the exception, or how
far a call that passes every check gets without a GPU.  Two trees refuse alike when their outputs are equal byte for byte.
``closest_point`` (the default): hip_renderer.chamfer, chamfer_grid, surface_distance, sort_keys and their four ``*_scratch`` functions
(profiles/closest_point_refactor_refusals.txt).
``image_terms``: pyramid_l2 and ssim_l2, all thirteen ``*_scratch`` functions, and the ``scratch=None`` path of the thirteen wrappers that keep a scratch
per stream, with and without a capture reported as on (profiles/image_terms_refactor_refusals.txt).  There ``torch.zeros`` / ``torch.empty`` of this
process refuse a device in words of this tool's, so that a line also says what a call would have allocated."""
import argparse
import contextlib
import os
import sys
import types

ap = argparse.ArgumentParser()
ap.add_argument("--family", choices=("closest_point", "image_terms"), default="closest_point")
ap.add_argument("root", nargs="?", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FAMILY, ROOT = ap.parse_args().family, os.path.abspath(ap.parse_args().root)
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


def closest_point():
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


def image_terms():
    capturing = [False]
    torch.cuda.device = lambda device: contextlib.nullcontext()
    torch.cuda.current_stream = lambda device=None: types.SimpleNamespace(cuda_stream=0)
    torch.cuda.is_current_stream_capturing = lambda: capturing[0]

    def no_gpu(name, allocate):
        def stand_in(*args, **kwargs):
            if kwargs.get("device") is not None and torch.device(kwargs["device"]).type == "cuda":
                raise RuntimeError(f"no GPU: torch.{name}({', '.join(map(str, args))}, dtype={kwargs.get('dtype')})")
            return allocate(*args, **kwargs)

        return stand_in

    torch.zeros, torch.empty = no_gpu("zeros", torch.zeros), no_gpu("empty", torch.empty)
    u8 = lambda count=64: dev(torch.zeros(count, dtype=torch.uint8))
    f32 = lambda *shape: dev(torch.zeros(*shape, dtype=torch.float32))
    n, H, W, C, levels = 2, 20, 30, 3, 5
    image, obs = f64(n, H, W, C), f64(n, H, W, C)
    terms = (
        ("pyramid_l2", lambda image=image, obs=obs, weights=None, number=levels, array=f64(levels + 1), **kw: hr.pyramid_l2(image, obs, weights, number, array, **kw),
         "level_weights", levels + 1, (0, 9, -1, 2.5, "3", None)),
        ("ssim_l2", lambda image=image, obs=obs, weights=None, number=1.0, array=f64(2), **kw: hr.ssim_l2(image, obs, weights, array, number, **kw),
         "mix", 2, (0.0, -1.0, float("inf"), float("nan"), "x", None)),
    )  # fmt: skip
    for name, call, array, length, bad_numbers in terms:
        given = dict(weights=f64(n, H, W), terms=f64(length), loss=f64(1), image_b=f64(n, H, W, C), scratch=u8())
        show(f"{name} good", call)
        show(f"{name} good, no gradient", call, want_gradient=False)
        show(f"{name} good, every optional array", call, **given)
        show(f"{name} good, every optional array, float32", call, image=f32(n, H, W, C), obs=f32(n, H, W, C), **dict(given, weights=f32(n, H, W), image_b=f32(n, H, W, C)))
        show(f"{name} image cpu", call, image=cpu(n, H, W, C))
        show(f"{name} image none", call, image=None)
        for shape in ((H, W, C), (n, H, W), (0, H, W, C), (n, 0, W, C), (n, H, W, 0), (n, H, W, C, 1)):
            show(f"{name} image {list(shape)}", call, image=f64(*shape))
        show(f"{name} image int32", call, image=i32(n, H, W, C))
        show(f"{name} image not contiguous", call, image=f64(H, n, W, C).transpose(0, 1))
        for bad in bad_numbers:
            show(f"{name} number {bad!r}", call, number=bad)
            show(f"{name} image shape + number {bad!r}", call, image=f64(H, W, C), number=bad)
            show(f"{name} number {bad!r} + obs cpu", call, number=bad, obs=cpu(n, H, W, C))
        show(f"{name} image float32 + obs float64", call, image=f32(n, H, W, C))
        show(f"{name} obs cpu", call, obs=cpu(n, H, W, C))
        show(f"{name} obs float32", call, obs=f32(n, H, W, C))
        show(f"{name} obs [n, H, W]", call, obs=f64(n, H, W))
        show(f"{name} obs not contiguous", call, obs=f64(n, W, H, C).transpose(1, 2))
        show(f"{name} obs shape + {array} shape", call, obs=f64(n, H, W), array=f64(length + 1))
        show(f"{name} {array} cpu", call, array=cpu(length))
        show(f"{name} {array} float32", call, array=f32(length))
        show(f"{name} {array} [{length + 1}]", call, array=f64(length + 1))
        show(f"{name} {array} [{length}, 1]", call, array=f64(length, 1))
        show(f"{name} {array} not contiguous", call, array=f64(2 * length)[::2])
        show(f"{name} {array} none", call, array=None)
        show(f"{name} {array} dtype + weights shape", call, array=f32(length), weights=f64(H, W))
        wrong = dict(weights=(cpu(n, H, W), f32(n, H, W), f64(H, W), f64(n, W, H).transpose(1, 2)), terms=(cpu(length), f32(length), f64(length + 1), f64(2 * length)[::2]),
                     loss=(cpu(1), f32(1), f64(2), f64(2)[::2]), image_b=(cpu(n, H, W, C), f32(n, H, W, C), f64(n, H, W), f64(n, W, H, C).transpose(1, 2)),
                     scratch=(torch.zeros(64, dtype=torch.uint8), f32(64), dev(torch.zeros(8, 8, dtype=torch.uint8)), u8(128)[::2]))  # fmt: skip
        for optional, tensors in wrong.items():
            for how, t in zip(("cpu", "dtype", "shape", "not contiguous"), tensors):
                show(f"{name} every optional array, {optional} {how}", call, **dict(given, **{optional: t}))
        show(f"{name} every optional array, terms shape + image_b dtype", call, **dict(given, terms=f64(length + 1), image_b=f32(n, H, W, C)))
        show(f"{name} every optional array, weights cpu + scratch dtype", call, **dict(given, weights=cpu(n, H, W), scratch=f32(64)))
        big = (1, 1, 10**6 + 1, 1)
        show(f"{name} outside the limits", call, image=f64(*big), obs=f64(*big))
        show(f"{name} outside the limits, every optional array", call, image=f64(*big), obs=f64(*big), **dict(given, weights=f64(*big[:3]), image_b=f64(*big)))
        show(f"{name} outside the limits + scratch dtype", call, image=f64(*big), obs=f64(*big), scratch=f32(64))
        show(f"{name} outside the limits + number", call, image=f64(*big), obs=f64(*big), number=bad_numbers[0])
    makers = (("texture_scratch", ()), ("basis_scratch", (4, 300, 2)), ("camera_scratch", (300, 2)), ("sh_scratch", (300, 2, 3)), ("skin_scratch", (300, 4, 2, 2)),
              ("pyramid_scratch", (n, H, W, C, levels)), ("ssim_scratch", (n, H, W, C)), ("spd_scratch", (300, 3)), ("arap_scratch", (300, 2)),
              ("chamfer_scratch", (5, 9, 2)), ("chamfer_grid_scratch", (5, 9, 2)), ("surface_scratch", (5, 4, 9, 2)), ("sort_keys_scratch", (300, 2, 12)))  # fmt: skip
    for label, dims in makers:
        show(f"{label} good", getattr(hr, label), *dims, "cuda")
        for at in range(len(dims)):
            show(f"{label} outside the limits, dimension {at}", getattr(hr, label), *dims[:at], 10**6 + 1, *dims[at + 1 :], "cuda")
        if dims:
            show(f"{label} a dimension that is no number", getattr(hr, label), "many", *dims[1:], "cuda")
    V, J, K, T = 5, 3, 2, 4
    wrappers = (
        ("texture_smoothness", lambda **kw: hr.texture_smoothness(f64(4, 6, 3), f64(4, 6, 3), 0.5, energy_out=f64(1), **kw)),
        ("basis_apply_b", lambda **kw: hr.basis_apply_b(f64(4, 300), f64(2, 300), out=f64(2, 4), **kw)),
        ("camera_project_b", lambda **kw: hr.camera_project_b(f64(n, V, 3), f64(n, 3, 4), f64(n, 3, 3), None, f64(n, V, 2), points_b=f64(n, V, 3),
                                                              extrinsic_b=f64(n, 3, 4), intrinsic_b=f64(n, 3, 3), **kw)),
        ("sh_shade_b", lambda **kw: hr.sh_shade_b(f64(n, V, 3), i32(T, 3), i32(V + 1), i32(3 * T), f64(9), luminosity_b=f64(n, V), posed_b=f64(n, V, 3), sh_b=f64(9), **kw)),
        ("skin_apply_b", lambda **kw: hr.skin_apply_b(f64(V, 3), f64(J, 3), i32(J), f64(n, J, 4), i32(V, K), f64(V, K), f64(n, J, 7), f64(n, V, 3), i32(J + 1), i32(V * K),
                                                      vertices_b=f64(V, 3), quaternions_b=f64(n, J, 4), joints_b=f64(J, 3), **kw)),
        ("pyramid_l2", lambda **kw: terms[0][1](terms=f64(levels + 1), loss=f64(1), image_b=f64(n, H, W, C), **kw)),
        ("ssim_l2", lambda **kw: terms[1][1](terms=f64(2), loss=f64(1), image_b=f64(n, H, W, C), **kw)),
        ("spd_solve", lambda **kw: hr.spd_solve(i32(V + 1), i32(3 * V), f64(3 * V), f64(V, 3), 4, x=f64(V, 3), residual=f64(3), **kw)),
        ("arap_energy", lambda **kw: hr.arap_energy(i32(V + 1), i32(3 * V), f64(3 * V), f64(V, 3), f64(n, V, 3), 1.0, energy=f64(n), gradient=f64(n, V, 3), **kw)),
        ("chamfer", lambda **kw: hr.chamfer(f64(n, V, 3), f64(n, 9, 3), f64(3), terms=f64(n, 2), loss=f64(n), vertices_b=f64(n, V, 3), **kw)),
        ("chamfer_grid", lambda **kw: hr.chamfer_grid(f64(n, V, 3), f64(n, 9, 3), f64(3), 0.5, terms=f64(n, 2), loss=f64(n), vertices_b=f64(n, V, 3), **kw)),
        ("surface_distance", lambda **kw: hr.surface_distance(f64(n, V, 3), i32(T, 3), i32(V + 1), i32(3 * T), f64(n, 9, 3), f64(3), terms=f64(n, 2), loss=f64(n),
                                                              vertices_b=f64(n, V, 3), **kw)),
        ("sort_keys", lambda **kw: hr.sort_keys(i32(n, 300), sorted_keys=i32(n, 300), order=i32(n, 300), **kw)),
    )  # fmt: skip
    for capturing[0] in (False, True):
        for name, call in wrappers:
            show(f"{name} every result given, scratch none, capturing {capturing[0]}", call)
            show(f"{name} every result given, scratch given, capturing {capturing[0]}", call, scratch=u8())
    hr._scratch_cache[("pyramid", torch.device("cuda", 0), 0)] = hr._scratch_cache[("ssim", torch.device("cuda", 0), 0)] = u8(4096)
    hr._scratch_cache[("texture", torch.device("cuda", 0), 0)] = u8(4096)
    for name in ("pyramid_l2", "ssim_l2", "texture_smoothness"):
        show(f"{name} scratch none, one cached, capturing", dict(wrappers)[name])
    hr._scratch_cache[("pyramid", torch.device("cuda", 0), 0)] = hr._scratch_cache[("ssim", torch.device("cuda", 0), 0)] = u8(4095)
    for name in ("pyramid_l2", "ssim_l2"):
        show(f"{name} scratch none, a smaller one cached, capturing", dict(wrappers)[name])


{"closest_point": closest_point, "image_terms": image_terms}[FAMILY]()
