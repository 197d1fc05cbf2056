"""The cases of tests/test_vertex_dtype_gpu.py -- float32 vertex arrays (``vertex_dtype = DEODR_HIP_F32``) on every instance of setup_bin_kernel and
finalize_kernel that reads or writes them -- and the helpers that need no GPU: the scenes, their regime, and the bound a float32 gradient array is
held to.  tests/test_vertex_dtype_cases.py checks all of this with the CPU checker alone.

The storage type of the vertex arrays reaches three pieces of device code: the ``ldv`` loads and the clearing loop of setup_bin_kernel<false, NC>;
the element size that places a view's gradient arrays, DeviceAdd's float branch and the vertex-table flush of finalize_kernel<false, NC, DET, TABLE>;
and the float branch of det_convert_kernel.  A case is the smallest launch that reaches one of their instances.

THE BOUND.  A float32 gradient element is the sum of its corner terms: what triangle k and k's own flagged edges contribute to corner i of k
(``unshared`` makes the checker deliver them one by one).  The device rounds every contribution to float32 and adds it with a float32 atomic; a
corner term reaches memory as at most three such additions (the triangle and two of its edges).  With n <= 3 A additions into an element that receives
A non-zero corner terms t, the first-order error is (n + 1) u sum |t|, u = 2^-24.  Relative to the largest entry of the array (hip_util.rel_err):

    B = 2 (3 A + 1) 2^-24 rho,    rho = max over elements of sum |t|  /  max |gradient|

The factor 2 pays for what the checker cannot separate: the magnitudes of a triangle's own part and of its edges' parts inside one corner term.  The
vertex table adds in double and flushes once, so it stays below the bound."""

import copy
from types import SimpleNamespace

import numpy as np

from deodr_amd import scenes
from test_finalize_paths_gpu import K, _SPHERE, drawn_edges, open_mesh_views, sparse_regime, table_regime

U32 = 2.0**-24  # unit round-off of float32
ROUNDED = ("ij", "depths", "colors", "shade", "uv")
VERTEX_GRADS = ("ij_b", "colors_b", "shade_b", "uv_b")


def checker(api, fixed=False):
    return api.ref(fixed=fixed) or api.port(fixed=fixed)


# ------------------------------------------------------------------------------------------------------------------ helpers


def rounded(scene):
    """a copy of `scene` whose vertex arrays hold float32 values (as float64 arrays): what the checker and both device runs see"""
    s = copy.deepcopy(scene)
    for name in ROUNDED:
        setattr(s, name, np.asarray(getattr(s, name), dtype=np.float64).astype(np.float32).astype(np.float64))
    return s


def live_triangles(s):
    """the triangles the reference draws: positive signed area, no vertex behind the camera (tests/test_finalize_paths_gpu.py: drawn_edges)"""
    f = np.asarray(s.faces, dtype=np.int64)
    v = np.asarray(s.ij, dtype=np.float64)[f]
    u, w = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    area = 0.5 * (u[:, 0] * w[:, 1] - w[:, 0] * u[:, 1]) * (1 if s.clockwise else -1)
    return (area > 0) & (np.asarray(s.depths)[f] >= 0).all(axis=1)


def no_depth_ties(s):
    """The depth sums of the drawn triangles are pairwise distinct.  Two equal sums leave the blending order of their silhouette edges to the
    reference's unstable sort (deodr_amd/scenes.py: sphere_scene), and rounding the depths to float32 makes such ties likelier."""
    f = np.asarray(s.faces, dtype=np.int64)
    d = np.asarray(s.depths, dtype=np.float64)[f]
    sums = ((d[:, 0] + d[:, 1]) + d[:, 2])[live_triangles(s)]
    return len(np.unique(sums)) == len(sums)


def unshared(s):
    """`s` with three vertices of its own per face: the same frame, and a gradient at corner (k, i) that is what triangle k and k's own flagged
    edges contribute to that vertex -- summed over the corners of a vertex, the gradient of `s`."""
    f = np.asarray(s.faces, dtype=np.int64).reshape(-1)
    fuv = np.asarray(s.faces_uv, dtype=np.int64).reshape(-1)
    own = np.arange(f.size, dtype=np.uint32).reshape(-1, 3)
    return scenes.Scene2D(
        faces=own, faces_uv=own.copy(), ij=np.ascontiguousarray(np.asarray(s.ij)[f]), depths=np.ascontiguousarray(np.asarray(s.depths)[f]),
        textured=np.asarray(s.textured).copy(), uv=np.ascontiguousarray(np.asarray(s.uv)[fuv]), shade=np.ascontiguousarray(np.asarray(s.shade)[f]),
        colors=np.ascontiguousarray(np.asarray(s.colors)[f]), shaded=np.asarray(s.shaded).copy(), edgeflags=np.asarray(s.edgeflags).copy(),
        height=s.height, width=s.width, nb_colors=s.nb_colors, texture=s.texture, background_image=getattr(s, "background_image", None),
        background_color=getattr(s, "background_color", None), clockwise=s.clockwise, backface_culling=s.backface_culling, strict_edge=s.strict_edge,
        perspective_correct=s.perspective_correct, integer_pixel_centers=s.integer_pixel_centers,
    )  # fmt: skip


def corner_sums(s, corner_grads):
    """the per-corner gradients of ``unshared(s)`` summed over the corners of every vertex of `s` -> {array: sum, array + "_abs": sum of magnitudes,
    array + "_n": number of non-zero terms}, in the shapes of the gradients of `s`"""
    f = np.asarray(s.faces, dtype=np.int64).reshape(-1)
    fuv = np.asarray(s.faces_uv, dtype=np.int64).reshape(-1)
    out = {}
    for k, index, shape in (("ij_b", f, np.shape(s.ij)), ("colors_b", f, np.shape(s.colors)), ("shade_b", f, np.shape(s.shade)), ("uv_b", fuv, np.shape(s.uv))):
        t = np.asarray(corner_grads[k], dtype=np.float64).reshape((index.size,) + tuple(shape[1:]))
        for suffix, terms in (("", t), ("_abs", np.abs(t)), ("_n", (t != 0).astype(np.float64))):
            acc = np.zeros(shape)
            np.add.at(acc, index, terms)
            out[k + suffix] = acc
    return out


def oracle_grads(api, s, sigma, image_b):
    """the checker's gradients of one view for `image_b` (its own frame and depth buffer)"""
    ref = checker(api)
    image, z = ref.render(s, sigma)
    return ref.grads(s, sigma, image, z, image_b)


def float32_bound(api, views, sigma, image_b_of, grads_of=None):
    """-> {array: (rho, A)} from the checker alone (see the module's docstring).  ``image_b_of(i)``: the seed of view i; ``grads_of(scene, i)``:
    another adjoint of view i (the antialiase_error one) in its place.  ij_b, colors_b and shade_b are per view: the largest ratio over the views.
    uv_b is summed over the views: terms, magnitudes and gradient are summed over the views first."""
    grads_of = grads_of or (lambda scene, i: oracle_grads(api, scene, sigma, image_b_of(i)))
    found = {k: (0.0, 0) for k in VERTEX_GRADS}
    uv = None
    for i, s in enumerate(views):
        c = corner_sums(s, grads_of(unshared(s), i))
        for k in ("ij_b", "colors_b", "shade_b"):
            top = np.abs(c[k]).max() if c[k].size else 0.0
            if top > 0:
                found[k] = (max(found[k][0], float(c[k + "_abs"].max() / top)), max(found[k][1], int(c[k + "_n"].max())))
        part = [c["uv_b"], c["uv_b_abs"], c["uv_b_n"]]
        uv = part if uv is None else [a + b for a, b in zip(uv, part)]
    if uv is not None and np.abs(uv[0]).max() > 0:
        found["uv_b"] = (float(uv[1].max() / np.abs(uv[0]).max()), int(uv[2].max()))
    return found


def bound(rho_A):
    """B of the module's docstring for one array's (rho, A)"""
    rho, A = rho_A
    return 2 * (3 * A + 1) * U32 * rho


# -------------------------------------------------------------------------------------------------------------------- scenes

SIGMA = 1.0
EXTRA_VERTICES = 3  # appended to the mesh cases, referenced by no face: clear_grads has to reach them, nothing else may


def with_extra_vertices(s, n=EXTRA_VERTICES):
    """`s` with `n` more vertices (and uv vertices) that no face references"""
    rs = np.random.RandomState(5)
    s.ij = np.vstack((s.ij, rs.rand(n, 2) * [s.width, s.height]))
    s.depths = np.concatenate((s.depths, 1.0 + rs.rand(n)))
    s.colors = np.vstack((s.colors, rs.rand(n, s.colors.shape[1])))
    s.shade = np.concatenate((s.shade, rs.rand(n)))
    s.uv = np.vstack((s.uv, rs.rand(n, 2)))
    return s


def mesh_views(vertices, faces, C, n_views, size, textured=False, extra=False):
    """`n_views` poses of a mesh, one winding flag for the launch (tests/test_finalize_paths_gpu.py: open_mesh_views, with a textured option)"""
    views, cw = [], None
    for a in np.linspace(-0.6, 0.6, n_views):
        s = scenes.mesh_scene(vertices, faces, size, size, nb_colors=C, rot=scenes.rotx(0.37) @ scenes.roty(0.23 + float(a)), depth_channel=C == 4,
                              textured=textured, texture_size=16, clockwise=cw)  # fmt: skip
        cw = s.clockwise
        views.append(with_extra_vertices(s) if extra else s)
    return views


def closed_sphere_views(C, n_views, textured=False):
    """the closed 16 x 17 sphere (544 triangles) at 64 x 64, three unreferenced vertices appended"""
    return mesh_views(*_SPHERE, C, n_views, 64, textured, extra=True)


def open_mesh_views_textured(T, C, n_views, size=32):
    """the textured twin of open_mesh_views: the first T triangles of the sphere, a 16 x 16 texture"""
    vertices, faces = _SPHERE
    return mesh_views(vertices, faces[:T], C, n_views, size, textured=True)


def soup_mixed_views(n_views):
    """a soup of Gouraud and textured triangles, every edge flagged, every 7th face turned over (back-facing: its flagged edges are not drawn)"""
    s = scenes.soup_scene(200, 64, 64, seed=20, flat=False, min_area=20, textured_ratio=0.4, texture_size=16)
    s.faces[::7] = s.faces[::7, ::-1].copy()
    s.faces_uv = s.faces.copy()
    return [s] * n_views


def _case(build, regime, setup, finalize, det=False, aa=False, recorded=None, **also):
    return SimpleNamespace(build=build, regime=regime, setup=setup, finalize=finalize, det=det, aa=aa, recorded=recorded or {}, **also)


# regime: "sparse" (up to SPARSE_MAX triangles in the launch: one edge slot per thread), "above_sparse" (four slots per thread, no vertex table),
# "table" (PRIM_TABLES_MIN and more).  setup / finalize: the instance (vtx_f64, NC, DET, TABLE) the float32 run is meant to reach
# (deodr_amd/csrc/dr_dispatch.h).  recorded: {array: (rho, A)} for image_b = 2 (image - rand), seed 1, measured with the reference; the CPU test
# recomputes them.
CASES = {
    "mesh_c1": _case(lambda: closed_sphere_views(1, 1), "sparse", (0, 0, 0, 0), (0, 0, 0, 0), recorded=dict(ij_b=(1.3, 6), colors_b=(1.2, 6))),
    "mesh_c2": _case(lambda: closed_sphere_views(2, 3), "sparse", (0, 0, 0, 0), (0, 0, 0, 0), recorded=dict(ij_b=(2.0, 6), colors_b=(1.2, 6))),
    "mesh_c3": _case(lambda: closed_sphere_views(3, 1), "sparse", (0, 3, 0, 0), (0, 3, 0, 0), aa=True, recorded=dict(ij_b=(1.8, 6), colors_b=(1.2, 6))),
    "mesh_c4": _case(lambda: closed_sphere_views(4, 3), "sparse", (0, 4, 0, 0), (0, 4, 0, 0), recorded=dict(ij_b=(1.5, 6), colors_b=(1.2, 6))),
    "mesh_c6": _case(lambda: closed_sphere_views(6, 1), "sparse", (0, 0, 0, 0), (0, 0, 0, 0), recorded=dict(ij_b=(1.25, 6), colors_b=(1.2, 6))),
    "mesh_tex": _case(lambda: closed_sphere_views(3, 3, textured=True), "sparse", (0, 3, 0, 0), (0, 3, 0, 0), recorded=dict(ij_b=(1.25, 6), shade_b=(1.2, 6), uv_b=(1.2, 18))),
    "soup_mixed": _case(lambda: soup_mixed_views(1), "sparse", (0, 3, 0, 0), (0, 3, 0, 0), aa=True, every_edge=True, recorded=dict(ij_b=(1.2, 1), colors_b=(1.2, 1), shade_b=(1.2, 1), uv_b=(1.2, 1))),
    "soup_mixed_x3": _case(lambda: soup_mixed_views(3), "sparse", (0, 3, 0, 0), (0, 3, 0, 0), every_edge=True, recorded=dict(ij_b=(1.2, 1), colors_b=(1.2, 1), shade_b=(1.2, 1), uv_b=(1.2, 3))),
    "above_sparse": _case(lambda: open_mesh_views(543, 3, 31), "above_sparse", (0, 3, 0, 0), (0, 3, 0, 0), recorded=dict(ij_b=(2.2, 6), colors_b=(1.25, 6))),
    "table_c1": _case(lambda: open_mesh_views(543, 1, 74), "table", (0, 0, 0, 0), (0, 0, 0, 1), recorded=dict(ij_b=(3.0, 6), colors_b=(1.3, 6))),
    "table_c3": _case(lambda: open_mesh_views(543, 3, 74), "table", (0, 3, 0, 0), (0, 3, 0, 1), recorded=dict(ij_b=(2.5, 6), colors_b=(1.35, 6))),
    "table_tex": _case(lambda: open_mesh_views_textured(543, 3, 74), "table", (0, 3, 0, 0), (0, 3, 0, 1), recorded=dict(ij_b=(1.65, 6), shade_b=(1.25, 6), uv_b=(1.2, 444))),
    "det_mesh_c4": _case(lambda: closed_sphere_views(4, 3), "sparse", (0, 4, 0, 0), (0, 0, 1, 0), det="global"),
    "det_mesh_c6": _case(lambda: closed_sphere_views(6, 1), "sparse", (0, 0, 0, 0), (0, 0, 1, 0), det="scene"),
    "det_soup_mixed": _case(lambda: soup_mixed_views(1), "sparse", (0, 3, 0, 0), (0, 0, 1, 0), det="scene", every_edge=True),
    "det_above_sparse": _case(lambda: open_mesh_views(543, 3, 31), "above_sparse", (0, 3, 0, 0), (0, 0, 1, 0), det="global"),
}

_views_cache = {}


def views_of(name):
    """the rounded views of a case, built once; nobody changes them"""
    if name not in _views_cache:
        _views_cache[name] = [rounded(s) for s in CASES[name].build()]
    return _views_cache[name]


def assert_regime(name):
    """the case is in the regime it exists for -- host formulas against the scene, they say what the launch holds"""
    c, views = CASES[name], views_of(name)
    n, T = len(views), len(views[0].faces)
    assert all(no_depth_ties(s) for s in views), "two drawn triangles of equal depth sum: the reference's blending order is undefined"
    if c.regime == "sparse":
        assert sparse_regime(n, T)
    elif c.regime == "above_sparse":
        assert not sparse_regime(n, T) and sparse_regime(n - 1, T) and not table_regime(n, T)
        # 3T odd: a view's flags start on a 32-bit word only in every fourth view -- byte path, word path and the tail of the array in one launch
        assert (3 * T) % 2 == 1 and n >= 4 and K["EDGE_SLOTS"] == 4
    else:
        assert c.regime == "table" and table_regime(n, T) and not table_regime(n - 1, T)
    drawn = [drawn_edges(s, SIGMA) for s in views]
    assert min(drawn) > 0
    if getattr(c, "every_edge", False):
        assert np.asarray(views[0].edgeflags).all() and drawn[0] < 3 * T  # every slot flagged, those of the turned faces not drawn
        assert drawn[0] > K["PRIM_BLOCK"]  # more drawn edges than one edge block has threads
        assert np.asarray(views[0].textured).any() and not np.asarray(views[0].textured).all()  # both kinds in one launch


def seeds(name, i, shape, what):
    """the random inputs of view i of a case, float32 values (exact in both pixel types): "obs" in [0, 1), "image_b" normal, "err_b" in [0, 1)"""
    rs = np.random.RandomState({"obs": 1000, "image_b": 2000, "err_b": 3000}[what] + 7 * i + sum(map(ord, name)))
    a = rs.randn(*shape) if what == "image_b" else rs.rand(*shape)
    return a.astype(np.float32).astype(np.float64)


# --------------------------------------------------------------------------------------------------------- end to end (Scene3DDevice)


# Frames of the float32 mesh against those of the float64 mesh: the vertices are projected in the camera's float64 arithmetic either way, and the
# scene of the float32 mesh then stores ij, colours and shade rounded to float32.  A coordinate below 128 moves by at most half an ulp, 2^-18 pixel;
# a pixel depends on the two coordinates of at most three vertices, and moves by at most its contrast (<= 1.5 here) per pixel of movement at an edge
# smoothed over sigma = 1 pixel: 6 x 2^-18 x 1.5 = 3.5e-5.
E2E_FRAME_TOL = 6 * 2.0**-18 * 1.5


def hand_scene3d(dtype, textured, device="cuda", size=128):
    """The hand mesh as a ``DeviceMesh(dtype=dtype)`` in a ``Scene3DDevice`` (float64 frames) and the default float64 camera; every value is a
    float32 value, so a float32 and a float64 mesh hold the same numbers.  -> (scene, mesh, camera, the leaf tensors that are differentiated)"""
    import os

    import torch

    from conftest import GOLDEN
    from deodr_amd.scene3d import DeviceCamera, DeviceMesh, Scene3DDevice

    f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)
    vertices, faces = scenes.load_hand_mesh(os.path.join(GOLDEN, "hand_mesh.npz"))
    rot = np.diag([1.0, -1.0, -1.0]) @ scenes.roty(0.2)
    fov = 2 * np.rad2deg(np.arctan(0.25))
    s = scenes.mesh_scene(vertices, faces, size, size, nb_colors=3, rot=rot, fov=fov, textured=textured, texture_size=32)
    cam = scenes.fit_camera(size, size, fov, vertices, rot)
    if textured:
        mesh = DeviceMesh(faces, f32(vertices), clockwise=s.clockwise, uv=f32(s.uv), faces_uv=faces, texture=f32(s.texture), device=device, dtype=dtype)
        mesh.texture.requires_grad_(True)
        leaves = {"vertices": mesh.vertices, "texture": mesh.texture}
    else:
        mesh = DeviceMesh(faces, f32(vertices), clockwise=s.clockwise, colors=f32(np.random.RandomState(2).rand(len(vertices), 3)), device=device, dtype=dtype)
        mesh.vertices_colors.requires_grad_(True)
        leaves = {"vertices": mesh.vertices, "colors": mesh.vertices_colors}
    mesh.vertices.requires_grad_(True)
    scene = Scene3DDevice(sigma=SIGMA, pixel_dtype=torch.float64)
    scene.set_mesh(mesh)
    scene.set_light(f32([-0.1, -0.5, -0.4]), 0.6)
    scene.set_background_color([0.5, 0.6, 0.7])
    camera = DeviceCamera(f32(cam.extrinsic), f32(cam.intrinsic), size, size, device=device)  # (float64, the default, for both meshes)
    return scene, mesh, camera, leaves


def l2_step(dtype, textured, device="cuda", size=128):
    """one ``render_l2`` + ``backward`` of hand_scene3d -> (loss, image, {leaf: gradient}) as float64 NumPy values"""
    import torch

    scene, mesh, camera, leaves = hand_scene3d(dtype, textured, device, size)
    obs = torch.as_tensor(seeds("e2e", 0, (1, size, size, 3), "obs")).to(mesh.device)
    loss, image = scene.render_l2(camera, obs)
    loss.backward()
    assert all(t.grad is not None and t.grad.dtype == dtype for t in leaves.values())
    return float(loss.detach()), image.detach().cpu().numpy().astype(np.float64), {k: t.grad.cpu().numpy().astype(np.float64) for k, t in leaves.items()}, scene
