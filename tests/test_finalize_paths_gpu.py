"""finalize_kernel (and the set-up kernel in front of it) where their launch geometry and their paths change: launches at and just below the
threshold of the vertex-table instance (PRIM_TABLES_MIN triangles per launch), triangle counts around one and two workgroups of 256, rows of
72 and of 96 bytes of accumulators, workgroups without a live triangle and with a single one, launches up to and above SPARSE_MAX, soups
with every edge flagged (more flagged slots than a workgroup takes in one round), and the state a step leaves in the workspace.

Everything is compared with oracle/_ref through the helpers of tests/test_hip_parity.py, at their tolerances.  A case that exists for a regime
asserts that it is in it: the constants are read from the kernel sources.  The `drawn_edges` assertions are such regime assertions (a host
formula against the scene the test built: they say what the launch holds, they do not check the device).

The edge blocks of both kernels read a thread's four flags as one 32-bit word where the word is aligned and inside the array
(compact_flagged_slots), and by the byte elsewhere.  Launches above SPARSE_MAX have four slots per thread: with T = 256 (3T a multiple of 4)
every view takes the word path; with T = 255, 257 and 513 (3T odd) a view's flags start on a word only in every fourth view, so the byte
path, the word path and the tail of the array (3T not a multiple of 4) are all run in one launch.  Launches up to SPARSE_MAX have one slot
per thread: the byte path only.

Not covered, and why: T = 1 in the table regime would be 40 000 views, and a view's workspace holds 3.7 MB whatever the scene (the saved
sweeps of the edge tiles): 147 GB.  T = 1 runs below the threshold only."""

import os
import re

import numpy as np
import pytest
import torch

from deodr_amd import scenes
from test_hip_parity import F32, F64, TOL, checker, compare_backward, compare_fit_step

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deodr_amd", "csrc")


def constants():
    """``constexpr int | long long NAME = value`` of the headers that decide the launch geometry of set-up and finalize"""
    found = {}
    for name in ("dr_setup.h", "dr_kernels.hip"):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        for stmt in re.findall(r"constexpr\s+(?:int|long long)\s+([^;]+);", text):
            found.update({k: int(v) for k, v in re.findall(r"(\w+)\s*=\s*(\d+)\s*(?:,|$)", stmt.strip())})
    missing = [k for k in ("PRIM_BLOCK", "EDGE_SLOTS", "SPARSE_MAX", "PRIM_TABLES_MIN") if k not in found]
    assert not missing, f"constants not found in the kernel headers: {missing}"
    return found


K = constants()


def table_regime(n_views, T):
    return n_views * T >= K["PRIM_TABLES_MIN"]


def sparse_regime(n_views, T):
    return n_views * T <= K["SPARSE_MAX"]


def drawn_edges(s, sigma):
    """Silhouette edges the reference draws (H.h:2751-2779, 2839-2853): flagged edges of the triangles whose signed area is positive and that
    have no vertex behind the camera -- whatever backface_culling says."""
    if not sigma > 0:
        return 0
    f = np.asarray(s.faces, dtype=np.int64)
    v = np.asarray(s.ij, dtype=np.float64)[f]
    u, w = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    area = 0.5 * (u[:, 0] * w[:, 1] - w[:, 0] * u[:, 1]) * (1 if s.clockwise else -1)
    live = (area > 0) & (np.asarray(s.depths)[f] >= 0).all(axis=1)
    return int((np.asarray(s.edgeflags, dtype=bool).reshape(-1, 3) & live[:, None]).sum())


def fit_step(views, sigma, pix=F32, vtx=F64, seed=11):
    """one fit step of `views` -> (ds, r, obs, image, z, gradients)"""
    from hip_util import device_scene
    from deodr_amd.hip_renderer import HipRasterizer

    ds = device_scene(views, pix, vtx)
    r = HipRasterizer.for_scene(ds)
    obs = torch.as_tensor(np.random.RandomState(seed).rand(ds.n_views, ds.height, ds.width, ds.nb_colors), device=ds.device, dtype=pix)
    image, z, g = r.render_fit(ds, obs, sigma, check_overflow=True, clear_grads=True)
    torch.cuda.synchronize()
    return ds, r, obs, image, z, g


_SPHERE = scenes.bumpy_sphere(16, 17)  # 544 triangles, ring by ring from one pole


def open_mesh_views(T, C, n_views, size=32):
    """the first T triangles of a small sphere (an open mesh: its border edges are flagged too), one pose per view"""
    vertices, faces = _SPHERE
    assert T <= len(faces)
    views, cw = [], None
    for a in np.linspace(-0.6, 0.6, n_views):
        s = scenes.mesh_scene(vertices, faces[:T], size, size, nb_colors=C, rot=scenes.rotx(0.37) @ scenes.roty(0.23 + float(a)), depth_channel=C == 4, clockwise=cw)
        cw = s.clockwise  # (one winding flag per launch)
        views.append(s)
    return views


def views_for(T, at_least):
    return -(-at_least // T)


# ---- workgroup boundaries of the triangle blocks: T around one and two blocks of 256, accumulator rows of 72 bytes (C = 3) and of 96 (C = 4)


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("T", [255, 256, 257, 513])
def test_triangle_block_boundaries_table_instance(oracle_api, T, C):
    n = views_for(T, K["PRIM_TABLES_MIN"])
    assert table_regime(n, T) and not table_regime(n - 1, T)
    compare_fit_step(oracle_api, open_mesh_views(T, C, n), 1.0, F32)


@pytest.mark.parametrize("C", [3, 4])
def test_just_below_the_table_threshold(oracle_api, C):
    T = 257
    n = views_for(T, K["PRIM_TABLES_MIN"]) - 1
    assert not table_regime(n, T) and table_regime(n + 1, T)
    compare_fit_step(oracle_api, open_mesh_views(T, C, n), 1.0, F32)


@pytest.mark.parametrize("C", [3, 4])
def test_one_triangle(oracle_api, C):
    views = open_mesh_views(1, C, 3)
    compare_fit_step(oracle_api, views, 1.0, F32)
    assert drawn_edges(views[0], 1.0) == 3  # regime: in the first pose (it decides the winding flag) the triangle is front-facing, three edges drawn


def closed_mesh_blocks(n_views, size=48):
    """A closed mesh of five blocks of 256 triangles, back-face culling on, its faces ordered so that block 0 holds ONE front-facing triangle,
    block 1 none, and the others the rest."""
    vertices, faces = scenes.bumpy_sphere(20, 32)
    rot = scenes.rotx(0.37) @ scenes.roty(0.23)
    s = scenes.mesh_scene(vertices, faces, size, size, nb_colors=4, rot=rot, depth_channel=True)
    v = s.ij[np.asarray(faces, dtype=np.int64)]
    u, w = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    front = (u[:, 0] * w[:, 1] - w[:, 0] * u[:, 1]) * (1 if s.clockwise else -1) > 0
    fi, bi = np.flatnonzero(front), np.flatnonzero(~front)
    assert len(faces) == 1280 and len(bi) >= 511
    order = np.concatenate((fi[:1], bi[:511], fi[1:], bi[511:]))
    s = scenes.mesh_scene(vertices, faces[order], size, size, nb_colors=4, rot=rot, depth_channel=True, clockwise=s.clockwise)
    assert s.backface_culling and front[order][:256].sum() == 1 and front[order][256:512].sum() == 0
    return [s] * n_views, s


def test_closed_mesh_blocks_without_and_with_one_live_triangle(oracle_api):
    n = views_for(1280, K["PRIM_TABLES_MIN"])
    views, s = closed_mesh_blocks(n)
    assert table_regime(n, 1280)
    compare_fit_step(oracle_api, views, 1.0, F32)
    # the flagged slots of a closed mesh are half back-facing (a silhouette edge is flagged in both faces): finalize drops those
    flagged = int(np.asarray(s.edgeflags).sum())
    assert 0 < drawn_edges(s, 1.0) < flagged  # regime


# ---- the edge blocks


def soup(T, seed, size=64, culled_every=0):
    s = scenes.soup_scene(n_tri=T, width=size, height=size, seed=seed, flat=False, min_area=20.0)
    if culled_every:  # every culled_every-th triangle turned over: back-facing, its three flagged edges are not drawn
        s.faces[::culled_every] = s.faces[::culled_every, ::-1].copy()
        s.faces_uv = s.faces.copy()
    return s


def test_no_edges(oracle_api):
    views = open_mesh_views(257, 3, 3)
    compare_fit_step(oracle_api, views, 0.0, F32)
    for s in views:
        s.edgeflags = np.zeros_like(s.edgeflags)
    compare_fit_step(oracle_api, views, 1.0, F32)
    assert [drawn_edges(s, 1.0) for s in views] == [0, 0, 0]  # regime: sigma > 0, no flag set


@pytest.mark.parametrize("n_views", [1, 3])
def test_soup_sparse_launch(oracle_api, n_views):
    """small launches: one slot per thread in the edge blocks of both kernels"""
    views = [soup(200, 20 + i, culled_every=7) for i in range(n_views)]
    assert sparse_regime(n_views, 200)
    compare_fit_step(oracle_api, views, 1.0, F32)
    assert min(drawn_edges(s, 1.0) for s in views) > K["PRIM_BLOCK"]  # regime: more drawn edges per view than one edge block has threads


def test_soup_every_edge_flagged_above_sparse_max(oracle_api):
    """a soup with every edge flagged in a launch above SPARSE_MAX: four slots per thread, more than one round per edge block"""
    T = 600
    n = K["SPARSE_MAX"] // T + 1
    views = [soup(T, 40, size=48, culled_every=5)] * n
    assert not sparse_regime(n, T) and sparse_regime(n - 1, T)
    # regime: every flag set, so an edge block (PRIM_BLOCK x EDGE_SLOTS slots) holds more flagged slots than one round takes, and there is more than one block
    assert np.asarray(views[0].edgeflags).all() and 3 * T > K["PRIM_BLOCK"] * K["EDGE_SLOTS"] and K["EDGE_SLOTS"] > 1
    assert 0 < drawn_edges(views[0], 1.0) < 3 * T  # regime: some of the flagged slots belong to culled triangles
    compare_fit_step(oracle_api, views[:1] * n, 1.0, F32)


def test_two_call_path_both_kernel_families(oracle_api):
    """render + render_backward on the default kernels and on the un-staged ones (deodr_hip_force_generic)"""
    from deodr_amd import hip_renderer as hr

    compare_backward(oracle_api, soup(200, 31, culled_every=3), 1.0, F32)
    hr.force_generic(True)
    try:
        compare_backward(oracle_api, soup(200, 32, culled_every=3), 1.0, F32)
    finally:
        hr.force_generic(False)


# ---- state


def grads_np(g):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in g.items() if v is not None}


def assert_same(a, b, tol):
    from hip_util import rel_err

    for k in a:
        assert rel_err(a[k], b[k]) < tol, k


# Two runs of the same step differ by the order in which the memory system executes the float64 atomics: a sum of n terms moves by at
# most n 2^-53 of the sum of their magnitudes; n < 1000 contributions per vertex here, and 100 x for cancellation: 1e-11 of the largest entry.
ORDER_TOL = 1e-11


def test_two_steps_in_a_row(oracle_api):
    """the accumulators are left clear and the counters follow the forward's parity: the second, third and fourth step are the first again"""
    n = views_for(513, K["PRIM_TABLES_MIN"])
    views = open_mesh_views(513, 4, n)
    ds, r, obs, image, z, g = fit_step(views, 1.0, pix=F64)
    first = grads_np(g)
    for _ in range(3):
        _image, _z, g = r.render_fit(ds, obs, 1.0, check_overflow=True, clear_grads=True)
        assert_same(grads_np(g), first, ORDER_TOL)
    views = [soup(200, 50, culled_every=4)]
    ds, r, obs, image, z, g = fit_step(views, 1.0, pix=F64)
    first = grads_np(g)
    _image, _z, g = r.render_fit(ds, obs, 1.0, check_overflow=True, clear_grads=True)
    assert_same(grads_np(g), first, ORDER_TOL)


def test_render_then_two_backwards(oracle_api):
    from hip_util import hip_grads, hip_render

    s = soup(200, 51, culled_every=4)
    ds, r, out = hip_render(s, 1.0, F64)
    image_b = np.random.RandomState(3).randn(*out[0][0].shape)
    a = hip_grads(ds, r, image_b=image_b)
    b = hip_grads(ds, r, image_b=image_b)
    g_ref = checker(oracle_api).grads(s, 1.0, *checker(oracle_api).render(s, 1.0), image_b)
    from hip_util import rel_err

    for k in ("ij_b", "colors_b"):
        assert rel_err(a[k], b[k]) < ORDER_TOL, k
        assert rel_err(b[k][0], g_ref[k]) < TOL[F64][1], k


def test_smaller_scene_after_a_step_and_fresh_workspace(oracle_api):
    """A step at sigma = 1, then a different, smaller scene, then the first scene again on a fresh workspace.  A HipRasterizer is bound to the
    dimensions of its scene, so "a smaller scene on a fresh workspace of the same rasterizer" is read as: the smaller scene on a rasterizer of
    its own in the same process (same library state), and the first scene again on a newly allocated, zero-filled workspace."""
    from deodr_amd.hip_renderer import HipRasterizer

    views = [soup(200, 52, culled_every=4)]
    ds, r, obs, image, z, g = fit_step(views, 1.0, pix=F64)
    first = grads_np(g)
    compare_fit_step(oracle_api, soup(40, 53, culled_every=3), 1.0, F64)
    fresh = HipRasterizer.for_scene(ds)
    _image, _z, g = fresh.render_fit(ds, obs, 1.0, check_overflow=True, clear_grads=True)
    assert_same(grads_np(g), first, ORDER_TOL)


# ---- dtypes


@pytest.mark.parametrize("pix", [F32, F64])
@pytest.mark.parametrize("vtx", [F32, F64])
def test_dtypes(oracle_api, pix, vtx):
    """float32 / float64 vertex arrays x pixel buffers, table instance.  compare_fit_step builds float64 vertex arrays; the float32 ones are
    compared here in the same way (every view, every per-view gradient, checker and two-call path).  The checker sees the vertex values the
    device sees (rounded to float32 first).  Float32 gradient arrays are summed by float32 atomics, 2^-24 per add and up to ~100 adds per entry
    whatever the frame's type: 6e-6 of the sum of magnitudes, so they are held to the float32 gradient tolerance (1e-4) against the checker
    and against the two-call path, also with float64 frames."""
    from hip_util import rel_err

    n = views_for(257, K["PRIM_TABLES_MIN"])
    views = open_mesh_views(257, 4, n)
    assert table_regime(n, 257)
    if vtx == F64:
        compare_fit_step(oracle_api, views, 1.0, pix)
        return
    for s in views:
        for name in ("ij", "depths", "colors", "shade", "uv"):
            setattr(s, name, np.asarray(getattr(s, name), dtype=np.float32).astype(np.float64))
    ds, r, obs, image, z, g = fit_step(views, 1.0, pix=pix, vtx=F32)
    g = grads_np(g)
    image2, z2 = r.render(ds, 1.0)
    g2 = grads_np(r.render_backward(ds, residual_obs=obs))
    assert torch.equal(image, image2) and torch.equal(z, z2)
    ref = checker(oracle_api)
    tol_img, tol = TOL[pix][0], TOL[F32][1]
    for i in range(n):
        img_ref, z_ref = ref.render(views[i], 1.0)
        assert np.abs(image[i].cpu().numpy() - img_ref).max() < tol_img
        image_b = 2 * (image[i].cpu().numpy().astype(np.float64) - obs[i].cpu().numpy().astype(np.float64))
        g_ref = ref.grads(views[i], 1.0, img_ref, z_ref, image_b)
        for k in ("ij_b", "colors_b", "shade_b"):
            assert rel_err(g[k][i], g_ref[k]) < tol, (k, "vs checker")
            assert rel_err(g[k][i], g2[k][i]) < tol, (k, "vs two calls")
