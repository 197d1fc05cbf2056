"""finalize_kernel's vertex table in its two modes (dr_finalize.h): a triangle block whose live table triangles span fewer than VT_SLOTS
vertex ids from an 8-aligned base indexes the table by `id - base` (window mode) and flushes it array by array; a block that does not fit
hashes the ids as before.  The cases: every block a window (both vertex dtypes, rows of 3 and 4 colours), every block hashed, both kinds in
one launch, the fit test at its boundary (`max - base` = VT_SLOTS - 1 and VT_SLOTS, with `min` at 0 and at 7 mod 8), a window that reaches
the last vertex of a view whose V is no multiple of 8 (a stray add would land in the next view's rows), and blocks with one live triangle
and with none beside window blocks.

Everything is compared with oracle/_ref through the helpers of tests/test_hip_parity.py and tests/test_finalize_paths_gpu.py, at their
tolerances, on 32 x 32 frames at sigma = 1, in the table regime.  Every case asserts its regime on the host: `block_modes` restates the
kernel's fit test over the live triangles (the formula of `drawn_edges`); the constants are read from the kernel sources.  These are
assertions about the scenes the tests build, not about the device."""

import copy
import os
import re

import numpy as np
import pytest
import torch

from deodr_amd import scenes
from test_finalize_paths_gpu import CSRC, K, closed_mesh_blocks, fit_step, grads_np, open_mesh_views, table_regime, views_for
from test_hip_parity import F32, F64, TOL, checker, compare_fit_step

pytestmark = pytest.mark.gpu


def vt_slots():
    with open(os.path.join(CSRC, "dr_finalize.h")) as f:
        found = re.search(r"constexpr\s+int\s+VT_SLOTS\s*=\s*(\d+)", f.read())
    assert found, "VT_SLOTS not found in dr_finalize.h"
    return int(found.group(1))


VT_SLOTS = vt_slots()
BLOCK = K["PRIM_BLOCK"]


# ---- the host's statement of the regime


def live_triangles(s):
    """triangles with a positive signed area and no vertex behind the camera (as `drawn_edges`); all of them interpolated here"""
    assert not np.asarray(s.textured).any()
    f = np.asarray(s.faces, dtype=np.int64)
    v = np.asarray(s.ij, dtype=np.float64)[f]
    u, w = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    area = 0.5 * (u[:, 0] * w[:, 1] - w[:, 0] * u[:, 1]) * (1 if s.clockwise else -1)
    return (area > 0) & (np.asarray(s.depths)[f] >= 0).all(axis=1)


def block_ranges(s):
    """per block of PRIM_BLOCK triangles: (number of live triangles, min id, max id) over the live ones (ids None without one)"""
    f, live = np.asarray(s.faces, dtype=np.int64), live_triangles(s)
    out = []
    for b in range(0, len(f), BLOCK):
        ids = f[b : b + BLOCK][live[b : b + BLOCK]]
        out.append((len(ids), int(ids.min()), int(ids.max())) if len(ids) else (0, None, None))
    return out


def block_modes(s):
    """per block: "none" (no live triangle: the block does not merge), "window" or "hash" -- the kernel's fit test"""
    modes = []
    for n, lo, hi in block_ranges(s):
        modes.append("none" if n == 0 else ("window" if hi - (lo & ~7) < VT_SLOTS else "hash"))
    return modes


# ---- meshes with relabelled vertex ids


def relabel(s, new_id, V):
    """the scene with vertex v renamed new_id[v] among V vertices; the vertices nobody names are padding (never referenced by a face)"""
    new_id = np.asarray(new_id, dtype=np.int64)
    assert len(np.unique(new_id)) == len(new_id) == len(s.ij) and new_id.min() >= 0 and new_id.max() < V
    t = copy.copy(s)
    for name in ("ij", "depths", "colors", "shade", "uv"):
        a = np.asarray(getattr(s, name))
        b = np.zeros((V,) + a.shape[1:], dtype=a.dtype)
        if name == "depths":
            b[:] = 1.0
        b[new_id] = a
        setattr(t, name, b)
    t.faces = new_id[np.asarray(s.faces, dtype=np.int64)].astype(np.uint32)
    t.faces_uv = t.faces.copy()
    return t


def sphere_views(nu, n_rings, n_views, C=4, T=None, n_poses=3, size=32):
    """`n_views` views of a small sphere (its first T triangles), cycling through n_poses poses"""
    vertices, faces = scenes.bumpy_sphere(nu, n_rings)
    faces = faces if T is None else faces[:T]
    poses, cw = [], None
    for a in np.linspace(-0.3, 0.3, n_poses):
        s = scenes.mesh_scene(vertices, faces, size, size, nb_colors=C, rot=scenes.rotx(0.37) @ scenes.roty(0.23 + float(a)), depth_channel=C == 4, clockwise=cw)
        cw = s.clockwise
        poses.append(s)
    return [poses[i % n_poses] for i in range(n_views)], poses


def scattered_ids(n, V, seed, keep=0):
    """an injection of n ids into V: the first `keep` stay, the others are drawn from the rest"""
    rs = np.random.RandomState(seed)
    ids = np.arange(n)
    ids[keep:] = keep + rs.permutation(V - keep)[: n - keep]
    return ids


def scattered_sphere(compact_first_block):
    """bumpy_sphere(24, 25) (T = 1200, five blocks) with its ids scattered over V = 2048; optionally the vertices of the first block keep the
    ids 0 ... k - 1"""
    T, V = 1200, 2048
    n = views_for(T, K["PRIM_TABLES_MIN"])
    views, poses = sphere_views(24, 25, n)
    assert len(poses[0].faces) == T and table_regime(n, T)
    nv = len(poses[0].ij)
    if compact_first_block:
        first = np.unique(np.asarray(poses[0].faces, dtype=np.int64)[:BLOCK])
        order = np.concatenate((first, np.setdiff1d(np.arange(nv), first)))
        ids = np.empty(nv, dtype=np.int64)
        ids[order] = scattered_ids(nv, V, 5, keep=len(first))
    else:
        ids = scattered_ids(nv, V, 5)
    done = {id(p): relabel(p, ids, V) for p in poses}
    return [done[id(v)] for v in views]


def pinned_range_views(lo, hi, V, T=256):
    """T = 256 triangles of bumpy_sphere(16, 17) (ONE block), relabelled so that in every view the smallest live id is `lo` and the largest `hi`:
    two vertices that are live in every pose take them, all the others lie in between"""
    n = views_for(T, K["PRIM_TABLES_MIN"])
    views, poses = sphere_views(16, 17, n, T=T)
    assert table_regime(n, T)
    nv = len(poses[0].ij)
    always = set(range(nv))
    for p in poses:
        always &= set(np.asarray(p.faces, dtype=np.int64)[live_triangles(p)].ravel().tolist())
    always = sorted(always)
    assert len(always) >= 2 and lo + nv - 1 <= hi < V
    a, b = always[0], always[-1]
    ids = np.empty(nv, dtype=np.int64)
    ids[a], ids[b] = lo, hi
    rest = [v for v in range(nv) if v not in (a, b)]
    ids[rest] = lo + 1 + np.arange(len(rest))
    done = {id(p): relabel(p, ids, V) for p in poses}
    return [done[id(v)] for v in views]


def compare_fit_step_vtx32(api, views, pix):
    """compare_fit_step for float32 vertex arrays (as test_dtypes of tests/test_finalize_paths_gpu.py: the checker sees the rounded values;
    float32 gradient arrays are held to the float32 gradient tolerance against the checker and against the two-call path)"""
    from hip_util import rel_err

    views = [copy.copy(s) for s in views]
    for s in views:
        for name in ("ij", "depths", "colors", "shade", "uv"):
            setattr(s, name, np.asarray(getattr(s, name), dtype=np.float32).astype(np.float64))
    ds, r, obs, image, z, g = fit_step(views, 1.0, pix=pix, vtx=F32)
    g = grads_np(g)
    image2, z2 = r.render(ds, 1.0)
    g2 = grads_np(r.render_backward(ds, residual_obs=obs))
    assert torch.equal(image, image2) and torch.equal(z, z2)
    ref = checker(api)
    tol_img, tol = TOL[pix][0], TOL[F32][1]
    for i, s in enumerate(views):
        img_ref, z_ref = ref.render(s, 1.0)
        assert np.abs(image[i].cpu().numpy() - img_ref).max() < tol_img
        image_b = 2 * (image[i].cpu().numpy().astype(np.float64) - obs[i].cpu().numpy().astype(np.float64))
        g_ref = ref.grads(s, 1.0, img_ref, z_ref, image_b)
        for k in ("ij_b", "colors_b", "shade_b"):
            assert rel_err(g[k][i], g_ref[k]) < tol, (k, "vs checker")
            assert rel_err(g[k][i], g2[k][i]) < tol, (k, "vs two calls")


# ---- the cases


@pytest.mark.parametrize("vtx", [F32, F64])
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("T", [257, 513])
def test_window_in_every_block(oracle_api, T, C, vtx):
    n = views_for(T, K["PRIM_TABLES_MIN"])
    views = open_mesh_views(T, C, n)
    assert table_regime(n, T)
    modes = [block_modes(s) for s in views]
    assert all(m in ("window", "none") for v in modes for m in v) and all("window" in v for v in modes)  # regime
    if vtx == F64:
        compare_fit_step(oracle_api, views, 1.0, F32)
    else:
        compare_fit_step_vtx32(oracle_api, views, F32)


def test_hash_in_every_block(oracle_api):
    views = scattered_sphere(False)
    modes = [block_modes(s) for s in views]
    assert all(m != "window" for v in modes for m in v) and all("hash" in v for v in modes)  # regime: no (view, block) is a window
    compare_fit_step(oracle_api, views, 1.0, F32)


def test_window_and_hash_blocks_in_one_launch(oracle_api):
    views = scattered_sphere(True)
    modes = [block_modes(s) for s in views]
    assert all(v[0] == "window" and "hash" in v[1:] for v in modes)  # regime: the compact first block, and a scattered one, in every view
    compare_fit_step(oracle_api, views, 1.0, F32)


@pytest.mark.parametrize("lo", [8, 15])  # min = 0 and 7 (mod 8): base = 8 both times
@pytest.mark.parametrize("span", [VT_SLOTS - 1, VT_SLOTS])
def test_fit_boundary(oracle_api, span, lo):
    base = lo & ~7
    views = pinned_range_views(lo, base + span, base + span + 5)
    for s in views[:3]:
        ((n, smin, smax),) = block_ranges(s)
        assert n > 0 and smin == lo and smax - (smin & ~7) == span  # regime
        assert block_modes(s) == ["window" if span < VT_SLOTS else "hash"]
    compare_fit_step(oracle_api, views, 1.0, F32)


@pytest.mark.parametrize("vtx", [F32, F64])
def test_window_reaches_the_last_vertex(oracle_api, vtx):
    V, lo = 301, 13
    views = pinned_range_views(lo, V - 1, V)
    assert V % 8 and (lo & ~7) + VT_SLOTS > V
    for s in views[:3]:
        ((n, smin, smax),) = block_ranges(s)
        assert n > 0 and smin == lo and smax == V - 1 and block_modes(s) == ["window"]  # regime
    assert len(views) > 1 and len(views[0].ij) == V  # a stray add beyond vertex V - 1 lands in the next view's rows
    if vtx == F64:
        compare_fit_step(oracle_api, views, 1.0, F32)
    else:
        compare_fit_step_vtx32(oracle_api, views, F32)


def closed_mesh_compact_ids():
    """`closed_mesh_blocks` (block 0: one live triangle, block 1: none, then the rest) with ids that keep the live blocks compact.  Its faces are
    sorted by their facing, which leaves the ids of a block all over the mesh: the vertices are numbered as the live faces meet them, then as
    the others do."""
    n = views_for(1280, K["PRIM_TABLES_MIN"])
    _views, s = closed_mesh_blocks(n, size=32)
    assert table_regime(n, 1280)
    f, live = np.asarray(s.faces, dtype=np.int64), live_triangles(s)
    named, first = np.unique(np.concatenate((f[live].ravel(), f[~live].ravel())), return_index=True)
    assert len(named) == len(s.ij)
    ids = np.empty(len(s.ij), dtype=np.int64)
    ids[named[np.argsort(first)]] = np.arange(len(named))
    s = relabel(s, ids, len(s.ij))
    return [s] * n, s


def test_blocks_with_one_live_triangle_and_with_none_beside_windows(oracle_api):
    views, s = closed_mesh_compact_ids()
    ranges, modes = block_ranges(s), block_modes(s)
    assert ranges[0][0] == 1 and modes[0] == "window" and modes[1] == "none" and "window" in modes[2:]  # regime
    compare_fit_step(oracle_api, views, 1.0, F32)
