"""GPU tests of the retained background fill (include/deodr_hip_retained.h, HipRasterizer(retain_frames=True)): a fit step that renders into the
buffers of the step before it fills only the tiles that have just become empty, and must leave the same frame as a step that fills everything.

Every check compares with the same scene rendered into FRESH buffers on a fresh workspace with ``retain_frames=False``: image and depth buffer
bit for bit (the fill writes constants, the walkers are the same code), gradients to the tolerance test_hip_parity.compare_fit_step uses for a
fit step (1e-4 float32 / 1e-8 float64, relative to the largest entry: the two runs differ by the order of their atomics only).

Frames: 64 x 64 (two bitmap words), 264 x 40 (165 tiles: neither a multiple of 32 nor of 64) and 70 x 52 (ragged width: the fill goes tile by
tile).  The scenes are clusters of small triangles that cover a third of the frame, shifted by about two tiles between the poses, so that
tiles change state in both directions."""

import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
GRAD_TOL = {F32: 1e-4, F64: 1e-8}
FRAMES = [(64, 64), (40, 264), (52, 70)]  # (height, width)
ENTRY = "deodr_hip_render_scene_fit_retained"
SENTINEL = 777.0


def cluster(height, width, n_views, n_colors, pose, dtype, background, n_tri=60, seed=3):
    """-> DeviceScene: `n_tri` small triangles around a centre that depends on `pose` (0 / 1: two tiles apart) and on the view, every edge flagged"""
    from deodr_amd.hip_renderer import DeviceScene

    rs = np.random.RandomState(seed)
    spread = np.array([0.22 * width, 0.22 * height])
    centres = (rs.rand(n_tri, 2) - 0.5) * 2 * spread  # (x, y) around the cluster's centre
    corners = (rs.rand(n_tri, 3, 2) - 0.5) * 14.0
    for t in range(n_tri):  # counter-clockwise in the library's convention (scenes.soup_scene, clockwise=False)
        u, v = corners[t, 1] - corners[t, 0], corners[t, 2] - corners[t, 0]
        if -(u[0] * v[1] - u[1] * v[0]) < 0:
            corners[t] = corners[t, ::-1]
    depths = np.repeat(rs.rand(n_tri) + 0.5, 3)
    colors = rs.rand(3 * n_tri, n_colors)
    ij = np.zeros((n_views, 3 * n_tri, 2))
    for view in range(n_views):
        shift = np.array([17.0, 3.0]) * pose + np.array([-9.0, 6.0]) * view
        xy = (centres[:, None, :] + corners).reshape(-1, 2) + np.array([0.45 * width, 0.5 * height]) + shift
        ij[view] = xy
    faces = np.arange(3 * n_tri, dtype=np.int32).reshape(-1, 3)
    bg_rs = np.random.RandomState(seed + 1)
    return DeviceScene(
        faces, faces.copy(), np.zeros(n_tri, np.uint8), np.zeros(n_tri, np.uint8), np.zeros((3 * n_tri, 2)), ij, np.tile(depths, (n_views, 1)),
        np.tile(colors, (n_views, 1, 1)), np.zeros((n_views, 3 * n_tri)), np.ones((n_views, n_tri, 3), np.uint8), height, width, texture=None,
        background_color=bg_rs.rand(n_colors) if background == "colour" else None,
        background_image=bg_rs.rand(n_views, height, width, n_colors) if background == "image" else None, pixel_dtype=dtype,
    )  # fmt: skip


def observation(ds, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((ds.n_views, ds.height, ds.width, ds.nb_colors), generator=g, dtype=torch.float64).to(device=ds.device, dtype=ds.pixel_dtype)


def buffers(ds, value=SENTINEL):
    shape = (ds.n_views, ds.height, ds.width)
    return (torch.full(shape + (ds.nb_colors,), value, dtype=ds.pixel_dtype, device=ds.device), torch.full(shape, value, dtype=ds.pixel_dtype, device=ds.device))


_reference_cache = {}


def reference(key, ds, obs):
    """the fit step of `ds` into fresh buffers on a fresh workspace that claims nothing (computed once per key, never written again)"""
    from deodr_amd.hip_renderer import HipRasterizer

    if key not in _reference_cache:
        r = HipRasterizer.for_scene(ds, retain_frames=False)
        image, z, g = r.render_fit(ds, obs, 1.0, out=buffers(ds), check_overflow=True, clear_grads=True)
        torch.cuda.synchronize()
        assert not (image == SENTINEL).any() and not (z == SENTINEL).any()
        _reference_cache[key] = (image, z, {k: v for k, v in g.items() if v is not None})
    return _reference_cache[key]


def assert_same(ds, got, ref):
    image, z, g = got
    torch.cuda.synchronize()
    assert torch.equal(image, ref[0]), "image"
    assert torch.equal(z, ref[1]), "depth buffer"
    for k, v in ref[2].items():
        scale = max(float(v.abs().max()), 1e-30)
        assert float((g[k] - v).abs().max()) / scale < GRAD_TOL[ds.pixel_dtype], k


@pytest.fixture
def spy(monkeypatch):
    """the values of `retained` the host layer passes to the library, in order"""
    from deodr_amd import hip_renderer as hr

    L, seen = hr.lib(), []
    entry = getattr(L, ENTRY)

    def recording(*args):
        seen.append(int(args[7]))
        return entry(*args)

    monkeypatch.setattr(L, ENTRY, recording)
    return seen


def poses(case, frame, n_views, n_colors, dtype, background):
    key = (case, frame, n_views, n_colors, dtype, background)
    scenes = [cluster(frame[0], frame[1], n_views, n_colors, pose, dtype, background) for pose in (0, 1)]
    scenes[1].background_color, scenes[1].background_image = scenes[0].background_color, scenes[0].background_image  # ONE background, unchanged
    obs = observation(scenes[0])
    return scenes, obs, [reference(key + (pose,), scenes[pose], obs) for pose in (0, 1)]


@pytest.mark.parametrize("n_colors", [3, 4])
@pytest.mark.parametrize("background", ["colour", "image"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n_views", [1, 2])
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[1]}x{f[0]}")
def test_moving_scene(spy, frame, n_views, dtype, background, n_colors):
    from deodr_amd.hip_renderer import HipRasterizer, tile_census

    (a, b), obs, refs = poses("moving", frame, n_views, n_colors, dtype, background)
    r = HipRasterizer.for_scene(a)
    out, grads = buffers(a), a.zero_grads()
    r.render_fit(a, obs, 1.0, grads=grads, out=out, check_overflow=False, clear_grads=True)
    assert spy == [0]  # nothing was rendered before
    census_a = tile_census(r, a)
    assert_same(a, (out[0], out[1], grads), refs[0])
    got = r.render_fit(b, obs, 1.0, grads=grads, out=out, check_overflow=False, clear_grads=True)
    assert spy == [0, 1], "the second step into the same buffers takes the claim"
    assert got[0] is out[0] and got[1] is out[1]
    assert_same(b, got, refs[1])
    # the poses differ in which tiles they cover, and two thirds of the frame stay background: the claim had something to skip and something to fill
    tiles = n_views * ((frame[0] + 7) // 8) * ((frame[1] + 7) // 8)
    assert 0 < census_a[0] < tiles and not torch.equal(refs[0][1] == float("inf"), refs[1][1] == float("inf"))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[1]}x{f[0]}")
def test_cycle(spy, frame, dtype):
    from deodr_amd.hip_renderer import HipRasterizer

    background = "image" if dtype == F64 else "colour"
    scenes, obs, refs = poses("cycle", frame, 2, 4, dtype, background)
    r = HipRasterizer.for_scene(scenes[0])
    out, grads = buffers(scenes[0]), scenes[0].zero_grads()
    for step in range(4):
        got = r.render_fit(scenes[step % 2], obs, 1.0, grads=grads, out=out, check_overflow=False, clear_grads=True)
        assert_same(scenes[step % 2], got, refs[step % 2])
    assert spy == [0, 1, 1, 1]


@pytest.mark.parametrize("what", ["image.fill_", "z.zero_", "new out", "background colour", "regrown workspace", "another stream"])
def test_claim_refused_by_the_host_layer(spy, what):
    from deodr_amd.hip_renderer import HipRasterizer

    (a, b), obs, refs = poses("refused", FRAMES[1], 2, 3, F32, "colour")
    r = HipRasterizer.for_scene(a)
    out, grads = buffers(a), a.zero_grads()
    r.render_fit(a, obs, 1.0, grads=grads, out=out, check_overflow=False, clear_grads=True)
    r.render_fit(b, obs, 1.0, grads=grads, out=out, check_overflow=False, clear_grads=True)
    assert spy == [0, 1]
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    ref = refs[0]
    if what == "image.fill_":
        out[0].fill_(7)
    elif what == "z.zero_":
        out[1].zero_()
    elif what == "new out":
        out = buffers(a)
    elif what == "background colour":
        a.background_color.mul_(0.5)  # (in place: the same tensor, another version)
        ref = reference(("refused", "half background"), a, obs)
    elif what == "regrown workspace":
        r._alloc(4096)
    else:
        stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = r.render_fit(a, obs, 1.0, grads=grads, out=out, check_overflow=False, clear_grads=True)
    assert spy == [0, 1, 0], what
    assert_same(a, got, ref)


def call_entry(r, ds, obs, out, grads, retained):
    from deodr_amd import hip_renderer as hr

    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = getattr(hr.lib(), ENTRY)(C.byref(ds.c_struct(grads)), ptr(out[0]), ptr(out[1]), 1.0, ptr(obs), 1, None, retained, ptr(r.workspace), r.nbytes,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))  # fmt: skip
    assert rc == 0, hr.lib().deodr_hip_last_error()
    return out[0], out[1], grads


@pytest.mark.parametrize("what", ["fresh workspace", "another image", "after an un-staged forward"])
def test_claim_ignored_by_the_library(what):
    """retained = 1 handed to the C entry where it is NOT true: the buffers hold a sentinel, and the frame is complete all the same"""
    from deodr_amd import hip_renderer as hr
    from deodr_amd.hip_renderer import HipRasterizer

    (a, b), obs, refs = poses("ignored", FRAMES[1], 2, 4, F32, "colour")
    r = HipRasterizer.for_scene(a)
    out, grads = buffers(a), a.zero_grads()
    if what != "fresh workspace":
        call_entry(r, a, obs, out, grads, 0)
    if what == "another image":
        out = (buffers(a)[0], out[1])
        out[1].fill_(SENTINEL)
    if what == "after an un-staged forward":
        hr.force_generic(True)
        try:
            call_entry(r, b, obs, out, grads, 0)
        finally:
            hr.force_generic(False)
        out[0].fill_(SENTINEL), out[1].fill_(SENTINEL)
    assert_same(a, call_entry(r, a, obs, out, grads, 1), refs[0])
    # ... and where it IS true the same entry skips the tiles that stay empty: a sentinel written there survives (the claim is the caller's)
    tile_empty_in_both = (refs[0][1][:, :8, :8] == float("inf")).all() and (refs[1][1][:, :8, :8] == float("inf")).all()
    assert tile_empty_in_both, "the scene leaves the first tile of both views empty in both poses"
    torch.cuda.synchronize()
    out[0][:, :8, :8] = SENTINEL
    got = call_entry(r, b, obs, out, grads, 1)
    torch.cuda.synchronize()
    assert (got[0][:, :8, :8] == SENTINEL).all() and torch.equal(got[1], refs[1][1])
    got[0][:, :8, :8] = refs[1][0][:, :8, :8]
    assert_same(b, got, refs[1])


def test_a_frame_shape_with_the_same_tile_count_is_not_believed():
    """64 x 64 and 32 x 128 pixels are 64 tiles each: same workspace layout, and here the same buffers -- the bitmap of the one must not be read as
    the other's"""
    from deodr_amd.hip_renderer import HipRasterizer

    (a, _b), obs, _refs = poses("shape", (64, 64), 1, 3, F32, "colour")
    (wide, _), obs_wide, refs_wide = poses("shape", (32, 128), 1, 3, F32, "colour")
    r = HipRasterizer.for_scene(a)
    assert r.nbytes == HipRasterizer.for_scene(wide).nbytes
    out, grads = buffers(a), a.zero_grads()
    call_entry(r, a, obs, out, grads, 0)
    torch.cuda.synchronize()
    out[0].fill_(SENTINEL), out[1].fill_(SENTINEL)
    out_wide = (out[0].view(1, 32, 128, 3), out[1].view(1, 32, 128))
    assert_same(wide, call_entry(r, wide, obs_wide, out_wide, grads, 1), refs_wide[0])


def test_large_frame_many_units(spy):
    """two views of 1024 x 1024: 512 bitmap words per view, so a retained share is several 64-word units per kernel and the forward's fill
    workgroups are dealt among its walkers; tiles that stay empty are skipped in both views, in the first unit and in the last"""
    from deodr_amd.hip_renderer import HipRasterizer

    (a, b), obs, refs = poses("large", (1024, 1024), 2, 3, F32, "colour")
    r = HipRasterizer.for_scene(a)
    out, grads = buffers(a), a.zero_grads()
    r.render_fit(a, obs, 1.0, grads=grads, out=out, check_overflow=False, clear_grads=True)
    assert_same(a, (out[0], out[1], grads), refs[0])
    corners = [(view, slice(y, y + 8), slice(x, x + 8)) for view in (0, 1) for y in (0, 504, 1016) for x in (0, 1016)]
    for view, ys, xs in corners:
        assert (refs[0][1][view, ys, xs] == float("inf")).all() and (refs[1][1][view, ys, xs] == float("inf")).all(), "empty in both poses"
        out[0][view, ys, xs] = SENTINEL
    torch.cuda.synchronize()
    r._kept = r._frame_state(a, out[0], out[1])  # the sentinel writes are this test's own: the claim is made all the same
    got = r.render_fit(b, obs, 1.0, grads=grads, out=out, check_overflow=False, clear_grads=True)
    assert spy == [0, 1]
    torch.cuda.synchronize()
    for view, ys, xs in corners:
        assert (got[0][view, ys, xs] == SENTINEL).all(), ("a tile that stayed empty was written", view, ys, xs)
        got[0][view, ys, xs] = refs[1][0][view, ys, xs]
    assert_same(b, got, refs[1])
    got = r.render_fit(a, obs, 1.0, grads=grads, out=out, check_overflow=False, clear_grads=True)  # (the writes above: refused, a full fill)
    assert spy == [0, 1, 0]
    assert_same(a, got, refs[0])


def test_fit_after_render_takes_the_claim(spy):
    from deodr_amd.hip_renderer import HipRasterizer

    (a, b), obs, refs = poses("after render", FRAMES[2], 2, 3, F64, "image")
    r = HipRasterizer.for_scene(a)
    out = buffers(a)
    r.render(a, 1.0, out=out, check_overflow=True)
    got = r.render_fit(b, obs, 1.0, out=out, check_overflow=False, clear_grads=True)
    assert spy == [1]
    assert_same(b, got, refs[1])


def test_census_of_a_retained_step():
    from deodr_amd.hip_renderer import HipRasterizer, tile_census

    (a, b), obs, _refs = poses("census", FRAMES[1], 2, 4, F32, "colour")
    plain, kept = HipRasterizer.for_scene(a, retain_frames=False), HipRasterizer.for_scene(a)
    out_plain, out_kept = buffers(a), buffers(a)
    for ds in (a, b, a):
        plain.render_fit(ds, obs, 1.0, out=out_plain, check_overflow=False, clear_grads=True)
        kept.render_fit(ds, obs, 1.0, out=out_kept, check_overflow=False, clear_grads=True)
        assert tile_census(kept, ds) == tile_census(plain, ds) and tile_census(plain, ds)[0] > 0
