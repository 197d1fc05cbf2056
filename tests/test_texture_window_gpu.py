"""The texture gradient where owner_adjoint (deodr_amd/csrc/dr_backward.h) changes its path: one window in LDS for the tile, one per 4 x 4-pixel
quadrant, none; both capacities; every shape of a flush pass; the borders of the texture; texture sides around 65 535.

Scenes and predictor: tests/texture_window_cases.py (its docstring says how a case is built); tests/test_texture_window_cases.py proves on the CPU that
every case is in the regime it is named for.  Here each test asserts that again from the checker's z-buffer before it runs the library, at the
capacity of the path it takes; the capacities (WIN_CAP_DEFAULT = 384, WIN_CAP_WAVE_LDS = 768) and the pairing rule's constants are read from the
kernel sources.  Which tiles hold an edge is also read back from the device (tile_census).

Regimes: a window well inside the capacity; exactly at 768 and at 384 for 1, 2, 3 and 4 channels, each with a twin one texel wider (quadrants that
all fit); quadrants mixed in one tile (one fits, one scatters, one untextured, one background) for 1 - 4 channels; every quadrant scatters; flush
rows of 6, 9, 12, 20, 21, 31 (several per pass), 33, 63 (one per pass, idle lanes), 64 (C = 4 and C = 1), 65 and 66 elements, in windows of 11 rows
and of 5 - 6; a window that touches texel 0 and the last texel on every side; uv beyond the texture on all four sides; a 2 x 2 texture; sides of
65 535 (packed bounds, u at the far end) and 65 537 along u and along v (unpacked bounds: one window that fits, one that must scatter).

Paths: (i) fit step, edge-free tile of an 8 x 8 frame (cannot pair: capacity 768); (ii) fit step, a textured PAIR (tile A at capacity, tile B with
mixed quadrants: the second call meets the table the first one used) -- in a 256 x 128 frame, the smallest the scan kernel pairs tiles in, with the
scene in its first two tiles; (iii) fit step, tile with a flagged textured edge at sigma > 0 (capacity 384; the edge's own taps are scattered);
(iv) render + render_backward with and without an edge (384); (v) the antialiase_error adjoint with and without an edge; (vi) the un-staged
family, compared with the staged one in every case and run on its own through the `family` fixture; (vii) 8 views in one launch of the 256 x 128
frame: the two-kernel form of the textured forward, texture_b summed over the views.  float32 and float64 frames everywhere.

Per case: frame and z as compare_forward checks them; ij_b, colors_b, shade_b, uv_b against the checker and texture_b against the repaired one at
TOL of tests/test_hip_parity.py (several views: the sum of the per-view references); the fit step's texture_b against the two-call path's and the
un-staged family's (1e-9 of the largest entry with float64 frames, 1e-5 with float32); with float64 frames a texel that is exactly 0 in the
reference is exactly 0.  texture_b is a contiguous view in the middle of a larger buffer filled with a sentinel (an odd number of elements in
front of it): after every call the bands on both sides are bit-identical to the sentinel, also when the step clears the gradients itself.

What the paths leave out: every case of tests/texture_window_cases.py::CASES runs on (i), (iv) and (vi).  The edge-tile paths (iii), (iv with
an edge) run EDGE_CASES: inside, at 384 and one texel beyond (1 - 4 channels), mixed quadrants (1 - 4 channels), every quadrant scatters, rows
of 9, 33, 64 and 66, uv beyond the texture, the u-long 65 537 side fitting and scattering -- not border_touch, the 2 x 2 texture, the 65 535 side,
the v-long 65 537 side and the other row lengths.  (v) runs AA_CASES, a subset of those.  The pair (ii) and the 8-view form (vii) run two
regimes: a window exactly at 768 next to mixed quadrants (with an edge in (vii)).  That the two tiles of (ii) were walked AS A PAIR is asserted
from a Python restatement of tile_scan_kernel's rule and of fwd_tile_blocks (texture_window_cases.pairs_up) only: the device keeps no record of
it, and tile_census tells the edge tiles alone.  If the rule in the kernel changes, the restatement has to follow.  Nor can a test that
compares results see which of two correct paths a tile took: `<=` made `<` at a capacity computes the same gradient.

Planted on copies of dr_backward.h, each defect failed these tests (and no other kind of assertion than texture_b against the repaired
checker): rows per pass one too many -- every row* case except the rows of 6 and 9 elements in windows of 5 - 6 rows (one pass holds them) -- 142 tests; a window side `+ 1` for `+ 2` -- 152 tests, every regime
with a window; no zeroing of a fitting quadrant's window -- the *_wider and mixed_* cases, the pair, the 8-view form, 76 tests; no scatter in the
unpacked branch -- the side_65537_*_scatters cases, 11 tests.  `<=` made `<`: none, as said.  (Rows per pass one too FEW must not be planted: for
rows of 33 - 63 elements the flush loop then never advances.)

Not covered: grads["texture_b"] = None for a scene WITH a texture -- the ABI refuses it before any kernel runs (as the reference does, H.h:2694;
asserted below), so "the other gradients without a texture gradient" cannot be observed; the deterministic mode's det_texture; windows of tiles
that are partly outside the frame (tests/test_hip_parity.py::test_partial_tiles_odd_frame_size renders such frames)."""

import copy

import numpy as np
import pytest
import torch

import texture_window_cases as twc
from test_hip_parity import F32, F64, TOL, checker
from texture_window_cases import CAP_EDGE, CAP_FREE, CASES, EDGE_CASES, K

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
STALE = 123.0  # what a previous step left in the gradient arrays (clear_grads must wipe it)
# fit step against the two-call path / the un-staged family, relative to the largest entry: the bounds the suite uses for such pairs (compare_fit_step, test_hip_round5.py)
PATHS_TOL = {F64: 1e-9, F32: 1e-5}


class Guarded:
    """texture_b [Ht, Wt, C] as a contiguous view in the middle of a larger buffer of sentinels"""

    def __init__(self, ds, fill):
        shape = tuple(ds.texture.shape)
        self.n = int(np.prod(shape))
        self.guard = max(4096, 2 * shape[1] * shape[2]) + 3  # (more than two rows of the texture; odd: the view is aligned to its elements only)
        self.buf = torch.full((2 * self.guard + self.n,), SENTINEL, dtype=ds.pixel_dtype, device=ds.device)
        self.view = self.buf[self.guard : self.guard + self.n].view(shape)
        assert self.view.is_contiguous() and self.view.data_ptr() == self.buf.data_ptr() + self.guard * self.buf.element_size()
        self.view.fill_(fill)

    def intact(self):
        band = torch.full((self.guard,), SENTINEL, dtype=self.buf.dtype, device=self.buf.device)
        return torch.equal(self.buf[: self.guard], band) and torch.equal(self.buf[self.guard + self.n :], band)


def grads_with_guard(ds, fill):
    g = ds.zero_grads()
    for v in g.values():
        v.fill_(fill)
    guard = Guarded(ds, fill)
    g["texture_b"] = guard.view
    return g, guard


def to_np(g):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in g.items()}


def check_frame(image, z, img_ref, z_ref, tol_img):
    from hip_util import image_report

    err, flipped = image_report(image, img_ref, z, z_ref, tol_img)
    assert flipped == 0, f"{flipped} pixels changed owner"
    assert err < tol_img, err
    fin = np.isfinite(z_ref)
    assert np.array_equal(np.isfinite(z), fin)
    if fin.any():
        assert np.abs(z[fin] - z_ref[fin]).max() < tol_img * max(1.0, np.abs(z_ref[fin]).max())


def check_grads(g, refs, fixes, dt, what, fixed_everything=False):
    """g: the library's gradients; refs / fixes: per view, the checker's and the repaired checker's"""
    from hip_util import rel_err

    tol = TOL[dt][1]
    per_view = fixes if fixed_everything else refs
    for i, r in enumerate(per_view):
        for k in ("ij_b", "colors_b", "shade_b"):
            assert rel_err(g[k][i], r[k]) < tol, (what, k, i)
    assert rel_err(g["uv_b"], sum(r["uv_b"] for r in per_view)) < tol, (what, "uv_b")
    tex_ref = sum(r["texture_b"] for r in fixes)
    assert np.abs(tex_ref).max() > 0
    assert rel_err(g["texture_b"], tex_ref) < tol, (what, "texture_b (vs repaired reference, defect D1)")
    if dt == F64:
        never = np.all([r["texture_b"] == 0 for r in fixes], axis=0)
        assert (g["texture_b"][never] == 0).all(), (what, "a texel the reference never touches is exactly 0")


def assert_same_paths(a, b, dt, what):
    from hip_util import rel_err

    assert rel_err(a["texture_b"], b["texture_b"]) < PATHS_TOL[dt], (what, "texture_b")
    assert rel_err(a["uv_b"], b["uv_b"]) < PATHS_TOL[dt], (what, "uv_b")


def assert_regimes(api, views, sigma, expect_by_tile, cap):
    """every view's tiles are in the regime the case names, at the capacity of the path about to run (from the checker's z-buffer)"""
    for s in views:
        z = checker(api).render(s, sigma)[1]
        for (tx, ty), expect in expect_by_tile.items():
            got = twc.tile_regime(s, z, cap, tx, ty)
            assert twc.matches(got, expect), ((tx, ty), cap, got)


def check_scene(api, views, sigma, dt, expect_free, expect_edge, edge_tiles, seed=11, unstaged_too=True, census=True):
    """Paths (i) / (ii) / (iii) / (vii) (whichever the scene is built for), (iv) and (vi) on one scene: fit step, render + render_backward, the
    un-staged fit step.  expect_free / expect_edge: {(tx, ty): expectation} for the tiles the fit step walks with the whole LDS / for the
    capacity of the two-call kernels and of tiles with edges; edge_tiles: tiles with a silhouette edge per view."""
    from hip_util import device_scene
    from deodr_amd import hip_renderer as hr
    from deodr_amd.hip_renderer import HipRasterizer, tile_census

    assert_regimes(api, views, sigma, expect_free, CAP_FREE)
    assert_regimes(api, views, sigma, expect_edge, CAP_EDGE)
    ds = device_scene(views, dt)
    r = HipRasterizer.for_scene(ds)
    n, H, W, C = ds.n_views, ds.height, ds.width, ds.nb_colors
    obs = np.random.RandomState(seed).rand(n, H, W, C)
    obs_t = torch.as_tensor(obs, device=ds.device, dtype=dt)
    # the fit step clears the gradients itself: exactly the array
    stale, guard = grads_with_guard(ds, STALE)
    image, z, g = r.render_fit(ds, obs_t, sigma, grads=stale, check_overflow=True, clear_grads=True)
    torch.cuda.synchronize()
    assert guard.intact(), "fit step: texture_b was written beyond the array"
    g_fit = to_np(g)
    # two calls
    image2, z2 = r.render(ds, sigma)
    edged = tile_census(r, ds)[1] if census else None  # (the staged forward's tile lists: the un-staged family keeps none)
    fresh, guard = grads_with_guard(ds, 0.0)
    g2 = r.render_backward(ds, residual_obs=obs_t, grads=fresh)
    torch.cuda.synchronize()
    assert guard.intact(), "render_backward: texture_b was written beyond the array"
    g_two = to_np(g2)
    assert torch.equal(image, image2) and torch.equal(z, z2), "the fused forward writes the same frame"
    assert edged is None or edged == n * edge_tiles, ("tiles with a silhouette edge", edged)
    # the checker, fed with the residual of the library's own frame
    refs, fixes = [], []
    image_np, z_np = image.cpu().numpy().astype(np.float64), z.cpu().numpy().astype(np.float64)
    for i, s in enumerate(views):
        img_ref, z_ref = checker(api).render(s, sigma)
        check_frame(image_np[i], z_np[i], img_ref, z_ref, TOL[dt][0])
        image_b = 2 * (image_np[i] - obs_t[i].cpu().numpy().astype(np.float64))
        refs.append(checker(api).grads(s, sigma, img_ref, z_ref, image_b))
        fixes.append(checker(api, fixed=True).grads(s, sigma, img_ref, z_ref, image_b))
    check_grads(g_fit, refs, fixes, dt, "fit step")
    check_grads(g_two, refs, fixes, dt, "two calls")
    assert_same_paths(g_fit, g_two, dt, "fit step vs two calls")
    if unstaged_too:
        hr.force_generic(True)
        try:
            stale, guard = grads_with_guard(ds, STALE)
            image3, _z3, g3 = HipRasterizer.for_scene(ds).render_fit(ds, obs_t, sigma, grads=stale, check_overflow=True, clear_grads=True)
            torch.cuda.synchronize()
        finally:
            hr.force_generic(False)
        assert guard.intact(), "un-staged fit step: texture_b was written beyond the array"
        g_gen = to_np(g3)
        check_grads(g_gen, refs, fixes, dt, "un-staged fit step")
        assert_same_paths(g_fit, g_gen, dt, "fit step vs un-staged family")
    return g_fit


def views_of(s, n):
    """n views of one mesh and texture: the same geometry (the same regimes), shades, colours and observations of their own"""
    views = []
    for i in range(n):
        v = copy.copy(s)
        rs = np.random.RandomState(100 + i)
        v.shade = np.where(s.shade > 0, 0.5 + 0.5 * rs.rand(*s.shade.shape), 0.0)
        v.colors = np.where(s.colors > 0, 0.2 + 0.8 * rs.rand(*s.colors.shape), 0.0)
        views.append(v)
    return views


# ---- (i), (iv), (vi): an edge-free tile that cannot pair -- the whole LDS in the fit step, the staging area in the two-call kernels


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_edge_free_tile(oracle_api, name, dt):
    c = CASES[name]
    s = twc.single_tile_scene(c)
    assert not twc.chunked_frame(s, 1, 1.0)  # regime: one plain work list, nothing pairs
    check_scene(oracle_api, [s], 1.0, dt, {(0, 0): c.expect[CAP_FREE]}, {(0, 0): c.expect[CAP_EDGE]}, edge_tiles=0)


# ---- (iii), (iv), (vi): a tile with a flagged textured edge -- the staging area on every path, the edge's taps through texture_scatter


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_tile_with_a_textured_edge(oracle_api, name, dt):
    c = EDGE_CASES[name]
    s = twc.single_tile_scene(c, edge=True)
    check_scene(oracle_api, [s], 1.0, dt, {}, {(0, 0): c.expect[CAP_EDGE]}, edge_tiles=1)


# ---- (ii): a textured pair


def pair_scene():
    return twc.two_tile_scene(CASES[f"cap{CAP_FREE}_c3"].builder, CASES["mixed_c3"].builder, (96, 96))


PAIR_EXPECT = {(0, 0): CASES[f"cap{CAP_FREE}_c3"].expect, (1, 0): CASES["mixed_c3"].expect}


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n_views", [1, 3])
def test_textured_pair(oracle_api, n_views, dt):
    views = views_of(pair_scene(), n_views)
    for s in views:
        z = checker(oracle_api).render(s, 1.0)[1]
        assert twc.pairs_up(s, z, n_views, 1.0, 0, 0)  # regime: the scan kernel's rule
    check_scene(oracle_api, views, 1.0, dt, {t: e[CAP_FREE] for t, e in PAIR_EXPECT.items()}, {t: e[CAP_EDGE] for t, e in PAIR_EXPECT.items()}, edge_tiles=0)


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_edge_free_tile_next_to_a_tile_with_an_edge(oracle_api, dt):
    """the same two tiles, the right one with a flagged textured edge: no pair; the left one is an entry of the rest of the work list (the
    edge-free instance, the whole LDS), the right one of its head (the staging area)"""
    s = twc.two_tile_scene(CASES[f"cap{CAP_FREE}_c3"].builder, EDGE_CASES["mixed_c3"].builder, (96, 96), edge_b=True)
    z = checker(oracle_api).render(s, 1.0)[1]
    assert twc.chunked_frame(s, 1, 1.0) and not twc.pairs_up(s, z, 1, 1.0, 0, 0)
    check_scene(oracle_api, [s], 1.0, dt, {(0, 0): PAIR_EXPECT[(0, 0)][CAP_FREE]}, {(0, 0): PAIR_EXPECT[(0, 0)][CAP_EDGE], (1, 0): EDGE_CASES["mixed_c3"].expect[CAP_EDGE]}, edge_tiles=1)


# ---- (vii): 8 views in one launch, the two-kernel form


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_eight_views_two_kernel_form(oracle_api, dt):
    n = K["TEX_TWO_KERNELS"]
    s = twc.two_tile_scene(CASES[f"cap{CAP_FREE}_c3"].builder, EDGE_CASES["mixed_c3"].builder, (96, 96), edge_b=True)
    views = views_of(s, n)
    z = checker(oracle_api).render(s, 1.0)[1]
    # regime (select_forward of dr_dispatch.h): a textured fit step at sigma > 0 of TEX_TWO_KERNELS views, walkers in whole units, the head a multiple of 8
    blocks = twc.fwd_tile_blocks(512, n, True)
    assert blocks % (8 * K["WORK_CHUNK"]) == 0 and blocks % 4 == 0 and (blocks // 4) % 8 == 0 and not twc.pairs_up(s, z, n, 1.0, 0, 0)
    check_scene(oracle_api, views, 1.0, dt, {(0, 0): PAIR_EXPECT[(0, 0)][CAP_FREE]}, {(0, 0): PAIR_EXPECT[(0, 0)][CAP_EDGE], (1, 0): EDGE_CASES["mixed_c3"].expect[CAP_EDGE]}, edge_tiles=1)


# ---- (v): the antialiase_error adjoint


AA_CASES = [("inside", False), (f"cap{CAP_EDGE}_c3", False), (f"cap{CAP_EDGE}_c3_wider", False), ("mixed_c3", False), ("side_65537_u_scatters", False),
            ("inside", True), (f"cap{CAP_EDGE}_c3", True), (f"cap{CAP_EDGE}_c3_wider", True), ("mixed_c3", True), ("all_scatter", True), ("row33_c3", True),
            ("border_beyond", True), ("side_65537_u_scatters", True)]  # fmt: skip


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name,edge", AA_CASES)
def test_antialiase_error_adjoint(oracle_api, name, edge, dt):
    """renderScene_B with antialiaseError (raster_bwd_fast_kernel for the tile without an edge, bwd_err_tile for the one with): every gradient
    against the repaired reference (defects D1 + D2), as tests/test_hip_parity.py::test_backward_parity_antialiase_error does"""
    from hip_util import device_scene
    from deodr_amd.hip_renderer import HipRasterizer, tile_census

    c = (EDGE_CASES if edge else CASES)[name]
    s = twc.single_tile_scene(c, edge=edge)
    sigma = 1.0
    assert_regimes(oracle_api, [s], sigma, {(0, 0): c.expect[CAP_EDGE]}, CAP_EDGE)
    rs = np.random.RandomState(11)
    obs, err_b = rs.rand(s.height, s.width, c.C), rs.rand(s.height, s.width)
    ds = device_scene(s, dt)
    r = HipRasterizer.for_scene(ds)
    out = r.render(ds, sigma, True, torch.as_tensor(obs).reshape(1, s.height, s.width, c.C), check_overflow=True)
    assert tile_census(r, ds)[1] == int(edge)
    stock, fixed = checker(oracle_api), checker(oracle_api, fixed=True)
    image, z, err = stock.render(s, sigma, True, obs)
    assert np.abs(out[2][0].cpu().numpy() - err).max() < 10 * TOL[dt][0] * max(1.0, err.max())
    fresh, guard = grads_with_guard(ds, 0.0)
    g = to_np(r.render_backward(ds, err_buffer_b=torch.as_tensor(err_b).reshape(1, s.height, s.width), grads=fresh))
    torch.cuda.synchronize()
    assert guard.intact(), "antialiase_error adjoint: texture_b was written beyond the array"
    check_grads(g, None, [fixed.grads(s, sigma, image, z, None, True, obs, err, err_b)], dt, "antialiase_error", fixed_everything=True)


# ---- (vi) on its own: every call on the un-staged kernels, and on the staged ones again


FAMILY_CASES = [("mixed_c3", False), (f"cap{CAP_FREE}_c3", False), ("all_scatter", False), ("side_65537_u_scatters", False), ("border_beyond", True), ("mixed_c4", True)]


@pytest.mark.parametrize("name,edge", FAMILY_CASES)
def test_both_kernel_families(oracle_api, family, name, edge):
    c = (EDGE_CASES if edge else CASES)[name]
    s = twc.single_tile_scene(c, edge=edge)
    check_scene(oracle_api, [s], 1.0, F64, {} if edge else {(0, 0): c.expect[CAP_FREE]}, {(0, 0): c.expect[CAP_EDGE]}, edge_tiles=int(edge), unstaged_too=False, census=family == "staged")


# ---- grads["texture_b"] = None


@pytest.mark.parametrize("edge", [False, True])
def test_texture_gradient_cannot_be_left_out(oracle_api, edge):
    """A scene with a texture needs texture_b on every path with an adjoint (the reference: H.h:2694): the call is refused before a kernel runs and
    the other gradient arrays are untouched"""
    from hip_util import device_scene
    from deodr_amd.hip_renderer import HipRasterizer

    s = twc.single_tile_scene((EDGE_CASES if edge else CASES)["mixed_c3"], edge=edge)
    ds = device_scene(s, F64)
    r = HipRasterizer.for_scene(ds)
    obs_t = torch.zeros(1, s.height, s.width, 3, dtype=F64, device=ds.device)
    g = ds.zero_grads()
    g["texture_b"] = None
    with pytest.raises(RuntimeError, match="texture_b == NULL"):
        r.render_fit(ds, obs_t, 1.0, grads=g, check_overflow=True, clear_grads=True)
    r.render(ds, 1.0)
    with pytest.raises(RuntimeError, match="texture_b == NULL"):
        r.render_backward(ds, residual_obs=obs_t, grads=g)
    torch.cuda.synchronize()
    assert all(float(v.abs().max()) == 0 for v in g.values() if v is not None)
