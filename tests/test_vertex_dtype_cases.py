"""Every case of tests/vertex_dtype_cases.py is what tests/test_vertex_dtype_gpu.py takes it for -- shown with the CPU checker and the host
compilation of deodr_amd/csrc/dr_dispatch.h alone, so that a case that drifts out of its regime fails here and not silently on the GPU -- and
the helpers the bound of the GPU test rests on do what they say."""

import ctypes

import numpy as np
import pytest

import sim_util
import vertex_dtype_cases as vc
from deodr_amd import scenes
from vertex_dtype_cases import CASES, SIGMA, VERTEX_GRADS


@pytest.fixture(scope="module")
def dispatch():
    return sim_util.dispatch_lib()


@pytest.mark.parametrize("name", list(CASES))
def test_case_is_in_its_regime_and_selects_its_instances(dispatch, name):
    c, views = CASES[name], vc.views_of(name)
    vc.assert_regime(name)  # (no two drawn triangles of equal depth sum, the launch's size class, the drawn edges)
    for s in views:
        for k in vc.ROUNDED:  # the values are float32 values: float32 and float64 vertex arrays hold the same numbers
            a = np.asarray(getattr(s, k))
            assert a.dtype == np.float64 and np.array_equal(a, a.astype(np.float32).astype(np.float64)), k
    n, T, C = len(views), len(views[0].faces), views[0].nb_colors
    assert all(len(s.faces) == T and s.nb_colors == C and s.clockwise == views[0].clockwise for s in views)
    out = (ctypes.c_int * 4)()
    dispatch.dispatch_setup(0, C, out)
    assert tuple(out) == c.setup
    dispatch.dispatch_finalize(0, C, int(bool(c.det)), int(vc.table_regime(n, T)), out)
    assert tuple(out) == c.finalize
    if name.startswith("mesh_") or name.startswith("det_mesh_"):  # the unreferenced vertices clear_grads has to reach
        V = len(views[0].depths)
        assert int(np.asarray(views[0].faces).max()) == V - 1 - vc.EXTRA_VERTICES and len(views[0].uv) == V


def test_the_float32_instances_the_cases_reach(dispatch):
    """together the cases run every float32 instance of both kernels but the ones an earlier test runs: {f32, 4, table} (test_finalize_paths_gpu.py:
    test_dtypes)"""
    setup = {c.setup for c in CASES.values()}
    finalize = {c.finalize for c in CASES.values()}
    have_setup = {r for r in _table(dispatch.dispatch_setup_table) if r[0] == 0}
    have_finalize = {r for r in _table(dispatch.dispatch_finalize_table) if r[0] == 0}
    assert setup == have_setup
    assert have_finalize - finalize == {(0, 4, 0, 1)} and finalize <= have_finalize


def _table(fn):
    out = (ctypes.c_int * (4 * 64))()
    n = fn(out, 64)
    return [tuple(out[4 * i : 4 * i + 4]) for i in range(n)]


@pytest.mark.parametrize("name", ["mesh_c4", "mesh_tex"])
def test_unshared_scene_has_the_same_frame_and_its_corner_gradients_sum_to_the_shared_ones(oracle_api, name):
    ref = vc.checker(oracle_api)
    for i, s in enumerate(vc.views_of(name)):
        u = vc.unshared(s)
        assert np.array_equal(u.faces.reshape(-1), np.arange(3 * len(s.faces)))
        image, z = ref.render(s, SIGMA)
        image_u, z_u = ref.render(u, SIGMA)
        assert np.array_equal(image, image_u) and np.array_equal(z, z_u)
        image_b = vc.seeds(name, i, image.shape, "image_b")
        g, corners = ref.grads(s, SIGMA, image, z, image_b), vc.corner_sums(s, ref.grads(u, SIGMA, image_u, z_u, image_b))
        for k in VERTEX_GRADS:
            top = np.abs(g[k]).max()
            assert (top > 0) == (k in c_nonzero(name))
            assert np.abs(corners[k] - g[k]).max() <= 1e-9 * top, k
            assert (corners[k + "_abs"] >= np.abs(corners[k]) - 1e-12 * max(top, 1.0)).all() and corners[k + "_n"].max() <= 6  # (a vertex of this sphere has at most six triangles)


def c_nonzero(name):
    return set(CASES[name].recorded)


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n].recorded])
def test_recorded_bounds_are_the_checkers(oracle_api, name):
    """(rho, A) of the case table, for image_b = 2 (image - rand), seed 1: not below what the checker gives here, not above 1.5 times it"""
    views = vc.views_of(name)
    ref = vc.checker(oracle_api)

    def image_b_of(i):
        image, _z = ref.render(views[i], SIGMA)
        return 2 * (image - np.random.RandomState(1).rand(*image.shape))

    found = vc.float32_bound(oracle_api, views, SIGMA, image_b_of)
    recorded = CASES[name].recorded
    for k in VERTEX_GRADS:
        rho, A = found[k]
        if k not in recorded:
            assert (rho, A) == (0.0, 0), (k, "an array with a gradient has no recorded bound")
            continue
        assert rho <= recorded[k][0] <= 1.5 * rho and A <= recorded[k][1] <= 1.5 * A, (k, found[k], recorded[k])
        assert vc.bound(recorded[k]) < 1e-4 or (k == "uv_b" and len(views) == 74)  # (uv_b over 74 views: there the 1e-4 contract binds)


def test_bound_formula():
    assert vc.bound((1.0, 6)) == 2 * 19 * 2.0**-24 and vc.bound((0.0, 0)) == 0.0


def test_a_scene_with_two_equal_depth_sums_is_rejected():
    """rounding the depths to float32 makes exact ties of depth sums likelier: this sphere has none in float64 and one after rounding"""
    s = scenes.sphere_scene(size=48, nu=50, n_rings=50, nb_colors=3, depth_channel=False)
    assert vc.no_depth_ties(s) and not vc.no_depth_ties(vc.rounded(s))


def test_float32_device_mesh_reaches_the_rasterizer_as_float32_arrays_on_the_host_layer(oracle_api):
    """the host side of the end-to-end GPU test, on CPU tensors with the checker behind the C ABI (tests/fake_hip.py): a float32 DeviceMesh seen by
    the default float64 camera renders, its scene holds float32 vertex arrays, its gradients come back float32 and are the float64 mesh's to 1e-4"""
    import torch

    import fake_hip
    from hip_util import rel_err

    with fake_hip.emulate(vc.checker(oracle_api), vc.checker(oracle_api, fixed=True)):
        for textured in (False, True):
            _loss, image64, grads64, _scene = vc.l2_step(torch.float64, textured, device="cpu", size=64)
            _loss, image32, grads32, scene = vc.l2_step(torch.float32, textured, device="cpu", size=64)
            ds = scene._state[1]
            assert ds.vertex_dtype == torch.float32 and ds.ij.dtype == torch.float32 and ds.uv.dtype == torch.float32
            assert np.abs(image32 - image64).max() < vc.E2E_FRAME_TOL
            for k in grads64:
                assert rel_err(grads32[k], grads64[k]) < 1e-4, k
