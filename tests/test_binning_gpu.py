"""The binning of setup_bin_kernel (deodr_amd/csrc/dr_setup.h, dr_binning.h) and the tile lists it writes, where their paths change: the cases of
tests/binning_cases.py.  tests/test_binning_cases.py proves on the CPU that every case is in the regime it is named for; the same assertions run
again when this module is imported (under a second), so a GPU run cannot compare a scene that left its regime.

Groups: boxes of 1 x 1 .. 13 x 10 tiles (0 .. 19 blocks for bin_rest), one by one in the sparse layout and as the eight views of a dense launch; a
triangle wavefront whose blocks total one less than a round of bin_rest, exactly one, one more and more than two, sparse (16 triangles per
wavefront) and dense (64), the widest boxes at the first and the last lane; the non-strict rule's kept column in a block bin_rest deals, the row of
an exactly horizontal edge that the same rule draws beyond the triangle (its tiles are kept by row), and their strict twins; boxes clamped at
every border, triangles outside on every side, a frame of 100 x 77; bands at sigma = 3 of several blocks, a dense edge block of more than PRIM_BLOCK flagged slots (a second round, itself of two rounds of bin_rest) and its sparse twin; stacks of K_TRI - 1 ..
K_TRI + 65 triangles in one tile (the pool; a chunk of 64 pairs with more matches than a batch has room for), in two tiles, textured; stacks of
K_EDGE - 1 .. EMAX + 1 edges in one tile.  Each group has a case of two and of four channels (the three setup_bin_kernel<., NC> instances).

Every case, on both kernel families: forward and the two-call adjoint of a free image_b (compare_backward; single views), the one-call fit step
against the checker and against the two-call adjoint of the residual (compare_fit_step), at TOL of tests/test_hip_parity.py with float64 frames,
one case per group with float32 frames too.  Then once more with the gradient arrays between NaN guards (tests/test_vertex_dtype_gpu.py): nothing
written outside, nothing left uncleared, and the figures of that run -- against the checker, computed once per case -- are kept for the last test,
which prints the worst of the file.  Staged family: tile_census after the fit step and after the forward equals the CPU census.

Out of reach: which lane served a block leaves no trace in the result; the order of pairs in a pool is decided by the atomics, so two tiles
interleaved in one chunk (tri_stack_two_tiles) are likely, not forced."""

import numpy as np
import pytest
import torch

import binning_cases as bc
from binning_cases import CASES
from test_hip_parity import F32, F64, TOL, checker, compare_backward, compare_fit_step
from test_vertex_dtype_gpu import Guarded, numpy64

pytestmark = pytest.mark.gpu

for _name in CASES:  # the regime of every case, before anything runs on the device
    bc.assert_regime(_name)

# the float32-frame run of each group
F32_CASES = {"boxes": "box_all_dense", "rounds": "rounds_twice_dense", "non_strict": "kept_column", "clipping": "clip_100x77",
             "bands": "bands_second_round_dense", "tri_lists": "tri_stack_textured", "edge_lists": "edge_stack_beyond_emax"}  # fmt: skip
assert sorted(F32_CASES) == bc.GROUPS and all(CASES[n].group == g for g, n in F32_CASES.items())

FOUND = []  # (case, family, dtype, figure, error in units of its tolerance)
_REFERENCE = {}


def reference(api, name):
    """Per view (image, z, gradients of sum (image - obs)^2; texture_b of the repaired checker), computed once per process, never written to"""
    if name not in _REFERENCE:
        views, sigma, _d = bc.built(name)
        obs = bc.observation(name)
        out = []
        for i, s in enumerate(views):
            image, z = checker(api).render(s, sigma)
            g = checker(api).grads(s, sigma, image, z, 2 * (image - obs[i]))
            if np.size(s.texture):
                g["texture_b"] = checker(api, fixed=True).grads(s, sigma, image, z, 2 * (image - obs[i]))["texture_b"]
            for a in (image, z, *g.values()):
                if isinstance(a, np.ndarray):
                    assert not np.isnan(a).any(), "the checker itself has no answer for this scene"
                    a.setflags(write=False)
            out.append((image, z, g))
        _REFERENCE[name] = out
    return _REFERENCE[name]


def guarded_run(api, name, dt, family):
    """fit step and two-call adjoint with the gradient arrays between NaN guards, the census, the figures"""
    from hip_util import device_scene, rel_err
    from deodr_amd.hip_renderer import HipRasterizer, tile_census

    views, sigma, d = bc.built(name)
    ds = device_scene(views, dt)
    r = HipRasterizer.for_scene(ds)
    obs = torch.as_tensor(bc.observation(name), device=ds.device, dtype=dt)
    cleared = Guarded(ds, float("nan"))
    image, z, _g = r.render_fit(ds, obs, sigma, grads=cleared.grads, check_overflow=True, clear_grads=True)
    runs = {"fit": numpy64(cleared.check("fit step, clear_grads"))}
    if family == "staged":  # (the un-staged family keeps no tile lists of the scan)
        assert tile_census(r, ds) == bc.census(d), "census after the fit step"
    frame = (image.cpu().numpy().astype(np.float64), z.cpu().numpy().astype(np.float64))
    r.render(ds, sigma, check_overflow=True)
    if family == "staged":
        assert tile_census(r, ds) == bc.census(d), "census after the forward"
    two = Guarded(ds, 0.0)
    r.render_backward(ds, residual_obs=obs, grads=two.grads)
    runs["two_calls"] = numpy64(two.check("render_backward(residual_obs)"))
    torch.cuda.synchronize()
    over, _need, errors = r.status(ds)
    assert not over and not errors

    refs = reference(api, name)
    tol_img, tol_g = TOL[dt]
    figures = {}
    for i, (image_ref, z_ref, g_ref) in enumerate(refs):
        assert np.array_equal(np.isfinite(frame[1][i]), np.isfinite(z_ref)), f"coverage of view {i}"
        figures[f"image[{i}]"] = float(np.abs(frame[0][i] - image_ref).max()) / tol_img
        for route, g in runs.items():
            for k in ("ij_b", "colors_b", "shade_b"):
                figures[f"{route} {k}[{i}]"] = rel_err(g[k][i], g_ref[k]) / tol_g
    for route, g in runs.items():
        figures[f"{route} uv_b"] = rel_err(g["uv_b"], sum(ref[2]["uv_b"] for ref in refs)) / tol_g
        if np.size(views[0].texture):
            figures[f"{route} texture_b"] = rel_err(g["texture_b"], sum(ref[2]["texture_b"] for ref in refs)) / tol_g
    worst_image = max(v for k, v in figures.items() if k.startswith("image"))
    worst_grad = max(v for k, v in figures.items() if not k.startswith("image"))
    print(f"{name} {family} {str(dt).split('.')[-1]}: image {worst_image:.2e}, gradients {worst_grad:.2e} (units of the tolerance)")
    FOUND.append((name, family, str(dt).split(".")[-1], worst_image, worst_grad))
    for k, v in figures.items():
        assert v < 1.0, (name, k, v)


def run_case(api, name, dt, family):
    views, sigma, _d = bc.built(name)
    if len(views) == 1:
        compare_backward(api, views[0], sigma, dt)
    compare_fit_step(api, views, sigma, dt)
    guarded_run(api, name, dt, family)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_float64_frames(oracle_api, family, name):
    run_case(oracle_api, name, F64, family)


@pytest.mark.parametrize("group", sorted(F32_CASES))
def test_group_float32_frames(oracle_api, family, group):
    run_case(oracle_api, F32_CASES[group], F32, family)


def test_report_worst_errors():
    """the worst image and gradient error of the file, in units of the tolerance (needs the tests above to have run in this process)"""
    for dtype in ("float64", "float32"):
        rows = [f for f in FOUND if f[2] == dtype]
        if rows:
            by_image, by_grad = max(rows, key=lambda f: f[3]), max(rows, key=lambda f: f[4])
            print(f"{dtype} frames, {len(rows)} runs: worst image error {by_image[3]:.2e} of the tolerance ({by_image[0]}, {by_image[1]}), "
                  f"worst gradient error {by_grad[4]:.2e} ({by_grad[0]}, {by_grad[1]})")  # fmt: skip
    assert all(f[3] < 1.0 and f[4] < 1.0 for f in FOUND)
