"""antialiase_error on the LDS-staged kernels where their paths change: the VAR = 1 instances of raster_fwd_fast_kernel, the p.aa_err branch of
bwd_fast_tile, bwd_err_tile / raster_bwd_edge_err_kernel (deodr_amd/csrc/dr_forward.h, dr_backward.h).

Scenes, constants and regime predicates: tests/aa_error_cases.py; tests/test_aa_error_cases.py proves on the CPU that every case is in the regime it
is named for.  The same assertions run again when this module is imported (milliseconds), so a GPU run cannot compare a scene that left its regime.

Regimes: a chunked frame (529 tiles, ragged: empty, edge-free and edge tiles, every edge list, a head and a rest of the work list; untextured with 4
channels, textured, and at sigma = 0, where everything goes through the owner-tile kernel); a fine mesh whose head of 194 entries holds edge-free
tiles as second entries of its 128 walkers (the owner-tile launch of the adjoint after `rank += stride`) and tiles of more than K_TRI triangles; a
head of 290 entries on 128 head walkers (a second and a
third entry per walker; tiles of exactly TB and TB + 1 edges); more than K_EDGE edges in a tile (the edge pool of gather_sorted_edges), exactly EMAX
= 128 (the last batch of tm[]), more than EMAX (the ordered-search branch of the forward, the un-staged adjoint inside bwd_err_tile); more edge tiles
(1 056) than persistent waves of raster_bwd_edge_err_kernel; one and two channels; a pixel centre 4.6e-7 pixels from an edge line (need_replay
over 32 edges behind it, 20 drawn over the pixel and 12 not: two batch boundaries, masks that differ from batch to batch) and its twin on the
un-blend branch; three views of a chunked frame.  Every case with float32 and float64 frames.

Per case and view, against the repaired checker (defects D1, D2): image, error buffer (relative to max(1, err.max())) and which pixels are covered;
ij_b, colors_b, shade_b; uv_b and texture_b against the sum over the views -- 1e-9 / 1e-8 with float64 frames, 1e-5 / 1e-4 with float32, the
tolerances of tests/test_hip_round6.py.  Each case prints what it measured.  The counts of tiles with work and with edges are read back from the
device (tile_census) and must be those of the CPU census.  chunked_head_twice runs once more on the un-staged family, held to the bounds of
test_hip_round6.py for the two families.  deodr_hip_render_scene_b refuses antialiase_error with image == NULL on the host, on both families.

What these tests cannot see: which walker took which entry (the device keeps no record; the restated formulas of aa_error_cases.py say so), and
which of two correct paths a tile took.  Left out: the permuted rank of fwd_tiles (strides of whole units of 512 walkers: frames of 640 x 640 and
more; tests/test_aa_error_cases.py::test_what_the_cases_leave_out_the_permuted_rank).

Planted on copies of the kernel sources, each defect failed these tests: the replay of bwd_err_tile reading tm[0] for every batch; the walkers of
raster_bwd_edge_err_kernel striding over every second tile; the mask of the eighth batch of tm[] dropped in pass A; forward walkers skipping their
second entry."""

import ctypes as C

import numpy as np
import pytest
import torch

import aa_error_cases as ac
from aa_error_cases import CASES

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
TOL = {F64: (1e-9, 1e-8), F32: (1e-5, 1e-4)}  # image / gradients: the project's own
FAMILIES_TOL = {F64: (1e-10, 1e-9), F32: (2e-6, 1e-5)}  # error buffer / gradients, staged against un-staged (tests/test_hip_round6.py)

for _name in CASES:  # the regime of every case, before anything runs on the device
    ac.assert_regime(_name)


def run(name, dt):
    """forward + adjoint of the case on the family in force -> (ds, rasterizer, [image, z, err], gradients)"""
    from hip_util import hip_grads, hip_render

    views, sigma, _cs = ac.case(name)
    obs, err_b = ac.inputs(name)
    ds, r, out = hip_render(views, sigma, dt, True, obs)
    return ds, r, out, hip_grads(ds, r, err_buffer_b=err_b)


def compare_with_checker(api, name, dt, out, g):
    """every figure of the comparison, printed, then asserted"""
    from hip_util import rel_err

    views, _sigma, _cs = ac.case(name)
    refs = ac.reference(api, name)
    tol_img, tol_g = TOL[dt]
    figures, covered = {}, True
    for i, (image, z, err, g_ref) in enumerate(refs):
        figures[f"image[{i}]"] = (float(np.abs(out[0][i] - image).max()), tol_img)
        figures[f"err[{i}]"] = (float(np.abs(out[2][i] - err).max() / max(1.0, err.max())), tol_img)
        covered = covered and bool((np.isfinite(out[1][i]) == np.isfinite(z)).all())
        for k in ("ij_b", "colors_b", "shade_b"):
            figures[f"{k}[{i}]"] = (rel_err(g[k][i], g_ref[k]), tol_g)
    if np.size(views[0].texture):
        figures["uv_b"] = (rel_err(g["uv_b"], sum(r[3]["uv_b"] for r in refs)), tol_g)
        figures["texture_b"] = (rel_err(g["texture_b"], sum(r[3]["texture_b"] for r in refs)), tol_g)
    print(f"{name} {str(dt).split('.')[-1]}: " + ", ".join(f"{k} {v:.2e}" for k, (v, _t) in figures.items()) + f", coverage equal {covered}")
    assert covered, "finiteness of z"
    for k, (v, t) in figures.items():
        assert v < t, (name, k, v, t)
    assert all(np.isfinite(v).all() for v in g.values() if v is not None)


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_case_against_the_repaired_checker(oracle_api, name, dt):
    from deodr_amd.hip_renderer import tile_census

    _views, _sigma, cs = ac.case(name)
    ds, r, out, g = run(name, dt)
    # the device binned what the CPU census says: tiles with work, tiles with silhouette edges, over the views
    assert tile_census(r, ds) == (sum(c.ntiles - c.empty for c in cs), sum(c.edge_tiles for c in cs))
    compare_with_checker(oracle_api, name, dt, out, g)


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_head_walked_twice_on_the_unstaged_family(oracle_api, dt):
    """chunked_head_twice on the un-staged kernels: against the checker as every case, and against the staged family at the bounds
    tests/test_hip_round6.py holds the two families to"""
    from deodr_amd import hip_renderer as hr
    from hip_util import rel_err

    name = "chunked_head_twice"
    _ds, _r, out, g = run(name, dt)
    hr.force_generic(True)
    try:
        _ds2, _r2, out2, g2 = run(name, dt)
    finally:
        hr.force_generic(False)
    compare_with_checker(oracle_api, name, dt, out2, g2)
    tol_err, tol_g = FAMILIES_TOL[dt]
    figures = {"err": float(np.abs(out[2][0] - out2[2][0]).max() / max(1.0, np.abs(out2[2][0]).max()))}
    figures.update({k: rel_err(g[k], g2[k]) for k in ("ij_b", "colors_b", "shade_b", "uv_b", "texture_b")})
    print(f"{name} {str(dt).split('.')[-1]} staged against un-staged: " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    assert figures.pop("err") < tol_err
    for k, v in figures.items():
        assert v < tol_g, (k, v)


PATTERN = 0.625  # what the gradient arrays hold before the refused call


def test_null_image_is_refused_on_the_host(family):
    """deodr_hip_render_scene_b with antialiase_error and image == NULL (through the C ABI directly): the staged kernels would read the frame of
    the tiles without silhouette edges through that pointer.  The call returns non-zero before anything is launched, the message names `image`,
    and the gradient arrays still hold the pattern they were filled with -- on either family."""
    from deodr_amd import hip_renderer as hr
    from hip_util import device_scene

    views, sigma, _cs = ac.case("few_channels_2")
    obs, err_b = ac.inputs("few_channels_2")
    s = views[0]
    ds = device_scene(views, F64)
    r = hr.HipRasterizer.for_scene(ds)
    obs_t = torch.as_tensor(obs, dtype=F64, device=ds.device).reshape(1, s.height, s.width, s.nb_colors)
    eb_t = torch.as_tensor(err_b, dtype=F64, device=ds.device).reshape(1, s.height, s.width)
    image, _z, _err = r.render(ds, sigma, True, obs_t, check_overflow=True)
    grads = ds.zero_grads()
    for v in grads.values():
        if v is not None:
            v.fill_(PATTERN)
    torch.cuda.synchronize()
    with torch.cuda.device(ds.device):
        args = (sigma, 1, hr._ptr(obs_t), None, hr._ptr(eb_t), hr._ptr(r.workspace), r.nbytes, 1, hr._stream(ds.device))
        rc = hr.lib().deodr_hip_render_scene_b(C.byref(ds.c_struct(grads)), None, None, None, *args)
        message = hr.lib().deodr_hip_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and "image" in message, (rc, message)
    for k, v in grads.items():
        assert v is None or bool((v == PATTERN).all()), k
    # the same call with the frame of the forward is accepted and accumulates onto the pattern
    with torch.cuda.device(ds.device):
        hr._check(hr.lib().deodr_hip_render_scene_b(C.byref(ds.c_struct(grads)), hr._ptr(image), None, None, *args))
    torch.cuda.synchronize()
    assert not bool((grads["ij_b"] == PATTERN).all())
