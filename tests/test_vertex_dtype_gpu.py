"""Float32 vertex arrays (``vertex_dtype = DEODR_HIP_F32``, ``DeviceMesh(dtype=torch.float32)``) on every instance of setup_bin_kernel,
finalize_kernel and det_convert_kernel that reads or writes them: the cases of tests/vertex_dtype_cases.py, each run with float32 and with float64
vertex arrays holding the same (float32) values, both compared with oracle/_ref.

Frames: all arithmetic is double on equal values, so the two runs write the same bits.  Gradients: the float64-vertex run is held to the existing
contract (TOL of tests/test_hip_parity.py), the float32-vertex run to 1e-4, and with float64 frames -- where nothing else rounds -- also to
``B + TOL[F64][1]`` per array, B being the bound of float32 accumulation that tests/vertex_dtype_cases.py derives from the checker alone.  The
deterministic mode is exact: the int64 shadows receive the same contributions in both runs, and the float32 array receives the float64 array's value
rounded once.

The gradient arrays of every call are carved out of NaN-filled buffers (64 elements on either side, which keeps torch's 16-byte alignment): a
wrong element size or stride in a view other than the first writes into the padding or leaves a NaN behind."""

import numpy as np
import pytest
import torch

import vertex_dtype_cases as vc
from test_hip_parity import F32, F64, TOL
from vertex_dtype_cases import CASES, SIGMA, VERTEX_GRADS

pytestmark = pytest.mark.gpu

PAD = 64
FOUND = []  # (case, route, array, error against the checker, B): printed by the last test, for the table of measured errors


# ---------------------------------------------------------------------------------------------------------------- device side


class Guarded:
    """the four vertex gradient arrays of `ds` inside NaN-filled buffers, filled with `fill`; texture_b as zero_grads() makes it"""

    def __init__(self, ds, fill):
        self.buffers, self.grads = {}, {}
        for k, like in (("ij_b", ds.ij), ("colors_b", ds.colors), ("shade_b", ds.shade), ("uv_b", ds.uv)):
            b = torch.full((like.numel() + 2 * PAD,), float("nan"), dtype=like.dtype, device=like.device)
            inner = b[PAD : PAD + like.numel()].view(like.shape)
            inner.fill_(fill)
            assert inner.data_ptr() % 16 == 0 and inner.is_contiguous()
            self.buffers[k], self.grads[k] = b, inner
        self.grads["texture_b"] = None if ds.texture is None else torch.zeros_like(ds.texture)

    def check(self, what):
        for k, b in self.buffers.items():
            n = self.grads[k].numel()
            assert bool(torch.isnan(b[:PAD]).all()) and bool(torch.isnan(b[PAD + n :]).all()), f"{what}: {k} was written outside the array"
            assert not bool(torch.isnan(self.grads[k]).any()), f"{what}: {k} holds a NaN (an element that was not cleared, or a NaN contribution)"
        return self.grads


def numpy64(g):
    return {k: (None if v is None else v.detach().cpu().numpy().astype(np.float64)) for k, v in g.items()}


def stacked(name, views, what):
    H, W, C = views[0].height, views[0].width, views[0].nb_colors
    return np.stack([vc.seeds(name, i, (H, W) if what == "err_b" else (H, W, C), what) for i in range(len(views))])


def device_run(name, views, pix, vtx, aa):
    """every route of one case with one vertex dtype -> dict of frames (tensors) and gradients (float64 NumPy)"""
    from hip_util import device_scene
    from deodr_amd.hip_renderer import HipRasterizer

    ds = device_scene(views, pix, vtx)
    assert ds.ij.dtype == vtx and ds.colors.dtype == vtx and ds.shade.dtype == vtx and ds.uv.dtype == vtx and ds.depths.dtype == vtx
    r = HipRasterizer.for_scene(ds)
    obs = torch.as_tensor(stacked(name, views, "obs"), device=ds.device, dtype=pix)
    image_b = torch.as_tensor(stacked(name, views, "image_b"), device=ds.device, dtype=pix)
    out = {}
    # the fit step over arrays that hold NaN: clear_grads has to reach every element (the three unreferenced vertices of the mesh cases too)
    cleared = Guarded(ds, float("nan"))
    image, z, _g = r.render_fit(ds, obs, SIGMA, grads=cleared.grads, check_overflow=True, clear_grads=True)
    out["fit"] = numpy64(cleared.check("fit step, clear_grads"))
    out["fit_frame"] = (image.clone(), z.clone())
    # the fit step accumulating into arrays that hold 0.25
    kept = Guarded(ds, 0.25)
    r.render_fit(ds, obs, SIGMA, grads=kept.grads, check_overflow=False, clear_grads=False)
    out["fit_accumulated"] = numpy64(kept.check("fit step, accumulating"))
    # the two-call adjoint, with a free image_b and with the residual
    image2, z2 = r.render(ds, SIGMA)
    out["render_frame"] = (image2.clone(), z2.clone())
    free = Guarded(ds, 0.0)
    r.render_backward(ds, image_b=image_b, grads=free.grads)
    out["image_b"] = numpy64(free.check("render_backward(image_b)"))
    two = Guarded(ds, 0.0)
    r.render_backward(ds, residual_obs=obs, grads=two.grads)
    out["residual"] = numpy64(two.check("render_backward(residual_obs)"))
    # 2. the types of the arrays the library's wrapper makes itself
    g = r.render_backward(ds, residual_obs=obs)
    assert all(g[k].dtype == vtx for k in VERTEX_GRADS) and (g["texture_b"] is None or g["texture_b"].dtype == pix)
    if aa:
        err_b = torch.as_tensor(stacked(name, views, "err_b"), device=ds.device, dtype=pix)
        _image, _z, err = r.render(ds, SIGMA, True, obs)  # (render_backward hands the frame of this forward to the library)
        out["err_buffer"] = err.clone()
        adj = Guarded(ds, 0.0)
        r.render_backward(ds, err_buffer_b=err_b, grads=adj.grads)
        out["antialiase_error"] = numpy64(adj.check("render_backward(err_buffer_b)"))
    torch.cuda.synchronize()
    over, _need, errors = r.status(ds)
    assert not over and not errors
    return out


# ---------------------------------------------------------------------------------------------------------------- checker side

_shared_refs = {}


def frames_ref(api, name, views):
    """the checker's frame of every view, computed once per case"""
    key = (name, "frames")
    if key not in _shared_refs:
        _shared_refs[key] = [vc.checker(api).render(s, SIGMA) for s in views]
    return _shared_refs[key]


def grads_ref(api, name, views, image_b, key=None):
    """per-view gradients of the checker for the seeds `image_b` [n,H,W,C] (texture_b of the repaired one), computed once per `key`"""
    if key is not None and (name, key) in _shared_refs:
        return _shared_refs[(name, key)]
    frames = frames_ref(api, name, views)
    textured = bool(np.asarray(views[0].textured).any())
    per_view = []
    for i, s in enumerate(views):
        g = vc.checker(api).grads(s, SIGMA, frames[i][0], frames[i][1], image_b[i])
        if textured:
            g["texture_b"] = vc.checker(api, fixed=True).grads(s, SIGMA, frames[i][0], frames[i][1], image_b[i])["texture_b"]
        per_view.append(g)
    if key is not None:
        _shared_refs[(name, key)] = per_view
    return per_view


def assert_frame(image, z, image_ref, z_ref, pix):
    """compare_forward's checks (tests/test_hip_parity.py) on a frame that is already rendered"""
    from hip_util import image_report

    image, z = image.cpu().numpy().astype(np.float64), z.cpu().numpy().astype(np.float64)
    tol = TOL[pix][0]
    err, flipped = image_report(image, image_ref, z, z_ref, tol)
    assert flipped == 0, f"{flipped} pixels changed owner"
    assert err < tol, err
    fin = np.isfinite(z_ref)
    assert np.array_equal(np.isfinite(z), fin)
    assert not fin.any() or np.abs(z[fin] - z_ref[fin]).max() < tol * max(1.0, np.abs(z_ref[fin]).max())


def compare(name, route, got, per_view, tols, offset=0.0):
    """`got` (all views) against the per-view references: ij_b, colors_b, shade_b view by view, uv_b and texture_b against the sum over the
    views; every array that is not identically zero at ``tols[array]``, the others exactly zero (``offset``: what the arrays held before)"""
    from hip_util import rel_err

    worst = {}
    for k in ("ij_b", "colors_b", "shade_b"):
        for i, g in enumerate(per_view):
            if np.abs(g[k]).max() > 0:
                worst[k] = max(worst.get(k, 0.0), rel_err(got[k][i], offset + g[k]))
            else:
                assert np.array_equal(got[k][i], np.full_like(got[k][i], offset)), (name, route, k, i, "the reference has no gradient here")
    for k in ("uv_b", "texture_b"):
        total = sum(g[k] for g in per_view)
        if got[k] is None or not np.size(total):
            continue
        if np.abs(total).max() > 0:
            worst[k] = rel_err(got[k], (offset if k == "uv_b" else 0.0) + total)
        else:
            assert np.array_equal(got[k], np.full_like(got[k], offset if k == "uv_b" else 0.0)), (name, route, k, "the reference has no gradient here")
    print(f"{name:18s} {route:24s} " + "  ".join(f"{k} {e:.2e} (tol {tols[k]:.2e})" for k, e in worst.items()))
    for k, e in worst.items():
        assert e < tols[k], (name, route, k, e, tols[k])
    return worst


def tolerances(pix, vtx, B=None):
    """{array: tolerance}: TOL[pix][1] for float64 vertex arrays; 1e-4 for float32 ones, and min(1e-4, B + TOL[F64][1]) with float64 frames;
    texture_b has the pixel type in both runs"""
    t = {k: (TOL[pix][1] if vtx == F64 else TOL[F32][1]) for k in VERTEX_GRADS}
    if vtx == F32 and pix == F64:
        t = {k: min(TOL[F32][1], vc.bound(B[k]) + TOL[F64][1]) for k in VERTEX_GRADS}
    t["texture_b"] = TOL[pix][1]
    return t


# ------------------------------------------------------------------------------------------------------------------ the cases


def check_case(api, name, pix):
    c, views = CASES[name], vc.views_of(name)
    vc.assert_regime(name)
    n = len(views)
    runs = {vtx: device_run(name, views, pix, vtx, c.aa) for vtx in (F32, F64)}
    a, b = runs[F32], runs[F64]
    # 1. frames: the same bits from both vertex types, fit step and plain render; the float32 run against the checker
    for which in ("fit_frame", "render_frame"):
        assert torch.equal(a[which][0], b[which][0]) and torch.equal(a[which][1], b[which][1]), which
    assert torch.equal(a["fit_frame"][0], a["render_frame"][0]) and torch.equal(a["fit_frame"][1], a["render_frame"][1])
    frames = frames_ref(api, name, views)
    for i in range(n):
        assert_frame(a["fit_frame"][0][i], a["fit_frame"][1][i], frames[i][0], frames[i][1], pix)
    # 3. gradients, three routes (2., the types, and 5., the guards, are asserted where the arrays are made: device_run)
    obs, image_b = stacked(name, views, "obs"), stacked(name, views, "image_b")
    residual = 2 * (a["fit_frame"][0].cpu().numpy().astype(np.float64) - obs)
    seeds = {"image_b": (image_b, "image_b"), "residual": (residual, None), "fit": (residual, None), "fit_accumulated": (residual, None)}
    bounds = {}
    for route, (seed, key) in seeds.items():
        ref = grads_ref(api, name, views, seed, key) if route in ("image_b", "residual") else ref  # (the three residual routes share one reference)
        if pix == F64 and route in ("image_b", "residual"):
            bounds[route] = vc.float32_bound(api, views, SIGMA, lambda i: seed[i])
        B = bounds.get("image_b" if route == "image_b" else "residual")
        if route == "fit_accumulated":
            # 5. clear_grads off: 0.25 + gradient; one more rounding, of the sum with what the array held
            tol32 = tolerances(pix, F32, B)
            if pix == F64:
                tol32 = {k: (t if k == "texture_b" else min(TOL[F32][1], t + vc.U32)) for k, t in tol32.items()}
            compare(name, route + " f32", a[route], ref, tol32, offset=0.25)
            compare(name, route + " f64", b[route], ref, tolerances(pix, F64), offset=0.25)
            continue
        worst = compare(name, route + " f32", a[route], ref, tolerances(pix, F32, B))
        compare(name, route + " f64", b[route], ref, tolerances(pix, F64))
        if pix == F64:
            FOUND.extend((name, route, k, e, vc.bound(B[k])) for k, e in worst.items() if k in VERTEX_GRADS)
    # 4. the antialiase_error adjoint, against the repaired reference
    if c.aa:
        stock, fixed = vc.checker(api), vc.checker(api, fixed=True)
        err_b = stacked(name, views, "err_b")
        per_view = []
        for i, s in enumerate(views):
            image, z, err = stock.render(s, SIGMA, True, obs[i])
            assert np.abs(a["err_buffer"][i].cpu().numpy() - err).max() < 10 * TOL[pix][0] * max(1.0, err.max())
            per_view.append(fixed.grads(s, SIGMA, image, z, None, True, obs[i], err, err_b[i]))

        def corner_adjoint(u, i):
            image, z, err = stock.render(u, SIGMA, True, obs[i])
            return fixed.grads(u, SIGMA, image, z, None, True, obs[i], err, err_b[i])

        B = vc.float32_bound(api, views, SIGMA, None, grads_of=corner_adjoint) if pix == F64 else None
        worst = compare(name, "antialiase_error f32", a["antialiase_error"], per_view, tolerances(pix, F32, B))
        compare(name, "antialiase_error f64", b["antialiase_error"], per_view, tolerances(pix, F64))
        if pix == F64:
            FOUND.extend((name, "antialiase_error", k, e, vc.bound(B[k])) for k, e in worst.items() if k in VERTEX_GRADS)


def deterministic_run(name, views, pix, vtx, how):
    from hip_util import device_scene
    from deodr_amd import hip_renderer as hr

    ds = device_scene(views, pix, vtx)
    if how == "scene":
        ds.deterministic = True
    else:
        hr.set_deterministic(True)
    try:
        r = hr.HipRasterizer.for_scene(ds)
        obs = torch.as_tensor(stacked(name, views, "obs"), device=ds.device, dtype=pix)
        image_b = torch.as_tensor(stacked(name, views, "image_b"), device=ds.device, dtype=pix)
        out = {}
        for again in ("", "_again"):
            cleared = Guarded(ds, float("nan"))
            image, _z, _g = r.render_fit(ds, obs, SIGMA, grads=cleared.grads, check_overflow=True, clear_grads=True)
            out["fit" + again] = {k: (None if v is None else v.clone()) for k, v in cleared.check("deterministic fit step").items()}
            r.render(ds, SIGMA)
            two = Guarded(ds, 0.0)
            r.render_backward(ds, image_b=image_b, grads=two.grads)
            out["image_b" + again] = {k: (None if v is None else v.clone()) for k, v in two.check("deterministic render_backward").items()}
        torch.cuda.synchronize()
        over, _need, errors = r.status(ds)
        assert not over and not errors & hr.ERR_DET_RANGE and not errors
        out["image"] = image.clone()
        return out
    finally:
        if how != "scene":
            hr.set_deterministic(False)


def check_deterministic(api, name, pix):
    c, views = CASES[name], vc.views_of(name)
    vc.assert_regime(name)
    a, b = (deterministic_run(name, views, pix, vtx, c.det) for vtx in (F32, F64))
    assert torch.equal(a["image"], b["image"])
    for route in ("fit", "image_b"):
        for k in VERTEX_GRADS:
            assert a[route][k].dtype == F32 and b[route][k].dtype == F64
            assert torch.equal(a[route][k], b[route][k].to(F32)), (route, k, "the float32 array is the float64 array rounded once")
            assert torch.equal(a[route][k], a[route + "_again"][k]) and torch.equal(b[route][k], b[route + "_again"][k]), (route, k, "a second call gives the same bits")
        if a[route]["texture_b"] is not None:
            assert torch.equal(a[route]["texture_b"], b[route]["texture_b"]) and torch.equal(a[route]["texture_b"], a[route + "_again"]["texture_b"]), route
    # (that the bits are the right ones: the float32 run against the checker, as in the default mode)
    obs, image_b = stacked(name, views, "obs"), stacked(name, views, "image_b")
    residual = 2 * (a["image"].cpu().numpy().astype(np.float64) - obs)
    # (texture_b too at 1e-4: a texel is a sum of hundreds of contributions, each rounded to the fixed point's 2^-32)
    tols = {k: TOL[F32][1] for k in VERTEX_GRADS + ("texture_b",)}
    compare(name, "det fit f32", numpy64(a["fit"]), grads_ref(api, name, views, residual), tols)
    compare(name, "det image_b f32", numpy64(a["image_b"]), grads_ref(api, name, views, image_b, "image_b"), tols)


@pytest.mark.parametrize("pix", [F32, F64], ids=["pix32", "pix64"])
@pytest.mark.parametrize("name", list(CASES))
def test_float32_vertex_arrays(oracle_api, name, pix):
    if CASES[name].det:
        check_deterministic(oracle_api, name, pix)
    else:
        check_case(oracle_api, name, pix)


def test_measured_errors_stay_below_the_bound(oracle_api):
    """the table of the float64-frame runs above: error of the float32 arrays against the checker, B, and their ratio (a ratio above 1 is a finding
    about the code; the runs above have asserted error < B + TOL[F64][1] already).  Runs `mesh_c4` itself when it is run alone.

    Measured on an MI355X, the worst route of each case (error / B):
      mesh_c1 ij_b 5.2e-8 / 2.3e-6, colors_b 6.1e-8 / 2.3e-6        mesh_c2 ij_b 1.1e-7 / 4.3e-6, colors_b 8.3e-8 / 2.3e-6
      mesh_c3 ij_b 5.8e-8 / 2.3e-6, colors_b 8.2e-8 / 2.3e-6        mesh_c4 ij_b 6.4e-8 / 2.8e-6, colors_b 1.2e-7 / 2.3e-6
      mesh_c6 ij_b 8.2e-8 / 2.7e-6, colors_b 8.1e-8 / 2.3e-6        mesh_tex ij_b 7.4e-8 / 2.5e-6, shade_b 1.0e-7 / 2.3e-6, uv_b 9.8e-8 / 6.6e-6
      soup_mixed ij_b 7.4e-8, colors_b 7.1e-8, shade_b 6.9e-8, uv_b 5.6e-8, each / 4.8e-7 (the largest ratio of all: 0.16)
      soup_mixed_x3 ij_b 6.6e-8, colors_b 6.7e-8, shade_b 7.1e-8, each / 4.8e-7, uv_b 2.5e-7 / 2.2e-6
      above_sparse ij_b 1.2e-7 / 3.7e-6, colors_b 1.3e-7 / 2.3e-6   table_c1 ij_b 1.1e-7 / 4.0e-6, colors_b 7.4e-8 / 2.9e-6
      table_c3 ij_b 1.1e-7 / 5.3e-6, colors_b 8.7e-8 / 2.4e-6       table_tex ij_b 1.6e-7 / 4.5e-6, shade_b 1.3e-7 / 2.6e-6, uv_b 3.1e-7 / 1.7e-4"""
    if not FOUND:
        check_case(oracle_api, "mesh_c4", F64)
    print()
    for name, route, k, e, B in FOUND:
        print(f"TABLE {name:14s} {route:18s} {k:9s} error {e:.3e}  B {B:.3e}  ratio {e / B:.3f}")
    assert all(e < B + TOL[F64][1] for _n, _r, _k, e, B in FOUND)


# ---------------------------------------------------------------------------------------------------------------- end to end

@pytest.mark.parametrize("textured", [False, True], ids=["colours", "texture"])
def test_float32_device_mesh_end_to_end(textured):
    """``DeviceMesh(dtype=torch.float32)`` in a ``Scene3DDevice`` at 128 x 128, ``render_l2`` and ``backward``, against the same mesh and values as
    float64: the scene it renders has float32 vertex arrays, the frame is the float64 mesh's, the gradients agree to 1e-4 of the largest entry"""
    from hip_util import rel_err

    loss64, image64, grads64, _scene = vc.l2_step(F64, textured)
    loss32, image32, grads32, scene = vc.l2_step(F32, textured)
    ds = scene._state[1]
    assert ds.vertex_dtype == F32 and ds.ij.dtype == F32 and ds.colors.dtype == F32 and ds.shade.dtype == F32 and ds.uv.dtype == F32
    assert np.abs(image32 - image64).max() < vc.E2E_FRAME_TOL
    assert sorted(grads32) == sorted(grads64) == sorted(["vertices", "texture" if textured else "colors"])
    for k in grads64:
        assert np.abs(grads64[k]).max() > 0
        assert rel_err(grads32[k], grads64[k]) < 1e-4, k
