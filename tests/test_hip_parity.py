"""GPU parity tests: the HIP path (through the C ABI) against the CPU checkers on identical Scene2D inputs.

Tolerances are the north star's: forward image / depth within 1e-5, gradients within 1e-4 (relative to the largest
entry of the reference gradient) with float32 pixel buffers; with float64 pixel buffers the same kernels must agree to
round-off (1e-9), which shows that the algorithm, not the tolerance, carries the parity.

`texture_b` (defect D1) and the antialiase_error `colors_b` (defect D2) are compared with the REPAIRED reference
(oracle.ref(fixed=True) / oracle.port(fixed=True)), everything else with the reference as shipped.
"""

import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_soup
from deodr_amd import scenes
from test_oracle import BACKWARD_CASES, FLAG_CASES, random_scene

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
TOL = {F32: (1e-5, 1e-4), F64: (1e-9, 1e-8)}


def checker(api, fixed=False):
    return api.ref(fixed=fixed) or api.port(fixed=fixed)


def compare_forward(api, s, sigma, dt, aa=False, obs=None):
    from hip_util import hip_render, image_report

    ref = checker(api)
    out_ref = ref.render(s, sigma, aa, obs)
    ds, r, out = hip_render(s, sigma, dt, aa, obs)
    tol_img = TOL[dt][0]
    err, flipped = image_report(out[0][0], out_ref[0], out[1][0], out_ref[1], tol_img)
    assert flipped == 0, f"{flipped} pixels changed owner"
    assert err < tol_img, err
    zr = out_ref[1]
    fin = np.isfinite(zr)
    assert np.array_equal(np.isfinite(out[1][0]), fin)
    assert np.abs(out[1][0][fin] - zr[fin]).max() < tol_img * max(1.0, np.abs(zr[fin]).max()) if fin.any() else True
    if aa:
        assert np.abs(out[2][0] - out_ref[2]).max() < 10 * tol_img * max(1.0, out_ref[2].max())
    return ds, r, out, out_ref


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("case", range(len(FLAG_CASES)))
@pytest.mark.parametrize("sigma", [0.0, 1.0, 2.5])
def test_forward_parity_flag_space(oracle_api, case, sigma, dt):
    s = random_scene(100 + case, **FLAG_CASES[case])
    if case in (0, 2):
        s.ij = np.round(s.ij)  # integer vertices exercise every tie of the fill rule
    obs = np.random.RandomState(5).rand(s.height, s.width, 3)
    compare_forward(oracle_api, s, sigma, dt)
    compare_forward(oracle_api, s, sigma, dt, True, obs)


def compare_backward(api, s, sigma, dt, seed=7):
    from hip_util import hip_grads, rel_err

    ds, r, out, out_ref = compare_forward(api, s, sigma, dt)
    rs = np.random.RandomState(seed)
    image_b = rs.randn(*out_ref[0].shape)
    g = hip_grads(ds, r, image_b=image_b)
    g_ref = checker(api).grads(s, sigma, out_ref[0], out_ref[1], image_b)
    g_fix = checker(api, fixed=True).grads(s, sigma, out_ref[0], out_ref[1], image_b)
    tol = TOL[dt][1]
    for k in ("ij_b", "colors_b", "uv_b", "shade_b"):
        assert rel_err(g[k][0] if k not in ("uv_b",) else g[k], g_ref[k]) < tol, k
    if g["texture_b"] is not None and np.size(s.texture):
        assert rel_err(g["texture_b"], g_fix["texture_b"]) < tol, "texture_b (vs repaired reference, defect D1)"
    return g, g_ref


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("case", BACKWARD_CASES)
@pytest.mark.parametrize("sigma", [0.0, 1.0, 2.5])
def test_backward_parity_flag_space(oracle_api, case, sigma, dt):
    s = random_scene(200 + case, **FLAG_CASES[case])
    s.backface_culling = True
    compare_backward(oracle_api, s, sigma, dt)


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("case", BACKWARD_CASES)
@pytest.mark.parametrize("sigma", [0.0, 1.0, 2.5])
def test_backward_parity_antialiase_error(oracle_api, case, sigma, dt):
    """renderScene_B with antialiaseError: every gradient against the REPAIRED reference (defects D1 + D2); uv_b / shade_b
    (untouched by the defects) also against the reference as shipped."""
    from hip_util import hip_grads, hip_render, rel_err

    s = random_scene(300 + case, **FLAG_CASES[case])
    s.backface_culling = True
    rs = np.random.RandomState(11)
    obs = rs.rand(s.height, s.width, 3)
    err_b = rs.rand(s.height, s.width)
    ds, r, out = hip_render(s, sigma, dt, True, obs)
    stock, fixed = checker(oracle_api), checker(oracle_api, fixed=True)
    image, z, err = stock.render(s, sigma, True, obs)
    assert np.abs(out[2][0] - err).max() < 10 * TOL[dt][0] * max(1.0, err.max())
    g = hip_grads(ds, r, err_buffer_b=err_b)
    g_fix = fixed.grads(s, sigma, image, z, None, True, obs, err, err_b)
    g_stock = stock.grads(s, sigma, image, z, None, True, obs, err, err_b)
    tol = TOL[dt][1]
    for k in ("ij_b", "colors_b", "shade_b"):
        assert rel_err(g[k][0], g_fix[k]) < tol, k
    assert rel_err(g["uv_b"], g_fix["uv_b"]) < tol
    assert rel_err(g["texture_b"], g_fix["texture_b"]) < tol
    assert rel_err(g["uv_b"], g_stock["uv_b"]) < tol and rel_err(g["shade_b"][0], g_stock["shade_b"]) < tol


@pytest.mark.parametrize("clockwise", [0, 1])
def test_reference_golden_soup(oracle_api, clockwise):
    """The scene of the reference's own triangle-soup tests (tests/golden/soup30_cw*.npz): image, z and every gradient."""
    from hip_util import hip_grads, hip_render, rel_err

    gt, d = golden_soup(clockwise, "gt_")
    target = checker(oracle_api).render(gt, 1)[0]
    init, _ = golden_soup(clockwise, "init_")
    ds, r, out = hip_render(init, 1.0, F32)
    image_ref = checker(oracle_api).render(init, 1)[0]
    assert np.abs(out[0][0] - image_ref).max() < 1e-5
    g = hip_grads(ds, r, image_b=2 * (image_ref - target))
    for k in ("ij_b", "colors_b", "uv_b", "shade_b"):
        got = g[k] if k == "uv_b" else g[k][0]
        assert rel_err(got, d["aa0_" + k]) < 1e-4, k  # the arrays the reference's own build produced


def test_config1_soup_256(oracle_api):
    """BASELINE configs[0]: 256x256, 200 flat-colour soup triangles."""
    s = scenes.soup_scene(n_tri=200, width=256, height=256, seed=2)
    rs = np.random.RandomState(2)
    s.ij = s.ij + rs.randn(*s.ij.shape)
    compare_backward(oracle_api, s, 1.0, F32)


def test_config2_hand_textured(oracle_api):
    """BASELINE configs[1]: 1024x1024 hand mesh, Gouraud + 256x256 texture: uv_b / shade_b / texture_b included."""
    s = scenes.hand_scene(os.path.join(GOLDEN, "hand_mesh.npz"), size=1024, textured=True)
    compare_backward(oracle_api, s, 1.0, F32)


def test_config3_sphere_20k(oracle_api):
    """BASELINE configs[2], the roofline config: 1024x1024, 20 000 triangles, RGB + depth channel."""
    s = scenes.sphere_scene()
    assert s.faces.shape[0] == 20000 and s.colors.shape[1] == 4
    compare_backward(oracle_api, s, 1.0, F32)


def test_batched_views_equal_single_views(oracle_api):
    """configs[3] shape: several poses of one mesh in one launch give exactly the per-view results."""
    from hip_util import hip_grads, hip_render

    path = os.path.join(GOLDEN, "hand_mesh.npz")
    views = [scenes.hand_scene(path, size=256, angle=a, textured=False) for a in np.linspace(-0.5, 0.5, 4)]
    ds, r, out = hip_render(views, 1.0, F32)
    rs = np.random.RandomState(0)
    image_b = rs.randn(4, 256, 256, 3)
    g = hip_grads(ds, r, image_b=image_b)
    for i, v in enumerate(views):
        ds1, r1, out1 = hip_render(v, 1.0, F32)
        assert np.array_equal(out1[0][0], out[0][i]) and np.array_equal(out1[1][0], out[1][i])
        g1 = hip_grads(ds1, r1, image_b=image_b[i])
        assert np.allclose(g1["ij_b"][0], g["ij_b"][i], rtol=1e-9, atol=1e-9)
        assert np.allclose(g1["colors_b"][0], g["colors_b"][i], rtol=1e-9, atol=1e-9)


def test_spill_pool_regrows(oracle_api):
    """Many large overlapping triangles overflow the fixed per-tile lists and a deliberately tiny spill pool."""
    from hip_util import hip_render

    s = scenes.soup_scene(n_tri=700, width=64, height=64, seed=9, min_area=600.0)  # (~150 triangles per tile: inline lists hold 64)
    ref = checker(oracle_api).render(s, 1.0)
    ds, r, out = hip_render(s, 1.0, F64, pool_pairs=16)
    assert r.pool_pairs > 16  # regrown
    assert np.abs(out[0][0] - ref[0]).max() < 1e-9


def test_known_answers_pixel_and_texel_centres():
    """The reference's tests/test_pixel_center_coordinates.py and tests/test_texture_coordinates.py, restated."""
    from deodr_amd.differentiable_renderer import Scene2D

    height, width, eps = 4, 3, 0.001
    corners = [(0, 0), (width - 1, 0), (0, height - 1), (width - 1, height - 1)]
    for integer_pixel_centers in (False, True):
        off = 0.0 if integer_pixel_centers else 0.5
        for cx, cy in corners:
            ij = np.array([[-eps, -eps], [-eps, eps], [eps, -eps]]) + np.array([cx + off, cy + off])
            sc = Scene2D(
                ij=ij, faces=np.array([[0, 2, 1]], dtype=np.uint32), faces_uv=np.array([[0, 2, 1]], dtype=np.uint32),
                uv=np.zeros((3, 2)), texture=np.ones((2, 2, 1)), height=height, width=width, nb_colors=1, background_image=None,
                background_color=np.array([0.0]), depths=np.array([1.0, 1, 1]), textured=np.array([0], dtype=bool),
                shade=np.array([1.0, 1, 1]), colors=np.array([[1.0], [1], [1]]), shaded=np.array([0], dtype=bool),
                edgeflags=np.zeros((1, 3), dtype=bool), strict_edge=False, perspective_correct=True, clockwise=True,
                integer_pixel_centers=integer_pixel_centers,
            )  # fmt: skip
            image, _ = sc.render(sigma=0)
            expected = np.zeros((height, width, 1))
            expected[cy, cx, 0] = 1
            assert np.allclose(expected, image)
    texture = np.array([[[1, 0, 0], [0, 1, 0]], [[0, 0, 1], [1, 1, 1]]], dtype=np.float64)
    for clockwise in (False, True):
        f = np.array([[0, 2, 1]] if clockwise else [[0, 1, 2]], dtype=np.uint32)
        sc = Scene2D(
            ij=np.array([[1.0, 1], [1, 15], [15, 1]]), faces=f, faces_uv=f.copy(), uv=np.array([[0.0, 0], [1, 0], [0, 1]]),
            texture=texture, height=40, width=60, nb_colors=3, background_image=None, background_color=np.zeros(3),
            depths=np.ones(3), textured=np.array([1], dtype=bool), shade=np.ones(3), colors=np.eye(3),
            shaded=np.array([1], dtype=bool), edgeflags=np.zeros((1, 3), dtype=bool), strict_edge=False, perspective_correct=True,
            clockwise=clockwise,
        )  # fmt: skip
        image, _ = sc.render(sigma=0)
        assert np.allclose(image[0, :, :], 0) and np.allclose(image[:, 0, :], 0)
        assert np.allclose(image[1, 1, :], [1, 0, 0]) and np.allclose(image[15, 1, :], [0, 1, 0]) and np.allclose(image[1, 15, :], [0, 0, 1])


def test_dropin_scene2d_matches_reference(oracle_api):
    """Scene2D.render_compare_and_backward through the NumPy drop-in entry points (stateless adjoint)."""
    from hip_util import rel_err

    gt, d = golden_soup(0, "gt_")
    target = checker(oracle_api).render(gt, 1)[0]
    s, _ = golden_soup(0, "init_")
    image, z, err_buffer, err = s.render_compare_and_backward(obs=target, sigma=1)
    assert abs(err - float(d["aa0_loss"])) < 1e-8 * float(d["aa0_loss"])
    for k in ("ij_b", "colors_b", "uv_b", "shade_b"):
        assert rel_err(getattr(s, k), d["aa0_" + k]) < 1e-9, k


def test_errors_are_returned(oracle_api):
    from hip_util import device_scene
    from deodr_amd.hip_renderer import HipRasterizer

    s = random_scene(1, backface_culling=False)
    ds = device_scene(s)
    r = HipRasterizer.for_scene(ds)
    r.render(ds, 1.0)
    with pytest.raises(RuntimeError, match="backface_culling"):
        r.render_backward(ds, image_b=torch.zeros(1, s.height, s.width, 3))


def test_autograd_function_matches_reference(oracle_api):
    """deodr.pytorch's operator signature: forward(ij, colors, scene) -> image, backward -> (ij_b, colors_b, None)."""
    from types import SimpleNamespace

    from hip_util import rel_err
    from deodr_amd.pytorch import TorchDifferentiableRender2D

    gt, d = golden_soup(0, "gt_")
    target = checker(oracle_api).render(gt, 1)[0]
    s, _ = golden_soup(0, "init_")
    scene = SimpleNamespace(scene_2d=s)
    for device in ("cpu", "cuda"):
        ij = torch.tensor(s.ij, dtype=torch.float64, device=device, requires_grad=True)
        colors = torch.tensor(s.colors, dtype=torch.float64, device=device, requires_grad=True)
        image = TorchDifferentiableRender2D(ij, colors, scene)
        assert image.device.type == device and image.shape == (s.height, s.width, 3)
        loss = ((image - torch.as_tensor(target, device=device)) ** 2).sum()
        loss.backward()
        assert abs(loss.item() - float(d["aa0_loss"])) < 1e-8 * float(d["aa0_loss"])
        assert rel_err(ij.grad.cpu().numpy(), d["aa0_ij_b"]) < 1e-9
        assert rel_err(colors.grad.cpu().numpy(), d["aa0_colors_b"]) < 1e-9


def test_autograd_batched_views(oracle_api):
    from hip_util import device_scene, rel_err
    from deodr_amd.hip_renderer import HipRasterizer
    from deodr_amd.pytorch import TorchDifferentiableRenderViews

    path = os.path.join(GOLDEN, "hand_mesh.npz")
    views = [scenes.hand_scene(path, size=128, angle=a, textured=False) for a in (-0.3, 0.4)]
    ds = device_scene(views, F32)
    r = HipRasterizer.for_scene(ds)
    ij = ds.ij.clone().requires_grad_(True)
    colors = ds.colors.clone().requires_grad_(True)
    image = TorchDifferentiableRenderViews(ij, colors, ds, r, 1.0)
    w = torch.as_tensor(np.random.RandomState(1).rand(*image.shape), device=image.device, dtype=image.dtype)
    (image * w).sum().backward()
    for i, v in enumerate(views):
        ref = checker(oracle_api)
        img_ref, z_ref = ref.render(v, 1.0)
        assert np.abs(image[i].detach().cpu().numpy() - img_ref).max() < 1e-5
        g_ref = ref.grads(v, 1.0, img_ref, z_ref, w[i].cpu().numpy().astype(np.float64))
        assert rel_err(ij.grad[i].cpu().numpy(), g_ref["ij_b"]) < 1e-4
        assert rel_err(colors.grad[i].cpu().numpy(), g_ref["colors_b"]) < 1e-4


def test_residual_mode_equals_explicit_image_b(oracle_api):
    """Extension of the C ABI: image_b == NULL + obs -> 2 (image - obs) is formed inside the adjoint kernel."""
    from hip_util import device_scene
    from deodr_amd.hip_renderer import HipRasterizer

    s = random_scene(400)
    s.backface_culling = True
    from hip_util import rel_err

    ds = device_scene(s, F32)
    r = HipRasterizer.for_scene(ds)
    image, z = r.render(ds, 1.0)
    obs = torch.as_tensor(np.random.RandomState(2).rand(1, s.height, s.width, 3).astype(np.float32), device=image.device)
    g_a = r.render_backward(ds, image_b=2 * (image - obs))
    g_b = r.render_backward(ds, residual_obs=obs)
    for k in ("ij_b", "colors_b", "uv_b", "shade_b", "texture_b"):  # image_b is rounded to float32 in one of the two paths
        assert rel_err(g_b[k].cpu().numpy(), g_a[k].cpu().numpy()) < 1e-5, k


def test_config5_shape_textured_2048(oracle_api):
    """One view of BASELINE configs[4]: 2048x2048, 100 352-triangle sphere, 1024x1024 texture (uv_b / shade_b / texture_b)."""
    s = scenes.sphere_scene(size=2048, nu=224, n_rings=224, nb_colors=3, textured=True, texture_size=1024)
    assert s.faces.shape[0] == 100352
    compare_backward(oracle_api, s, 1.0, F32)


def compare_fit_step(api, views, sigma, dt, seed=11):
    """deodr_hip_render_scene_fit (fused forward + adjoint of sum (image - obs)^2) against the CPU checker fed with
    image_b = 2 (image - obs), and against the two-call path of the same library."""
    from hip_util import device_scene, rel_err

    if not isinstance(views, (list, tuple)):
        views = [views]
    ds = device_scene(views, dt)
    r = HipRasterizer_for(ds)
    n, H, W, Cc = ds.n_views, ds.height, ds.width, ds.nb_colors
    obs = np.random.RandomState(seed).rand(n, H, W, Cc)
    obs_t = torch.as_tensor(obs, device=ds.device, dtype=dt)
    stale = ds.zero_grads()
    for v in stale.values():
        if v is not None:
            v.fill_(123.0)  # clear_grads must wipe whatever a previous step left
    image, z, g = r.render_fit(ds, obs_t, sigma, grads=stale, check_overflow=True, clear_grads=True)
    image2, z2 = r.render(ds, sigma)
    g2 = r.render_backward(ds, residual_obs=obs_t)
    torch.cuda.synchronize()
    assert torch.equal(image, image2) and torch.equal(z, z2), "the fused forward writes the same frame"
    tol_img, tol = TOL[dt]
    uv_ref, tex_ref = 0.0, 0.0  # (shared by the views: the sum of the per-view references)
    for i, s in enumerate(views):
        ref = checker(api)
        img_ref, z_ref = ref.render(s, sigma)
        assert np.abs(image[i].cpu().numpy() - img_ref).max() < tol_img
        image_b = 2 * (image[i].cpu().numpy().astype(np.float64) - obs_t[i].cpu().numpy().astype(np.float64))
        g_ref = ref.grads(s, sigma, img_ref, z_ref, image_b)
        g_fix = checker(api, fixed=True).grads(s, sigma, img_ref, z_ref, image_b)
        for k in ("ij_b", "colors_b", "shade_b"):
            assert rel_err(g[k][i].cpu().numpy(), g_ref[k]) < tol, (k, "vs checker")
            # (float32 frames: the fit step of an untextured scene sums a tile's residuals in float32 -- owner_adjoint_slots --, the two-call
            # path in double)
            assert rel_err(g[k][i].cpu().numpy(), g2[k][i].cpu().numpy()) < (1e-9 if dt == F64 else 5e-6), (k, "vs two calls")
        uv_ref, tex_ref = uv_ref + g_ref["uv_b"], tex_ref + g_fix["texture_b"]
    assert rel_err(g["uv_b"].cpu().numpy(), uv_ref) < tol, "uv_b"
    assert rel_err(g["uv_b"].cpu().numpy(), g2["uv_b"].cpu().numpy()) < 1e-9
    if g["texture_b"] is not None and np.size(views[0].texture):
        assert rel_err(g["texture_b"].cpu().numpy(), tex_ref) < tol, "texture_b (vs repaired reference, defect D1)"
        # float64 frames: round-off of the atomics' order; float32 texture_b: float32 atomics in both paths (tests/test_hip_round5.py)
        assert rel_err(g["texture_b"].cpu().numpy(), g2["texture_b"].cpu().numpy()) < (1e-9 if dt == F64 else 1e-5), ("texture_b", "vs two calls")


def HipRasterizer_for(ds):
    from deodr_amd.hip_renderer import HipRasterizer

    return HipRasterizer.for_scene(ds)


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("case", BACKWARD_CASES)
@pytest.mark.parametrize("sigma", [0.0, 1.0, 2.5])
def test_fit_step_flag_space(oracle_api, case, sigma, dt):
    s = random_scene(300 + case, **FLAG_CASES[case])
    s.backface_culling = True
    compare_fit_step(oracle_api, s, sigma, dt)


def test_fit_step_sphere_20k(oracle_api):
    compare_fit_step(oracle_api, scenes.sphere_scene(), 1.0, F32)


def test_fit_step_hand_textured_views(oracle_api):
    path = os.path.join(GOLDEN, "hand_mesh.npz")
    compare_fit_step(oracle_api, scenes.hand_scene(path, size=256, angle=0.2, textured=True), 1.0, F32)
    compare_fit_step(oracle_api, [scenes.hand_scene(path, size=256, angle=a, textured=False) for a in (-0.4, 0.1, 0.5)], 1.0, F32)


def test_autograd_l2_loss_op_equals_render_then_loss(oracle_api):
    """TorchRenderViewsL2Loss (one fused call) against TorchDifferentiableRenderViews + a torch loss (two passes)."""
    from hip_util import device_scene, rel_err
    from deodr_amd.hip_renderer import HipRasterizer
    from deodr_amd.pytorch import TorchDifferentiableRenderViews, TorchRenderViewsL2Loss

    path = os.path.join(GOLDEN, "hand_mesh.npz")
    views = [scenes.hand_scene(path, size=128, angle=a, textured=False) for a in (-0.3, 0.4)]
    ds = device_scene(views, F32)
    r = HipRasterizer.for_scene(ds)
    obs = torch.as_tensor(np.random.RandomState(4).rand(2, 128, 128, 3).astype(np.float32), device=ds.device)
    grads = []
    for fused in (True, False):
        ij = ds.ij.clone().requires_grad_(True)
        colors = ds.colors.clone().requires_grad_(True)
        if fused:
            loss = TorchRenderViewsL2Loss(ij, colors, obs, ds, r, 1.0)
        else:
            loss = ((TorchDifferentiableRenderViews(ij, colors, ds, r, 1.0).double() - obs.double()) ** 2).sum()
        (3.0 * loss).backward()
        grads.append((float(loss), ij.grad.cpu().numpy(), colors.grad.cpu().numpy()))
    assert abs(grads[0][0] - grads[1][0]) <= 1e-9 * abs(grads[1][0])
    assert rel_err(grads[0][1], grads[1][1]) < 1e-5 and rel_err(grads[0][2], grads[1][2]) < 1e-5


@pytest.mark.parametrize("dt", [F32, F64])
def test_partial_tiles_odd_frame_size(oracle_api, dt):
    """Frame sizes that are not multiples of the 8 x 8 tile (the last tile row / column is partly outside the frame), two-call
    path, fit step, and a 3-view batch whose tile rows cannot be dealt to the XCDs in strips (tiles_y = 5)."""
    def scene(seed):
        s = scenes.soup_scene(n_tri=30, width=53, height=37, seed=seed, textured_ratio=0.4, flat=False, texture_size=16)
        s.depths = s.depths + 0.05 * np.random.RandomState(seed).rand(s.depths.shape[0]) + 0.2
        return s

    compare_backward(oracle_api, scene(5), 1.0, dt)
    compare_fit_step(oracle_api, scene(6), 1.5, dt)
    views = [scene(7) for _ in range(3)]
    for i, v in enumerate(views):  # same topology / texture, different vertex positions and colours
        rs = np.random.RandomState(70 + i)
        v.ij = v.ij + rs.randn(*v.ij.shape)
        v.colors = rs.rand(*v.colors.shape) * (v.colors != 0)
    compare_fit_step(oracle_api, views, 1.0, dt)
