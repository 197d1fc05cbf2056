"""CPU checks of the ``pyramid_levels=`` / ``pyramid_weights=`` keywords of the colour fitters and of the camera fitter on the checker-backed rasterizer
of tests/cpu_raster.py: 0 levels change nothing, the first step's energy and vertex gradient are those of the torch formulas, the refusals, the
per-pixel weights reach the term, and a colour fit of the hand from a start shifted by a few pixels."""

import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

SIZE = 64


def hand_fitter(views, device, pixel_dtype=torch.float64, shift_pixels=(0.0, 0.0), weights=None, size=SIZE, **keywords):
    """the hand at ``size`` x ``size`` (64 x 64) under ``views`` views (1: MeshRGBFitterWithPose): the target is the fitter's own rendering at the initial pose, the start that
    pose translated by ``shift_pixels`` (x, y) in the image"""
    from deodr_amd import scenes
    from deodr_amd.mesh_fitter import MeshRGBFitterWithPose, MeshRGBFitterWithPoseMultiFrame

    d = np.load(os.path.join(GOLDEN, "rgb_hand_fit.npz"))
    _, faces = scenes.load_hand_mesh(os.path.join(GOLDEN, "hand_mesh.npz"))
    args = (d["default_color"], d["default_light_directional"], float(d["default_light_ambient"]))
    common = dict(cregu=1000, device=device, pixel_dtype=pixel_dtype, **keywords)
    if views == 1:
        f = MeshRGBFitterWithPose(d["vertices_centered"], faces, np.zeros(3), d["translation_init"], *args, **common)
    else:
        eulers = np.array([[0.0, 0.5 * v, 0.0] for v in range(views)])
        f = MeshRGBFitterWithPoseMultiFrame(d["vertices_centered"], faces, eulers, np.tile(d["translation_init"], (views, 1)), *args, **common)
    f.set_background_color(d["background_color"])
    set_images = (lambda images, **kw: f.set_image(images[0], **kw)) if views == 1 else (lambda images, **kw: f.set_images(list(images), **kw))
    set_images(np.zeros((views, size, size, 3)))
    target = f.render().cpu().numpy()
    assert target.shape == (views, size, size, 3) and target.std() > 0.01
    f.reset()
    set_images(target, **({} if weights is None else dict(weights=weights[0] if views == 1 else weights)))
    # the camera looks down -z from 9 (one view) or 6 (several) radii with a focal length of 2 * size pixels
    per_pixel = (9 if views == 1 else 6) * f.object_radius / (2 * size)
    move = np.array([shift_pixels[0], -shift_pixels[1], 0.0]) * per_pixel
    f.transform_translation_init = f.transform_translation_init + torch.as_tensor(move, device=f.device)
    f.reset()
    return f


def camera_fitter(**keywords):
    import camera_reference as cr

    problem = cr.calibration_problem(2, 48, ("extrinsic", "focal"), arc=np.pi)
    photos = cr.photographs(problem, "cpu")
    fitter = cr.make_camera_fitter(problem, problem["start"], ("extrinsic", "focal"), "cpu", **keywords)
    fitter.set_images(photos)
    return fitter


PARAMETERS = ("vertices", "transform_quaternion", "transform_translation", "mesh_color", "light_directional", "light_ambient", "quaternions", "translations", "focal")


def test_zero_levels_and_no_keyword_are_the_same_fit(oracle_api):
    import cpu_raster

    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        for make in (lambda **kw: hand_fitter(1, "cpu", shift_pixels=(2, 1), **kw), lambda **kw: hand_fitter(2, "cpu", shift_pixels=(2, 1), **kw), camera_fitter):
            plain, zero = make(), make(pyramid_levels=0, pyramid_weights=None)
            assert zero.pyramid_levels == 0 and zero.pyramid_weights is None
            assert [plain.step()[0] for _ in range(5)] == [zero.step()[0] for _ in range(5)]
            compared = [k for k in PARAMETERS if torch.is_tensor(getattr(plain, k, None))]
            assert len(compared) >= 3 and all(torch.equal(getattr(plain, k), getattr(zero, k)) for k in compared)
            assert set(plain.momentum.speed) == set(zero.momentum.speed)


@pytest.mark.parametrize("views", [1, 2])
def test_first_step_is_the_torch_formulas(oracle_api, views):
    """energy = data_weight * pyramid_l2_torch(rendered, obs) + the rigid energy, and the vertex gradient the update gets is autograd's through them"""
    import cpu_raster
    from deodr_amd.pyramid import pyramid_l2_torch

    lam = [0.5, 1.0, 2.0, 0.25]
    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        f = hand_fitter(views, "cpu", shift_pixels=(3, -2), pyramid_levels=3, pyramid_weights=lam)
        assert f._direct_iteration(3, True) is None and f.pyramid_weights.dtype == torch.float64 and f.pyramid_weights.tolist() == lam
        # by hand, at the parameters of the first step
        leaves = f._leaves(f._appearance_leaves())
        f._pose_scene()
        image = f.scene.render(f.camera)
        expected = f.data_weight * pyramid_l2_torch(image, f.mesh_image, None, 3, torch.as_tensor(lam))
        g_vertices = torch.autograd.grad(expected, leaves[0])[0]
        e_rigid, _ = f.rigid_energy.evaluate(f.vertices.detach())
        seen = {}
        update_all = f.momentum.update_all
        f.momentum.update_all = lambda entries: seen.update({e[0]: e[2].clone() for e in entries}) or update_all(entries)
        energy, image_step, diff = f.step()
        # (equal up to the order of the additions inside torch's sums, which depends on how it splits them over its threads)
        assert energy == pytest.approx(float(expected.detach() + e_rigid), rel=1e-13, abs=0)
        pick = (lambda a: a) if views > 1 else (lambda a: a[0])
        print("largest difference of the step's image:", np.abs(image_step - pick(image.detach().numpy())).max())
        assert np.allclose(image_step, pick(image.detach().numpy()), rtol=0, atol=1e-12)  # (the leaves are re-centred at every call: not the same bits)
        assert np.allclose(diff, pick(((image.detach() - f.mesh_image) ** 2).sum(dim=-1).numpy()), rtol=0, atol=1e-12)  # unchanged in meaning
        # (the update gets the gradient projected on zero-mean displacements, as without the keyword)
        assert float(g_vertices.abs().max()) > 0
        assert torch.allclose(seen["vertices"], g_vertices - g_vertices.mean(dim=0, keepdim=True), rtol=0, atol=1e-12 * float(g_vertices.abs().max()))
        assert float(expected.detach()) > 0


def test_camera_fitter_takes_the_term(oracle_api):
    import cpu_raster
    from deodr_amd.pyramid import pyramid_l2_torch

    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        plain, f = camera_fitter(), camera_fitter(pyramid_levels=2, pyramid_weights=[1.0, 0.5, 0.25])
        assert f._direct is None and f.pyramid_levels == 2
        _grads, image = plain.gradients()
        expected = pyramid_l2_torch(image, f._obs, None, 2, f.pyramid_weights)
        energies = [f.step()[0] for _ in range(5)]
        assert energies[0] == pytest.approx(float(expected), rel=1e-13, abs=0) and energies[0] > float(plain.energy())  # term_0 is the plain energy
        assert energies[-1] < energies[0] and f.iter == 5


def test_refusals():
    import camera_reference as cr
    from deodr_amd import scenes
    from deodr_amd.mesh_fitter import MeshRGBFitterWithPose, MeshRGBFitterWithPoseMultiFrame

    d = np.load(os.path.join(GOLDEN, "rgb_hand_fit.npz"))
    _, faces = scenes.load_hand_mesh(os.path.join(GOLDEN, "hand_mesh.npz"))
    args = (d["vertices_centered"], faces, np.zeros(3), d["translation_init"], d["default_color"], d["default_light_directional"], float(d["default_light_ambient"]))
    problem = cr.calibration_problem(2, 48, ("extrinsic",), arc=np.pi)
    makers = [lambda **kw: MeshRGBFitterWithPose(*args, device="cpu", **kw), lambda **kw: MeshRGBFitterWithPoseMultiFrame(*args, device="cpu", **kw),
              lambda **kw: cr.make_camera_fitter(problem, problem["start"], ("extrinsic",), "cpu", **kw)]  # fmt: skip
    for make in makers:
        for levels in (-1, 9, 2.5):
            with pytest.raises(ValueError, match="pyramid_levels must be an integer in 0 .. 8"):
                make(pyramid_levels=levels)
        for bad in ([1.0, 1.0, 1.0], [1.0] * 5, [[1.0] * 4]):
            with pytest.raises(ValueError, match="pyramid_weights must have pyramid_levels \\+ 1 = 4 entries"):
                make(pyramid_levels=3, pyramid_weights=bad)
        for bad in ([1.0, -0.5, 1.0, 1.0], [1.0, np.nan, 1.0, 1.0]):
            with pytest.raises(ValueError, match="pyramid_weights must be >= 0"):
                make(pyramid_levels=3, pyramid_weights=bad)
        with pytest.raises(ValueError, match="pyramid_weights needs pyramid_levels > 0"):
            make(pyramid_weights=[1.0])
        assert make(pyramid_levels=8).pyramid_weights.tolist() == [1.0] * 9  # the default: all ones


def test_pixel_weights_reach_the_term(oracle_api):
    import cpu_raster
    from deodr_amd.pyramid import pyramid_l2_torch

    rs = np.random.RandomState(5)
    w = 0.25 + rs.rand(2, SIZE, SIZE)
    w[:, 24:40, 16:48] = 0
    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        for views in (1, 2):
            f = hand_fitter(views, "cpu", shift_pixels=(3, 0), weights=w[:views], pyramid_levels=2)
            unweighted = hand_fitter(views, "cpu", shift_pixels=(3, 0), pyramid_levels=2)
            f._leaves(f._appearance_leaves())
            f._pose_scene()
            image = f.scene.render(f.camera).detach()
            expected = f.data_weight * pyramid_l2_torch(image, f.mesh_image, torch.as_tensor(w[:views]), 2, torch.ones(3, dtype=torch.float64))
            e_rigid, _ = f.rigid_energy.evaluate(f.vertices.detach())
            energy = f.step()[0]
            assert energy == pytest.approx(float(expected + e_rigid), rel=1e-13, abs=0) and abs(energy - unweighted.step()[0]) > 1e-3 * energy


def shifted_fit(oracle_api, levels, iterations=40, **keywords):
    import cpu_raster

    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        f = hand_fitter(1, "cpu", shift_pixels=(4, 3), pyramid_levels=levels, **keywords)
        start = f.transform_translation.clone()
        energies = [f.step()[0] for _ in range(iterations)]
        # how far the start is from the pose the target was rendered at, and how much of that the fit has undone
        d = np.load(os.path.join(GOLDEN, "rgb_hand_fit.npz"))
        truth = torch.as_tensor(np.atleast_2d(d["translation_init"]))
        moved = float((start - truth).norm()), float((f.transform_translation - truth).norm())
    return energies, moved


def test_shifted_colour_fit_lowers_its_energy(oracle_api):
    """The 64 x 64 colour fit of the hand from a start 4 pixels right and 3 pixels down of the pose its target was rendered at, ``pyramid_levels=3``, all
    level weights 1, 40 iterations.  Measured on the checker: energy every 5 iterations 455.144, 278.696, 160.113, 125.870, 67.635, 54.675, 19.978,
    20.446, then 15.352 after the last: a fraction of 0.0337; distance to the true translation 0.1909 -> 0.0182.  The bound is twice the measured
    fraction.  The same fit with ``pyramid_levels=0`` (printed, not asserted): energy 182.986 -> 12.144, a fraction of 0.0664, distance 0.1909 ->
    0.0216."""
    energies, moved = shifted_fit(oracle_api, 3)
    plain, moved_plain = shifted_fit(oracle_api, 0)
    curve = ", ".join(f"{e:.3f}" for e in energies[::5] + energies[-1:])
    print(f"pyramid_levels=3: energy every 5 iterations {curve}; fraction {energies[-1] / energies[0]:.4f}; distance to the true translation {moved[0]:.4f} -> {moved[1]:.4f}")
    print(f"pyramid_levels=0: energy {plain[0]:.3f} -> {plain[-1]:.3f}, fraction {plain[-1] / plain[0]:.4f}; distance {moved_plain[0]:.4f} -> {moved_plain[1]:.4f}")
    assert energies[-1] < MEASURED_BOUND * energies[0]
    assert moved[1] < moved[0]


MEASURED_BOUND = 0.07  # twice the measured fraction of 0.0337, rounded up
