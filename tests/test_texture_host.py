"""CPU checks of texture estimation above the kernels: the torch formulation of the two formulas (what runs on tensors the library does not take)
against NumPy restatements, the texture / uv inputs of the autograd functions through a checker-backed stand-in of the rasterizer
(tests/cpu_raster_texture.py, the REPAIRED reference's texture_b / uv_b), and MeshTextureFitterMultiFrame against a loop written out here."""

import numpy as np
import pytest
import torch

import cpu_raster_texture as crt

SHAPES = [(2, 2, 1), (2, 2, 3), (5, 7, 3), (7, 5, 1), (6, 9, 4), (16, 11, 3), (3, 2, 5)]  # Wt * C odd, the smallest texture, rows shorter than a vector


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("shape", SHAPES)
def test_torch_smoothness_equals_the_numpy_restatement_and_autograd(shape):
    from deodr_amd.mesh_fitter import texture_smoothness_torch

    rs = np.random.RandomState(sum(shape))
    t, g0, weight = rs.rand(*shape), rs.randn(*shape), 0.37
    e_np, g_np = crt.np_smoothness(t, weight)
    gradient = torch.as_tensor(g0.copy())
    energy = texture_smoothness_torch(torch.as_tensor(t), gradient, weight)
    assert abs(float(energy) - e_np) <= 1e-14 * abs(e_np)
    assert rel(gradient.numpy(), g0 + g_np) <= 1e-14  # accumulated into, not overwritten
    # the gradient is that of the energy expression (exact algebra: 1e-12 of the largest entry)
    leaf = torch.as_tensor(t).requires_grad_(True)
    e = 0.5 * weight * (((leaf[:, 1:] - leaf[:, :-1]) ** 2).sum() + ((leaf[1:] - leaf[:-1]) ** 2).sum())
    (g_auto,) = torch.autograd.grad(e, leaf)
    assert rel(g_np, g_auto.numpy()) <= 1e-12 and abs(float(e.detach()) - e_np) <= 1e-14 * abs(e_np)
    # float32 storage: float64 arithmetic, one rounding
    g32 = torch.as_tensor(g0.astype(np.float32))
    t32 = t.astype(np.float32)
    energy32 = texture_smoothness_torch(torch.as_tensor(t32), g32, weight)
    e32_np, g32_np = crt.np_smoothness(t32, weight)
    assert torch.equal(g32, torch.as_tensor((g0.astype(np.float32).astype(np.float64) + g32_np).astype(np.float32)))
    assert abs(float(energy32) - e32_np) <= 1e-14 * abs(e32_np)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_torch_step_equals_the_formula_with_clamp_and_zeroed_speed_at_the_wall(dtype):
    from deodr_amd.mesh_fitter import texture_step_torch

    rs = np.random.RandomState(3)
    shape = (5, 7, 3)
    t0, s0, g = rs.rand(*shape).astype(dtype), (0.05 * rs.randn(*shape)).astype(dtype), (3 * rs.randn(*shape)).astype(dtype)
    for kwargs in (dict(), dict(step_max=0.1), dict(inertia=0.9, damping=0.05), dict(inertia=0.8, damping=0.1, step_max=0.2, clamp=(0.0, 1.0)),
                   dict(clamp=(0.25, 0.75))):  # fmt: skip
        t, s = torch.as_tensor(t0.copy()), torch.as_tensor(s0.copy())
        texture_step_torch(t, s, torch.as_tensor(g), 0.3, **kwargs)
        # the formula, written out
        step = -0.3 * g.astype(np.float64)
        if kwargs.get("step_max"):
            step = np.clip(step, -kwargs["step_max"], kwargs["step_max"])
        s_new = (1 - kwargs.get("damping", 0.0)) * (kwargs.get("inertia", 0.0) * s0.astype(np.float64) + (1 - kwargs.get("inertia", 0.0)) * step)
        t_new = t0.astype(np.float64) + s_new
        if "clamp" in kwargs:
            lo, hi = kwargs["clamp"]
            wall = (t_new < lo) | (t_new > hi)
            assert wall.any() and not wall.all()
            t_new, s_new = np.clip(t_new, lo, hi), np.where(wall, 0.0, s_new)
            assert float(t.min()) >= lo and float(t.max()) <= hi
            assert (s.numpy()[wall] == 0).all() and (s.numpy()[~wall] != 0).all()  # the momentum does not keep pushing into the wall
        assert np.array_equal(t.numpy(), t_new.astype(dtype)) and np.array_equal(s.numpy(), s_new.astype(dtype)), kwargs
        t_ref, s_ref = crt.np_step(t0, s0, g, 0.3, **kwargs)
        assert np.array_equal(t_ref, t_new) and np.array_equal(s_ref, s_new)  # (the harness's restatement, used by the GPU tests, says the same)


def _small():
    return crt.sphere_views(n_views=2, size=48, texture_size=12, nu=14, n_rings=10)


def _scene3d(v, texture, uv=None):
    from deodr_amd.scene3d import DeviceCamera, DeviceMesh, Scene3DDevice

    mesh = DeviceMesh(v["faces"], v["vertices"], clockwise=v["clockwise"], uv=v["uv"] if uv is None else uv, faces_uv=v["faces"], texture=texture, device="cpu")
    scene = Scene3DDevice(pixel_dtype=torch.float64)
    scene.set_mesh(mesh)
    scene.set_light(v["light"], v["ambient"])
    scene.set_background_color(v["background"])
    return scene, mesh, DeviceCamera.stack(v["cameras"], "cpu")


def test_texture_and_uv_gradients_through_scene3d_render():
    v = _small()
    scene, mesh, camera = _scene3d(v, v["texture"])
    rs = np.random.RandomState(5)
    with crt.emulate() as calls:
        # no requires_grad: the rasterizer entry receives no extra argument
        image0 = scene.render(camera)
        assert calls[-1] == dict(entry="_rasterize", given=[])
        mesh.texture.requires_grad_()
        image = scene.render(camera)
        assert calls[-1] == dict(entry="_rasterize", given=["texture"])
        assert torch.equal(image.detach(), image0)
        image_b = rs.randn(*image.shape)
        image.backward(torch.as_tensor(image_b))
        # = the checker's texture_b of the same 2.5-D scenes, summed over the views
        s2d = crt.view_scenes(scene.last, v["faces"], v["uv"], v["texture"], 48, 48, v["background"], v["clockwise"])
        expected = np.zeros(v["texture"].shape)
        for i, s in enumerate(s2d):
            im, z = crt.checker().render(s, scene.sigma)
            assert np.array_equal(im, image0[i].numpy())
            expected += crt.checker().grads(s, scene.sigma, im, z, image_b[i])["texture_b"]
        assert np.abs(expected).max() > 0 and rel(mesh.texture.grad.numpy(), expected) <= 1e-14
        # the image is linear in the texture: <render(T + E) - render(T), image_b> = <texture_b, E>
        direction = rs.randn(*v["texture"].shape)
        with torch.no_grad():
            mesh.texture += torch.as_tensor(direction)  # in place: the next render reads the new value
        moved = scene.render(camera).detach().numpy()
        lhs, rhs = float(np.sum((moved - image0.numpy()) * image_b)), float(np.sum(expected * direction))
        assert abs(lhs - rhs) <= 1e-10 * abs(rhs)
        # uv as well
        mesh.uv.requires_grad_()
        mesh.texture.grad = None
        image = scene.render(camera)
        assert calls[-1] == dict(entry="_rasterize", given=["texture", "uv"])
        image.backward(torch.as_tensor(image_b))
        assert mesh.uv.grad is not None and tuple(mesh.uv.grad.shape) == tuple(mesh.uv.shape) and float(mesh.uv.grad.abs().max()) > 0
        expected_uv = np.zeros(v["uv"].shape)
        for i, s in enumerate(crt.view_scenes(scene.last, v["faces"], v["uv"], mesh.texture.detach().numpy(), 48, 48, v["background"], v["clockwise"])):
            im, z = crt.checker().render(s, scene.sigma)
            expected_uv += crt.checker().grads(s, scene.sigma, im, z, image_b[i])["uv_b"]
        assert rel(mesh.uv.grad.numpy(), expected_uv) <= 1e-14


def test_render_l2_passes_texture_weights_and_nothing_else():
    v = _small()
    scene, mesh, camera = _scene3d(v, v["texture"])
    obs = torch.as_tensor(np.random.RandomState(2).rand(2, 48, 48, 3))
    weights = torch.as_tensor(np.random.RandomState(3).rand(2, 48, 48))
    with crt.emulate() as calls:
        scene.render_l2(camera, obs)
        assert calls[-1] == dict(entry="_rasterize_l2", given=[], weights=False)
        mesh.texture.requires_grad_()
        loss, image = scene.render_l2(camera, obs, weights=weights)
        assert calls[-1] == dict(entry="_rasterize_l2", given=["texture"], weights=True)
        loss.backward()
        s2d = crt.view_scenes(scene.last, v["faces"], v["uv"], v["texture"], 48, 48, v["background"], v["clockwise"])
        loss_np, texture_b, _ = crt.oracle_gradient(s2d, v["texture"], obs.numpy(), weights.numpy(), scene.sigma)
        assert abs(float(loss.detach()) - loss_np) <= 1e-12 * loss_np and rel(mesh.texture.grad.numpy(), texture_b) <= 1e-12


def test_a_stand_in_that_does_not_know_the_new_inputs_fails():
    """the differentiated texture travels as a keyword argument passed only when given: the older harness, which knows none, must fail, not ignore it"""
    import cpu_raster
    from oracle import api

    v = _small()
    scene, mesh, camera = _scene3d(v, v["texture"])
    with cpu_raster.emulate(api.port()):
        scene.render(camera)  # nothing requires grad: the call of always
        mesh.texture.requires_grad_()
        with pytest.raises(TypeError, match="texture"):
            scene.render(camera)


@pytest.mark.parametrize("masked", [False, True])
def test_texture_fitter_on_cpu_follows_the_loop_written_out(masked):
    from deodr_amd.pytorch import MeshTextureFitterMultiFrame

    v = _small()
    n, size = 2, 48
    grey = np.full(v["texture"].shape, 0.5)
    params = dict(smoothness=0.2, inertia=0.9, damping=0.05, clamp=(0.0, 1.0))
    fitter = MeshTextureFitterMultiFrame(v["vertices"], v["faces"], v["uv"], v["faces"], grey, v["light"], v["ambient"], cameras=v["cameras"],
                                         clockwise=v["clockwise"], device="cpu", pixel_dtype=torch.float64, **params)  # fmt: skip
    fitter.set_background_color(v["background"])
    # the observations: the ground-truth texture through the checker, on the views as the fitter itself projects them
    weights = None
    if masked:
        weights = np.ones((n, size, size))
        weights[1, :, : size // 2] = 0.0
    with crt.emulate() as calls:
        fitter.set_images(np.zeros((n, size, size, 3)), weights=weights)
        s2d = crt.view_scenes(fitter._views, v["faces"], v["uv"], v["texture"], size, size, v["background"], v["clockwise"])
        obs = np.stack([crt.checker().render(s, 1.0)[0] for s in s2d])
        fitter.set_images(obs, weights=weights)
        energies = [fitter.step()[0] for _ in range(10)]
        assert calls[-1] == dict(entry="_rasterize_l2", given=["texture"], weights=masked) and fitter.iter == 10
    expected, _trajectory, final = crt.oracle_fit(s2d, grey, obs, weights, 1.0, 10, params["smoothness"], fitter.step_factor_texture, None,
                                                  params["inertia"], params["damping"], params["clamp"])  # fmt: skip
    assert np.abs(np.array(energies) - expected).max() <= 1e-12 * expected[0]
    assert rel(fitter.texture.numpy(), final) <= 1e-12
    assert energies[-1] < energies[0]
