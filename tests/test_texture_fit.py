"""GPU tests of texture estimation: the two kernels of include/deodr_hip_texture.h against NumPy restatements, texture / uv gradients through
autograd against the rasterizer's own adjoint and the repaired oracle, MeshTextureFitterMultiFrame in lock-step with an oracle-driven loop, masks,
and the iteration replayed as a HIP graph."""

import numpy as np
import pytest
import torch

import cpu_raster_texture as crt

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64

# Ht, Wt (every one with C = 1, 3, 4): the smallest texture, rows shorter than / not a multiple of a 16-byte vector, a row length not divisible by 4
# (37 C is odd for C = 1, 3), the sizes of a real texture
SIZES = [(2, 2), (5, 7), (33, 37), (64, 64), (1024, 1024)]


def repaired(oracle_api):
    return oracle_api.ref(fixed=True) or oracle_api.port(fixed=True)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def close_in_storage(got, expected64, dtype, what):
    """float64 buffers: within 1e-14 of the largest entry; float32 buffers: within one float32 ulp of the double result rounded to float32"""
    got = got.cpu().numpy()
    if dtype == F64:
        err = np.abs(got - expected64).max() / np.abs(expected64).max()
        print(f"{what}: float64, max error / largest entry = {err:.3e}")
        assert err <= 1e-14, what
    else:
        rounded = expected64.astype(np.float32)
        ulps = np.abs(got.astype(np.float64) - rounded.astype(np.float64)) / np.spacing(np.abs(rounded)).astype(np.float64)
        print(f"{what}: float32, max distance = {ulps.max():.2f} ulp, {int((ulps > 0).sum())} of {ulps.size} values differ")
        assert ulps.max() <= 1.0, what


def on_device(a, dtype, misalign=False):
    """a contiguous device tensor holding `a`; misalign: a slice of a larger buffer that starts one element behind a 16-byte boundary"""
    t = torch.as_tensor(a).to(dtype)
    if not misalign:
        return t.cuda().contiguous()
    buffer = torch.empty(t.numel() + 8, dtype=dtype, device="cuda")
    assert buffer.data_ptr() % 16 == 0
    out = buffer[1 : 1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == out.element_size()
    return out


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_kernels_against_the_numpy_restatement(dtype, C, misalign):
    from deodr_amd import hip_renderer as hr

    np_dtype = np.float32 if dtype == F32 else np.float64
    for Ht, Wt in SIZES:
        if misalign and Ht == 1024:
            continue  # (the misaligned rows are covered by the smaller sizes)
        rs = np.random.RandomState(Ht * 131 + Wt * 7 + C)
        t0, g0 = rs.rand(Ht, Wt, C).astype(np_dtype), rs.randn(Ht, Wt, C).astype(np_dtype)
        s0 = (0.05 * rs.randn(Ht, Wt, C)).astype(np_dtype)
        # two texels that meet the walls of every clamp below whatever the size: at rest on 0 and on 1, pushed outwards
        t0.reshape(-1)[:2], s0.reshape(-1)[:2], g0.reshape(-1)[:2] = (0.0, 1.0), (0.0, 0.0), (5.0, -5.0)
        weight = 0.37
        what = f"{Ht}x{Wt}x{C}{' misaligned' if misalign else ''}"
        # ---- smoothness: accumulated into the gradient, deterministic energy, texture untouched
        e_np, g_np = crt.np_smoothness(t0, weight)
        runs = []
        for _ in range(2):
            texture, gradient = on_device(t0, dtype, misalign), on_device(g0, dtype, misalign)
            energy = hr.texture_smoothness(texture, gradient, weight)
            torch.cuda.synchronize()
            runs.append((gradient.clone(), energy.clone()))
            assert np.array_equal(texture.cpu().numpy(), t0)  # read-only
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), what  # bit-identical, energy included
        close_in_storage(runs[0][0], g0.astype(np.float64) + g_np, dtype, f"smoothness gradient {what}")
        e_err = abs(float(runs[0][1]) - e_np) / e_np
        print(f"smoothness energy {what}: relative error {e_err:.3e}")
        assert e_err <= 1e-12, what
        zero = on_device(np.zeros_like(g0), dtype, misalign)
        hr.texture_smoothness(texture, zero, weight)
        assert not torch.equal(zero, runs[0][0])  # (accumulated into, not overwritten: g0 is in the first result)
        # ---- step, with and without the clamp
        for kwargs in (dict(inertia=0.9, damping=0.05, step_max=0.2, clamp=(0.0, 1.0)), dict(inertia=0.5), dict(clamp=(0.25, 0.75))):
            results = []
            for _ in range(2):
                texture, speed, gradient = on_device(t0, dtype, misalign), on_device(s0, dtype, misalign), on_device(g0, dtype, misalign)
                hr.texture_step(texture, speed, gradient, 0.3, **kwargs)
                torch.cuda.synchronize()
                results.append((texture.clone(), speed.clone()))
                assert np.array_equal(gradient.cpu().numpy(), g0)  # only read
            assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
            t_np, s_np = crt.np_step(t0, s0, g0, 0.3, **kwargs)
            close_in_storage(results[0][0], t_np, dtype, f"step texture {what} {sorted(kwargs)}")
            if dtype == F64:
                close_in_storage(results[0][1], s_np, dtype, f"step speed {what} {sorted(kwargs)}")
            else:  # (a speed that is exactly 0 at the wall has no ulp to be measured in)
                got, want = results[0][1].cpu().numpy(), s_np.astype(np.float32)
                assert np.array_equal(got == 0, want == 0)
                close_in_storage(results[0][1][results[0][1] != 0], s_np[want != 0], dtype, f"step speed {what} {sorted(kwargs)}")
            if "clamp" in kwargs:
                lo, hi = kwargs["clamp"]
                got_t, got_s = results[0][0].cpu().numpy(), results[0][1].cpu().numpy()
                assert got_t.min() >= lo and got_t.max() <= hi
                wall = s_np == 0  # (where the restatement clipped: no other speed is exactly 0)
                assert wall.reshape(-1)[:2].all() and (got_s[wall] == 0).all() and (got_s[~wall] != 0).all()
                assert np.isin(got_t[wall], (np_dtype(lo), np_dtype(hi))).all()


def test_host_wrappers_refuse_what_the_library_would_misread():
    from deodr_amd import hip_renderer as hr

    t = torch.zeros(8, 8, 3, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        hr.texture_smoothness(t, torch.zeros(8, 3, 8, device="cuda").permute(0, 2, 1), 1.0)
    with pytest.raises(ValueError, match="shape, dtype and device"):
        hr.texture_smoothness(t, torch.zeros(8, 8, 3, device="cuda", dtype=F64), 1.0)
    with pytest.raises(ValueError, match="shape, dtype and device"):
        hr.texture_step(t, torch.zeros(8, 8, 4, device="cuda"), torch.zeros_like(t), 0.1)
    with pytest.raises(ValueError, match="shape"):
        hr.texture_smoothness(torch.zeros(1, 8, 3, device="cuda"), torch.zeros(1, 8, 3, device="cuda"), 1.0)
    with pytest.raises(RuntimeError, match="gradient must not overlap texture"):
        hr.texture_smoothness(t, t, 1.0)


# ---- autograd ----------------------------------------------------------------------------------------------------------------------


def _scene3d(v, pixel_dtype, n_views):
    from deodr_amd.scene3d import DeviceCamera, DeviceMesh, Scene3DDevice

    mesh = DeviceMesh(v["faces"], v["vertices"], clockwise=v["clockwise"], uv=v["uv"], faces_uv=v["faces"], texture=v["texture"], device="cuda")
    scene = Scene3DDevice(pixel_dtype=pixel_dtype)
    scene.set_mesh(mesh)
    scene.set_light(v["light"], v["ambient"])
    scene.set_background_color(v["background"])
    return scene, mesh, DeviceCamera.stack(v["cameras"][:n_views], "cuda")


@pytest.fixture(scope="module")
def views():
    return crt.sphere_views(n_views=4, size=128, texture_size=64, nu=60, n_rings=40)


@pytest.mark.parametrize("n_views", [1, 4])
@pytest.mark.parametrize("pixel_dtype", [F32, F64])
def test_texture_and_uv_gradients_through_autograd(oracle_api, views, pixel_dtype, n_views):
    from deodr_amd import hip_renderer as hr

    v, size = views, views["size"]
    rs = np.random.RandomState(11)
    image_b = torch.as_tensor(rs.randn(n_views, size, size, 3), device="cuda").to(pixel_dtype)
    obs = torch.as_tensor(rs.rand(n_views, size, size, 3), device="cuda").to(pixel_dtype)
    tol = 1e-4 if pixel_dtype == F32 else 1e-8
    # ---- against the repaired oracle, on the floating-point path
    scene, mesh, camera = _scene3d(v, pixel_dtype, n_views)
    mesh.texture.requires_grad_()
    mesh.uv.requires_grad_()
    image = scene.render(camera)
    image.backward(image_b)
    s2d = crt.view_scenes(scene.last, v["faces"], v["uv"], v["texture"], size, size, v["background"], v["clockwise"])
    ref = repaired(oracle_api)
    texture_b, uv_b = np.zeros(v["texture"].shape), np.zeros(v["uv"].shape)
    for i, s in enumerate(s2d):
        im, z = ref.render(s, scene.sigma)
        g = ref.grads(s, scene.sigma, im, z, image_b[i].cpu().numpy().astype(np.float64))
        texture_b, uv_b = texture_b + g["texture_b"], uv_b + g["uv_b"]
    assert mesh.texture.grad.dtype == mesh.texture.dtype and mesh.uv.grad.dtype == mesh.uv.dtype
    errs = rel(mesh.texture.grad.cpu().numpy(), texture_b), rel(mesh.uv.grad.cpu().numpy(), uv_b)
    print(f"render, {n_views} views, {pixel_dtype}: texture_b {errs[0]:.3e}, uv_b {errs[1]:.3e} against the repaired oracle")
    assert np.abs(texture_b).max() > 0 and np.abs(uv_b).max() > 0 and max(errs) < tol
    mesh.texture.grad = mesh.uv.grad = None
    loss, _image = scene.render_l2(camera, obs)
    loss.backward()
    loss_np, texture_b, _ = crt.oracle_gradient(s2d, v["texture"], obs.cpu().numpy().astype(np.float64), None, scene.sigma, ref)
    errs = abs(float(loss.detach()) - loss_np) / loss_np, rel(mesh.texture.grad.cpu().numpy(), texture_b)
    print(f"render_l2, {n_views} views, {pixel_dtype}: loss {errs[0]:.3e}, texture_b {errs[1]:.3e} against the repaired oracle")
    assert max(errs) < tol and float(mesh.uv.grad.abs().max()) > 0
    # ---- bit for bit the rasterizer's own texture_b / uv_b, in the deterministic mode
    hr.set_deterministic(True)
    try:
        scene, mesh, camera = _scene3d(v, pixel_dtype, n_views)
        mesh.texture.requires_grad_()
        mesh.uv.requires_grad_()
        scene.render(camera).backward(image_b)
        _key, ds, r = scene._state
        r.render(ds, scene.sigma)
        own = r.render_backward(ds, image_b=image_b)
        assert torch.equal(mesh.texture.grad, own["texture_b"].to(mesh.texture.dtype)) and torch.equal(mesh.uv.grad, own["uv_b"].to(mesh.uv.dtype))
        mesh.texture.grad = mesh.uv.grad = None
        loss, _image = scene.render_l2(camera, obs)
        (3.0 * loss).backward()  # (loss_b scales the gradients the forward left)
        r.render(ds, scene.sigma)
        own = r.render_backward(ds, residual_obs=obs)
        d_t = float((mesh.texture.grad - 3.0 * own["texture_b"].to(mesh.texture.dtype)).abs().max())
        d_uv = float((mesh.uv.grad - 3.0 * own["uv_b"].to(mesh.uv.dtype)).abs().max())
        print(f"render_l2 deterministic, {n_views} views, {pixel_dtype}: max difference to render_backward texture_b {d_t:.3e}, uv_b {d_uv:.3e}")
        assert torch.equal(mesh.texture.grad, 3.0 * own["texture_b"].to(mesh.texture.dtype)) and torch.equal(mesh.uv.grad, 3.0 * own["uv_b"].to(mesh.uv.dtype))
    finally:
        hr.set_deterministic(False)


@pytest.mark.parametrize("pixel_dtype", [F32, F64])
def test_an_in_place_edit_of_the_texture_is_rendered(views, pixel_dtype):
    """the stale copy: DeviceScene.texture used to be a conversion made once (mesh.texture is float64; with float32 pixels the scene holds a copy)"""
    scene, mesh, camera = _scene3d(views, pixel_dtype, 2)
    first = scene.render(camera).clone()
    state = scene._state
    with torch.no_grad():
        mesh.texture.mul_(0.5)
    second = scene.render(camera).clone()
    assert scene._state is state  # (no rebuild of the scene)
    assert not torch.equal(first, second)
    mesh.texture = (2.0 * mesh.texture).detach()  # a rebound tensor of the same shape: the same scene again, the first image again
    third = scene.render(camera)
    assert scene._state is state and torch.equal(third, first)


# ---- the fitter --------------------------------------------------------------------------------------------------------------------

PARAMS = dict(smoothness=0.2, inertia=0.9, damping=0.05, clamp=(0.0, 1.0))


def _fitter(v, cameras, pixel_dtype=F64):
    from deodr_amd.pytorch import MeshTextureFitterMultiFrame

    grey = np.full(v["texture"].shape, 0.5)
    f = MeshTextureFitterMultiFrame(v["vertices"], v["faces"], v["uv"], v["faces"], grey, v["light"], v["ambient"], cameras=cameras, clockwise=v["clockwise"],
                                    device="cuda", pixel_dtype=pixel_dtype, **PARAMS)  # fmt: skip
    f.set_background_color(v["background"])
    return f, grey


@pytest.fixture(scope="module")
def fit_problem(oracle_api):
    """sphere_scene(textured=True) at 4 views of 128 x 128, a 64 x 64 texture; the photographs are the ground-truth texture through the repaired oracle"""
    v = crt.sphere_views(n_views=4, size=128, texture_size=64)
    f, _grey = _fitter(v, v["cameras"])
    f.set_images(np.zeros((4, 128, 128, 3)))
    s2d = crt.view_scenes(f._views, v["faces"], v["uv"], v["texture"], 128, 128, v["background"], v["clockwise"])
    ref = repaired(oracle_api)
    obs = np.stack([ref.render(s, 1.0)[0] for s in s2d])
    return v, s2d, obs


def test_texture_fit_20_iterations_lockstep(oracle_api, fit_problem):
    v, s2d, obs = fit_problem
    ref = repaired(oracle_api)
    lock, grey = _fitter(v, v["cameras"])
    free, _ = _fitter(v, v["cameras"])
    lock.set_images(obs)
    free.set_images(obs)
    expected, trajectory, _final = crt.oracle_fit(s2d, grey, obs, None, 1.0, 20, PARAMS["smoothness"], lock.step_factor_texture, None, PARAMS["inertia"],
                                                  PARAMS["damping"], PARAMS["clamp"], ref)  # fmt: skip
    energies_free = []
    for it, (texture_k, texture_b_k) in enumerate(trajectory):
        lock.texture.copy_(torch.as_tensor(texture_k))  # the GPU at the oracle's trajectory
        texture_b, _image = lock._gradient()
        loss = float(lock.e_data + lock.e_smooth)
        e_err, g_err = abs(loss - expected[it]) / expected[it], rel(texture_b.cpu().numpy(), texture_b_k)
        print(f"iteration {it}: loss {loss:.12e} (oracle {expected[it]:.12e}, relative {e_err:.2e}), texture_b {g_err:.2e}")
        assert e_err <= 1e-9 and g_err < 1e-8, it
        energies_free.append(float(free.step_device()[0]))
    final_err = abs(energies_free[-1] - expected[-1]) / expected[-1]
    print(f"free-running: final loss {energies_free[-1]:.12e}, oracle loop {expected[-1]:.12e}, relative {final_err:.2e}; initial {energies_free[0]:.6e}")
    assert final_err <= 1e-6
    assert energies_free[-1] < energies_free[0]


def test_a_view_of_weight_zero_does_not_move_the_texture(fit_problem):
    v, _s2d, obs = fit_problem
    weights = np.ones((4, 128, 128))
    weights[3] = 0.0
    masked, _ = _fitter(v, v["cameras"])
    masked.set_images(obs, weights=weights)
    without, _ = _fitter(v, v["cameras"][:3])
    without.set_images(obs[:3])
    for _ in range(10):
        e_masked, e_without = float(masked.step_device()[0]), float(without.step_device()[0])
        assert abs(e_masked - e_without) <= 1e-9 * e_without
    err = rel(masked.texture.cpu().numpy(), without.texture.cpu().numpy())
    print(f"weights = 0 on one view against a fit without it: textures differ by {err:.3e} of the largest texel")
    assert err < 1e-8


def test_graph_replay_equals_eager_steps(fit_problem):
    from deodr_amd.mesh_fitter import GraphedStep

    v, _s2d, obs = fit_problem
    eager, _ = _fitter(v, v["cameras"])
    graphed, _ = _fitter(v, v["cameras"])
    eager.set_images(obs)
    graphed.set_images(obs)
    step = GraphedStep(graphed)
    before = graphed.iter
    for _ in range(before):  # (capturing took this many eager steps on the other fitter)
        eager.step_device()
    for _ in range(10):
        e_graph = float(step.step_device()[0])
        e_eager = float(eager.step_device()[0])
        assert abs(e_graph - e_eager) <= 1e-9 * e_eager
    assert graphed.iter == before + 10 == eager.iter
    assert rel(graphed.texture.cpu().numpy(), eager.texture.cpu().numpy()) <= 1e-9
    assert rel(graphed.momentum.speed["texture"].cpu().numpy(), eager.momentum.speed["texture"].cpu().numpy()) <= 1e-9
