"""CPU checks of linear bases (deodr_amd/basis.py): the torch formulation of the map and of its adjoint (what runs on tensors the library does not
take, and what the kernels are tested against in tests/test_basis_gpu.py) against NumPy, its derivatives, and the ``shape_basis`` / ``texture_basis``
keywords of the fitters on the checker-backed rasterizers of tests/cpu_raster.py and tests/cpu_raster_texture.py."""

import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

EPS = float(np.finfo(np.float64).eps)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def hand():
    d = np.load(os.path.join(GOLDEN, "hand_mesh.npz"))
    return d["vertices"], d["faces"].astype(np.int64)


def hand_modes(K=4, seed=0):
    """K smooth displacement fields of the hand [K,526,3] with orthonormal rows: low-frequency waves along random directions"""
    vertices, _faces = hand()
    rs = np.random.RandomState(seed)
    centred = (vertices - vertices.mean(axis=0)) / np.abs(vertices - vertices.mean(axis=0)).max()
    fields = [np.sin(centred @ rs.randn(3) * 2.0 + rs.rand() * 6.0)[:, None] * rs.randn(3)[None, :] for _ in range(K)]
    q, _r = np.linalg.qr(np.stack(fields).reshape(K, -1).T)
    return q.T.reshape(K, *vertices.shape).copy()


# ---- the map and its adjoint (torch fallback)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("with_mean", [True, False])
def test_torch_fallback_against_numpy(dtype, with_mean):
    from deodr_amd.basis import LinearBasis

    rs = np.random.RandomState(3)
    K, shape = 5, (7, 3)
    components, mean, c = rs.randn(K, *shape), rs.randn(*shape), rs.randn(4, K)
    basis = LinearBasis(components, mean if with_mean else None, device="cpu", dtype=dtype)
    assert (basis.K, basis.N, basis.shape) == (K, 21, shape) and basis.components.dtype == dtype and basis.components.shape == (K, 21)
    assert not basis.uses_kernel(torch.as_tensor(c))
    stored = components.astype(np.float32 if dtype == torch.float32 else np.float64).astype(np.float64).reshape(K, -1)  # arithmetic is double on the stored tables
    stored_mean = mean.astype(np.float32 if dtype == torch.float32 else np.float64).astype(np.float64).reshape(-1) if with_mean else 0.0
    expected = c @ stored + stored_mean
    y = basis.apply(torch.as_tensor(c))
    assert y.shape == (4, *shape) and y.dtype == torch.float64 and rel(y.numpy().reshape(4, -1), expected) <= 8 * EPS
    one = basis.apply(torch.as_tensor(c[2]))  # [K] -> [*shape]
    assert one.shape == shape and rel(one.numpy().reshape(-1), expected[2]) <= 8 * EPS
    y32 = basis.apply(torch.as_tensor(c), out_dtype=torch.float32)
    assert y32.dtype == torch.float32 and np.array_equal(y32.numpy().reshape(4, -1), (c @ stored + stored_mean).astype(np.float32))
    g = rs.randn(4, *shape)
    c_b = basis.apply_b(torch.as_tensor(g))
    assert c_b.shape == (4, K) and c_b.dtype == torch.float64 and rel(c_b.numpy(), g.reshape(4, -1) @ stored.T) <= 8 * EPS
    assert basis.apply_b(torch.as_tensor(g[1])).shape == (K,)
    with pytest.raises(ValueError, match=r"expected coefficients \[5\] or \[batch, 5\]"):
        basis.apply(torch.zeros(6, dtype=torch.float64))
    with pytest.raises(ValueError, match="mean must have shape"):
        LinearBasis(components, mean[:-1], device="cpu")
    with pytest.raises(ValueError, match="float32 or torch.float64"):
        LinearBasis(components, device="cpu", dtype=torch.float16)


def test_gradcheck_and_gradgradcheck_of_the_torch_fallback():
    from deodr_amd.basis import LinearBasis

    rs = np.random.RandomState(0)
    for mean in (rs.randn(3, 2, 2), None):
        basis = LinearBasis(rs.randn(4, 3, 2, 2), mean, device="cpu", dtype=torch.float64)
        for c in (torch.tensor(rs.randn(4), requires_grad=True), torch.tensor(rs.randn(3, 4), requires_grad=True)):
            assert torch.autograd.gradcheck(basis.apply, (c,))
            assert torch.autograd.gradgradcheck(basis.apply, (c,))
        g = torch.tensor(rs.randn(2, 3, 2, 2), requires_grad=True)
        assert torch.autograd.gradcheck(basis.apply_b, (g,)) and torch.autograd.gradgradcheck(basis.apply_b, (g,))


def test_backward_is_the_transposed_matrix():
    from deodr_amd.basis import LinearBasis

    rs = np.random.RandomState(1)
    components = hand_modes(6)
    basis = LinearBasis(components, hand()[0], device="cpu", dtype=torch.float64)
    c, w = torch.tensor(rs.randn(6), requires_grad=True), torch.tensor(rs.randn(526, 3))
    y = basis.apply(c)
    (c_b,) = torch.autograd.grad(y, c, w, create_graph=True)
    assert rel(c_b.detach().numpy(), components.reshape(6, -1) @ w.numpy().reshape(-1)) <= 1e-14
    # <B^T c, w> = <c, B w> (without the mean), and the backward of the backward is apply again, without the mean
    lhs, rhs = float(((y.detach() - basis.mean.reshape(526, 3)) * w).sum()), float((c.detach() * c_b.detach()).sum())
    assert abs(lhs - rhs) <= 1e-13 * float(y.detach().norm()) * float(w.norm())
    u = torch.tensor(rs.randn(6))
    w2 = w.clone().requires_grad_(True)
    (c_b2,) = torch.autograd.grad(basis.apply(c), c, w2, create_graph=True)
    (w_b,) = torch.autograd.grad(c_b2, w2, u)
    assert rel(w_b.numpy().reshape(-1), u.numpy() @ components.reshape(6, -1)) <= 1e-14


# ---- shape_basis on the pose fitters


def reduced_depth_inputs(factor=4):
    d = np.load(os.path.join(GOLDEN, "depth_hand_fit.npz"))
    depth = d["depth_raw_f32"].astype(np.float64)
    depth[depth == 0] = float(d["max_depth"])
    return d, (depth / float(d["max_depth"]))[::factor, ::factor].copy(), 241.0 / factor


def depth_fitter(d, image, focal, **keywords):
    from deodr_amd.mesh_fitter import MeshDepthFitter

    mean, faces = hand()
    f = MeshDepthFitter(mean, faces, d["euler_init"], d["translation_init"], cregu=1000, device="cpu", **keywords)
    f.set_image(image, focal=focal, distortion=d["distortion"])
    f.set_max_depth(1)
    f.set_depth_scale(float(d["depth_scale"]))
    return f


def data_vertex_gradient(plain):
    """the data gradient of a fitter WITHOUT a basis at its current vertices, through the fitter's own graph (centring included)"""
    leaf = plain._leaves()[0]
    e_data, _e_rigid, _g, _depth, _diff = plain.energy()
    (g_data,) = torch.autograd.grad(e_data, [leaf])
    return g_data.numpy()


@pytest.mark.parametrize("subdivisions", [0, 1])
def test_depth_fit_with_a_shape_basis_on_the_checker(oracle_api, subdivisions):
    import cpu_raster

    d, image, focal = reduced_depth_inputs()
    mean, _faces = hand()
    B = hand_modes(4)
    regu, sigmas = 3.0, np.array([1.0, 2.0, 0.5, 4.0])
    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        f = depth_fitter(d, image, focal, shape_basis=B, coefficient_regu=regu, sigmas=sigmas, subdivisions=subdivisions)
        assert f.coefficients.shape == (4,) and f.coefficients.dtype == torch.float64 and not f.coefficients.any()
        assert f._direct_iteration(1, False) is None  # through autograd
        assert torch.equal(f.vertices, f.vertices_init)
        # one step from coefficients that are not zero: the coefficient gradient is the contraction of B with the total vertex gradient of the SAME
        # fitter without the basis at vertices = mean + B c (rigid energy against the mean), plus the prior's
        c0 = np.array([0.3, -0.2, 0.1, 0.25]) * float(np.abs(mean).max()) * 0.2
        f.coefficients = torch.as_tensor(c0.copy())
        derived = mean + np.tensordot(c0, B, axes=1)
        plain = depth_fitter(d, image, focal, subdivisions=subdivisions)  # (the same mean: the same camera and reference shape)
        plain.vertices = torch.as_tensor(derived.copy())
        g_data = data_vertex_gradient(plain)
        e_rigid, g_rigid = f.rigid_energy.evaluate(torch.as_tensor(derived))  # (f's: the reference shape is the mean)
        expected = np.tensordot(B, g_data + g_rigid.numpy(), axes=([1, 2], [0, 1])) + 2 * regu * c0 / sigmas**2
        seen = {}
        update_all = f.momentum.update_all
        f.momentum.update_all = lambda entries: seen.update({e[0]: (e[2].clone(), None if e[3] is None else e[3].clone()) for e in entries}) or update_all(entries)
        energy = f.step()[0]
        f.momentum.update_all = update_all
        assert rel(f.vertices.numpy(), derived) <= 4 * EPS  # the derived vertices of the step
        g_c = (seen["coefficients"][0] + seen["coefficients"][1]).numpy()
        print(f"subdivisions={subdivisions}: coefficient gradient against einsum(B, total vertex gradient) + prior: {rel(g_c, expected):.3e}")
        # (the two fitters pose vertices that differ by the rounding of one more centring: a few ulp, far from any pixel's decision)
        assert np.abs(expected).max() > 0 and rel(g_c, expected) <= 1e-10
        assert "vertices" not in seen and f.iter == 1
        # the energy of that step: data + rigid against the mean + prior
        e_plain = float(plain.energy()[0].detach()) + float(e_rigid) + regu * float(np.sum((c0 / sigmas) ** 2))
        assert abs(energy - e_plain) <= 1e-10 * abs(e_plain)
        # the update is the momentum rule on the coefficients
        step = np.clip(-f.step_factor_coefficients * g_c, -1, 1)
        assert rel(f.coefficients.numpy(), c0 + (1 - f.damping) * (1 - f.inertia) * step) <= 1e-14
        if subdivisions == 0:
            f.reset()
            energies = [f.step()[0] for _ in range(10)]
            print("energies:", energies)
            assert f.iter == 10 and f.coefficients.shape == (4,) and f.coefficients.abs().max() > 0
            assert energies[9] < energies[0]


def test_keywords_left_at_none_change_nothing(oracle_api):
    import cpu_raster
    import cpu_raster_texture as crt
    from deodr_amd.pytorch import MeshTextureFitterMultiFrame

    d, image, focal = reduced_depth_inputs()
    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        plain, none = depth_fitter(d, image, focal), depth_fitter(d, image, focal, shape_basis=None, coefficient_regu=0.0, sigmas=None)
        assert none.shape_basis is None and not hasattr(none, "coefficients")
        assert [plain.step()[0] for _ in range(3)] == [none.step()[0] for _ in range(3)]
        assert torch.equal(plain.vertices, none.vertices) and torch.equal(plain.transform_quaternion, none.transform_quaternion)
        assert set(plain.momentum.speed) == set(none.momentum.speed) == {"vertices", "quaternion", "translation"}
    v = crt.sphere_views(n_views=2, size=48, texture_size=12, nu=14, n_rings=10)
    fitters = []
    for keywords in ({}, dict(texture_basis=None, coefficient_regu=0.0, sigmas=None)):
        f = MeshTextureFitterMultiFrame(v["vertices"], v["faces"], v["uv"], v["faces"], np.full(v["texture"].shape, 0.5), v["light"], v["ambient"],
                                        cameras=v["cameras"], clockwise=v["clockwise"], device="cpu", pixel_dtype=torch.float64, **keywords)  # fmt: skip
        f.set_background_color(v["background"])
        fitters.append(f)
    with crt.emulate():
        obs = np.random.RandomState(0).rand(2, 48, 48, 3)
        energies = []
        for f in fitters:
            f.set_images(obs)
            energies.append([f.step()[0] for _ in range(3)])
    assert energies[0] == energies[1] and torch.equal(fitters[0].texture, fitters[1].texture)
    assert fitters[1].texture_basis is None and not hasattr(fitters[1], "coefficients")


# ---- texture_basis on the texture fitter


def texture_modes(K, shape, seed=0):
    """K smooth random fields [K, *shape] with orthonormal rows"""
    rs = np.random.RandomState(seed)
    ys, xs = np.meshgrid(np.linspace(0, 1, shape[0]), np.linspace(0, 1, shape[1]), indexing="ij")
    fields = [np.stack([np.sin(2 * np.pi * (rs.rand() * xs * 1.5 + rs.rand() * ys * 1.5) + 6 * rs.rand()) for _ in range(shape[2])], axis=-1) for _ in range(K)]
    q, _r = np.linalg.qr(np.stack(fields).reshape(K, -1).T)
    return q.T.reshape(K, *shape).copy()


def test_texture_basis_fit_follows_the_formula():
    import cpu_raster_texture as crt
    from deodr_amd.pytorch import MeshTextureFitterMultiFrame

    v = crt.sphere_views(n_views=2, size=48, texture_size=12, nu=14, n_rings=10)
    shape = v["texture"].shape
    K, regu, sigmas = 4, 0.7, np.array([1.0, 0.5, 2.0, 3.0])
    B, mean = texture_modes(K, shape), np.full(shape, 0.5)
    truth = mean + np.tensordot(np.array([0.8, -0.6, 0.5, 0.3]), B, axes=1)
    params = dict(smoothness=0.2, inertia=0.9, damping=0.05, step_max=0.3)
    f = MeshTextureFitterMultiFrame(v["vertices"], v["faces"], v["uv"], v["faces"], mean, v["light"], v["ambient"], cameras=v["cameras"],
                                    clockwise=v["clockwise"], device="cpu", pixel_dtype=torch.float64, texture_basis=B, coefficient_regu=regu, sigmas=sigmas,
                                    **params)  # fmt: skip
    f.set_background_color(v["background"])
    assert f.coefficients.shape == (K,) and not f.coefficients.any() and f.texture_basis.K == K
    with crt.emulate():
        f.set_images(np.zeros((2, 48, 48, 3)))
        s2d = crt.view_scenes(f._views, v["faces"], v["uv"], truth, 48, 48, v["background"], v["clockwise"])
        obs = np.stack([crt.checker().render(s, 1.0)[0] for s in s2d])
        f.set_images(obs)
        texture_tensor = f.texture
        c, s = np.zeros(K), np.zeros(K)
        energies = []
        for it in range(10):
            # the step written out: texture of the coefficients, texture_b of the checker + smoothness, contraction with B + prior, momentum
            t = mean + np.tensordot(c, B, axes=1)
            loss, texture_b, _images = crt.oracle_gradient(s2d, t, obs, None, 1.0)
            e_smooth, g_smooth = crt.np_smoothness(t, params["smoothness"])
            c_b = np.tensordot(B, texture_b + g_smooth, axes=([1, 2, 3], [0, 1, 2])) + 2 * regu * c / sigmas**2
            expected_energy = loss + e_smooth + regu * np.sum((c / sigmas) ** 2)
            s = (1 - params["damping"]) * (params["inertia"] * s + (1 - params["inertia"]) * np.clip(-f.step_factor_coefficients * c_b, -0.3, 0.3))
            c = c + s
            energy = f.step()[0]
            energies.append(energy)
            assert abs(energy - expected_energy) <= 1e-12 * expected_energy, it
            assert rel(f.coefficients_b.numpy(), c_b) <= 1e-12 and rel(f.coefficients.numpy(), c) <= 1e-12, it
            assert rel(f.texture.numpy(), t) <= 4 * EPS  # the texture the step rendered: written in place, not clamped
        assert f.texture is texture_tensor is f.mesh.texture and f.iter == 10
        print("energies:", energies)
        assert energies[-1] < energies[0]
        c_now, now = f.coefficients.clone(), float(f.energy())  # energy(): the same three terms at the current coefficients, nothing updated
        terms = float(f.e_data + f.e_smooth) + regu * float(((f.coefficients / torch.as_tensor(sigmas)) ** 2).sum())
        assert abs(now - terms) <= 1e-14 * terms and now < energies[0] and torch.equal(f.coefficients, c_now) and f.iter == 10
    with pytest.raises(ValueError, match="texture_basis must be"):
        MeshTextureFitterMultiFrame(v["vertices"], v["faces"], v["uv"], v["faces"], mean, v["light"], v["ambient"], cameras=v["cameras"], device="cpu",
                                    texture_basis=B[:, :-1])  # fmt: skip
