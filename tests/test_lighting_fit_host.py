"""MeshRGBFitterWithPose with spherical-harmonic lighting and a per-vertex albedo on CPU tensors, the checker standing in for the rasterizer
(tests/cpu_raster.emulate): the iteration that runs as autograd through fronthalf.sh_shade's torch fallback and Scene3DDevice.render_l2.

Both fits are of the hand at 64 x 64 with the geometry held (step factors of vertices and pose set to zero) and the step factor of what is fitted
scaled to the small frame (the defaults are those of the reference's 200 x 200 photographs: a gradient is a sum over pixels).  A sign error in any
grad Y_k, or in the albedo's adjoint, makes the energy rise."""

import os
import sys

import numpy as np
import torch

import cpu_raster
import fititer_reference as fr

SIZE, ITERATIONS = 64, 100


def hand_fit():
    from deodr_amd import scenes

    d = np.load(os.path.join(fr.HERE, "golden", "rgb_hand_fit.npz"))
    _, faces = scenes.load_hand_mesh(os.path.join(fr.HERE, "golden", "hand_mesh.npz"))
    return d, faces


def make(d, faces, image=None, **keywords):
    from deodr_amd.mesh_fitter import MeshRGBFitterWithPose

    f = MeshRGBFitterWithPose(d["vertices_centered"], faces, np.zeros(3), d["translation_init"], d["default_color"], d["default_light_directional"],
                              float(d["default_light_ambient"]), cregu=1000, device="cpu", **keywords)  # fmt: skip
    f.set_background_color(d["background_color"])
    f.set_image(np.zeros((SIZE, SIZE, 3)) if image is None else image)
    return f


def hold_geometry(f):
    f.step_factor_vertices = f.step_factor_quaternion = f.step_factor_translation = 0.0


def true_lighting(d):
    from deodr_amd import lighting

    return lighting.sh_from_directional(torch.tensor(d["default_light_directional"]), float(d["default_light_ambient"])).numpy()


def test_sh_lighting_is_recovered_from_a_wrong_directional_light(oracle_api):
    """Target: the hand under the SH coefficients of its own directional + ambient pair.  Start: those of another light, (0.5, -0.2, -0.6) with ambient
    0.3.  Geometry and colour held, SH free.  Measured on this path (100 iterations, step factor 0.001): energy 35.37 -> 1.10, a fraction 0.031 of the
    start, decreasing at every iteration; asserted below 0.062 (a factor 2)."""
    from deodr_amd import lighting

    d, faces = hand_fit()
    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        truth = make(d, faces, light_sh_init=true_lighting(d))
        target = truth.render()[0].numpy()
        assert target.std() > 0.05
        wrong = lighting.sh_from_directional(torch.tensor([0.5, -0.2, -0.6]), 0.3).numpy()
        f = make(d, faces, target, light_sh_init=wrong, update_color=False)
        hold_geometry(f)
        f.step_factor_light_sh = 0.001
        before = {k: getattr(f, k).clone() for k in ("vertices", "transform_quaternion", "transform_translation", "mesh_color")}
        energies = np.array([f.step()[0] for _ in range(ITERATIONS)])
    print(f"energy {energies[0]:.4g} -> {energies[-1]:.4g}: {energies[-1] / energies[0]:.4f}")
    assert tuple(f.light_sh.shape) == (9,) and f.iter == ITERATIONS
    assert np.all(np.diff(energies[5:]) < 0)  # (after the momentum's transient; here it decreases from the first iteration on)
    assert energies[-1] < 0.062 * energies[0]
    assert torch.equal(f.mesh_color, before["mesh_color"])  # update_color=False
    assert float((f.vertices - before["vertices"]).abs().max()) < 1e-12 and torch.equal(f.transform_translation, before["transform_translation"])
    assert np.abs(f.light_sh.numpy() - true_lighting(d)).max() < np.abs(wrong - true_lighting(d)).max()


def test_a_per_vertex_albedo_is_fitted_under_a_smoothness_term(oracle_api):
    """Target: the hand with an albedo that varies smoothly over it (+- 40 % of the default colour along x), under known SH lighting.  Start: the default
    colour at every vertex.  ``vertex_albedo=True, albedo_regu=1``, lighting and geometry held.  Measured (100 iterations, step factor 0.005): energy
    3.128 -> 0.507, a fraction 0.162, decreasing at every iteration; the mean albedo error 0.0287 -> 0.0194.  Asserted: below 0.324 (a factor 2)."""
    d, faces = hand_fit()
    v = d["vertices_centered"]
    albedo = np.clip(d["default_color"][None] * (1 + 0.4 * np.sin(3 * v[:, :1] / np.abs(v).max()) * np.array([[1.0, -0.5, 0.7]])), 0.05, 1.0)
    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        truth = make(d, faces, light_sh_init=true_lighting(d), vertex_albedo=True)
        assert tuple(truth.mesh_color.shape) == (len(v), 3) and torch.equal(truth.mesh_color[7], torch.tensor(d["default_color"]))
        truth.mesh_color = torch.tensor(albedo)
        target = truth.render()[0].numpy()
        f = make(d, faces, target, light_sh_init=true_lighting(d), vertex_albedo=True, albedo_regu=1.0, update_lights=False)
        hold_geometry(f)
        f.step_factor_albedo = 0.005
        sh_before = f.light_sh.clone()
        energies = np.array([f.step()[0] for _ in range(ITERATIONS)])
        # the smoothness term is in the energy: 0.5 albedo_regu sum_c a_c^T (L^T L) a_c of the albedo the last step started from
        smooth, gradient = f._albedo_smoothness()
        a = f.mesh_color
        expected = 0.5 * sum(float(a[:, c] @ f.mesh.topology.laplacian_quadratic(a)[:, c]) for c in range(3))
        assert abs(float(smooth) - expected) <= 1e-12 * expected and float(smooth) > 0
        assert torch.allclose(gradient, f.mesh.topology.laplacian_quadratic(a), rtol=1e-12, atol=0)
    print(f"energy {energies[0]:.4g} -> {energies[-1]:.4g}: {energies[-1] / energies[0]:.4f}")
    assert np.all(np.diff(energies[5:]) < 0)
    assert energies[-1] < 0.324 * energies[0]
    assert torch.equal(f.light_sh, sh_before)  # update_lights=False
    assert np.abs(f.mesh_color.numpy() - albedo).mean() < np.abs(d["default_color"][None] - albedo).mean()


def test_the_new_keywords_are_checked():
    import pytest

    d, faces = hand_fit()
    with pytest.raises(ValueError, match="light_sh_init must have shape"):
        make(d, faces, light_sh_init=np.zeros(8))
    with pytest.raises(ValueError, match="vertex_albedo needs light_sh_init"):
        make(d, faces, vertex_albedo=True)
    from deodr_amd.mesh_fitter import MeshRGBFitterWithPose

    with pytest.raises(ValueError, match="albedo_regu needs a colour of 3 channels"):
        MeshRGBFitterWithPose(d["vertices_centered"], faces, np.zeros(3), d["translation_init"], np.array([0.5]), d["default_light_directional"], 0.5,
                              device="cpu", light_sh_init=np.zeros(9), vertex_albedo=True, albedo_regu=1.0)  # fmt: skip
    f = make(d, faces, light_sh_init=np.zeros((9, 3)), vertex_albedo=True)
    assert tuple(f.light_sh.shape) == (9, 3) and f._albedo_energy is None  # albedo_regu = 0: no smoothness term


def make_multi(d, faces, images):
    from deodr_amd.mesh_fitter import MeshRGBFitterWithPoseMultiFrame

    n = len(images)
    eulers = np.array([[0.0, 0.4 * v, 0.0] for v in range(n)])
    f = MeshRGBFitterWithPoseMultiFrame(d["vertices_centered"], faces, eulers, np.tile(d["translation_init"], (n, 1)), d["default_color"],
                                        d["default_light_directional"], float(d["default_light_ambient"]), cregu=1000, device="cpu")  # fmt: skip
    f.set_background_color(d["background_color"])
    f.set_images(images)
    return f


def test_without_the_new_keywords_nothing_changes(oracle_api):
    """five iterations of each directional-light fitter (single view; two views) built while deodr_amd.lighting is not even imported, and five of one
    built after importing it: the same energies bit for bit; a fitter without the keywords never imports the module, has no SH state and takes the
    code it took before"""
    d, faces = hand_fit()
    rs = np.random.RandomState(0)
    image, images = rs.rand(SIZE, SIZE, 3), list(rs.rand(2, SIZE, SIZE, 3))
    builders = (lambda: make(d, faces, image), lambda: make_multi(d, faces, images))
    saved = sys.modules.pop("deodr_amd.lighting", None)
    try:
        with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
            before = []
            for build in builders:
                f = build()
                before.append([f.step()[0] for _ in range(5)])
                assert f.light_sh is None and f.scene.light_sh is None and tuple(f.mesh_color.shape) == (3,)
            assert "deodr_amd.lighting" not in sys.modules
            import deodr_amd.lighting  # noqa: F401

            after = [[f.step()[0] for _ in range(5)] for f in (build() for build in builders)]
    finally:
        if saved is not None:
            sys.modules["deodr_amd.lighting"] = saved
    assert before == after
    for energies in before:
        assert energies[0] > 0 and len(set(energies)) == 5
