"""CPU checks of the ``rigidity=`` / ``arap_weights=`` keywords of the pose fitters on the checker-backed rasterizer of tests/cpu_raster.py:
"laplacian" is the fit without the keyword bit for bit, "arap" fits run finite and lower their energy -- depth, one-view colour, two views, with
``subdivisions=1``, ``skin=``, ``shape_basis=`` and ``smoothing=16`` --, the refusals, the NumPy-level ``ArapEnergy``, and the comparison of the two
regularisers on a target whose mesh is bent (printed for DESIGN.md 4l, not asserted).  64 x 64 frames, as in the other ``*_fit_host`` files."""

import numpy as np
import pytest
import torch

import skinning_reference as skr
from test_pyramid_fit_host import PARAMETERS, hand_fitter
from test_skinning_fit_host import SIZE, render_target, rig_fitter
from test_smoothing_fit_host import MAKERS, depth_fitter, skinned_fitter


def basis_fitter(**keywords):
    """the depth fit of the hand with three shape modes against its own depth image at known coefficients, from coefficients 0"""
    from test_basis import hand_modes

    f, _, focal = rig_fitter(skin="omit", shape_basis=hand_modes(3), **keywords)
    f.set_image(np.ones((SIZE, SIZE)), focal=focal)
    f.coefficients = torch.as_tensor([1.0, -0.7, 0.5], dtype=torch.float64) * 0.02
    f._leaves()
    with torch.no_grad():
        target = f.energy()[3].detach().cpu().numpy().copy()
    f.reset()
    f.set_image(target, focal=focal)
    return f


def test_laplacian_and_no_keyword_are_the_same_fit(oracle_api):
    import cpu_raster
    from deodr_amd.scene3d import LaplacianRigidEnergyDevice

    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        for name, make in MAKERS.items():
            plain, same = make(), make(rigidity="laplacian", arap_weights="cotangent")
            assert type(same.rigid_energy) is LaplacianRigidEnergyDevice and same.rigidity == plain.rigidity == "laplacian"
            assert [plain.step()[0] for _ in range(5)] == [same.step()[0] for _ in range(5)], name
            compared = [k for k in PARAMETERS if torch.is_tensor(getattr(plain, k, None))]
            assert len(compared) >= 3 and all(torch.equal(getattr(plain, k), getattr(same, k)) for k in compared)
            assert set(plain.momentum.speed) == set(same.momentum.speed)


def test_arap_fits_run_finite_and_lower_their_energy(oracle_api):
    """depth, one view, two views; through a subdivided cage (the energy on the cage), with a skin (on the rest vertices), with a shape basis (on
    the derived vertices, the gradient through the basis adjoint) and with smoothed steps"""
    import cpu_raster
    from deodr_amd.arap import ArapEnergyDevice

    makers = dict(MAKERS, **{"colour, subdivisions=1": lambda **kw: hand_fitter(1, "cpu", shift_pixels=(2, 1), subdivisions=1, **kw),
                             "depth, skin": skinned_fitter,
                             "depth, shape_basis": basis_fitter,
                             "colour, smoothing=16": lambda **kw: hand_fitter(1, "cpu", shift_pixels=(2, 1), smoothing=16.0, **kw),
                             "depth, cotangent": lambda **kw: depth_fitter(arap_weights="cotangent", **kw)})  # fmt: skip
    N = 25
    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        for name, make in makers.items():
            f = make(rigidity="arap")
            assert type(f.rigid_energy) is ArapEnergyDevice and f.rigid_energy.nb_vertices == f.control_mesh.nb_vertices
            assert f._direct_iteration(3, True) is None  # through autograd
            energies = [f.step()[0] for _ in range(N)]
            print(f"{name}: rigidity='arap' energy after {N} iterations {energies[0]:.4f} -> {energies[-1]:.4f}")
            assert np.all(np.isfinite(energies)) and energies[-1] < energies[0], (name, energies)
            assert bool(torch.isfinite(f.vertices).all())


def test_refusals():
    import os

    from conftest import GOLDEN
    from deodr_amd import scenes
    from deodr_amd.arap import ArapEnergyDevice
    from deodr_amd.mesh_fitter import MeshDepthFitter, MeshRGBFitterWithPose, MeshRGBFitterWithPoseMultiFrame

    d = np.load(os.path.join(GOLDEN, "rgb_hand_fit.npz"))
    vertices, faces = d["vertices_centered"], scenes.load_hand_mesh(os.path.join(GOLDEN, "hand_mesh.npz"))[1]
    colour = (d["default_color"], d["default_light_directional"], float(d["default_light_ambient"]))
    makers = [lambda **kw: MeshDepthFitter(vertices, faces, np.zeros(3), d["translation_init"], device="cpu", **kw),
              lambda **kw: MeshRGBFitterWithPose(vertices, faces, np.zeros(3), d["translation_init"], *colour, device="cpu", **kw),
              lambda **kw: MeshRGBFitterWithPoseMultiFrame(vertices, faces, np.zeros((2, 3)), np.tile(d["translation_init"], (2, 1)), *colour, device="cpu", **kw)]  # fmt: skip
    for make in makers:
        for bad in ("ARAP", "rigid", None, 1, True):
            with pytest.raises(ValueError, match='rigidity must be "laplacian" or "arap"'):
                make(rigidity=bad)
        with pytest.raises(ValueError, match='weights must be "uniform", "cotangent" or an array'):
            make(rigidity="arap", arap_weights="cot")
        with pytest.raises(ValueError, match="cregu must be >= 0"):
            make(rigidity="arap", cregu=-1.0)
        f = make(rigidity="arap", arap_weights="cotangent")
        assert float(f.rigid_energy.weights.min()) >= 0 and f.rigid_energy.weights.dtype == torch.float64
    # the tables of the class itself
    V = len(vertices)
    good = ArapEnergyDevice(faces, vertices, 1.0, device="cpu")
    w = good.weights.numpy().copy()
    for bad, message in ((w[:-1], "one value per stored entry"), (-w, "finite and >= 0"), (np.where(np.arange(len(w)) == 0, 2.0, w), "must be symmetric"),
                         (np.where(np.arange(len(w)) == 3, np.nan, w), "finite and >= 0")):  # fmt: skip
        with pytest.raises(ValueError, match=message):
            ArapEnergyDevice(faces, vertices, 1.0, bad, device="cpu")
    with pytest.raises(ValueError, match=rf"vertices_ref must be \[{V}, 3\]"):
        ArapEnergyDevice(faces, vertices[:, :2], 1.0, device="cpu")
    with pytest.raises(ValueError, match="vertices must be"):
        good.evaluate(torch.zeros((V + 1, 3), dtype=torch.float64))
    offsets, cols = good.offsets.numpy().astype(np.int64), good.cols.numpy().astype(np.int64)
    for o, c, message in ((offsets[::-1].copy(), cols, "non-decreasing"), (offsets, np.where(np.arange(len(cols)) == 0, V, cols), "out of range"),
                          (offsets, np.where(np.arange(len(cols)) == 0, 0, cols), "diagonal"), (offsets, np.roll(cols, 1), "symmetric|diagonal")):  # fmt: skip
        with pytest.raises(ValueError, match=message):
            ArapEnergyDevice._check(o, c, w, V)
    # several components are fine
    two = ArapEnergyDevice(np.array([[0, 1, 2], [3, 4, 5]]), np.random.RandomState(0).rand(6, 3), 1.0, device="cpu")
    assert float(two.evaluate(two.vertices_ref.clone())[0]) == 0.0


def test_numpy_level_energy_on_the_tetrahedron():
    import arap_reference as ar
    import deodr_amd
    from deodr_amd.scene3d import MeshTopology

    q, faces, _ = ar.mesh("tetrahedron")

    class Mesh:  # what ArapEnergy asks of a mesh
        vertices = q
        adjacencies = type("A", (), dict(topology=MeshTopology(faces, 4, device="cpu")))()

    c = ar.case("tetrahedron", ("noise30",))
    energy = deodr_amd.ArapEnergy(Mesh, c["cregu"])
    e, g, H = energy.evaluate(c["p"][0], True, True)
    assert abs(e - float(c["energy"][0])) <= 1e-13 * float(c["e_scale"][0])
    assert np.abs(g - c["gradient"][0].astype(np.float64)).max() <= 1e-13 * float(c["g_scale"][0])
    assert H.shape == (12, 12) and abs(H - H.T).max() == 0
    lam = np.linalg.eigvalsh(H.toarray())
    assert lam.min() >= -1e-12 * lam.max() and np.sum(lam < 1e-9 * lam.max()) == 3  # positive semidefinite; the null space: translations
    assert np.allclose(H.toarray()[::3, ::3], 2 * c["cregu"] * (3 * np.eye(4) - (1 - np.eye(4))))  # 2 c L of the complete graph
    assert isinstance(energy.evaluate(q, False, False), float) and energy.evaluate(q, False, False) == 0.0
    assert len(energy.evaluate(q, True, False)) == 2


def test_bent_target_laplacian_against_arap(oracle_api):
    """Does it help at 64 x 64?  The depth image of the hand with its fingers bent by the rig (``skin_torch`` through the fitter's own model), fitted
    WITHOUT a skin under both regularisers, 60 iterations: the data term, the regulariser's own energy and the distance of the fitted vertices to the
    bent ones.  Printed, not asserted (DESIGN.md 4l has the figures of the last run)."""
    import cpu_raster

    q_true = skr.hand_target_quaternions()
    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        truth, rig, focal = rig_fitter()
        target = render_target(truth, focal, q_true)
        rest = truth.vertices.detach().clone()
        bent = rig.apply(rest, torch.as_tensor(q_true)).detach()
        rows = []
        for label, keywords in (("laplacian cregu=1000", {}), ("arap cregu=1000", dict(rigidity="arap")), ("arap cotangent cregu=1000", dict(rigidity="arap", arap_weights="cotangent"))):
            f, _, _ = rig_fitter(skin="omit", **keywords)
            f.set_image(target, focal=focal)
            energies = [f.step()[0] for _ in range(60)]
            v = f.vertices.detach()
            moved = v - v.mean(dim=0) + rest.mean(dim=0)  # (the fit without a skin keeps its vertices centred)
            rows.append((label, energies[0], energies[-1], float((moved - bent).norm(dim=1).mean()), float((rest - bent).norm(dim=1).mean())))
            assert np.all(np.isfinite(energies))
    for label, first, last, err, err0 in rows:
        print(f"bent target, {label}: energy {first:.4f} -> {last:.4f}; mean vertex distance to the bent mesh {err0:.5f} -> {err:.5f}")
