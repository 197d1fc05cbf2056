"""CPU checks (torch fallback of the point-to-surface term) of ``MeshPointCloudFitter(metric="surface")``: the hand (526 vertices, 1 048 faces)
against 4 000 area-uniform samples of its own surface under the known pose of tests/test_chamfer_fit_host.py -- plain, with ``skin``,
``shape_basis``, ``subdivisions=1``, ``smoothing``, ``rigidity="arap"``, and points -> mesh alone with a finite ``max_distance`` --: energies finite
and lower after 25 iterations, the recovered translation error printed for both metrics (not asserted); two poses with clouds of unequal length;
``metric="vertex"`` builds what the fitter has always built, and an unknown metric is refused."""

import numpy as np
import pytest
import torch

from test_chamfer_fit_host import EULER, SHIFT, hand

N_POINTS = 4000


def posed_surface_cloud(vertices, faces, count=N_POINTS, seed=0):
    """-> (``count`` samples of the surface under the known pose, the translation of that pose)"""
    from deodr_amd.mesh_fitter import _quat_from_euler_zyx, qrot
    from deodr_amd.surface import sample_surface

    t_true = SHIFT * vertices.std()
    q = torch.as_tensor(_quat_from_euler_zyx(EULER))
    posed = qrot(q[None], torch.as_tensor(vertices - vertices.mean(axis=0))[None])[0].numpy() + t_true
    return sample_surface(posed, faces, count, seed)[0], t_true


def surface_fitter(device="cpu", vertices=None, faces=None, metric="surface", count=N_POINTS, **keywords):
    from deodr_amd.pytorch import MeshPointCloudFitter

    if vertices is None:
        vertices, faces = hand()
    f = MeshPointCloudFitter(vertices, faces, np.zeros(3), np.zeros(3), device=device, metric=metric, **keywords)
    cloud, f.t_true = posed_surface_cloud(np.asarray(vertices, dtype=np.float64), np.asarray(faces), count)
    f.set_point_cloud(cloud)
    return f


def makers():
    import skinning_reference as skr
    from deodr_amd.skinning import Skin
    from test_basis import hand_modes

    def skinned(**kw):
        v, faces, joints, parents, w = skr.hand_rig(measured_from="near")
        return surface_fitter(vertices=v, faces=faces, skin=Skin(joints, parents, w, device="cpu"), **kw)

    scale = hand()[0].std()
    return {"plain": surface_fitter, "skin": skinned, "shape_basis": lambda **kw: surface_fitter(shape_basis=hand_modes(3), coefficient_regu=1e-3, **kw),
            "subdivisions=1": lambda **kw: surface_fitter(subdivisions=1, **kw), "smoothing=16": lambda **kw: surface_fitter(smoothing=16.0, **kw),
            'rigidity="arap"': lambda **kw: surface_fitter(rigidity="arap", **kw),
            "points_to_mesh, max_distance": lambda **kw: surface_fitter(directions="points_to_mesh", max_distance=2 * scale, **kw)}  # fmt: skip


@pytest.mark.parametrize("name", ["plain", "skin", "shape_basis", "subdivisions=1", "smoothing=16", 'rigidity="arap"', "points_to_mesh, max_distance"])
def test_fits_run_finite_and_lower_their_energy(name):
    from deodr_amd.surface import PointSurfaceTerm

    f = makers()[name]()
    assert isinstance(f.term, PointSurfaceTerm) and not f.term.uses_kernel(f.vertices) and f.term.n == 1 and f.term.nb_points == N_POINTS
    assert (f.term.nb_faces, f.term.nb_vertices) == (f.mesh.nb_faces, f.mesh.nb_vertices)  # with subdivisions: the fine faces meet the cloud
    assert f.term.nb_faces == (4 * 1048 if name == "subdivisions=1" else 1048)
    assert (f.term.directions, float(f.term.params[2])) == ((1, 2 * hand()[0].std()) if name.startswith("points") else (3, float("inf")))
    N = 25
    energies, posed = [], None
    for _ in range(N):
        energy, terms, posed = f.step()
        energies.append(energy)
        assert terms.shape == (1, 2) and posed.shape[0] == 1 and posed.shape[2] == 3
    error = np.linalg.norm(f.transform_translation[0].numpy() - f.t_true) / np.linalg.norm(f.t_true)
    print(f"{name}, metric=surface: energy after {N} iterations {energies[0]:.5f} -> {energies[-1]:.5f}; translation error / |translation| 1 -> {error:.3f}")
    assert np.all(np.isfinite(energies)) and energies[-1] < energies[0], (name, energies)
    assert bool(torch.isfinite(f.vertices).all()) and f.iter == N
    assert posed.shape[1] == f.mesh.nb_vertices
    if name == "plain":  # the same cloud under the vertex metric, for the record
        g = surface_fitter(metric="vertex")
        e_vertex = [g.step()[0] for _ in range(N)]
        error_v = np.linalg.norm(g.transform_translation[0].numpy() - g.t_true) / np.linalg.norm(g.t_true)
        print(f"{name}, metric=vertex: energy after {N} iterations {e_vertex[0]:.5f} -> {e_vertex[-1]:.5f}; translation error / |translation| 1 -> {error_v:.3f}")


def test_two_poses_with_clouds_of_unequal_length():
    from deodr_amd.pytorch import MeshPointCloudFitter

    vertices, faces = hand()
    cloud, _ = posed_surface_cloud(vertices, faces, 600)
    f = MeshPointCloudFitter(vertices, faces, np.zeros((2, 3)), np.zeros((2, 3)), device="cpu", n_poses=2, metric="surface")
    f.set_point_clouds([cloud, cloud[:150] + 0.1], weights=[None, np.linspace(0.0, 1.0, 150)])
    assert tuple(f.term.points.shape) == (2, 600, 3) and f.term.lengths == [600, 150]
    assert torch.equal(f.term.points[1, 150:], f.term.points[1, :1].expand(450, 3)) and not bool(f.term.point_weights[1, 150:].any())
    energies = [f.step()[0] for _ in range(15)]
    assert np.all(np.isfinite(energies)) and energies[-1] < energies[0]
    nf, bary, npt = f.term.correspondences(f._transformed(f.vertices_leaf).detach())
    assert tuple(nf.shape) == (2, 600) and tuple(bary.shape) == (2, 600, 3) and tuple(npt.shape) == (2, 526) and nf.dtype == torch.int64
    assert int(nf.max()) < 1048 and bool((nf[1, 150:] == nf[1, 0]).all()) and torch.equal(bary[1, 150:], bary[1, :1].expand(450, 3))
    assert int(npt[1].max()) < 150  # a padded point is a copy of the first and never the nearest
    assert float((bary.sum(dim=-1) - 1).abs().max()) < 1e-12 and float(bary.min()) > -1e-12
    with pytest.raises(ValueError, match="1 clouds for a fitter of 2 poses"):
        f.set_point_clouds([cloud])


def test_the_vertex_metric_is_what_it_was_and_an_unknown_one_is_refused():
    from deodr_amd.chamfer import PointCloudTerm
    from deodr_amd.pytorch import MeshPointCloudFitter
    from deodr_amd.surface import PointSurfaceTerm

    vertices, faces = hand()
    cloud = np.random.RandomState(0).rand(40, 3)
    for keywords in ({}, dict(metric="vertex")):
        f = MeshPointCloudFitter(vertices, faces, np.zeros(3), np.zeros(3), device="cpu", **keywords)
        f.set_point_cloud(cloud)
        assert type(f.term) is PointCloudTerm and f.metric == "vertex"
    default, named = (MeshPointCloudFitter(vertices, faces, np.zeros(3), np.zeros(3), device="cpu", **kw) for kw in ({}, dict(metric="vertex")))
    default.set_point_cloud(cloud), named.set_point_cloud(cloud)
    assert [default.step()[0] for _ in range(3)] == [named.step()[0] for _ in range(3)]
    f = MeshPointCloudFitter(vertices, faces, np.zeros(3), np.zeros(3), device="cpu", metric="surface")
    f.set_point_cloud(cloud)
    assert type(f.term) is PointSurfaceTerm and f.step_factor_vertices == MeshPointCloudFitter.step_factor_vertices * 526
    for bad in ("face", "", None, "Surface"):
        with pytest.raises(ValueError, match='metric must be "vertex" or "surface"'):
            MeshPointCloudFitter(vertices, faces, np.zeros(3), np.zeros(3), device="cpu", metric=bad)
