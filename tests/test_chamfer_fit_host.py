"""CPU checks (torch fallback of the closest-point term) of ``MeshPointCloudFitter``: the hand (526 vertices) against 400 of its own vertices under
a known pose -- plain, with ``skin``, ``shape_basis``, ``subdivisions=1``, ``smoothing``, ``rigidity="arap"``, and points -> mesh alone with a finite
``max_distance`` --: energies finite and lower after 25 iterations, the recovered translation error printed (not asserted); two poses with clouds of
unequal length; ``PointCloudTerm``'s host checks, ``depth_to_points`` against the camera's own projection, and the refusals."""

import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN


def hand():
    from deodr_amd import scenes

    vertices, faces = scenes.load_hand_mesh(os.path.join(GOLDEN, "hand_mesh.npz"))[:2]
    return np.asarray(vertices, dtype=np.float64), np.asarray(faces)


EULER, SHIFT = np.array([0.1, -0.15, 0.2]), np.array([0.3, -0.2, 0.5])  # the known pose (the shift in units of the hand's standard deviation)


def posed_cloud(vertices, count=400, seed=0):
    """-> (``count`` of the vertices under the known pose, the translation of that pose)"""
    from deodr_amd.mesh_fitter import _quat_from_euler_zyx, qrot

    t_true = SHIFT * vertices.std()
    q = torch.as_tensor(_quat_from_euler_zyx(EULER))
    posed = qrot(q[None], torch.as_tensor(vertices - vertices.mean(axis=0))[None])[0].numpy() + t_true
    return posed[np.random.RandomState(seed).permutation(len(vertices))[:count]], t_true


def cloud_fitter(device="cpu", vertices=None, faces=None, **keywords):
    from deodr_amd.pytorch import MeshPointCloudFitter

    if vertices is None:
        vertices, faces = hand()
    f = MeshPointCloudFitter(vertices, faces, np.zeros(3), np.zeros(3), device=device, **keywords)
    cloud, f.t_true = posed_cloud(np.asarray(vertices, dtype=np.float64))
    f.set_point_cloud(cloud)
    return f


def makers():
    import skinning_reference as sr
    from deodr_amd.skinning import Skin
    from test_basis import hand_modes

    def skinned(**kw):
        v, faces, joints, parents, w = sr.hand_rig(measured_from="near")
        return cloud_fitter(vertices=v, faces=faces, skin=Skin(joints, parents, w, device="cpu"), **kw)

    scale = hand()[0].std()
    return {"plain": cloud_fitter, "skin": skinned, "shape_basis": lambda **kw: cloud_fitter(shape_basis=hand_modes(3), coefficient_regu=1e-3, **kw),
            "subdivisions=1": lambda **kw: cloud_fitter(subdivisions=1, **kw), "smoothing=16": lambda **kw: cloud_fitter(smoothing=16.0, **kw),
            'rigidity="arap"': lambda **kw: cloud_fitter(rigidity="arap", **kw),
            "points_to_mesh, max_distance": lambda **kw: cloud_fitter(directions="points_to_mesh", max_distance=2 * scale, **kw)}  # fmt: skip


@pytest.mark.parametrize("name", ["plain", "skin", "shape_basis", "subdivisions=1", "smoothing=16", 'rigidity="arap"', "points_to_mesh, max_distance"])
def test_fits_run_finite_and_lower_their_energy(name):
    f = makers()[name]()
    assert not f.term.uses_kernel(f.vertices) and f.term.n == 1 and f.term.nb_points == 400
    assert (f.term.directions, float(f.term.params[2])) == ((1, 2 * hand()[0].std()) if name.startswith("points") else (3, float("inf")))
    N = 25
    energies, posed = [], None
    for _ in range(N):
        energy, terms, posed = f.step()
        energies.append(energy)
        assert terms.shape == (1, 2) and posed.shape[0] == 1 and posed.shape[2] == 3
    error = np.linalg.norm(f.transform_translation[0].numpy() - f.t_true) / np.linalg.norm(f.t_true)
    print(f"{name}: energy after {N} iterations {energies[0]:.5f} -> {energies[-1]:.5f}; translation error / |translation| 1 -> {error:.3f}")
    assert np.all(np.isfinite(energies)) and energies[-1] < energies[0], (name, energies)
    assert bool(torch.isfinite(f.vertices).all()) and f.iter == N
    assert posed.shape[1] == (f.mesh.nb_vertices if name == "subdivisions=1" else 526)


def test_two_poses_with_clouds_of_unequal_length():
    from deodr_amd.pytorch import MeshPointCloudFitter

    vertices, faces = hand()
    cloud, _ = posed_cloud(vertices)
    f = MeshPointCloudFitter(vertices, faces, np.zeros((2, 3)), np.zeros((2, 3)), device="cpu", n_poses=2)
    f.set_point_clouds([cloud, cloud[:150] + 0.1], weights=[None, np.linspace(0.0, 1.0, 150)])
    assert tuple(f.term.points.shape) == (2, 400, 3) and f.term.lengths == [400, 150]
    assert torch.equal(f.term.points[1, 150:], f.term.points[1, :1].expand(250, 3)) and not bool(f.term.point_weights[1, 150:].any())
    assert abs(float(f.term.point_weights[1].sum()) - 1) < 1e-12
    energies = [f.step()[0] for _ in range(15)]
    assert np.all(np.isfinite(energies)) and energies[-1] < energies[0]
    nv, npt = f.term.correspondences(f._transformed(f.vertices_leaf).detach())
    assert tuple(nv.shape) == (2, 400) and tuple(npt.shape) == (2, 526) and nv.dtype == torch.int64
    assert bool((nv[1, 150:] == nv[1, 0]).all()) and int(npt[1].max()) < 150  # a padded point is a copy of the first and never the nearest
    with pytest.raises(ValueError, match="1 clouds for a fitter of 2 poses"):
        f.set_point_clouds([cloud])
    with pytest.raises(ValueError, match=r"points must be \[P, 3\]"):
        f.set_point_cloud(np.zeros((2, 5, 3)))


def test_term_checks_its_tables_on_the_host():
    from deodr_amd.chamfer import PointCloudTerm, chamfer_torch

    rs = np.random.RandomState(0)
    cloud = rs.rand(30, 3)
    make = lambda points=cloud, **kw: PointCloudTerm(points, device="cpu", **kw)
    for bad, message in ((dict(directions="points"), "directions must be"), (dict(max_distance=0.0), "max_distance must be > 0"),
                         (dict(max_distance=float("nan")), "max_distance must be > 0"), (dict(mix=(1.0, float("inf"))), "mix must be two finite values"),
                         (dict(mix=(1.0,)), "mix must be two finite values"), (dict(point_weights=-np.ones(30)), "point_weights must be finite and >= 0"),
                         (dict(point_weights=np.zeros(30)), "sum to 0"), (dict(point_weights=np.ones(29)), "has 30 points and weights of shape"),
                         (dict(vertex_weights=np.full(7, np.nan)), "vertex_weights must be finite and >= 0"), (dict(vertex_weights=np.ones((7, 1))), r"vertex_weights must be \[V\]")):  # fmt: skip
        with pytest.raises(ValueError, match=message):
            make(**bad)
    for bad in (np.zeros((0, 3)), np.zeros((5, 2)), np.zeros(3), [], [cloud, np.zeros((0, 3))]):
        with pytest.raises(ValueError, match="points must be"):
            make(bad)
    with pytest.raises(ValueError, match="coordinates of the points must be finite"):
        make(np.where(np.arange(90).reshape(30, 3) == 4, np.inf, cloud))
    term = make(vertex_weights=np.ones(7), normalise=False, max_distance=0.4, mix=(2.0, 0.5))
    assert term.params.tolist() == [2.0, 0.5, 0.4] and term.params.dtype == torch.float64 and float(term.point_weights.sum()) == 30.0
    with pytest.raises(ValueError, match="7 vertex weights for 8 vertices"):
        term.evaluate(torch.zeros((8, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match=r"vertices must be \[V, 3\] or \[1, V, 3\]"):
        term.evaluate(torch.zeros((2, 7, 3), dtype=torch.float64))
    v = torch.tensor(rs.rand(7, 3), requires_grad=True)
    loss, terms = term.evaluate(v)  # [V,3]: the same mesh against every cloud
    (g,) = torch.autograd.grad(loss.sum(), v)
    ref = chamfer_torch(v.detach()[None], term.points, term.params, term.point_weights, term.vertex_weights)
    assert torch.equal(g, ref[2][0]) and torch.equal(terms, ref[0]) and torch.equal(loss.detach(), ref[1]) and not terms.requires_grad
    assert make(normalise=True)._vertex_weights(4).tolist() == [0.25] * 4 and make(normalise=False)._vertex_weights(4) is None
    term.params.copy_(torch.tensor([4.0, 1.0, 0.4], dtype=torch.float64))  # read at every call
    assert float(term.evaluate(v)[0].detach()) == 2 * float(loss.detach())


def test_depth_to_points_inverts_the_projection():
    from deodr_amd.chamfer import depth_to_points
    from deodr_amd.scene3d import DeviceCamera

    rs = np.random.RandomState(1)
    angle = 0.3
    R = np.array([[np.cos(angle), 0, np.sin(angle)], [0, 1, 0], [-np.sin(angle), 0, np.cos(angle)]])
    extrinsic = np.column_stack((R, [0.1, -0.2, 3.0]))
    intrinsic = np.array([[80.0, 0.5, 15.5], [0, 75.0, 11.0], [0, 0, 1]])
    camera = DeviceCamera(extrinsic, intrinsic, 24, 32, device="cpu")
    depth = 2.0 + rs.rand(24, 32)
    depth[3:6, 4:9] = 0.0  # holes
    points = depth_to_points(depth, camera)
    assert tuple(points.shape) == (24 * 32 - 15, 3)
    ij, z = camera.project_points(points)
    rows, cols = np.nonzero(depth > 0)
    assert np.abs(ij[0].numpy() - np.column_stack((cols, rows))).max() < 1e-9 and np.abs(z[0].numpy() - depth[rows, cols]).max() < 1e-12
    mask = np.zeros((24, 32), dtype=bool)
    mask[10, 20] = True
    assert tuple(depth_to_points(depth, camera, mask=mask).shape) == (1, 3)
    half = depth_to_points(depth, camera, mask=mask, integer_pixel_centers=False)
    assert np.abs(camera.project_points(half)[0][0, 0].numpy() - [20.5, 10.5]).max() < 1e-9
    assert isinstance(depth_to_points(depth[None], camera), list)
    with pytest.raises(ValueError, match="the camera has distortion"):
        depth_to_points(depth, DeviceCamera(extrinsic, intrinsic, 24, 32, distortion=[0.1, 0, 0, 0, 0], device="cpu"))
    with pytest.raises(ValueError, match=r"depth must be \[24, 32\]"):
        depth_to_points(depth[:, :30], camera)


def test_fitter_refusals():
    from deodr_amd.pytorch import MeshPointCloudFitter

    vertices, faces = hand()
    make = lambda **kw: MeshPointCloudFitter(vertices, faces, np.zeros(3), np.zeros(3), device="cpu", **kw)
    with pytest.raises(RuntimeError, match="set_point_cloud"):
        make().step()
    with pytest.raises(ValueError, match="directions must be"):
        make(directions="mesh").set_point_cloud(np.zeros((4, 3)))
    with pytest.raises(ValueError, match="max_distance must be > 0"):
        make(max_distance=-1.0).set_point_cloud(np.zeros((4, 3)))
    with pytest.raises(ValueError, match='rigidity must be "laplacian" or "arap"'):
        make(rigidity="rigid")
    with pytest.raises(ValueError, match="526 vertices|vertex weights for 526"):
        f = make()
        f.set_point_cloud(np.random.RandomState(0).rand(9, 3), vertex_weights=np.ones(5))
        f.step()
    f = make()
    assert f.step_factor_vertices == MeshPointCloudFitter.step_factor_vertices * 526 and f.term is None
