"""The drop-ins against the reference's single-view PyTorch interface ("drops into mesh_fitter.py").

* ``deodr_amd.pytorch.{CameraPytorch, Scene3DPytorch}`` return what the reference's ``deodr/pytorch/mesh_fitter_pytorch.py`` reads
  from its own classes: shapes, devices, gradients that reach the mesh vertices;
* ``deodr_amd.pytorch`` exports every public name of the reference's ``deodr/pytorch`` package, and its adjacency class computes the
  reference's face normals, vertex normals and silhouette flags (tests/golden/hand_adjacency.npz, written by the reference's
  ``TriMeshAdjacencies``: tests/golden/make_golden.py).

Without a GPU the rasterizer behind the drop-ins is the CPU checker (tests/cpu_raster.py: the one device call of the Scene3D pipeline),
so what is exercised here is the boundary itself: marshalling, shapes, gradient rebinding, devices.  The reference's fit loop written
against the drop-ins, checked against its 50-iteration energy curves (tests/golden/depth_hand_fit.npz), is in tests/test_scene3d.py."""

import os

import numpy as np

from conftest import GOLDEN


def test_single_view_classes_have_the_reference_shapes(oracle_api):
    """render -> [H,W,C], render_depth -> [H,W,1], project_points -> ([V,2], [V]) on the device of the inputs; gradients reach
    mesh.vertices (deodr/pytorch/differentiable_renderer_pytorch.py:13-38, 84-109; callers mesh_fitter_pytorch.py:279-283, 458)"""
    import cpu_raster
    import torch

    import deodr_amd.pytorch.differentiable_renderer_pytorch as ours
    from deodr_amd.scene3d import DeviceMesh

    d = np.load(os.path.join(GOLDEN, "hand_mesh.npz"))
    vertices, faces = d["vertices"], d["faces"]
    checker = oracle_api.ref() or oracle_api.port()
    with cpu_raster.emulate(checker):
        saved = ours._resolve_device
        ours._resolve_device = lambda device: torch.device("cpu")
        try:
            center = vertices.mean(axis=0)
            rot = np.array([[1.0, 0, 0], [0, -1, 0], [0, 0, -1]])
            cam_center = center + np.array([0, 0, 9.0]) * np.max(np.std(vertices, axis=0))
            cam = ours.CameraPytorch(np.column_stack((rot, -rot.T.dot(cam_center))), np.array([[128.0, 0, 32], [0, 128.0, 24], [0, 0, 1]]), 48, 64)
            v = torch.tensor(vertices, requires_grad=True)
            ij, depths = cam.project_points(v)
            assert ij.shape == (len(vertices), 2) and depths.shape == (len(vertices),) and not ij.is_cuda
            scene = ours.Scene3DPytorch()
            mesh = DeviceMesh(faces, v, colors=np.random.RandomState(0).rand(len(vertices), 3), device="cpu")
            scene.set_mesh(mesh)
            scene.set_light(np.array([-0.1, -0.5, -0.4]), 0.6)
            scene.set_background_color([0.5, 0.6, 0.7])
            image, z = scene.render(cam, return_z_buffer=True)
            assert image.shape == (48, 64, 3) and z.shape == (48, 64)
            scene.batched.background_color = None
            scene.set_background_color([1.0])
            depth = scene.render_depth(cam, depth_scale=0.1)
            assert depth.shape == (48, 64, 1)
            (torch.sum(depth**2) + torch.sum(image**2)).backward()  # two renders of one scene in one graph
            assert v.grad is not None and bool(torch.isfinite(v.grad).all()) and float(v.grad.abs().max()) > 0
        finally:
            ours._resolve_device = saved


def test_pytorch_package_exports_the_reference_names():
    """every public name of deodr/pytorch/*.py has a counterpart in deodr_amd.pytorch (differentiable_renderer_pytorch.py:13, 41, 84;
    laplacian_rigid_energy_pytorch.py:25; mesh_fitter_pytorch.py:26, 34, 124, 177, 334; triangulated_mesh_pytorch.py:20, 55), and the
    adjacency class computes the reference's normals"""
    import torch

    import deodr_amd.pytorch as ours

    for name in ("CameraPytorch", "TorchDifferentiableRenderer2DFunc", "Scene3DPytorch", "LaplacianRigidEnergyPytorch", "qrot", "MeshDepthFitterEnergy",
                 "MeshDepthFitterPytorchOptim", "MeshDepthFitter", "MeshRGBFitterWithPose", "TriMeshAdjacenciesPytorch", "ColoredTriMeshPytorch"):  # fmt: skip
        assert hasattr(ours, name), name
    d = np.load(os.path.join(GOLDEN, "hand_mesh.npz"))
    adjacency = ours.TriMeshAdjacenciesPytorch(d["faces"].astype(np.int64), clockwise=False, device="cpu")
    vertices = torch.tensor(d["vertices"])
    face_normals = adjacency.compute_face_normals(vertices)
    vertex_normals = adjacency.compute_vertex_normals(face_normals)
    ref = np.load(os.path.join(GOLDEN, "hand_adjacency.npz"))  # the reference's TriMeshAdjacencies on the same mesh
    assert np.abs(face_normals.numpy() - ref["face_normals"]).max() < 1e-14 and np.abs(vertex_normals.numpy() - ref["vertex_normals"]).max() < 1e-14
    assert np.array_equal(adjacency.edge_on_silhouette(vertices[:, :2]).numpy().astype(bool), ref["edge_on_silhouette"])
