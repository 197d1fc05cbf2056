"""The hand fitted to unorganised 3-D points with the closest-point (Chamfer) term -- no camera, no render (deodr_amd/chamfer.py,
``deodr_amd.pytorch.MeshPointCloudFitter``).  Two targets:

1. the reference's depth image of the hand (examples/depth_image_hand_fitting.py), back-projected to a cloud by ``depth_to_points`` through the
   pinhole camera of that example WITHOUT its distortion (a distorted projection has no closed-form inverse; the cloud is bent by up to a pixel or
   two at the border, which a fit with a deformable mesh absorbs).  A depth image sees one side of the hand: ``directions="points_to_mesh"`` --
   every point pulls its nearest vertex, the vertices of the far side are free --, truncated at ``max_distance`` = the hand's standard deviation.
2. 400 of the hand's own vertices under a known pose, both directions: the recovered translation is printed against the known one.

    python examples/point_cloud_hand_fitting.py [--iterations 150] [--eager] [--device cuda]

Per iteration: the pose, ``deodr_hip_chamfer`` (four launches: two tiled brute-force searches, their combine steps; the gradient is gathered in the
second walk), the rigid energy, one momentum update; replayed as one HIP graph.  The step factors are the fitter's defaults, which were chosen on
target 2 (``MeshPointCloudFitter``'s docstring says how)."""
import argparse

import numpy as np

from _common import golden, hand_mesh


def iterate(fitter, iterations, label, graph):
    import torch

    from deodr_amd.mesh_fitter import GraphedStep

    stepper = GraphedStep(fitter) if graph else fitter
    start = fitter.iter
    energies = [stepper.step_device()[0].detach().clone() for _ in range(iterations)]
    values = torch.stack(energies).cpu().numpy()
    for i in range(0, iterations, max(iterations // 10, 1)):
        print(f"{label}: iteration {start + i:4d}  energy {values[i]:.6f}")
    print(f"{label}: iteration {start + iterations - 1:4d}  energy {values[-1]:.6f}")
    return values


def depth_cloud(device):
    """the reference's depth image as points in the frame the depth fitter poses the hand in"""
    from deodr_amd.chamfer import depth_to_points
    from deodr_amd.mesh_fitter import _default_camera
    from deodr_amd.scene3d import DeviceCamera

    d = golden("depth_hand_fit.npz")
    depth = d["depth_raw_f32"].astype(np.float64)
    vertices, _ = hand_mesh()
    centre, radius = vertices.mean(axis=0), float(np.max(np.std(vertices, axis=0)))
    height, width = depth.shape
    camera = DeviceCamera(*_default_camera(height, width, 241, centre + np.array([-0.5, 0, 5]) * radius), height, width, None, device)
    valid = (depth > 0) & (depth < float(d["max_depth"]))
    z = depth / float(d["max_depth"]) / float(d["depth_scale"])  # (the fitter renders depth_scale * z against depth / max_depth)
    return depth_to_points(z, camera, mask=valid), d


def main(iterations=150, graph=True, device="cuda"):
    import torch

    from deodr_amd.pytorch import MeshPointCloudFitter

    vertices, faces = hand_mesh()
    scale = float(np.std(vertices))
    cloud, d = depth_cloud(device)
    print(f"depth image: {len(cloud)} points")
    fitter = MeshPointCloudFitter(vertices, faces, d["euler_init"], d["translation_init"], device=device, directions="points_to_mesh", max_distance=scale)
    fitter.set_point_cloud(cloud)
    scan = iterate(fitter, iterations, "depth image, points -> mesh", graph)
    fitter._leaves()  # (the parameters as they are now)
    nearest_vertex, _ = fitter.term.correspondences(fitter._transformed(fitter.vertices_leaf).detach())
    print(f"depth image: {len(torch.unique(nearest_vertex))} of {len(vertices)} vertices are the nearest one of some point")

    from deodr_amd.mesh_fitter import _quat_from_euler_zyx, qrot

    t_true = np.array([0.3, -0.2, 0.5]) * scale
    q = torch.as_tensor(_quat_from_euler_zyx(np.array([0.1, -0.15, 0.2])))
    posed = qrot(q[None], torch.as_tensor(vertices - vertices.mean(axis=0))[None])[0].numpy() + t_true
    fitter = MeshPointCloudFitter(vertices, faces, np.zeros(3), np.zeros(3), device=device)
    fitter.set_point_cloud(posed[np.random.RandomState(0).permutation(len(vertices))[:400]])
    own = iterate(fitter, iterations, "400 own vertices, both directions", graph)
    error = float(np.linalg.norm(fitter.transform_translation[0].cpu().numpy() - t_true) / np.linalg.norm(t_true))
    print(f"400 own vertices: translation error / |translation| 1 -> {error:.4f}")
    assert np.all(np.isfinite(scan)) and np.all(np.isfinite(own)) and scan[-1] < scan[0] and own[-1] < own[0]
    return scan, own


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=150)
    ap.add_argument("--eager", action="store_true", help="launch the kernels of every iteration from the host instead of replaying a HIP graph")
    ap.add_argument("--device", default="cuda", help='"cpu" runs the torch formulation of the term (slow; implies --eager)')
    a = ap.parse_args()
    main(a.iterations, not a.eager and a.device != "cpu", a.device)
