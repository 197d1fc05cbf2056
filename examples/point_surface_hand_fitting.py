"""The hand fitted to a cloud that is DENSER than the mesh, with the point-to-surface term (deodr_amd/surface.py,
``deodr_amd.pytorch.MeshPointCloudFitter(metric="surface")``) beside the point-to-vertex term of examples/point_cloud_hand_fitting.py.

The target: 4 000 area-uniform samples of the hand's own surface (526 vertices, 1 048 faces) under a known pose.  Against the VERTICES such a
cloud has a floor it cannot go under -- a sample in the middle of a large triangle is far from all three corners, pays for it and pulls on
them, and the fit trades that pull off against the rigid energy --; against the SURFACE a sample of a face that is in place costs nothing.  Both
fits run with the same step factors (``MeshPointCloudFitter``'s docstring says why they carry over); the recovered translation is printed against
the known one for both.

    python examples/point_surface_hand_fitting.py [--iterations 150] [--points 4000] [--eager] [--device cuda]

Per iteration with ``metric="surface"``: the pose, ``deodr_hip_surface_distance`` (six launches: the face records, the point-major search over
them and its combine step, the face-major gather, the vertex-major search of the Chamfer operator, the per-vertex combine step), the rigid
energy, one momentum update; replayed as one HIP graph."""
import argparse

import numpy as np

from _common import hand_mesh
from point_cloud_hand_fitting import iterate


def main(iterations=150, points=4000, graph=True, device="cuda"):
    import torch

    from deodr_amd.mesh_fitter import _quat_from_euler_zyx, qrot
    from deodr_amd.pytorch import MeshPointCloudFitter
    from deodr_amd.surface import sample_surface

    vertices, faces = hand_mesh()
    scale = float(np.std(vertices))
    t_true = np.array([0.3, -0.2, 0.5]) * scale
    q = torch.as_tensor(_quat_from_euler_zyx(np.array([0.1, -0.15, 0.2])))
    posed = qrot(q[None], torch.as_tensor(vertices - vertices.mean(axis=0))[None])[0].numpy() + t_true
    cloud = sample_surface(posed, faces, points, seed=0)[0]
    print(f"{len(cloud)} samples of the surface of {len(vertices)} vertices, {len(faces)} faces")
    results = {}
    for metric in ("surface", "vertex"):
        fitter = MeshPointCloudFitter(vertices, faces, np.zeros(3), np.zeros(3), device=device, metric=metric)
        fitter.set_point_cloud(cloud)
        energies = iterate(fitter, iterations, f"metric={metric}", graph)
        error = float(np.linalg.norm(fitter.transform_translation[0].cpu().numpy() - t_true) / np.linalg.norm(t_true))
        print(f"metric={metric}: translation error / |translation| 1 -> {error:.4f}")
        assert np.all(np.isfinite(energies)) and energies[-1] < energies[0]
        results[metric] = (energies, error)
    fitter = MeshPointCloudFitter(vertices, faces, np.zeros(3), np.zeros(3), device=device, metric="surface")
    fitter.set_point_cloud(cloud)
    nearest_face, barycentric, _ = fitter.term.correspondences(torch.as_tensor(posed, device=fitter.vertices.device)[None])
    print(f"at the true pose {len(torch.unique(nearest_face))} of {len(faces)} faces are the closest one of some sample; "
          f"the smallest barycentric coordinate is {float(barycentric.min()):.2e}")  # fmt: skip
    return results


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=150)
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--eager", action="store_true", help="launch the kernels of every iteration from the host instead of replaying a HIP graph")
    ap.add_argument("--device", default="cuda", help='"cpu" runs the torch formulation of the term (slow; implies --eager)')
    a = ap.parse_args()
    main(a.iterations, a.points, not a.eager and a.device != "cpu", a.device)
