"""The subdivided hand fitted to a whole VGA depth frame with the point-to-SURFACE term over the uniform grid of triangles --
``MeshPointCloudFitter(metric="surface", surface_search="grid")`` (deodr_amd/surface.py, include_staged/deodr_hip_surface_grid.h).  A 640 x 480
depth frame is synthesised: the hand under a known pose in front of a wall, z-buffered through a pinhole camera, so EVERY pixel has a depth;
``depth_to_points`` back-projects all 307 200 of them.  The mesh that meets the cloud is the hand after ``subdivisions=2``: 16 768 faces.  That is
5.2e9 (point, face) pairs, above the cap of the brute-force surface term (2^32), which refuses it; the grid keys every face by one cell and every
point looks around its own cell only.  ``directions="points_to_mesh"`` (a depth frame sees one side), truncated at ``max_distance`` = half
the hand's standard deviation: the wall's points find no face within it, pay the constant and pull nothing.

    python examples/point_surface_depth_frame_fitting.py [--iterations 60] [--eager] [--device cuda]

Prints the energies, the share of the points with a face within ``max_distance`` at the end, the recovered translation against the known one,
and the milliseconds per iteration.  Measured on an MI355X: 23.6 ms per graphed iteration, 18.5 % of the frame's points within ``max_distance`` of the
hand at the end.  The hand's mesh has a few triangles a dozen mean edges long, and the cell edge of the face grid is never below the longest
side of a face's bounding box, so this mesh is the grid's slow case (an evenly triangulated sphere of the same size against the
same number of points takes 4 ms per call); it is shown because it is the size the brute-force term cannot run at all."""
import argparse
import time

import numpy as np

from _common import hand_mesh

HEIGHT, WIDTH = 480, 640


def depth_frame(vertices, faces, device, samples=4_000_000):
    """-> (depth [HEIGHT, WIDTH], every pixel seen: the hand under the known pose, z-buffered, or the wall behind it; the camera; the known
    translation)"""
    import torch

    from deodr_amd.mesh_fitter import _quat_from_euler_zyx, qrot
    from deodr_amd.scene3d import DeviceCamera
    from deodr_amd.surface import sample_surface

    scale = float(np.std(vertices))
    t_true = np.array([0.3, -0.2, 0.5]) * scale
    q = torch.as_tensor(_quat_from_euler_zyx(np.array([0.1, -0.15, 0.2])))
    posed = qrot(q[None], torch.as_tensor(vertices - vertices.mean(axis=0))[None])[0].numpy() + t_true
    turn = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])  # the camera on its side: the hand's long axis along the frame's width
    seen = posed @ turn.T
    centre, extent = (seen.max(axis=0) + seen.min(axis=0))[:2] / 2, (seen.max(axis=0) - seen.min(axis=0))[:2] / 2
    distance = 12.0 * scale
    focal = 0.49 * min(WIDTH / extent[0], HEIGHT / extent[1]) * (distance + seen[:, 2].min())  # the nearest part still inside the frame
    extrinsic = np.column_stack((turn, [-centre[0], -centre[1], distance]))
    intrinsic = np.array([[focal, 0, (WIDTH - 1) / 2], [0, focal, (HEIGHT - 1) / 2], [0, 0, 1]])
    camera = DeviceCamera(extrinsic, intrinsic, HEIGHT, WIDTH, None, device)
    points = torch.as_tensor(sample_surface(posed, faces, samples)[0], dtype=camera.dtype, device=camera.device)
    ij, z = camera.project_points(points)
    cols, rows = torch.round(ij[0, :, 0]).long(), torch.round(ij[0, :, 1]).long()
    inside = (cols >= 0) & (cols < WIDTH) & (rows >= 0) & (rows < HEIGHT)
    wall = distance + seen[:, 2].max() + 3.0 * scale  # three standard deviations behind the farthest part of the hand
    depth = torch.full((HEIGHT * WIDTH,), float(wall), dtype=camera.dtype, device=camera.device)
    depth.scatter_reduce_(0, (rows * WIDTH + cols)[inside], z[0][inside], reduce="amin")
    return depth.reshape(HEIGHT, WIDTH), camera, t_true


def main(iterations=60, graph=True, device="cuda"):
    import torch

    from deodr_amd import hip_renderer as hr
    from deodr_amd.chamfer import depth_to_points
    from deodr_amd.mesh_fitter import GraphedStep
    from deodr_amd.pytorch import MeshPointCloudFitter

    vertices, faces = hand_mesh()
    scale = float(np.std(vertices))
    depth, camera, t_true = depth_frame(vertices, faces, device)
    cloud = depth_to_points(depth, camera)
    assert len(cloud) == HEIGHT * WIDTH
    fitter = MeshPointCloudFitter(vertices, faces, np.zeros(3), np.zeros(3), device=device, metric="surface", surface_search="grid", subdivisions=2,
                                  directions="points_to_mesh", max_distance=0.5 * scale)  # fmt: skip
    fitter.set_point_cloud(cloud)
    F, P = fitter.term.nb_faces, fitter.term.nb_points
    print(f"depth frame {WIDTH} x {HEIGHT}: {P} points against {F} faces, {F * P:.2e} pairs (the brute-force cap is {hr.SURFACE_MAX_PAIRS:.2e})")
    assert F * P > hr.SURFACE_MAX_PAIRS
    print(f"cell_size {fitter.term.cell_size:.4f} (the cloud's default), max_distance {0.5 * scale:.4f}")
    stepper = GraphedStep(fitter) if graph else fitter
    start = fitter.iter
    if device != "cpu":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    energies = [stepper.step_device()[0].detach().clone() for _ in range(iterations)]
    if device != "cpu":
        torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / iterations * 1e3
    values = torch.stack(energies).cpu().numpy()
    for i in range(0, iterations, max(iterations // 10, 1)):
        print(f"iteration {start + i:4d}  energy {values[i]:.6f}")
    print(f"iteration {start + iterations - 1:4d}  energy {values[-1]:.6f}   ({ms:.3f} ms per iteration)")
    face = fitter.term.correspondences(fitter.energy()[4].detach())[0]  # (the posed vertices that meet the cloud: the subdivided ones)
    print(f"points with a face within max_distance: {float((face >= 0).double().mean()):.3f} of the frame")
    error = float(np.linalg.norm(fitter.transform_translation[0].cpu().numpy() - t_true) / np.linalg.norm(t_true))
    print(f"translation error / |translation| 1 -> {error:.4f}")
    assert np.all(np.isfinite(values)) and values[-1] < values[0]
    return values


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=60)
    ap.add_argument("--eager", action="store_true", help="launch the kernels of every iteration from the host instead of replaying a HIP graph")
    ap.add_argument("--device", default="cuda", help='"cpu" runs the torch formulation of the term (very slow at this size; implies --eager)')
    a = ap.parse_args()
    main(a.iterations, not a.eager and a.device != "cpu", a.device)
