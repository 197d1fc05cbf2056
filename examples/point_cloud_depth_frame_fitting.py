"""The hand fitted to a FULL depth frame with the closest-point term over the uniform grid -- ``MeshPointCloudFitter(search="grid")``
(deodr_amd/chamfer.py, include/deodr_hip_chamfer_grid.h).  A 1280 x 960 depth frame of the hand under a known pose is synthesised (a z-buffer of
eight million samples of its surface through a pinhole camera that lets the hand fill the frame), back-projected to a cloud by
``depth_to_points`` -- more than 10^5 points, every pixel the hand covers -- and the hand is fitted to it from the rest pose:
``directions="points_to_mesh"`` (a depth frame sees one side), truncated at ``max_distance`` = half the hand's standard deviation, which is what
makes the grid exact.  The brute-force search visits 526 x P pairs per iteration; the grid sorts the vertices into cells of
``max(cell_size, max_distance / 4)`` and every point looks around its own cell only.

    python examples/point_cloud_depth_frame_fitting.py [--iterations 100] [--eager] [--search grid] [--device cuda]

Prints the energies, the recovered translation against the known one, and the milliseconds per iteration; ``--search brute`` runs the same fit
with the brute-force search (the same energies up to the order of the gradient's sums).  Measured on an MI355X: 224 662 points, 0.86 ms per
graphed iteration with the grid and 0.67 ms with brute force -- with the hand's 526 vertices this size is still below the crossover (DESIGN.md
4o: the grid wins from about 10 000 vertices against 40 000 points upwards); the example shows the interface at the size of a real frame, and a
denser mesh (``subdivisions``) is where the grid pays."""
import argparse
import time

import numpy as np

from _common import hand_mesh

HEIGHT, WIDTH = 960, 1280  # (the spread hand covers 18 % of a frame it fills: 57 000 pixels of 640 x 480, 227 000 of this one)


def depth_frame(vertices, faces, device, samples=8_000_000):
    """-> (depth [HEIGHT, WIDTH] with 0 where nothing is seen, the camera, the known translation): the hand under the known pose, z-buffered"""
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
    depth = torch.full((HEIGHT * WIDTH,), float("inf"), dtype=camera.dtype, device=camera.device)
    depth.scatter_reduce_(0, (rows * WIDTH + cols)[inside], z[0][inside], reduce="amin")
    depth = torch.where(torch.isfinite(depth), depth, torch.zeros_like(depth)).reshape(HEIGHT, WIDTH)
    return depth, camera, t_true


def main(iterations=100, graph=True, device="cuda", search="grid"):
    import torch

    from deodr_amd.chamfer import depth_to_points
    from deodr_amd.mesh_fitter import GraphedStep
    from deodr_amd.pytorch import MeshPointCloudFitter

    vertices, faces = hand_mesh()
    scale = float(np.std(vertices))
    depth, camera, t_true = depth_frame(vertices, faces, device)
    cloud = depth_to_points(depth, camera)
    print(f"depth frame {WIDTH} x {HEIGHT}: {len(cloud)} points")
    assert len(cloud) >= 100_000
    keywords = dict(search="grid") if search == "grid" else {}
    fitter = MeshPointCloudFitter(vertices, faces, np.zeros(3), np.zeros(3), device=device, directions="points_to_mesh", max_distance=0.5 * scale, **keywords)
    fitter.set_point_cloud(cloud)
    if search == "grid":
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
        print(f'search="{search}": iteration {start + i:4d}  energy {values[i]:.6f}')
    print(f'search="{search}": iteration {start + iterations - 1:4d}  energy {values[-1]:.6f}   ({ms:.3f} ms per iteration)')
    error = float(np.linalg.norm(fitter.transform_translation[0].cpu().numpy() - t_true) / np.linalg.norm(t_true))
    print(f"translation error / |translation| 1 -> {error:.4f}")
    assert np.all(np.isfinite(values)) and values[-1] < values[0]
    return values


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--eager", action="store_true", help="launch the kernels of every iteration from the host instead of replaying a HIP graph")
    ap.add_argument("--search", default="grid", choices=("grid", "brute"))
    ap.add_argument("--device", default="cuda", help='"cpu" runs the torch formulation of the term (slow; implies --eager)')
    a = ap.parse_args()
    main(a.iterations, not a.eager and a.device != "cpu", a.device, a.search)
