"""Calibrate the cameras of a ring of views of a known mesh, on the device: the hand mesh, `--views` photographs rendered from ground-truth cameras (one
physical camera with OpenCV distortion, `deodr_amd.scenes.calibration_scene`), start from perturbed extrinsics, focal lengths and distortion.  One
iteration is `deodr_hip_camera_assemble`, the projection, the silhouette flags, the rasterizer's one-call fit step, `deodr_hip_camera_project_b`,
`deodr_hip_camera_assemble_b` and one momentum update -- replayed as one HIP graph.  Prints the parameter errors every 10 iterations.

    python examples/camera_calibration.py [--iterations 100] [--eager] [--size 256] [--views 6] [--update extrinsic,focal,distortion]

The principal point is left out of `--update` by default: with the object in the middle of every frame a shift of the principal point is (almost) a
rotation of the camera, and the fit slides along that valley instead of coming back.
"""
import argparse

import numpy as np

from _common import hand_mesh


def main(iterations=100, graph=True, size=256, views=6, update=("extrinsic", "focal", "distortion")):
    import torch
    from scipy.spatial.transform import Rotation

    from deodr_amd import scenes
    from deodr_amd.mesh_fitter import CameraFitterMultiFrame, GraphedStep

    dev = torch.device("cuda", torch.cuda.current_device())
    vertices, faces = hand_mesh()
    vertices = vertices - vertices.mean(axis=0)
    problem = scenes.calibration_scene(vertices, views, size)
    truth, start = problem["truth"], problem["start"]
    groups = {"quaternions": "extrinsic", "translations": "extrinsic", "focal": "focal", "center": "center", "distortion": "distortion"}
    start = {k: (start[k] if groups[k] in update else truth[k]) for k in start}  # what does not move is known
    colors, light, ambient, background = np.tile([0.8, 0.6, 0.5], (len(vertices), 1)), np.array([-0.3, -0.4, -0.6]), 0.4, np.array([0.1, 0.2, 0.3])

    def fitter_of(p, moving):
        f = CameraFitterMultiFrame(vertices, faces, p["quaternions"], p["translations"], p["focal"], p["center"], p["distortion"], colors=colors,
                                   light_directional=light, light_ambient=ambient, update=moving, device=dev)  # fmt: skip
        f.set_background_color(background)
        return f

    camera_of_truth = fitter_of(truth, ())
    camera_of_truth.set_images(np.zeros((views, size, size, 3)))
    photographs = camera_of_truth.gradients()[1].cpu().numpy()  # the ground truth through the same renderer

    fitter = fitter_of(start, update)
    fitter.set_images(photographs)
    frame = lambda q, t: np.einsum("nij,vj->nvi", Rotation.from_quat(q).as_matrix(), vertices) + t[:, None, :]

    def errors():
        get = lambda k: getattr(fitter, k).cpu().numpy()
        e = np.linalg.norm(frame(get("quaternions"), get("translations")) - frame(truth["quaternions"], truth["translations"]), axis=-1).mean(axis=1).max()
        return f"extrinsic {e:.5f} (mean vertex distance)  focal {np.abs(get('focal') - truth['focal']).max():.4f} px  " \
               f"center {np.abs(get('center') - truth['center']).max():.4f} px  distortion {np.abs(get('distortion') - truth['distortion']).max():.5f}"

    label = f"camera calibration, {views} views of {size}^2, moving {', '.join(update)}"
    print(f"{label}: start           energy {float(fitter.energy()):.6f}  {errors()}")
    stepper = GraphedStep(fitter) if graph else fitter  # (capturing takes the first five iterations, eager)
    energies = []
    for i in range(fitter.iter, iterations):
        if i % 10 == 0:
            print(f"{label}: iteration {i:4d}  energy {float(fitter.energy()):.6f}  {errors()}")
        energies.append(stepper.step_device()[0].clone())
    print(f"{label}: iteration {iterations:4d}  energy {float(fitter.energy()):.6f}  {errors()}")
    return torch.stack(energies).cpu().numpy()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--update", default="extrinsic,focal,distortion")
    a = ap.parse_args()
    main(a.iterations, not a.eager, a.size, a.views, tuple(g for g in a.update.split(",") if g))
