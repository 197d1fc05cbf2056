"""The colour fit of the hand (examples/rgb_image_hand_fitting.py) from a start translated by about 8 pixels, with the plain L2 data term and with the
multi-scale one (``pyramid_levels=``, deodr_amd/pyramid.py): residuals are also compared after summing over 2 x 2, ..., 2^L x 2^L cells, so a
displacement of several pixels still gives a smooth pull.  The multi-scale fit runs a two-stage schedule: coarse-heavy ``pyramid_weights`` first, then
``[1, 0, ...]`` -- the plain term -- copied into the same device tensor, which the replayed HIP graph reads as it is at each replay.

    python examples/pyramid_hand_fitting.py [--iterations 200] [--levels 4] [--shift 8] [--eager]

Prints both energy curves (each in its own data term) and, for comparison, the plain squared residual of both fits at the end.
"""
import argparse

import numpy as np

from _common import golden, hand_mesh, run


def make_fitter(shift, **keywords):
    from deodr_amd.mesh_fitter import MeshRGBFitterWithPose

    r = golden("rgb_hand_fit.npz")  # hand.png of the reference, the constants of its example
    _vertices, faces = hand_mesh()
    image = r["image_u8"].astype(np.float64) / 255
    fitter = MeshRGBFitterWithPose(r["vertices_centered"], faces, np.zeros(3), r["translation_init"], r["default_color"], r["default_light_directional"],
                                   float(r["default_light_ambient"]), cregu=1000, **keywords)  # fmt: skip
    fitter.set_image(image)
    fitter.set_background_color(r["background_color"])
    # the camera looks down -z from 9 radii with a focal length of 2 * width pixels: `shift` pixels to the right and down
    per_pixel = 9 * fitter.object_radius / (2 * image.shape[1])
    fitter.transform_translation = fitter.transform_translation + fitter.transform_translation.new_tensor([shift * per_pixel, -shift * per_pixel, 0.0]) / np.sqrt(2)
    return fitter


def squared_residual(fitter):
    return float(fitter.diff_image(fitter.render()).sum())


def main(iterations=200, levels=4, shift=8.0, graph=True):
    import torch

    from deodr_amd.mesh_fitter import GraphedStep

    plain = make_fitter(shift)
    stepper = GraphedStep(plain) if graph else plain
    plain_curve = run(lambda: stepper.step_device()[0], iterations, max(iterations // 10, 1), "plain L2")

    # stage 1: the coarse levels carry the weight (level l sums 4^l pixels: 2^-l keeps the levels of one order); stage 2: the plain term
    coarse_heavy = np.array([0.25] + [2.0**-l for l in range(1, levels + 1)])
    fine_only = np.array([1.0] + [0.0] * levels)
    pyramid = make_fitter(shift, pyramid_levels=levels, pyramid_weights=coarse_heavy)
    stepper = GraphedStep(pyramid) if graph else pyramid  # (captured once: the schedule below changes what the replays read, not the graph)
    first = iterations // 2
    stage_1 = run(lambda: stepper.step_device()[0], first, max(first // 5, 1), f"pyramid, levels = {levels}, coarse-heavy")
    pyramid.pyramid_weights.copy_(torch.as_tensor(fine_only))
    stage_2 = run(lambda: stepper.step_device()[0], iterations - first, max((iterations - first) // 5, 1), "pyramid, then [1, 0, ...]")
    print(f"plain squared residual after {iterations} iterations from {shift} pixels off: plain L2 {squared_residual(plain):.3f}, two-stage pyramid {squared_residual(pyramid):.3f}")
    return plain_curve, np.concatenate((stage_1, stage_2))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--shift", type=float, default=8.0)
    ap.add_argument("--eager", action="store_true", help="launch the kernels of every iteration from the host instead of replaying a HIP graph")
    a = ap.parse_args()
    main(a.iterations, a.levels, a.shift, not a.eager)
