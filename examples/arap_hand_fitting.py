"""The colour fit of the hand (examples/rgb_image_hand_fitting.py) under the two regularisers: the reference's Laplacian energy
``0.5 c d^T (L^T L) d`` of the displacement ``d`` (``rigidity="laplacian"``, the default) and the as-rigid-as-possible energy of Sorkine and Alexa
(``rigidity="arap"``, deodr_amd/arap.py), which gives every vertex the rotation that best maps its rest one-ring onto its current one and charges
only what that rotation cannot explain -- a finger that bends is not charged as if it stretched.  Two launches of ``deodr_hip_arap_energy`` inside
the autograd graph, the iteration replayed as one HIP graph.

    python examples/arap_hand_fitting.py [--iterations 200] [--cregu 3500] [--weights uniform] [--eager]

``cregu`` does not have the Laplacian energy's scale.  The default here was not tuned on a result; it is the value at which ONE displaced vertex of
valence ``v = 6`` costs what it costs under the Laplacian energy at the example's ``cregu = 1000``: there ``0.5 c (v^2 + v) |d|^2``, here
``c v |d|^2`` (the rotations held), a ratio of ``(v + 1) / 2 = 3.5``.

Prints both energy curves, and of both results the data term, the Laplacian energy and the ARAP energy of the displacement (each at cregu = 1).
"""
import argparse

import numpy as np

from _common import golden, run
from ssim_hand_fitting import make_fitter


def main(iterations=200, cregu=3500.0, weights="uniform", graph=True):
    import torch

    from deodr_amd.arap import ArapEnergyDevice
    from deodr_amd.mesh_fitter import GraphedStep

    photograph = golden("rgb_hand_fit.npz")["image_u8"].astype(np.float64) / 255
    curves, fitters = [], []
    for label, keywords in (("rigidity = laplacian, cregu = 1000", {}), (f"rigidity = arap, cregu = {cregu:g}, {weights} weights", dict(rigidity="arap", arap_weights=weights))):
        fitter = make_fitter(photograph, **keywords)
        if keywords:
            fitter.cregu = fitter.rigid_energy.cregu = float(cregu)
        stepper = GraphedStep(fitter) if graph else fitter
        curves.append(run(lambda: stepper.step_device()[0], iterations, max(iterations // 10, 1), label))
        fitters.append((label, fitter))
    for label, fitter in fitters:
        moved = fitter.vertices - fitter.vertices_init + (fitter.vertices_init.mean(dim=0) - fitter.vertices.mean(dim=0))
        laplacian = 0.5 * float((moved * fitter.mesh.topology.laplacian_quadratic(moved)).sum())
        arap = ArapEnergyDevice(fitter.mesh.topology, fitter.vertices_init, 1.0, weights)
        with torch.no_grad():
            e_arap = float(arap.evaluate(fitter.vertices_init + moved)[0])
        print(f"{label}: after {iterations} iterations: Laplacian energy of the displacement {laplacian:.4e}, ARAP energy {e_arap:.4e} (both at cregu = 1)")
    assert all(torch.isfinite(f.vertices).all() for _, f in fitters)
    return curves


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--cregu", type=float, default=3500.0)
    ap.add_argument("--weights", default="uniform", choices=("uniform", "cotangent"))
    ap.add_argument("--eager", action="store_true", help="launch the kernels of every iteration from the host instead of replaying a HIP graph")
    a = ap.parse_args()
    main(a.iterations, a.cregu, a.weights, not a.eager)
