"""The colour fit of the hand (examples/rgb_image_hand_fitting.py) with the vertices stepping in the metric ``I + lambda L`` of the mesh Laplacian
(``smoothing=``, deodr_amd/smoothing.py): the vertex gradient of every iteration -- sparse and rough, most of it on silhouettes and shading edges --
is replaced by ``u = (I + lambda L)^-1 g``, sixteen steps of conjugate gradients in one launch on the device, before the clamp and the momentum see it.
``u`` is smaller than ``g`` (its rough part is gone), so the smoothed fit is run with a larger ``step_factor_vertices``.

    python examples/smoothed_hand_fitting.py [--iterations 200] [--smoothing 16] [--step-scale 10] [--eager]

Prints both energy curves, the residual the last solve ended with and the roughness ``sum |L (v - v0)|^2`` of both results.
"""
import argparse

import numpy as np

from _common import golden, run
from ssim_hand_fitting import make_fitter


def main(iterations=200, smoothing=16.0, step_scale=10.0, graph=True):
    import torch

    from deodr_amd.mesh_fitter import GraphedStep

    photograph = golden("rgb_hand_fit.npz")["image_u8"].astype(np.float64) / 255
    curves, fitters = [], []
    for label, keywords, scale in (("plain steps", {}, 1.0), (f"smoothing = {smoothing}, step factor x {step_scale}", dict(smoothing=smoothing), step_scale)):
        fitter = make_fitter(photograph, **keywords)
        fitter.step_factor_vertices = fitter.step_factor_vertices * scale
        stepper = GraphedStep(fitter) if graph else fitter
        curves.append(run(lambda: stepper.step_device()[0], iterations, max(iterations // 10, 1), label))
        fitters.append((label, fitter))
    for label, fitter in fitters:
        moved = fitter.vertices - fitter.vertices_init + (fitter.vertices_init.mean(dim=0) - fitter.vertices.mean(dim=0))
        rough = float((moved * fitter.mesh.topology.laplacian_quadratic(moved)).sum())
        solve = "" if fitter.smoothing_residual is None else f", squared relative residual of the last solve {[float(f'{v:.1e}') for v in fitter.smoothing_residual.tolist()]}"
        print(f"{label}: after {iterations} iterations: roughness of the displacement {rough:.4e}{solve}")
    assert all(torch.isfinite(f.vertices).all() for _, f in fitters)
    return curves


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--smoothing", type=float, default=16.0)
    ap.add_argument("--step-scale", type=float, default=10.0)
    ap.add_argument("--eager", action="store_true", help="launch the kernels of every iteration from the host instead of replaying a HIP graph")
    a = ap.parse_args()
    main(a.iterations, a.smoothing, a.step_scale, not a.eager)
