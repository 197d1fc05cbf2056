"""Fit spherical-harmonic lighting and a per-vertex albedo on the device: the hand mesh rendered under known SH lighting (the order-2 coefficients of a
directional + ambient pair, tinted per channel) with a known albedo that varies smoothly over it; start from the coefficients of another light and one
colour for the whole mesh.  One iteration is pose + projection, the front launch (flags, rigid energy), `deodr_hip_sh_shade`, the rasterizer's one-call fit
step, `deodr_hip_sh_shade_b`, the albedo's smoothness term and one momentum update -- replayed as one HIP graph.  Geometry and pose are held, so that
what is printed is the lighting and the albedo.

    python examples/sh_lighting_fitting.py [--iterations 300] [--eager] [--size 256] [--albedo-regu 1.0]
"""
import argparse

import numpy as np

from _common import golden, hand_mesh, run


def main(iterations=300, graph=True, size=256, albedo_regu=1.0):
    import torch

    from deodr_amd import lighting
    from deodr_amd.mesh_fitter import GraphedStep, MeshRGBFitterWithPose

    d = golden("rgb_hand_fit.npz")
    _, faces = hand_mesh()
    vertices, color = d["vertices_centered"], d["default_color"]
    tint = np.array([1.0, 0.9, 0.8])
    sh_true = lighting.sh_from_directional(torch.tensor(d["default_light_directional"]), float(d["default_light_ambient"])).numpy()[:, None] * tint
    sh_start = lighting.sh_from_directional(torch.tensor([0.5, -0.2, -0.6]), 0.3).numpy()[:, None] * np.ones(3)
    albedo_true = np.clip(color[None] * (1 + 0.4 * np.sin(3 * vertices[:, :1] / np.abs(vertices).max()) * np.array([[1.0, -0.5, 0.7]])), 0.05, 1.0)

    def fitter_of(sh, **keywords):
        f = MeshRGBFitterWithPose(vertices, faces, np.zeros(3), d["translation_init"], color, d["default_light_directional"], float(d["default_light_ambient"]),
                                  cregu=1000, light_sh_init=sh, vertex_albedo=True, **keywords)  # fmt: skip
        f.set_background_color(d["background_color"])
        f.set_image(np.zeros((size, size, 3)))
        return f

    truth = fitter_of(sh_true)
    truth.mesh_color = torch.as_tensor(albedo_true, device=truth.device)
    target = truth.render()[0].cpu().numpy()

    fitter = fitter_of(sh_start, albedo_regu=albedo_regu)
    fitter.set_image(target)
    fitter.step_factor_vertices = fitter.step_factor_quaternion = fitter.step_factor_translation = 0.0  # geometry and pose are known here
    scale = (200 / size) ** 2  # the step factors are those of the reference's 200 x 200 photographs: a gradient is a sum over pixels
    fitter.step_factor_light_sh, fitter.step_factor_albedo = 0.0001 * scale, 0.0005 * scale

    def errors():
        sh, albedo = fitter.light_sh.cpu().numpy(), fitter.mesh_color.cpu().numpy()
        # (lighting and albedo share a scale per channel: what the image fixes is their product)
        shading = lambda s, a: a.mean(axis=0) * s[0]
        return f"|sh - truth| {np.abs(sh - sh_true).max():.4f}  |albedo - truth| {np.abs(albedo - albedo_true).mean():.4f}  " \
               f"|mean albedo x sh0 - truth| {np.abs(shading(sh, albedo) - shading(sh_true, albedo_true)).max():.4f}"

    label = f"SH lighting + per-vertex albedo, {size}^2"
    print(f"{label}: start  {errors()}")
    stepper = GraphedStep(fitter) if graph else fitter  # (capturing takes the first five iterations, eager)
    values = run(lambda: stepper.step_device()[0], iterations - fitter.iter, max(1, iterations // 10), label)
    print(f"{label}: end    {errors()}")
    return values


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--albedo-regu", type=float, default=1.0)
    a = ap.parse_args()
    main(a.iterations, not a.eager, a.size, a.albedo_regu)
