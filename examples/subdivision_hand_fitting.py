"""Fit the control cage of a Loop subdivision surface to a depth image: the fit of examples/depth_image_hand_fitting.py with
``subdivisions=1`` -- the 526 vertices of the hand mesh are the cage (the parameter, with the Laplacian rigid energy on it), what is posed,
projected and rasterized is the subdivided mesh S cage (2 098 vertices, 4 192 triangles; ``--subdivisions 2``: 8 386 and 16 768).  S and
its adjoint S^T are one kernel launch each (include/deodr_hip_subdiv.h); the iteration is replayed as one HIP graph.

    python examples/subdivision_hand_fitting.py [--iterations 100] [--subdivisions 1] [--eager] [--save out.npz]
"""
import argparse

import numpy as np

from _common import golden, hand_mesh, run


def main(iterations=100, subdivisions=1, graph=True, save=None):
    from deodr_amd.mesh_fitter import GraphedStep, MeshDepthFitter

    d = golden("depth_hand_fit.npz")
    depth = d["depth_raw_f32"].astype(np.float64)
    max_depth = float(d["max_depth"])
    depth[depth == 0] = max_depth
    vertices, faces = hand_mesh()
    fitter = MeshDepthFitter(vertices, faces, d["euler_init"], d["translation_init"], cregu=1000, subdivisions=subdivisions)
    fitter.set_image(depth / max_depth, focal=241, distortion=d["distortion"])
    fitter.set_max_depth(1)
    fitter.set_depth_scale(float(d["depth_scale"]))
    print(f"cage: {fitter.control_mesh.nb_vertices} vertices; rendered: {fitter.mesh.nb_vertices} vertices, {fitter.mesh.nb_faces} triangles")
    stepper = GraphedStep(fitter) if graph else fitter  # (GraphedStep runs iterations 0 .. 4 eagerly while it sets itself up)
    energies = run(lambda: stepper.step_device()[0], iterations, max(iterations // 10, 1), "subdivided depth fit")
    if save:
        _e, depth_image, diff_image = stepper.step_device()
        surface = fitter.subdivision.apply(fitter.vertices) if subdivisions else fitter.vertices
        np.savez(save, energies=energies, cage=fitter.vertices.cpu().numpy(), surface=surface.cpu().numpy(), faces=fitter.mesh.faces_np,
                 depth=depth_image.cpu().numpy(), diff=diff_image.cpu().numpy())  # fmt: skip
    return energies


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--subdivisions", type=int, default=1)
    ap.add_argument("--eager", action="store_true", help="launch the kernels of every iteration from the host instead of replaying a HIP graph")
    ap.add_argument("--save", default=None)
    a = ap.parse_args()
    main(a.iterations, a.subdivisions, not a.eager, a.save)
