"""Fit the pose of a skeleton to a depth image: the hand mesh with a synthetic chain of four joints (tests/skinning_reference.py::hand_rig: cuts
through palm and fingers, two influences per vertex), a target rendered from known joint rotations, and ``MeshDepthFitter(..., skin=)`` looking for
them from the rest pose with geometry and rigid pose held.  Linear blend skinning is two launches forward and three backward
(include/deodr_hip_skinning.h); the iteration runs through autograd and is replayed as one HIP graph.

    python examples/skinned_hand_fitting.py [--iterations 150] [--size 64] [--eager]
"""
import argparse
import os
import sys

import numpy as np

from _common import ROOT, golden, run

sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(iterations=150, size=64, graph=True):
    import torch

    import skinning_reference as sr
    from deodr_amd.mesh_fitter import GraphedStep, MeshDepthFitter
    from deodr_amd.skinning import Skin

    d = golden("depth_hand_fit.npz")
    vertices, faces, joints, parents, weights = sr.hand_rig(measured_from="far")
    rig = Skin(joints, parents, weights)
    fitter = MeshDepthFitter(vertices, faces, d["euler_init"], d["translation_init"], cregu=1000, skin=rig)
    fitter.set_max_depth(1)
    fitter.set_depth_scale(float(d["depth_scale"]))
    focal = 241.0 * size / 200
    # the target: the fitter's own model at the joint rotations to be found
    q_true = torch.as_tensor(sr.hand_target_quaternions(), device=fitter.joint_quaternions.device)
    fitter.set_image(np.ones((size, size)), focal=focal)
    fitter.joint_quaternions = q_true
    fitter._leaves()
    with torch.no_grad():
        target = fitter.energy()[3].cpu().numpy()
    fitter.reset()
    fitter.set_image(target, focal=focal)
    fitter.step_factor_vertices = fitter.step_factor_quaternion = fitter.step_factor_translation = 0.0  # geometry and rigid pose held
    fitter.step_factor_joints = 1e-4 * (64 / size) ** 2  # (the data gradient is a sum over the pixels)
    distance = lambda: float((1 - (fitter.joint_quaternions * q_true).sum(dim=1).abs()).max())
    print(f"{rig.J} joints, {rig.K} influences per vertex, {rig.V} vertices; largest 1 - |<q, q_true>| at the start: {distance():.5f}")
    stepper = GraphedStep(fitter) if graph else fitter  # (GraphedStep runs iterations 0 .. 4 eagerly while it sets itself up)
    energies = run(lambda: stepper.step_device()[0], iterations, max(iterations // 10, 1), "skinned depth fit")
    print(f"largest 1 - |<q, q_true>| at the end: {distance():.5f}")
    return energies


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=150)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--eager", action="store_true", help="launch the kernels of every iteration from the host instead of replaying a HIP graph")
    a = ap.parse_args()
    main(a.iterations, a.size, not a.eager)
