"""Time of linear blend skinning, forward + adjoint (deodr_hip_skin_apply + deodr_hip_skin_apply_b with all three gradients), against the same
formulas as torch ops (deodr_amd.skinning.skin_torch under autograd) on the same device and tensors (profiles/README.md, "Linear blend skinning").

    python tools/skin_times.py [--launches 200]

Device time stamps around `launches` back-to-back forward + adjoint pairs, after 10 warm-up pairs, best of 5 windows: issued from the host one by one
(`kernels_us`: five launches with their argument checks, host-bound), and the same five launches replayed as one HIP graph (`graph_us`: what the
kernels cost).  The torch side is what a user has without the kernels; its time is dominated by the number of small launches, which grows with the
number of joints."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(call, launches):
    """-> microseconds per call"""
    for _ in range(10):
        call()
    best = float("inf")
    for _ in range(5):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(launches):
            call()
        stop.record()
        stop.synchronize()
        best = min(best, start.elapsed_time(stop) / launches * 1e3)
    return best


def graphed(call):
    """-> the replay of `call` captured in a HIP graph"""
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        call()
    return graph.replay


def chain_rig(vertices, J, K, seed=0):
    """J joints spread along the longest axis of the mesh, a chain; every vertex weighted by its K nearest joints"""
    rs = np.random.RandomState(seed)
    v = vertices - vertices.mean(axis=0)
    axis = int(np.argmax(np.ptp(v, axis=0)))
    joints = np.zeros((J, 3))
    joints[:, axis] = np.linspace(v[:, axis].min(), v[:, axis].max(), J + 2)[1:-1]
    K = min(K, J)
    distance = np.abs(v[:, axis, None] - joints[None, :, axis])
    indices = np.argsort(distance, axis=1)[:, :K]
    weights = 1.0 / (np.take_along_axis(distance, indices, axis=1) + 0.05 * np.ptp(v[:, axis]))
    weights /= weights.sum(axis=1, keepdims=True)
    return v, joints, np.array([-1] + list(range(J - 1))), indices, weights, rs


def main(launches):
    import skinning_reference as sr
    from deodr_amd import hip_renderer as hr
    from deodr_amd.skinning import Skin, skin_torch

    dev = torch.device("cuda", torch.cuda.current_device())
    hand = sr.hand()[0]
    rs = np.random.RandomState(1)
    sphere = rs.randn(10002, 3)
    sphere /= np.linalg.norm(sphere, axis=1, keepdims=True)
    for name, vertices, J, K, n in (("hand", hand, 4, 4, 1), ("hand", hand, 4, 4, 8), ("hand", hand, 16, 4, 1), ("hand", hand, 16, 4, 8),
                                    ("10 002 vertices", sphere, 16, 4, 1), ("10 002 vertices", sphere, 16, 4, 8)):  # fmt: skip
        v, joints, parents, indices, weights, rs = chain_rig(vertices, J, K)
        skin = Skin(joints, parents, (indices, weights), device=dev)
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
        vt, q, g = t(v), t(rs.randn(n, J, 4)), t(rs.randn(n, skin.V, 3))
        world, posed = hr.skin_apply(vt, skin.joints, skin.parents, q, skin.indices, skin.weights)
        outs = hr.skin_apply_b(vt, skin.joints, skin.parents, q, skin.indices, skin.weights, world, g, skin.joint_offsets, skin.joint_slots)
        scratch = hr.skin_scratch(skin.V, skin.J, skin.K, n, dev)

        def kernels():
            hr.skin_apply(vt, skin.joints, skin.parents, q, skin.indices, skin.weights, world=world, posed=posed)
            hr.skin_apply_b(vt, skin.joints, skin.parents, q, skin.indices, skin.weights, world, g, skin.joint_offsets, skin.joint_slots,
                            vertices_b=outs[0], quaternions_b=outs[1], joints_b=outs[2], scratch=scratch)  # fmt: skip

        leaves = [x.clone().requires_grad_(True) for x in (vt, q, skin.joints)]

        def torch_ops():
            out = skin_torch(leaves[0], leaves[1], leaves[2], skin.parents_np, skin._indices_long, skin.weights)
            return torch.autograd.grad(out, leaves, g)

        reference = torch_ops()
        diff = max(float((a - b).abs().max()) for a, b in zip(outs, reference))
        print(json.dumps(dict(mesh=name, V=skin.V, J=J, K=skin.K, n=n, kernels_us=round(timed(kernels, launches), 2),
                              graph_us=round(timed(graphed(kernels), launches), 2),
                              torch_us=round(timed(torch_ops, max(launches // 10, 5)), 1), max_abs_diff_of_the_gradients=diff)))  # fmt: skip


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    main(ap.parse_args().launches)
