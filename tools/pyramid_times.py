"""Time of the multi-scale L2 data term (deodr_hip_pyramid_l2: terms, loss and image_b in one call) against the same formulas as torch ops
(deodr_amd.pyramid.pyramid_l2_torch under autograd) on the same device and tensors, and of a whole fit iteration with the term computed either way
(profiles/README.md, "Pyramid loss").

    python tools/pyramid_times.py [--launches 200] [--steps 200]

Kernels: device time stamps around `launches` back-to-back calls, after 10 warm-up calls, best of 5 windows: issued from the host one by one
(`call_us`) and replayed as one HIP graph (`graph_us`: what the kernels cost); `GBps` is the bytes the passes have to move (the frames read once with
levels <= 3 and twice above, image_b written once) over `graph_us`.  Iteration: `MeshRGBFitterWithPoseMultiFrame(pyramid_levels=...)` on views of the
hand under `GraphedStep`, `steps` timed replays, with the kernels, with the torch formulas in their place (render + torch ops + render_backward: what a
user could write before the kernels existed), and with `pyramid_levels=0` (the one-call fit step) for scale."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from skin_times import graphed, timed  # noqa: E402


def kernel_times(launches):
    from deodr_amd import hip_renderer as hr
    from deodr_amd.pyramid import pyramid_l2_torch

    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(dev).manual_seed(0)
    for (n, H, W, C), dtype, levels, weighted in (((8, 1024, 1024, 4), torch.float32, 3, True), ((8, 1024, 1024, 4), torch.float32, 6, True),
                                                  ((8, 1024, 1024, 4), torch.float32, 6, False), ((8, 1024, 1024, 3), torch.float32, 6, True),
                                                  ((8, 1024, 1024, 3), torch.float64, 6, True), ((2, 256, 256, 3), torch.float64, 5, True)):  # fmt: skip
        image, obs = (torch.rand((n, H, W, C), dtype=dtype, device=dev, generator=gen) for _ in range(2))
        weights = torch.rand((n, H, W), dtype=dtype, device=dev, generator=gen) if weighted else None
        lam = torch.ones(levels + 1, dtype=torch.float64, device=dev)
        scratch = hr.pyramid_scratch(n, H, W, C, levels, dev)
        terms, loss, image_b = hr.pyramid_l2(image, obs, weights, levels, lam, scratch=scratch)
        both = lambda: hr.pyramid_l2(image, obs, weights, levels, lam, terms=terms, loss=loss, image_b=image_b, scratch=scratch)
        value = lambda: hr.pyramid_l2(image, obs, weights, levels, lam, terms=terms, loss=loss, scratch=scratch, want_gradient=False)
        leaf = image.clone().requires_grad_(True)

        def torch_ops():
            return torch.autograd.grad(pyramid_l2_torch(leaf, obs, weights, levels, lam), leaf)[0]

        reference = torch_ops()
        scale = float(reference.abs().max())
        elem = image.element_size()
        frames = n * H * W * (2 * C + (1 if weighted else 0)) * elem
        moved = frames * (1 if levels <= 3 else 2) + n * H * W * C * elem
        graph_us = timed(graphed(both), launches)
        print(json.dumps(dict(frame=[n, H, W, C], dtype=str(dtype).replace("torch.", ""), levels=levels, weights=weighted, call_us=round(timed(both, launches), 1),
                              graph_us=round(graph_us, 1), GBps=round(moved / graph_us / 1e3), value_only_graph_us=round(timed(graphed(value), launches), 1),
                              torch_us=round(timed(torch_ops, max(launches // 20, 5)), 1),
                              max_diff_of_the_gradients_relative=float((image_b - reference).abs().max()) / scale)))  # fmt: skip
        del reference, leaf


def iteration_times(steps, views, size, levels):
    from deodr_amd import pyramid
    from deodr_amd.mesh_fitter import GraphedStep
    from test_pyramid_fit_host import hand_fitter

    def per_step(fitter):
        g = GraphedStep(fitter, warmup=3)
        return timed(g.step_device, steps)

    row = dict(views=views, size=size, levels=levels)
    row["kernels_us"] = round(per_step(hand_fitter(views, "cuda", torch.float32, shift_pixels=(4, 3), size=size, pyramid_levels=levels)), 1)
    uses_kernel = pyramid.uses_kernel
    pyramid.uses_kernel = lambda *tensors: False  # the torch formulas in the kernels' place
    try:
        row["torch_ops_us"] = round(per_step(hand_fitter(views, "cuda", torch.float32, shift_pixels=(4, 3), size=size, pyramid_levels=levels)), 1)
    finally:
        pyramid.uses_kernel = uses_kernel
    row["plain_l2_fit_step_us"] = round(per_step(hand_fitter(views, "cuda", torch.float32, shift_pixels=(4, 3), size=size)), 1)
    print(json.dumps(row))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    kernel_times(a.launches)
    for views, size, levels in ((8, 256, 5), (8, 1024, 6)):
        iteration_times(a.steps, views, size, levels)
