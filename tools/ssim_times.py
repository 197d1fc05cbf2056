"""Time of the structural (SSIM) data term (deodr_hip_ssim_l2: terms, loss and image_b in one call) against the same formulas as torch ops
(deodr_amd.ssim.ssim_l2_torch under autograd: ten depthwise conv2d and the elementwise chain, each way) on the same device and tensors, and of a whole
fit iteration with the term computed either way (profiles/README.md, "SSIM loss").

    python tools/ssim_times.py [--launches 100] [--steps 100]

Kernels: device time stamps around `launches` back-to-back calls, after 10 warm-up calls, best of 5 windows: issued from the host one by one
(`call_us`) and replayed as one HIP graph (`graph_us`: what the kernels cost); `estimate_us` is the bytes the two passes have to move (the frames and
the weights read by both, the three maps written and read as doubles, image_b written once) at the copy probe's 6.2 TB/s, `GBps` those bytes over
`graph_us`.  The torch formulas are timed eagerly (`torch_us`) and, where the capture succeeds, as a graph replay too (`torch_graph_us`).  Iteration:
`MeshRGBFitterWithPoseMultiFrame(ssim_weight=0.2)` on views of the hand under `GraphedStep`, `steps` timed replays, with the kernels, with the torch
formulas in their place (render + torch ops + render_backward: what a user could write before the kernels existed), and without the keyword (the
one-call fit step) for scale."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from skin_times import graphed, timed  # noqa: E402

COPY_PROBE_BYTES_PER_US = 6.2e6  # 6.2 TB/s


def kernel_times(launches):
    from deodr_amd import hip_renderer as hr
    from deodr_amd.ssim import ssim_l2_torch

    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(dev).manual_seed(0)
    for (n, H, W, C), dtype, weighted in (((8, 1024, 1024, 4), torch.float32, True), ((8, 1024, 1024, 4), torch.float32, False),
                                          ((8, 1024, 1024, 3), torch.float32, True), ((8, 1024, 1024, 3), torch.float64, True),
                                          ((2, 256, 256, 3), torch.float64, True)):  # fmt: skip
        image, obs = (torch.rand((n, H, W, C), dtype=dtype, device=dev, generator=gen) for _ in range(2))
        weights = torch.rand((n, H, W), dtype=dtype, device=dev, generator=gen) if weighted else None
        mix = torch.tensor([0.8, 0.2], dtype=torch.float64, device=dev)
        scratch = hr.ssim_scratch(n, H, W, C, dev)
        terms, loss, image_b = hr.ssim_l2(image, obs, weights, mix, scratch=scratch)
        both = lambda: hr.ssim_l2(image, obs, weights, mix, terms=terms, loss=loss, image_b=image_b, scratch=scratch)
        value = lambda: hr.ssim_l2(image, obs, weights, mix, terms=terms, loss=loss, scratch=scratch, want_gradient=False)
        leaf = image.clone().requires_grad_(True)

        def torch_ops():
            return torch.autograd.grad(ssim_l2_torch(leaf, obs, weights, mix), leaf)[0]

        reference = torch_ops()
        scale = float(reference.abs().max())
        elem = image.element_size()
        frames = n * H * W * (2 * C + (1 if weighted else 0)) * elem
        moved = 2 * frames + 2 * 24 * n * H * W * C + n * H * W * C * elem
        graph_us = timed(graphed(both), launches)
        few = max(launches // 20, 5)
        call_us, value_us, torch_us = timed(both, launches), timed(graphed(value), launches), timed(torch_ops, few)
        try:
            torch_graph_us = round(timed(graphed(torch_ops), few), 1)
        except Exception as e:  # (a capture the torch ops do not allow: the eager time stands alone)
            torch_graph_us = f"not captured: {type(e).__name__}"
        print(json.dumps(dict(frame=[n, H, W, C], dtype=str(dtype).replace("torch.", ""), weights=weighted, call_us=round(call_us, 1),
                              graph_us=round(graph_us, 1), estimate_us=round(moved / COPY_PROBE_BYTES_PER_US, 1), GBps=round(moved / graph_us / 1e3),
                              value_only_graph_us=round(value_us, 1), torch_us=round(torch_us, 1),
                              torch_graph_us=torch_graph_us,
                              max_diff_of_the_gradients_relative=float((image_b - reference).abs().max()) / scale)), flush=True)  # fmt: skip
        del reference, leaf


def iteration_times(steps, views, size):
    from deodr_amd import ssim
    from deodr_amd.mesh_fitter import GraphedStep
    from test_pyramid_fit_host import hand_fitter

    def per_step(fitter):
        g = GraphedStep(fitter, warmup=3)
        return timed(g.step_device, steps)

    row = dict(views=views, size=size, ssim_weight=0.2)
    row["kernels_us"] = round(per_step(hand_fitter(views, "cuda", torch.float32, shift_pixels=(2, 1), size=size, ssim_weight=0.2)), 1)
    uses_kernel = ssim.uses_kernel
    ssim.uses_kernel = lambda *tensors: False  # the torch formulas in the kernels' place
    try:
        row["torch_ops_us"] = round(per_step(hand_fitter(views, "cuda", torch.float32, shift_pixels=(2, 1), size=size, ssim_weight=0.2)), 1)
    finally:
        ssim.uses_kernel = uses_kernel
    row["plain_l2_fit_step_us"] = round(per_step(hand_fitter(views, "cuda", torch.float32, shift_pixels=(2, 1), size=size)), 1)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    a = ap.parse_args()
    kernel_times(a.launches)
    for views, size in ((8, 256), (8, 1024)):
        iteration_times(a.steps, views, size)
