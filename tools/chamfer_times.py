"""Time of the closest-point (Chamfer) term (deodr_hip_chamfer: four launches, two with mesh -> points alone) against the same definition as torch
ops (deodr_amd.chamfer.chamfer_torch, eager, chunked to 64 MB of distances) on the same device and tensors, and of a whole iteration of
``MeshPointCloudFitter`` on the hand under ``GraphedStep`` (profiles/README.md, "Closest-point term").

    python tools/chamfer_times.py [--launches 20] [--steps 100] [--no-torch]

Sizes: (V, P) = (526, 4 096), (526, 40 000), (10 002, 40 000); n = 1 and 8 poses; both directions and points -> mesh alone.  Points and vertices
uniform in the unit cube.  Device time stamps around `launches` back-to-back replays of the call captured as one HIP graph (`graph_us`: what the
kernels cost) and around calls issued from the host one by one (`call_us`), after 10 warm-up calls, best of 5 windows; the torch ops run eager
(`torch_us`, a tenth of the launches).  Then the ratio of the adversarial distribution -- every point nearest ONE vertex -- to the uniform one at
(10 002, 40 000), both directions, n = 1: the gather is a compare per pair wherever the points fall, so it is expected near 1."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES = ((526, 4096), (526, 40000), (10002, 40000))


def problem(V, P, n, dev, adversarial=False):
    g = torch.Generator(dev).manual_seed(V + P + n)
    v = torch.rand((n, V, 3), dtype=torch.float64, device=dev, generator=g)
    p = torch.rand((n, P, 3), dtype=torch.float64, device=dev, generator=g)
    if adversarial:  # every point within 1e-4 of vertex V / 2: nearer to it than to any other vertex of a uniform set of this size
        p = v[:, V // 2 : V // 2 + 1, :] + 1e-4 * (p - 0.5)
    w = 0.5 + torch.rand((n, P), dtype=torch.float64, device=dev, generator=g)
    u = 0.5 + torch.rand(V, dtype=torch.float64, device=dev, generator=g)
    return v, p, w, u


def kernel_call(V, P, n, directions, dev, adversarial=False):
    from deodr_amd import hip_renderer as hr

    v, p, w, u = problem(V, P, n, dev, adversarial)
    params = torch.tensor([1.0, 1.0, float("inf")], dtype=torch.float64, device=dev)
    scratch = hr.chamfer_scratch(V, P, n, dev)
    outs = hr.chamfer(v, p, params, w, u, directions, scratch=scratch)[:3]
    return (lambda: hr.chamfer(v, p, params, w, u, directions, *outs, scratch=scratch)), (v, p, params, w, u), outs


def term_times(launches, with_torch=True):
    from deodr_amd import chamfer
    from deodr_amd import hip_renderer as hr
    from skin_times import graphed, timed

    dev = torch.device("cuda", torch.cuda.current_device())
    for V, P in SIZES:
        for n in (1, 8):
            for directions in (3, 1):
                call, (v, p, params, w, u), outs = kernel_call(V, P, n, directions, dev)
                row = dict(V=V, P=P, n=n, directions=directions, launches=hr.chamfer_launches(V, P, n, directions),
                           segments=[hr.chamfer_segments(P, V), hr.chamfer_segments(V, P)], call_us=round(timed(call, launches), 1),
                           graph_us=round(timed(graphed(call), launches), 1))  # fmt: skip
                row["ps_per_pair_and_direction"] = round(row["graph_us"] * 1e6 / (n * V * P * (2 if directions == 3 else 1)), 3)
                if with_torch:
                    torch_ops = lambda: chamfer.chamfer_torch(v, p, params, w, u, directions)
                    row["torch_us"] = round(timed(torch_ops, max(launches // 10, 2)), 1)
                    row["max_gradient_diff_to_torch_relative"] = float((outs[2] - torch_ops()[2]).abs().max() / outs[2].abs().max())
                print(json.dumps(row), flush=True)


def adversarial_ratio(launches, V=10002, P=40000):
    from skin_times import graphed, timed

    dev = torch.device("cuda", torch.cuda.current_device())
    times = {}
    for name, adversarial in (("uniform", False), ("all_points_nearest_one_vertex", True)):
        call, _, _ = kernel_call(V, P, 1, 3, dev, adversarial)
        times[name] = timed(graphed(call), launches)
    print(json.dumps(dict(V=V, P=P, n=1, directions=3, uniform_us=round(times["uniform"], 1), adversarial_us=round(times["all_points_nearest_one_vertex"], 1),
                          ratio=round(times["all_points_nearest_one_vertex"] / times["uniform"], 3))), flush=True)  # fmt: skip


def iteration_times(steps):
    from deodr_amd.mesh_fitter import GraphedStep
    from skin_times import timed
    from test_chamfer_fit_host import cloud_fitter

    for keywords in ({}, dict(directions="points_to_mesh"), dict(rigidity="arap")):
        eager = cloud_fitter("cuda", **keywords)
        row = dict(fitter="MeshPointCloudFitter, hand, 400 points", **keywords, eager_step_us=round(timed(eager.step_device, steps), 1))
        g = GraphedStep(cloud_fitter("cuda", **keywords), warmup=3)
        row["graphed_step_us"] = round(timed(g.step_device, steps), 1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch ops (the slowest part)")
    a = ap.parse_args()
    adversarial_ratio(a.launches)
    iteration_times(a.steps)
    term_times(a.launches, not a.no_torch)
