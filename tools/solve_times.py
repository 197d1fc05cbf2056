"""Time of the sparse symmetric positive definite solve (deodr_hip_spd_solve) on ``I + lambda L`` of a mesh against the same recurrence as torch ops
(deodr_amd.smoothing.spd_solve_torch) on the same device and tensors, against ONE ``torch.mm`` with the explicit dense inverse -- a yardstick only:
not a shipped path, 8 V^2 bytes, impossible at 50 000 vertices --, and of a whole fit iteration with and without ``smoothing=``
(profiles/README.md, "Smoothed steps").

    python tools/solve_times.py [--launches 100] [--steps 100] [--table]

First the table the default number of steps rests on (``--table``: only that; it runs on the CPU): the hand mesh, lambda = 4 / 16 / 64, the squared
relative residual after 8 / 16 / 32 / 64 steps.

The solve: V = 526 (the hand: the one-workgroup instance) and V = 10 002 (the benchmark's sphere: 2 + 2 m launches), D = 3, lambda = 16, the default
number of steps.  Device time stamps around `launches` back-to-back calls after 10 warm-up calls, best of 5 windows: issued from the host one by one
(`call_us`) and replayed as one HIP graph (`graph_us`: what the kernels cost).  Iteration: ``MeshRGBFitterWithPoseMultiFrame`` on 8 views of the hand
under ``GraphedStep``, without the keyword (the fixed kernel sequence), with it, and with it while the torch recurrence stands in for the kernel."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from skin_times import graphed, timed  # noqa: E402


def meshes():
    from deodr_amd import scenes

    yield "hand", scenes.load_hand_mesh(os.path.join(ROOT, "tests", "golden", "hand_mesh.npz"))
    yield "sphere 100 x 100", scenes.bumpy_sphere(100, 100)


def solve_times(launches, lam=16.0):
    from deodr_amd import hip_renderer as hr
    from deodr_amd import smoothing

    dev = torch.device("cuda", torch.cuda.current_device())
    m = smoothing.DEFAULT_ITERATIONS
    for name, (vertices, faces) in meshes():
        V = len(vertices)
        system = smoothing.laplacian_system(np.asarray(faces).astype(np.int64), lam, V, device=dev)
        b = torch.randn((V, 3), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(0))
        b -= b.mean(dim=0, keepdim=True)
        scratch = hr.spd_scratch(V, 3, dev)
        x, residual = hr.spd_solve(system.offsets, system.cols, system.vals, b, m, scratch=scratch)
        kernel = lambda: hr.spd_solve(system.offsets, system.cols, system.vals, b, m, x=x, residual=residual, scratch=scratch)
        torch_ops = lambda: smoothing.spd_solve_torch(system, b, m)
        inverse = torch.as_tensor(np.linalg.inv(system.to_scipy().toarray()), device=dev)  # (inverted on the host, once: the yardstick is the product)
        dense = lambda: torch.mm(inverse, b)
        few = max(launches // 10, 5)
        row = dict(mesh=name, V=V, nnz=system.nnz, D=3, lam=lam, iterations=m, launches=hr.spd_launches(V, system.nnz, 3, m),
                   call_us=round(timed(kernel, launches), 1), graph_us=round(timed(graphed(kernel), launches), 1),
                   torch_us=round(timed(torch_ops, few), 1), dense_inverse_mm_graph_us=round(timed(graphed(dense), launches), 1),
                   dense_inverse_megabytes=round(8 * V * V / 1e6, 1), residual=[float(f"{v:.2e}") for v in residual.tolist()],
                   max_diff_to_torch_relative=float((x - torch_ops()[0]).abs().max() / x.abs().max()))  # fmt: skip
        try:
            row["torch_graph_us"] = round(timed(graphed(torch_ops), few), 1)
        except Exception as e:  # (a capture the torch ops do not allow: the eager time stands alone)
            row["torch_graph_us"] = f"not captured: {type(e).__name__}"
        print(json.dumps(row), flush=True)


def residual_table(lams=(4.0, 16.0, 64.0), steps=(8, 16, 32, 64)):
    """what the default number of steps rests on: the hand mesh, a random zero-mean right-hand side, the condition number of
    ``I + lambda L`` and the largest squared relative residual of the three columns after 8 / 16 / 32 / 64 steps of the float64 recurrence.  Runs on
    the CPU: no device needed."""
    from deodr_amd import smoothing

    (_, (vertices, faces)), *_ = meshes()
    b = np.random.RandomState(0).randn(len(vertices), 3)
    b = torch.as_tensor(b - b.mean(axis=0))
    for lam in lams:
        system = smoothing.laplacian_system(np.asarray(faces).astype(np.int64), lam, len(vertices), device="cpu")
        eigenvalues = np.linalg.eigvalsh(system.to_scipy().toarray())
        row = dict(mesh="hand", V=len(vertices), lam=lam, kappa=round(float(eigenvalues[-1] / eigenvalues[0])))
        row.update({f"residual_after_{m}": float(f"{float(smoothing.spd_solve_torch(system, b, m)[1].max()):.1e}") for m in steps})
        print(json.dumps(row), flush=True)


def iteration_times(steps, views=8, size=256):
    from deodr_amd import smoothing
    from deodr_amd.mesh_fitter import GraphedStep
    from test_pyramid_fit_host import hand_fitter

    def per_step(fitter):
        g = GraphedStep(fitter, warmup=3)
        return timed(g.step_device, steps)

    make = lambda **kw: hand_fitter(views, "cuda", torch.float32, shift_pixels=(2, 1), size=size, **kw)
    row = dict(views=views, size=size, smoothing=16.0, iterations=smoothing.DEFAULT_ITERATIONS)
    row["plain_fixed_sequence_us"] = round(per_step(make()), 1)
    plain = make()
    plain.direct = False  # the same iteration through autograd, as a smoothed fit runs: what the solve itself adds is the difference to this one
    row["plain_autograd_us"] = round(per_step(plain), 1)
    row["smoothing_us"] = round(per_step(make(smoothing=16.0)), 1)
    uses_kernel, smoothing.uses_kernel = smoothing.uses_kernel, lambda system, b: False  # the torch recurrence in the kernel's place
    try:
        row["smoothing_torch_ops_us"] = round(per_step(make(smoothing=16.0)), 1)
    finally:
        smoothing.uses_kernel = uses_kernel
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--table", action="store_true", help="only the residual table the default number of steps rests on (CPU)")
    a = ap.parse_args()
    residual_table()
    if not a.table:
        solve_times(a.launches)
        iteration_times(a.steps)
