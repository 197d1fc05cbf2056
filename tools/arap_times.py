"""Time of the as-rigid-as-possible energy (deodr_hip_arap_energy: two launches) against the same definition as torch ops
(deodr_amd.arap.arap_energy_torch: batched SVD, gathers, index_add) on the same device and tensors, and of a whole fit iteration with
``rigidity="laplacian"`` and ``rigidity="arap"`` (profiles/README.md, "As-rigid-as-possible energy").

    python tools/arap_times.py [--launches 100] [--steps 100] [--table] [--torch-graphs]

First the table DEODR_HIP_ARAP_SWEEPS rests on (``--table``: only that; it runs on the CPU): the cells of the test tables of
tests/arap_reference.py, the largest off-diagonal norm of Horn's matrix relative to its norm after 1 .. 7 sweeps of cyclic Jacobi in long double,
and the largest distance of the rotation to the one of Kabsch / SVD times the cell's conditioning gamma.

The energy: V = 526 (the hand) and V = 10 002 (the benchmark's sphere), n = 1 and 8 poses (the rest mesh plus noise of 5 % of an edge).  Device time
stamps around `launches` back-to-back calls after 10 warm-up calls, best of 5 windows: issued from the host one by one (`call_us`) and replayed as
one HIP graph (`graph_us`: what the kernels cost).  Iteration: ``MeshRGBFitterWithPoseMultiFrame`` on 8 views of the hand at 256 x 256 under
``GraphedStep``: the fixed kernel sequence, the same iteration through autograd (how an ARAP fit runs), ``rigidity="arap"``, and ``rigidity="arap"``
while the torch ops stand in for the kernels.  The captures of the torch ops (a batched SVD inside a graph) are tried only with ``--torch-graphs``:
a capture that the SVD does not allow ends the measurements that would follow it, so the others run without."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def meshes():
    from deodr_amd import scenes

    yield "hand", scenes.load_hand_mesh(os.path.join(ROOT, "tests", "golden", "hand_mesh.npz"))
    yield "sphere 100 x 100", scenes.bumpy_sphere(100, 100)


def sweep_table(sweeps=range(1, 8)):
    import arap_reference as ar

    cases = [ar.case(name, hows) for name, hows in ar.parity_cases()]
    S = np.concatenate([c["S"].reshape(-1, 3, 3) for c in cases]).astype(ar.LD)
    gamma = np.concatenate([c["gamma"].reshape(-1) for c in cases])
    kabsch = ar.kabsch(S)
    for m in sweeps:
        lam, E, off = ar.jacobi(ar.horn(S), m)
        R = ar.rotation_matrix(ar.top_quaternion(lam, E)).astype(np.float64)
        distance = np.abs(R - kabsch).max(axis=(-1, -2)) * np.where(np.isfinite(gamma), gamma, 1.0)
        print(json.dumps(dict(cells=len(S), sweeps=m, off_diagonal_relative=float(f"{float(off.max()):.1e}"),
                              rotation_distance_times_gamma=float(f"{float(distance.max()):.1e}"))), flush=True)  # fmt: skip


def energy_times(launches, torch_graphs=False):
    from deodr_amd import arap
    from deodr_amd import hip_renderer as hr
    from skin_times import graphed, timed

    dev = torch.device("cuda", torch.cuda.current_device())
    for name, (vertices, faces) in meshes():
        vertices, faces = np.asarray(vertices, dtype=np.float64), np.asarray(faces).astype(np.int64)
        energy_of = arap.ArapEnergyDevice(faces, vertices, 1.0, device=dev)
        V = energy_of.nb_vertices
        edge = float(np.linalg.norm(vertices[faces[:, 0]] - vertices[faces[:, 1]], axis=1).mean())
        for n in (1, 8):
            p = energy_of.vertices_ref[None] + 0.05 * edge * torch.randn((n, V, 3), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(0))
            scratch = hr.arap_scratch(V, n, dev)
            tables = (energy_of.offsets, energy_of.cols, energy_of.weights, energy_of.vertices_ref)
            energy, gradient, _ = hr.arap_energy(*tables, p, 1.0, scratch=scratch)
            kernel = lambda: hr.arap_energy(*tables, p, 1.0, energy=energy, gradient=gradient, scratch=scratch)
            torch_ops = lambda: arap.arap_energy_torch(energy_of.rows, energy_of.columns, energy_of.weights, energy_of.vertices_ref, p, 1.0)
            few = max(launches // 10, 5)
            row = dict(mesh=name, V=V, nnz=energy_of.nnz, n=n, launches=hr.arap_launches(V, energy_of.nnz, n), blocks=hr.arap_blocks(V),
                       call_us=round(timed(kernel, launches), 1), graph_us=round(timed(graphed(kernel), launches), 1),
                       torch_us=round(timed(torch_ops, few), 1),
                       max_gradient_diff_to_torch_relative=float((gradient - torch_ops()[1]).abs().max() / gradient.abs().max()))  # fmt: skip
            if torch_graphs:
                try:
                    row["torch_graph_us"] = round(timed(graphed(torch_ops), few), 1)
                except Exception as e:  # (a capture the torch ops do not allow: the eager time stands alone)
                    row["torch_graph_us"] = f"not captured: {type(e).__name__}"
            print(json.dumps(row), flush=True)


def iteration_times(steps, views=8, size=256, torch_graphs=False):
    from deodr_amd import arap
    from deodr_amd.mesh_fitter import GraphedStep
    from skin_times import timed
    from test_pyramid_fit_host import hand_fitter

    def per_step(fitter):
        g = GraphedStep(fitter, warmup=3)
        return timed(g.step_device, steps)

    make = lambda **kw: hand_fitter(views, "cuda", torch.float32, shift_pixels=(2, 1), size=size, **kw)
    row = dict(views=views, size=size)
    row["laplacian_fixed_sequence_us"] = round(per_step(make()), 1)
    plain = make()
    plain.direct = False  # the same iteration through autograd, as an ARAP fit runs: what the energy itself costs is the difference to this one
    row["laplacian_autograd_us"] = round(per_step(plain), 1)
    row["arap_us"] = round(per_step(make(rigidity="arap")), 1)
    if not torch_graphs:
        print(json.dumps(row), flush=True)
        return
    uses_kernel = arap.ArapEnergyDevice.uses_kernel
    arap.ArapEnergyDevice.uses_kernel = lambda self, vertices: False  # the torch ops in the kernels' place
    try:
        row["arap_torch_ops_us"] = round(per_step(make(rigidity="arap")), 1)
    except Exception as e:  # (a capture the torch ops do not allow)
        row["arap_torch_ops_us"] = f"not captured: {type(e).__name__}"
    finally:
        arap.ArapEnergyDevice.uses_kernel = uses_kernel
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--table", action="store_true", help="only the table the number of sweeps rests on (CPU)")
    ap.add_argument("--torch-graphs", action="store_true", help="also capture the torch ops into graphs (energy and iteration)")
    a = ap.parse_args()
    sweep_table()
    if not a.table:
        energy_times(a.launches, a.torch_graphs)
        iteration_times(a.steps, torch_graphs=a.torch_graphs)
