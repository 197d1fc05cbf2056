"""Time of the point-to-surface term (deodr_hip_surface_distance: six launches, five with points -> mesh alone) against the same definition as torch
ops (deodr_amd.surface.surface_distance_torch, eager, chunked to 64 MB of intermediate values) on the same device and tensors, and of a whole
iteration of ``MeshPointCloudFitter(metric="surface")`` on the hand, eager and under ``GraphedStep`` (DESIGN.md 4n has the numbers).

    python tools/surface_times.py [--launches 20] [--steps 100] [--no-torch]

Meshes and clouds: the hand (526 vertices, 1 048 faces) against 4 096 and 40 000 area-uniform samples of its own surface, moved off it by noise
of a tenth of the mean edge; a latitude-longitude sphere of 10 002 vertices and 20 000 faces against 40 000 points sampled the same way.
n = 1 and 8 poses; both directions and points -> mesh alone.  Device time stamps around `launches` back-to-back replays of the call captured as one HIP graph (`graph_us`: what the kernels cost) and
around calls issued from the host one by one (`call_us`), after 10 warm-up calls, best of 5 windows; the torch ops run eager (`torch_us`, a tenth
of the launches; where one call takes more than half a second, one call after one warm-up call).  `ps_per_pair`: graph_us over n F P (+ n V P with both directions).  Then the ratio of the adversarial distribution -- every
point nearest ONE face -- to the uniform one on the sphere, both directions, n = 1."""
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


def uv_sphere(rings=101, sectors=100):
    """a closed latitude-longitude sphere: 2 + (rings - 1) * sectors vertices, 2 * sectors * (rings - 1) faces (101, 100: 10 002 and 20 000)"""
    theta = np.pi * np.arange(1, rings) / rings
    phi = 2 * np.pi * np.arange(sectors) / sectors
    ring = np.stack((np.sin(theta)[:, None] * np.cos(phi)[None], np.sin(theta)[:, None] * np.sin(phi)[None], np.repeat(np.cos(theta)[:, None], sectors, axis=1)), axis=-1)
    v = np.concatenate(([[0, 0, 1.0]], ring.reshape(-1, 3), [[0, 0, -1.0]]))
    at = lambda r, s: 1 + r * sectors + s % sectors
    f = [[0, at(0, s), at(0, s + 1)] for s in range(sectors)]
    for r in range(rings - 2):
        for s in range(sectors):
            f += [[at(r, s), at(r + 1, s), at(r + 1, s + 1)], [at(r, s), at(r + 1, s + 1), at(r, s + 1)]]
    f += [[len(v) - 1, at(rings - 2, s + 1), at(rings - 2, s)] for s in range(sectors)]
    return v, np.array(f)


def hand():
    from deodr_amd import scenes

    vertices, faces = scenes.load_hand_mesh(os.path.join(ROOT, "tests", "golden", "hand_mesh.npz"))[:2]
    return np.asarray(vertices, dtype=np.float64), np.asarray(faces)


def problem(mesh, P, n, dev, adversarial=False):
    """-> device tensors (vertices [n,V,3], faces, corner table, points [n,P,3], weights)"""
    from deodr_amd.surface import corner_table, sample_surface

    v, f = mesh
    rs = np.random.RandomState(P + n)
    edge = np.linalg.norm(v[f[:, 0]] - v[f[:, 1]], axis=1).mean()
    posed = np.stack([v + 0.01 * edge * rs.randn(*v.shape) for _ in range(n)])
    if adversarial:  # every point within a hundredth of an edge of the centroid of face F / 2, on its outer side
        a, b, c = (posed[:, f[len(f) // 2, k]] for k in range(3))
        centre = (a + b + c) / 3
        p = centre[:, None, :] * 1.001 + 0.01 * edge * (rs.rand(n, P, 3) - 0.5) * 0.1
    else:
        p = np.stack([sample_surface(posed[b], f, P, seed=b)[0] for b in range(n)]) + 0.1 * edge * rs.randn(n, P, 3)
    offsets, corners = corner_table(f, len(v))
    t = lambda a, dtype=None: torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=dev)
    return t(posed), t(f, np.int32), t(offsets), t(corners), t(p), t(0.5 + rs.rand(n, P)), t(0.5 + rs.rand(len(v)))


def kernel_call(mesh, P, n, directions, dev, adversarial=False):
    from deodr_amd import hip_renderer as hr

    v, f, offsets, corners, p, w, u = problem(mesh, P, n, dev, adversarial)
    params = torch.tensor([1.0, 1.0, float("inf")], dtype=torch.float64, device=dev)
    scratch = hr.surface_scratch(v.shape[1], f.shape[0], P, n, dev)
    outs = hr.surface_distance(v, f, offsets, corners, p, params, w, u, directions, scratch=scratch)[:3]
    return (lambda: hr.surface_distance(v, f, offsets, corners, p, params, w, u, directions, *outs, scratch=scratch)), (v, f, p, params, w, u), outs


def timed_slow(call, launches):
    """-> microseconds per call: ``skin_times.timed``, or, where one call takes more than half a second, one call after one warm-up call"""
    from skin_times import timed

    def once():
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3

    return once() if once() > 5e5 else timed(call, launches)


def term_times(launches, with_torch=True):
    from deodr_amd import hip_renderer as hr
    from deodr_amd import surface
    from skin_times import graphed, timed

    dev = torch.device("cuda", torch.cuda.current_device())
    for name, mesh, P in (("hand", hand(), 4096), ("hand", hand(), 40000), ("sphere", uv_sphere(), 40000)):
        V, F = len(mesh[0]), len(mesh[1])
        for n in (1, 8):
            for directions in (3, 1):
                call, (v, f, p, params, w, u), outs = kernel_call(mesh, P, n, directions, dev)
                row = dict(mesh=name, V=V, F=F, P=P, n=n, directions=directions, launches=hr.surface_launches(V, F, P, n, directions),
                           segments=[hr.chamfer_segments(P, F), hr.chamfer_segments(F, P), hr.chamfer_segments(V, P)],
                           call_us=round(timed(call, launches), 1), graph_us=round(timed(graphed(call), launches), 1))  # fmt: skip
                row["ps_per_pair"] = round(row["graph_us"] * 1e6 / (n * P * (F + (V if directions == 3 else 0))), 3)
                if with_torch:
                    torch_ops = lambda: surface.surface_distance_torch(v, f, p, params, w, u, directions)
                    row["torch_us"] = round(timed_slow(torch_ops, max(launches // 10, 2)), 1)
                    row["torch_over_graph"] = round(row["torch_us"] / row["graph_us"], 1)
                    row["max_gradient_diff_to_torch_relative"] = float((outs[2] - torch_ops()[2]).abs().max() / outs[2].abs().max())
                print(json.dumps(row), flush=True)


def adversarial_ratio(launches, P=40000):
    from skin_times import graphed, timed

    dev = torch.device("cuda", torch.cuda.current_device())
    mesh, times = uv_sphere(), {}
    for name, adversarial in (("uniform", False), ("all_points_nearest_one_face", True)):
        call, _, _ = kernel_call(mesh, P, 1, 3, dev, adversarial)
        times[name] = timed(graphed(call), launches)
    print(json.dumps(dict(mesh="sphere", F=len(mesh[1]), P=P, n=1, directions=3, uniform_us=round(times["uniform"], 1),
                          adversarial_us=round(times["all_points_nearest_one_face"], 1),
                          ratio=round(times["all_points_nearest_one_face"] / times["uniform"], 3))), flush=True)  # fmt: skip


def iteration_times(steps):
    from deodr_amd.mesh_fitter import GraphedStep
    from skin_times import timed
    from test_surface_fit_host import surface_fitter

    for keywords in ({}, dict(directions="points_to_mesh"), dict(metric="vertex")):
        eager = surface_fitter("cuda", **keywords)
        row = dict(fitter="MeshPointCloudFitter, hand, 4000 surface samples", metric=eager.metric, **{k: v for k, v in keywords.items() if k != "metric"},
                   eager_step_us=round(timed(eager.step_device, steps), 1))  # fmt: skip
        g = GraphedStep(surface_fitter("cuda", **keywords), warmup=3)
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
