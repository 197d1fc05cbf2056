"""Time of the point-to-surface term over the uniform grid of triangles (deodr_hip_surface_grid) against the brute-force operator
(deodr_hip_surface_distance) on the same device and tensors (DESIGN.md 4p has the numbers).

    python tools/surface_grid_times.py [--launches 20] [--no-table] [--long] [--outliers] [--sweep] [--trace-sizes]

Sizes: the hand (526 vertices, 1 048 faces) against 40 000 points; a latitude-longitude sphere of 10 002 vertices and 20 000 faces against 40 000,
200 000 (under the brute-force cap: both operators run) and 307 200 points (a VGA depth frame: above the cap, the grid alone); the hand after
two Loop subdivisions (16 768 faces) against 307 200 points (above the cap too).  n = 1 and 8 poses; points -> mesh alone and both directions.
The clouds are `sample_surface` samples of the mesh with noise of a tenth of the mean edge, max_distance is three mean edges, the cell size is
`deodr_amd.chamfer.default_cell_size` of the cloud.  Device time stamps around `launches` back-to-back replays of the call captured as one HIP
graph, after 10 warm-up replays, best of 5 windows; grid and brute force on the same tensors in the same run.  --long: the sphere with ONE
triangle across it, against 4 096 and 40 000 points (E makes h_f large for the whole pose: the weakness the header names).  --outliers: a tenth of the points far from the mesh
(their search visits every shell).  --sweep: the cell size from a quarter of to eight times the default at (20 000 faces, 200 000 points).  --trace-sizes: the rows at 307 200 points
alone, the grid alone -- what a `rocprofv3 --kernel-trace --stats` run of this tool takes the shares of the kernels from."""
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


def subdivided_hand(levels=2):
    """the hand after `levels` Loop subdivisions (16 768 faces after two), by the package's own subdivision matrix"""
    from deodr_amd.subdivision import LoopSubdivision
    from surface_times import hand

    v, f = hand()
    s = LoopSubdivision(f, len(v), n_iter=levels, device="cpu")
    return np.asarray(s.matrix @ v), np.asarray(s.faces_fine)


def problem(mesh, P, n, long_face=False, outliers=False, seed=0):
    """-> NumPy (vertices [n,V,3], faces [F,3], points [n,P,3], max_distance): the mesh scaled into the unit cube, its samples with noise"""
    from deodr_amd.surface import sample_surface

    v, f = mesh
    v = v / np.abs(v).max()
    edge = np.linalg.norm(v[f[:, 0]] - v[f[:, 1]], axis=1).mean()
    rs = np.random.RandomState(seed + P + n)
    posed = np.stack([v + 0.01 * edge * rs.randn(*v.shape) for _ in range(n)])
    points = np.stack([sample_surface(posed[b], f, P, seed=b)[0] + 0.1 * edge * rs.randn(P, 3) for b in range(n)])
    if long_face:  # one triangle from pole to pole and a quarter of the way round: its box is the longest by far
        f = np.concatenate((f, [[0, len(v) - 1, len(v) // 4]]))
    if outliers:
        points[:, ::10] += 50.0 * 3.0 * edge
    return posed, f, points, 3.0 * edge


def calls(v, f, p, tau, cell, directions, dev):
    """-> (replay of the grid call, replay of the brute-force call | None, the launches of the grid call, what the two results differ by)"""
    from deodr_amd import hip_renderer as hr
    from deodr_amd.surface import corner_table
    from skin_times import graphed

    offsets, corners = corner_table(f, v.shape[1])
    t = lambda a, dtype=np.float64: torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=dev)
    v, p, f, offsets, corners = t(v), t(p), t(f, np.int32), t(offsets, np.int32), t(corners, np.int32)
    n, V, P, F = int(v.shape[0]), int(v.shape[1]), int(p.shape[1]), int(f.shape[0])
    g = torch.Generator(dev).manual_seed(V + P + n)
    w = 0.5 + torch.rand((n, P), dtype=torch.float64, device=dev, generator=g)
    u = 0.5 + torch.rand(V, dtype=torch.float64, device=dev, generator=g)
    params = torch.tensor([1.0, 1.0, tau], dtype=torch.float64, device=dev)
    scratch = hr.surface_grid_scratch(V, F, P, n, dev)
    outs = hr.surface_grid(v, f, offsets, corners, p, params, cell, w, u, directions, scratch=scratch, want_nearest=True)
    grid = graphed(lambda: hr.surface_grid(v, f, offsets, corners, p, params, cell, w, u, directions, *outs, scratch=scratch))
    launches = hr.surface_grid_launches(V, F, P, n, directions)
    if not hr.surface_launches(V, F, P, n, directions):
        return grid, None, launches, None
    bscratch = hr.surface_scratch(V, F, P, n, dev)
    bouts = hr.surface_distance(v, f, offsets, corners, p, params, w, u, directions, scratch=bscratch, want_nearest=True)
    found = outs[3] != -1 if outs[3] is not None else None
    same = dict(terms_equal=bool(torch.equal(outs[0], bouts[0])), gradient_difference_relative=float((outs[2] - bouts[2]).abs().max() / bouts[2].abs().max().clamp_min(1e-300)))
    if found is not None:
        same.update(faces_equal=bool(torch.equal(outs[3][found], bouts[3][found])), barycentric_equal=bool(torch.equal(outs[4][found], bouts[4][found])),
                    without_face=round(float((~found).double().mean()), 4))  # fmt: skip
    return grid, graphed(lambda: hr.surface_distance(v, f, offsets, corners, p, params, w, u, directions, *bouts, scratch=bscratch)), launches, same


def row_of(name, mesh, P, n, directions, launches, dev, cell_factor=1.0, **how):
    from deodr_amd.chamfer import default_cell_size
    from skin_times import timed

    v, f, p, tau = problem(mesh, P, n, **how)
    cell = cell_factor * default_cell_size(list(p[:, 1::10] if how.get("outliers") else p))
    grid, brute, count, same = calls(v, f, p, tau, cell, directions, dev)
    row = dict(mesh=name, V=int(v.shape[1]), F=len(f), P=P, n=n, directions=directions, pairs=f"{len(f) * P:.2e}", max_distance=round(tau, 5), cell_size=round(cell, 5),
               launches=count, grid_us=round(timed(grid, launches), 1), **({"cell_size_over_default": cell_factor} if cell_factor != 1.0 else {}))  # fmt: skip
    if brute is not None:
        row["brute_us"] = round(timed(brute, max(launches // 4, 3)), 1)
        row["brute_over_grid"] = round(row["brute_us"] / row["grid_us"], 2)
        row.update(same)
    print(json.dumps(row), flush=True)
    torch.cuda.empty_cache()
    return row


def main(a):
    from surface_times import hand, uv_sphere

    dev = torch.device("cuda", torch.cuda.current_device())
    sphere = uv_sphere(101, 100)
    if not a.no_table:
        table = [("hand", hand(), 40000), ("sphere", sphere, 40000), ("sphere", sphere, 200000), ("sphere", sphere, 307200), ("hand, subdivisions=2", subdivided_hand(2), 307200)]
        for name, mesh, P in table:
            for n in (1, 8):
                for directions in (1, 3):
                    row_of(name, mesh, P, n, directions, a.launches, dev)
    if a.trace_sizes:
        for name, mesh in (("sphere", sphere), ("hand, subdivisions=2", subdivided_hand(2))):
            for n in (1, 8):
                for directions in (1, 3):
                    row_of(name, mesh, 307200, n, directions, a.launches, dev)
    if a.long:
        for P in (4096, 40000):  # (every point visits every face: a tenth of the launches)
            row_of("sphere with one triangle across it", sphere, P, 1, 1, max(a.launches // 10, 2), dev, long_face=True)
    if a.outliers:
        for directions in (1, 3):
            row_of("sphere, a tenth of the points outliers", sphere, 200000, 1, directions, a.launches, dev, outliers=True)
    if a.sweep:
        for factor in (0.25, 0.5, 2.0, 4.0, 8.0):
            row_of("sphere", sphere, 200000, 1, 1, a.launches, dev, cell_factor=factor)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--no-table", action="store_true", help="skip the table of sizes")
    ap.add_argument("--long", action="store_true", help="one very long triangle: E decides the cell edge")
    ap.add_argument("--outliers", action="store_true", help="a tenth of the points with no face within max_distance")
    ap.add_argument("--sweep", action="store_true", help="the cell size around the default")
    ap.add_argument("--trace-sizes", action="store_true", help="the rows at 307 200 points alone (for a kernel trace of the tool)")
    main(ap.parse_args())
