"""Time of the closest-point term over the uniform grid (deodr_hip_chamfer_grid) against the brute-force operator (deodr_hip_chamfer) on the same
device and tensors (profiles/README.md, "Closest-point term over a grid").

    python tools/chamfer_grid_times.py [--launches 20] [--largest] [--no-table] [--sweep] [--adversarial] [--outliers] [--build-variants] [--lib PATH]

Sizes: (V, P) = (526, 4 096), (526, 40 000), (10 002, 40 000), (10 002, 307 200) and, with --largest, (100 000, 1 000 000) -- above the cap of the
brute-force operator, the grid alone --; n = 1 and 8 poses, both directions.  Clouds: "cube" (vertices and points uniform in the unit cube,
max_distance twice the spacing V^(-1/3) of the vertices) and "surface" (the points are `sample_surface` samples of the mesh -- the hand, a
latitude-longitude sphere of 10 002 or 99 858 vertices -- with noise of a tenth of an edge, max_distance three mean edges).  The cell size is
`deodr_amd.chamfer.default_cell_size` of the cloud.  Device time stamps around `launches` back-to-back replays of the call captured as one HIP
graph, after 10 warm-up replays, best of 5 windows.  --sweep: the cell size from a quarter of to eight times the default at (10 002, 40 000) and
(10 002, 307 200), n = 1.  --adversarial: every point within 1e-4 of one vertex, and 100 000 coincident points, at V = 10 002.
--outliers: a tenth of the points far from the mesh (no neighbour within max_distance: the search of such a point probes every ring), and
padded clouds (1 000 and 100 000 copies of the first point at weight 0).

RINGS and the load of the table are constants of the header that a build may override: `--build-variants` compiles the library with
-DDEODR_HIP_CHAMFER_GRID_RINGS=2 / 8 and -DDEODR_HIP_CHAMFER_GRID_TABLE_LOAD=1 / 4 into tools/variants/ (no GPU needed), and `--lib PATH` times
that library instead of the package's (the sizes the Python layer asks it for are the variant's own)."""
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

SIZES = ((526, 4096), (526, 40000), (10002, 40000), (10002, 307200))
LARGEST = (100000, 1000000)


VARIANTS = {"rings2": "-DDEODR_HIP_CHAMFER_GRID_RINGS=2", "rings8": "-DDEODR_HIP_CHAMFER_GRID_RINGS=8", "load1": "-DDEODR_HIP_CHAMFER_GRID_TABLE_LOAD=1",
            "load4": "-DDEODR_HIP_CHAMFER_GRID_TABLE_LOAD=4"}  # fmt: skip


def build_variants():
    """the library with each override of VARIANTS -> tools/variants/libdeodr_hip_<name>.so, compiled side by side"""
    import subprocess

    import __graft_entry__ as g

    out = os.path.join(ROOT, "tools", "variants")
    os.makedirs(out, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    jobs = [subprocess.Popen([hipcc] + g.HIPCC_FLAGS + [flag, "-o", os.path.join(out, f"libdeodr_hip_{name}.so"), os.path.join(g.CSRC, "dr_kernels.hip")], cwd=g.CSRC)
            for name, flag in VARIANTS.items()]  # fmt: skip
    assert all(job.wait() == 0 for job in jobs)


def cube(V, P, n, seed=0):
    rs = np.random.RandomState(seed + V + P + n)
    return rs.rand(n, V, 3), rs.rand(n, P, 3), 2.0 * V ** (-1.0 / 3.0)


def surface(V, P, n, seed=0):
    """-> (vertices [n,V',3], points [n,P,3], max_distance): V' the vertices of the mesh nearest in size to V"""
    from deodr_amd.surface import sample_surface
    from surface_times import hand, uv_sphere

    v, f = hand() if V < 1000 else uv_sphere(101, 100) if V < 50000 else uv_sphere(317, 316)
    v = v / np.abs(v).max()
    edge = np.linalg.norm(v[f[:, 0]] - v[f[:, 1]], axis=1).mean()
    rs = np.random.RandomState(seed + P + n)
    posed = np.stack([v + 0.01 * edge * rs.randn(*v.shape) for _ in range(n)])
    points = np.stack([sample_surface(posed[b], f, P, seed=b)[0] + 0.1 * edge * rs.randn(P, 3) for b in range(n)])
    return posed, points, 3.0 * edge


def calls(v, p, tau, cell, dev, brute=True):
    """-> (replay of the grid call, replay of the brute-force call | None, the launches of the grid call, largest |difference| of the gradients / largest gradient)"""
    from deodr_amd import hip_renderer as hr
    from skin_times import graphed

    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    v, p = t(v), t(p)
    n, V, P = int(v.shape[0]), int(v.shape[1]), int(p.shape[1])
    g = torch.Generator(dev).manual_seed(V + P + n)
    w = 0.5 + torch.rand((n, P), dtype=torch.float64, device=dev, generator=g)
    u = 0.5 + torch.rand(V, dtype=torch.float64, device=dev, generator=g)
    params = torch.tensor([1.0, 1.0, tau], dtype=torch.float64, device=dev)
    scratch = hr.chamfer_grid_scratch(V, P, n, dev)
    outs = hr.chamfer_grid(v, p, params, cell, w, u, 3, scratch=scratch)[:3]
    grid = graphed(lambda: hr.chamfer_grid(v, p, params, cell, w, u, 3, *outs, scratch=scratch))
    if not brute or hr.lib().deodr_hip_chamfer_scratch_bytes(V, P, n) == 0:
        return grid, None, hr.chamfer_grid_launches(V, P, n, 3), None
    bscratch = hr.chamfer_scratch(V, P, n, dev)
    bouts = hr.chamfer(v, p, params, w, u, 3, scratch=bscratch)[:3]
    difference = float((outs[2] - bouts[2]).abs().max() / bouts[2].abs().max().clamp_min(1e-300))
    return grid, graphed(lambda: hr.chamfer(v, p, params, w, u, 3, *bouts, scratch=bscratch)), hr.chamfer_grid_launches(V, P, n, 3), difference


def row_of(kind, v, p, tau, cell, launches, dev, brute=True, **more):
    from skin_times import timed

    grid, brute_call, count, difference = calls(v, p, tau, cell, dev, brute)
    row = dict(cloud=kind, V=int(v.shape[1]), P=int(p.shape[1]), n=int(v.shape[0]), max_distance=round(tau, 5), cell_size=round(cell, 5), launches=count, **more,
               grid_us=round(timed(grid, launches), 1))  # fmt: skip
    if brute_call is not None:
        row["brute_us"] = round(timed(brute_call, max(launches // 4, 3)), 1)
        row["brute_over_grid"], row["gradient_difference_relative"] = round(row["brute_us"] / row["grid_us"], 2), difference
    print(json.dumps(row), flush=True)
    torch.cuda.empty_cache()
    return row


def main(a):
    from deodr_amd.chamfer import default_cell_size

    dev = torch.device("cuda", torch.cuda.current_device())
    for V, P in (() if a.no_table else SIZES) + ((LARGEST,) if a.largest else ()):
        for n in (1, 8):
            for kind, make in (("cube", cube), ("surface", surface)):
                v, p, tau = make(V, P, n)
                row_of(kind, v, p, tau, default_cell_size(list(p)), a.launches, dev)
    if a.sweep:
        for V, P in ((10002, 40000), (10002, 307200)):
            for kind, make in (("cube", cube), ("surface", surface)):
                v, p, tau = make(V, P, 1)
                default = default_cell_size(list(p))
                for factor in (0.25, 0.5, 1.0, 2.0, 4.0, 8.0):
                    row_of(kind, v, p, tau, factor * default, a.launches, dev, brute=False, cell_size_over_default=factor)
    if a.outliers:
        for kind, make in (("cube", cube), ("surface", surface)):
            v, p, tau = make(10002, 307200, 1)
            p[:, ::10] += 50.0 * tau  # a tenth of the points with nothing within max_distance
            row_of(kind + ", a tenth of the points outliers", v, p, tau, default_cell_size(list(p[:, 1::10])), a.launches, dev)
            for copies in (1000, 100000):
                v, p, tau = make(10002, 307200, 1)
                p[:, -copies:] = p[:, :1]
                row_of(kind + f", padded with {copies} copies of the first point", v, p, tau, default_cell_size(list(p[:, :-copies])), a.launches, dev)
    if a.adversarial:
        v, p, tau = cube(10002, 40000, 1)
        near_one = v[:, 5001:5002, :] + 1e-4 * (p - 0.5)
        row_of("every point within 1e-4 of one vertex", v, near_one, tau, default_cell_size(list(p)), a.launches, dev)
        v, p, tau = cube(10002, 100000, 1)
        row_of("100 000 coincident points", v, np.repeat(p[:, :1, :], 100000, axis=1), tau, default_cell_size(list(p)), a.launches, dev)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--largest", action="store_true", help="also (100 000, 1 000 000): the grid alone")
    ap.add_argument("--no-table", action="store_true", help="skip the table of sizes")
    ap.add_argument("--sweep", action="store_true", help="the cell size around the default")
    ap.add_argument("--adversarial", action="store_true")
    ap.add_argument("--outliers", action="store_true", help="outlier and padded-cloud rows at (10 002, 307 200)")
    ap.add_argument("--build-variants", action="store_true", help="compile the RINGS / table-load variants of the library and stop")
    ap.add_argument("--lib", default=None, help="time this build of the library (a variant) instead of the package's")
    a = ap.parse_args()
    if a.build_variants:
        build_variants()
        sys.exit(0)
    if a.lib:
        from deodr_amd import hip_renderer

        hip_renderer.LIB_PATH = os.path.abspath(a.lib)
        print(json.dumps(dict(library=os.path.relpath(hip_renderer.LIB_PATH, ROOT))), flush=True)
    main(a)
