"""Timings of Loop subdivision on the device, all in ONE process and GPU visit, variants alternated after a warm-up (prints; redirect into
profiles/subdiv_times.txt):
  1. deodr_hip_subdiv_apply for the hand at 1 and 2 levels, with S and with S^T, batch 1, float64 [n, 3]: us per launch from device events, next to
     the torch ops of the same map on the same device (index_select, multiply, index_add_ over the COO triplets: what LoopSubdivision runs on
     tensors the kernel does not take);
  2. one MeshDepthFitter iteration on the reference's depth image with subdivisions = 0 (the fixed kernel sequence), 1 and 2: eager and as a
     GraphedStep replay, wall clock per iteration.
"""
import os, sys, time, statistics
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deodr_amd import hip_renderer as hr
from deodr_amd.mesh_fitter import GraphedStep, MeshDepthFitter
from deodr_amd.subdivision import LoopSubdivision

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
dev = torch.device("cuda:0")


def event_us(fn, reps=200):
    """us per call of `fn` from a device event pair around `reps` back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def graph_us(fn, reps=50, launches=20):
    """us per call of `fn` inside a captured graph of `reps` calls (no launch overhead between them: the kernels' own time)"""
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    return event_us(g.replay, launches) / reps


def wall_ms(fn, steps=100):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def spread(values):
    return f"median {statistics.median(values):8.2f}  (min {min(values):8.2f}, max {max(values):8.2f})"


hand = np.load(os.path.join(GOLDEN, "hand_mesh.npz"))
vertices, faces = hand["vertices"], hand["faces"].astype(np.int64)

# ---- 1. the kernel against the torch ops -------------------------------------------------------------------------------------------------
print("deodr_hip_subdiv_apply against torch ops (index_select, multiply, index_add_), hand, batch 1, float64 [n, 3]; us per call")
for n_iter in (1, 2):
    sub = LoopSubdivision(faces, 526, n_iter, device=dev)
    for transposed in (False, True):
        operator = sub._vertices
        m = operator.transposed if transposed else operator.matrix
        tables = sub.tables(transposed)
        rows, cols, vals = operator.coo_tables(transposed, dev)
        x = torch.randn(1, m.shape[1], 3, dtype=torch.float64, device=dev)
        out = torch.empty(1, m.shape[0], 3, dtype=torch.float64, device=dev)
        kernel = lambda: hr.sparse_rows_apply(*tables, x, out=out)
        torch_ops = lambda: torch.zeros(1, m.shape[0], 3, dtype=torch.float64, device=dev).index_add_(-2, rows, vals[:, None] * x.index_select(-2, cols))
        fns = {"kernel, in a graph": lambda: graph_us(kernel), "torch ops, in a graph": lambda: graph_us(torch_ops),
               "kernel, launched one by one": lambda: event_us(kernel), "torch ops, launched one by one": lambda: event_us(torch_ops)}
        for fn in (kernel, torch_ops):
            for _ in range(30):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(5):
            for k, fn in fns.items():
                times[k].append(fn())
        lengths = np.diff(m.indptr)
        print(f"  {n_iter} level(s), {'S^T' if transposed else 'S  '}: {m.shape[0]} rows of {lengths.min()} - {lengths.max()} entries, nnz {m.nnz}, {sub.lanes(transposed)} lanes per row")
        for k, v in times.items():
            print(f"      {k:32s} {spread(v)}")

# ---- 2. a depth-fit iteration ------------------------------------------------------------------------------------------------------------
d = np.load(os.path.join(GOLDEN, "depth_hand_fit.npz"))
depth = d["depth_raw_f32"].astype(np.float64)
depth[depth == 0] = float(d["max_depth"])


def fitter(subdivisions):
    f = MeshDepthFitter(vertices, faces, d["euler_init"], d["translation_init"], cregu=1000, subdivisions=subdivisions)
    f.set_image(depth / float(d["max_depth"]), focal=241, distortion=d["distortion"])
    f.set_max_depth(1)
    f.set_depth_scale(float(d["depth_scale"]))
    return f


print("one MeshDepthFitter iteration (200 x 200 depth image of the reference's example); ms per iteration, wall clock over 100 iterations")
for subdivisions in (0, 1, 2):
    eager = fitter(subdivisions)
    for _ in range(10):
        eager.step_device()
    graphed = GraphedStep(fitter(subdivisions))
    for _ in range(10):
        graphed.step_device()
    e = [wall_ms(eager.step_device) for _ in range(3)]
    g = [wall_ms(graphed.step_device) for _ in range(3)]
    print(f"  subdivisions = {subdivisions} ({eager.mesh.nb_faces} triangles rendered): eager {spread(e)}   graph replay {spread(g)}")
