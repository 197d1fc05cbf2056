"""Time of deodr_hip_basis_apply / deodr_hip_basis_apply_b against torch.matmul on the same tensors (profiles/README.md, "Linear bases").

    python tools/basis_times.py [--launches 200]

Device time stamps around `launches` back-to-back launches, warm, best of 5 windows; `K N 4` bytes / time is quoted against the copy bandwidth
bench.py's hbm_probe measures on the same box (best_copy_GBps)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROBLEMS = [("eigen-faces", 150, 64 * 64 * 1, 1), ("a face model", 199, 160470, 1), ("a face model", 199, 160470, 8), ("an eigen-texture", 100, 1024 * 1024 * 3, 1)]


def timed(call, launches):
    """-> microseconds per launch"""
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


def main(launches):
    import bench
    from deodr_amd import hip_renderer as hr

    dev = torch.device("cuda", torch.cuda.current_device())
    copy = bench.hbm_probe(dev)["best_copy_GBps"]
    print(json.dumps({"copy_GBps": copy}))
    for name, K, N, batch in PROBLEMS:
        g = torch.Generator(device=dev).manual_seed(0)
        B = torch.randn(K, N, device=dev, generator=g)
        mean = torch.randn(N, device=dev, generator=g)
        c = torch.randn(batch, K, dtype=torch.float64, device=dev, generator=g)
        grad = torch.randn(batch, N, device=dev, generator=g)
        y, c_b = torch.empty(batch, N, device=dev), torch.empty(batch, K, dtype=torch.float64, device=dev)
        scratch = hr.basis_scratch(K, N, batch, dev)
        c32, y_mm, c_mm = c.float(), torch.empty(batch, N, device=dev), torch.empty(batch, K, device=dev)
        rows = {
            "apply_us": timed(lambda: hr.basis_apply(B, mean, c, out=y), launches),
            "apply_b_us": timed(lambda: hr.basis_apply_b(B, grad, out=c_b, scratch=scratch), launches),
            "matmul_apply_us": timed(lambda: torch.addmm(mean, c32, B, out=y_mm), launches),  # float32 throughout: what torch offers on a float32 basis
            "matmul_apply_b_us": timed(lambda: torch.matmul(grad, B.T, out=c_mm), launches),
        }
        nbytes = K * N * 4
        rows.update(problem=name, K=K, N=N, batch=batch, segments=hr.basis_segments(K, N),
                    apply_frac_of_copy=nbytes / (rows["apply_us"] * 1e-6) / 1e9 / copy, apply_b_frac_of_copy=nbytes / (rows["apply_b_us"] * 1e-6) / 1e9 / copy,
                    max_diff_apply=float((y - y_mm).abs().max()), max_diff_apply_b=float((c_b - c_mm.double()).abs().max()))  # fmt: skip
        print(json.dumps(rows))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    main(ap.parse_args().launches)
