"""Timings for the weighted fit step.  Modes:
  ab --lib PATH --abi N      : the UNWEIGHTED step of configs[2] (1 and 8 views) on the given library build (one process per build, alternated by the caller)
  weighted                   : fused weighted step vs the two-call route a user had to take, and vs the fused unweighted step; depth-fitter GraphedStep
"""
import os, sys, time, statistics
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deodr_amd import scenes, hip_renderer as hr
from deodr_amd.hip_renderer import DeviceScene, HipRasterizer

arg = lambda name, default: type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
mode = sys.argv[1]
dev = torch.device("cuda:0")


def scene(B, S=1024):
    views = [scenes.sphere_scene(size=S, angle=float(a)) for a in np.linspace(-0.5, 0.5, B)]
    s0 = views[0]
    stack = lambda n: np.stack([np.asarray(getattr(v, n)) for v in views])
    ds = DeviceScene(s0.faces, s0.faces_uv, s0.textured, s0.shaded, s0.uv, stack("ij"), stack("depths"), stack("colors"), stack("shade"), stack("edgeflags"), S, S,
                     texture=None, background_color=s0.background_color, clockwise=s0.clockwise, vertex_dtype=torch.float64, pixel_dtype=torch.float32, device=dev)
    return ds, HipRasterizer.for_scene(ds)


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def alternate(fns, steps=200, rounds=5, warm=20):
    """every function in turn, `rounds` times; -> {name: [ms per step of every round]}"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, steps))
    return out


def report(tag, res):
    for k, v in res.items():
        print(f"{tag} {k}: median {statistics.median(v):.4f} ms  min {min(v):.4f}  max {max(v):.4f}  rounds {' '.join(f'{x:.4f}' for x in v)}", flush=True)


if mode == "ab":
    hr.LIB_PATH = os.path.abspath(arg("--lib", ""))
    hr.ABI_VERSION = arg("--abi", 13)
    for B in (1, 8):
        ds, r = scene(B)
        obs = torch.rand((B, 1024, 1024, 4), dtype=torch.float32, device=dev)
        image, z = torch.empty((B, 1024, 1024, 4), dtype=torch.float32, device=dev), torch.empty((B, 1024, 1024), dtype=torch.float32, device=dev)
        grads = ds.zero_grads()
        r.render(ds, 1.0, out=(image, z), check_overflow=True)
        fit = lambda: r.render_fit(ds, obs, 1.0, grads=grads, out=(image, z), check_overflow=False, clear_grads=True)
        report(f"[{arg('--tag', '?')}] unweighted fit step, {B} view(s)", alternate({"fit": fit}, steps=200, rounds=3))
elif mode == "weighted":
    for B in (1, 8):
        ds, r = scene(B)
        obs = torch.rand((B, 1024, 1024, 4), dtype=torch.float32, device=dev)
        w = (2 * torch.rand((B, 1024, 1024), dtype=torch.float32, device=dev)).contiguous()
        w[:, :128] = 0
        image, z = torch.empty((B, 1024, 1024, 4), dtype=torch.float32, device=dev), torch.empty((B, 1024, 1024), dtype=torch.float32, device=dev)
        grads = ds.zero_grads()
        loss = torch.zeros(1, dtype=torch.float64, device=dev)
        r.render(ds, 1.0, out=(image, z), check_overflow=True)
        image_b = torch.empty_like(image)

        def two_call(with_loss):
            def f():
                for g in grads.values():
                    if g is not None:
                        g.zero_()
                r.render(ds, 1.0, out=(image, z), check_overflow=False)
                d = image - obs
                torch.mul(d, w[..., None], out=image_b)
                if with_loss:
                    l = (image_b.double() * d.double()).sum()
                image_b.mul_(2)
                r.render_backward(ds, image_b=image_b, grads=grads)
            return f

        fns = {
            "two-call (render, torch residual, render_backward)": two_call(False),
            "two-call + torch loss": two_call(True),
            "fused weighted": lambda: r.render_fit(ds, obs, 1.0, grads=grads, out=(image, z), check_overflow=False, clear_grads=True, weights=w),
            "fused weighted + loss": lambda: r.render_fit(ds, obs, 1.0, grads=grads, out=(image, z), check_overflow=False, clear_grads=True, weights=w, loss_out=loss),
            "fused unweighted": lambda: r.render_fit(ds, obs, 1.0, grads=grads, out=(image, z), check_overflow=False, clear_grads=True),
            "fused unweighted + loss": lambda: r.render_fit(ds, obs, 1.0, grads=grads, out=(image, z), check_overflow=False, clear_grads=True, loss_out=loss),
        }
        report(f"configs[2] {B} view(s)", alternate(fns, steps=200, rounds=5))
    # the depth fitter's step (200^2-ish, C = 1, clamp) as a GraphedStep replay, with and without weights
    from deodr_amd.mesh_fitter import GraphedStep, MeshDepthFitter
    G = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    d, hand = np.load(os.path.join(G, "depth_hand_fit.npz")), np.load(os.path.join(G, "hand_mesh.npz"))
    depth = d["depth_raw_f32"].astype(np.float64)
    depth[depth == 0] = float(d["max_depth"])
    mask = np.ones(depth.shape)
    mask[40:80, 60:120] = 0
    steppers = {}
    for name, wgt in (("unweighted", None), ("weighted", mask)):
        f = MeshDepthFitter(hand["vertices"], hand["faces"].astype(np.int64), d["euler_init"], d["translation_init"], cregu=1000)
        f.set_image(depth / float(d["max_depth"]), focal=241, distortion=d["distortion"], weights=wgt)
        f.set_max_depth(1)
        f.set_depth_scale(float(d["depth_scale"]))
        g = GraphedStep(f)
        steppers[f"GraphedStep replay, {name}"] = g.step_device
    print("depth image", depth.shape, flush=True)
    report("depth fitter", alternate(steppers, steps=200, rounds=5))
elif mode == "trace":
    B = 8
    ds, r = scene(B)
    obs = torch.rand((B, 1024, 1024, 4), dtype=torch.float32, device=dev)
    w = torch.rand((B, 1024, 1024), dtype=torch.float32, device=dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    grads = ds.zero_grads()
    for _ in range(10):
        r.render_fit(ds, obs, 1.0, grads=grads, check_overflow=False, clear_grads=True, weights=w, loss_out=loss)
    torch.cuda.synchronize()
