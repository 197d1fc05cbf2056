"""Time of ONE ITERATION of the colour fitters with spherical-harmonic lighting, in the manner of tools/camera_fit_times.py: the directional-light
iteration, SH lighting + one colour, SH lighting + per-vertex albedo (with its smoothness term), each as the fixed kernel sequence eager and as one
HIP-graph replay, 1 view and 8 views of 1024 x 1024 of the hand mesh.  GPU box.

    python tools/sh_fit_times.py [--f32] [--size 1024]
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deodr_amd import scenes
from deodr_amd.mesh_fitter import GraphedStep, MeshRGBFitterWithPose, MeshRGBFitterWithPoseMultiFrame

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
size, steps = arg("--size", 1024), 30
only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None  # one mode: for a kernel trace
pixel_dtype = torch.float32 if "--f32" in sys.argv else torch.float64
vertices, faces = scenes.load_hand_mesh(os.path.join(GOLD, "hand_mesh.npz"))
faces = faces.astype(np.int64)
color, light, ambient = np.array([0.8, 0.6, 0.5]), np.array([0.1, 0.5, 0.4]), 0.6
SH = {}
try:
    from deodr_amd import lighting

    sh = lighting.sh_from_directional(torch.tensor(light), ambient).numpy()
    SH = {"SH + one colour": dict(light_sh_init=sh), "SH + per-vertex albedo": dict(light_sh_init=sh[:, None] * np.ones(3), vertex_albedo=True, albedo_regu=1.0)}
except ImportError:  # (the parent commit: the directional iteration alone)
    pass


def build(views, keywords):
    eul = np.stack([np.array([0, a, 0]) for a in np.linspace(-0.5, 0.5, views)])

    def make(euler, color):
        if views == 1:
            f = MeshRGBFitterWithPose(vertices, faces, euler[0], np.zeros(3), color, light, ambient, cregu=2000, pixel_dtype=pixel_dtype, **keywords)
            f.set_image(np.zeros((size, size, 3)))
        else:
            f = MeshRGBFitterWithPoseMultiFrame(vertices, faces, euler, np.zeros((views, 3)), color, light, ambient, cregu=2000, pixel_dtype=pixel_dtype, **keywords)
            f.set_images([np.zeros((size, size, 3))] * views)
        f.set_background_color(np.array([0.5, 0.6, 0.7]))
        return f

    target = make(eul + np.array([0.04, 0.06, -0.03]), np.array([0.7, 0.65, 0.55])).render().detach().cpu().numpy()
    f = make(eul, color)
    f.set_image(target[0]) if views == 1 else f.set_images(list(target))
    return f


def timed(run, count):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / count


for views in (1, 8):
    for name, keywords in {"directional light + one colour": {}, **SH}.items():
        if only is not None and only not in name:
            continue
        f = build(views, keywords)
        for _ in range(5):
            f.step_device()
        assert f._direct_state is not None
        eager = timed(f.step_device, steps)
        g = GraphedStep(build(views, keywords), warmup=3)
        graphed = timed(g.step_device, steps)
        print(f"{name}: {views} view(s) of {size}^2, {str(pixel_dtype).replace('torch.', '')} frames: step_device {eager * 1e3:.3f} ms, one HIP-graph replay per step {graphed * 1e3:.3f} ms", flush=True)
