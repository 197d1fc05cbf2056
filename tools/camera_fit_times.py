"""Time of ONE ITERATION of CameraFitterMultiFrame (8 views of 1024 x 1024 of the hand mesh), in the manner of tools/fit_times.py: the fixed kernel
sequence eager and as one HIP-graph replay, the same iteration on the autograd path (``direct = False``) eager and graphed, and -- as context -- the
8-view MeshRGBFitterWithPoseMultiFrame iteration of tools/fit_times.py on the same box.  GPU box.

    python tools/camera_fit_times.py [--f32] [--views 8] [--size 1024]
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deodr_amd import scenes
from deodr_amd.mesh_fitter import CameraFitterMultiFrame, GraphedStep, MeshRGBFitterWithPoseMultiFrame

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
views, size, steps = arg("--views", 8), arg("--size", 1024), 30
pixel_dtype = torch.float32 if "--f32" in sys.argv else torch.float64
vertices, faces = scenes.load_hand_mesh(os.path.join(GOLD, "hand_mesh.npz"))
faces = faces.astype(np.int64)
problem = scenes.calibration_scene(vertices, views, size)
colors, light, ambient, bg = np.tile([0.8, 0.6, 0.5], (len(vertices), 1)), np.array([-0.3, -0.4, -0.6]), 0.4, np.array([0.1, 0.2, 0.3])
UPDATE = ("extrinsic", "focal", "distortion")


def camera_fitter(p, update, direct=True):
    f = CameraFitterMultiFrame(vertices, faces, p["quaternions"], p["translations"], p["focal"], p["center"], p["distortion"], colors=colors,
                               light_directional=light, light_ambient=ambient, update=update, pixel_dtype=pixel_dtype)
    f.direct = direct
    f.set_background_color(bg)
    return f


truth = camera_fitter(problem["truth"], ())
truth.set_images(np.zeros((views, size, size, 3)))
photographs = truth.gradients()[1].cpu().numpy()
del truth


def build(direct):
    f = camera_fitter(problem["start"], UPDATE, direct)
    f.set_images(photographs)
    return f


def build_multi8():
    color, l, amb = np.array([0.8, 0.6, 0.5]), np.array([0.1, 0.5, 0.4]), 0.6
    eul = np.stack([np.array([0, a, 0]) for a in np.linspace(-0.5, 0.5, views)])

    def make(euler, color):
        f = MeshRGBFitterWithPoseMultiFrame(vertices, faces, euler, np.zeros((views, 3)), color, l, amb, cregu=2000, pixel_dtype=pixel_dtype)
        f.set_images([np.zeros((size, size, 3))] * views)
        f.set_background_color(np.array([0.5, 0.6, 0.7]))
        return f

    target = make(eul + np.array([0.04, 0.06, -0.03]), np.array([0.7, 0.65, 0.55])).render().detach().cpu().numpy()
    f = make(eul, color)
    f.set_images(list(target))
    return f


def timed(run, count):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / count


for name, make in (("camera fit, fixed kernel sequence", lambda: build(True)), ("camera fit, autograd path", lambda: build(False)),
                   ("MeshRGBFitterWithPoseMultiFrame (context)", build_multi8)):
    f = make()
    for _ in range(5):
        f.step_device()
    eager = timed(f.step_device, steps)
    g = GraphedStep(make(), warmup=3)
    graphed = timed(g.step_device, steps)
    print(f"{name}: {views} views of {size}^2, {str(pixel_dtype).replace('torch.', '')} frames: step_device {eager * 1e3:.3f} ms, one HIP-graph replay per step {graphed * 1e3:.3f} ms", flush=True)
