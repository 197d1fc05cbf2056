"""Trajectory digest of the five fitters of deodr_amd/mesh_fitter.py: for a fixed list of configurations, 5 steps from fixed seeds and one line per
configuration with a SHA-256 over the bytes of every parameter, every momentum speed and the energy each step returned.  Two trees that print the
same lines compute the same fits; the check of a change that is meant to change nothing.

    python tools/fit_trajectory.py [--device cpu|cuda] [--only SUBSTRING] [--no-graph] [--dump FILE.npz]
    python tools/fit_trajectory.py --compare A.npz B.npz [C.npz]

``--device cpu`` (the default): CPU tensors, the checker standing in for the rasterizer (tests/cpu_raster.py, tests/cpu_raster_texture.py): the autograd
paths.  ``--device cuda``: ``hip_renderer.set_deterministic(True)``, the same configurations (the fixed kernel sequences where the fitter has one) plus a
``GraphedStep`` of each with 3 replays after the capture.  ``--dump`` keeps the hashed arrays; ``--compare`` prints, per configuration, whether B (and C)
equal A bit for bit and otherwise the largest relative difference ``max |a - b| / max |a|`` over the arrays -- with three files, A-vs-B next to A-vs-C.
"""
import hashlib, os, sys
import numpy as np, torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")
STEPS, REPLAYS = 5, 3
arg = lambda name, default=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default

PARAMETERS = ("vertices", "coefficients", "transform_quaternion", "transform_translation", "mesh_color", "light_directional", "light_ambient", "light_sh",
              "texture", "quaternions", "translations", "focal", "center", "distortion")  # fmt: skip


def compare(paths):
    files = [np.load(p) for p in paths]
    names = sorted({k.rsplit("|", 1)[0] for k in files[0].files})
    worst = [0.0] * (len(files) - 1)
    for name in names:
        keys = [k for k in files[0].files if k.rsplit("|", 1)[0] == name]
        out = []
        for i, other in enumerate(files[1:]):
            if any(k not in other.files for k in keys):
                out.append("missing")
                continue
            rel = max(float(np.abs(files[0][k].astype(np.float64) - other[k].astype(np.float64)).max() / max(np.abs(files[0][k]).max(), 1e-300)) if files[0][k].size else 0.0
                      for k in keys)  # fmt: skip
            same = all(files[0][k].tobytes() == other[k].tobytes() for k in keys)
            worst[i] = max(worst[i], rel)
            out.append("equal" if same else f"{rel:.3e}")
        print(f"{name:58s} " + "  ".join(f"{os.path.basename(p)}: {o}" for p, o in zip(paths[1:], out)))
    print("largest relative difference: " + "  ".join(f"{os.path.basename(p)}: {w:.3e}" for p, w in zip(paths[1:], worst)))


if "--compare" in sys.argv:
    compare(sys.argv[sys.argv.index("--compare") + 1 :])
    sys.exit(0)

from deodr_amd import mesh_fitter as mf, scenes

device = arg("--device", "cpu")
cpu = device == "cpu"
hand_v, hand_f = scenes.load_hand_mesh(os.path.join(GOLD, "hand_mesh.npz"))
hand_f = hand_f.astype(np.int64)


def depth(**keywords):
    d = np.load(os.path.join(GOLD, "depth_hand_fit.npz"))
    image = d["depth_raw_f32"].astype(np.float64)[::2, ::2]  # 100 x 100
    image[image == 0] = float(d["max_depth"])
    weights = keywords.pop("weights", None)
    f = mf.MeshDepthFitter(np.load(os.path.join(GOLD, "hand_mesh.npz"))["vertices"], hand_f, d["euler_init"], d["translation_init"], cregu=1000, device=device, **keywords)
    f.set_image(image / float(d["max_depth"]), focal=120.5, distortion=d["distortion"], weights=weights)
    f.set_max_depth(1)
    f.set_depth_scale(float(d["depth_scale"]))
    return f


def shape_basis(K=4):
    rs = np.random.RandomState(11)
    return dict(shape_basis=0.02 * rs.randn(K, len(hand_v), 3), coefficient_regu=0.3, sigmas=0.5 + rs.rand(K))


def rgb(views=1, size=64, **keywords):
    d = np.load(os.path.join(GOLD, "rgb_hand_fit.npz"))
    rs = np.random.RandomState(5)
    common = (d["default_color"], d["default_light_directional"], float(d["default_light_ambient"]))
    if views == 1:
        f = mf.MeshRGBFitterWithPose(d["vertices_centered"], hand_f, np.zeros(3), d["translation_init"], *common, cregu=1000, device=device, **keywords)
        f.set_background_color(d["background_color"])
        f.set_image(rs.rand(size, size, 3))
        return f
    eulers = np.array([[0.0, 0.4 * v, 0.0] for v in range(views)])
    f = mf.MeshRGBFitterWithPoseMultiFrame(d["vertices_centered"], hand_f, eulers, np.tile(d["translation_init"], (views, 1)), *common, cregu=1000, device=device,
                                           **keywords)  # fmt: skip
    f.set_background_color(d["background_color"])
    f.set_images(list(rs.rand(views, size, size, 3)))
    return f


def sh(shape):
    return 0.3 + 0.2 * np.random.RandomState(7).rand(*shape)


def texture(views=2, size=48, texture_size=12, nu=14, n_rings=10, basis=False, **keywords):
    vertices, faces = scenes.bumpy_sphere(nu, n_rings)
    faces = faces.astype(np.int64)
    s0 = scenes.sphere_scene(size, nu, n_rings, nb_colors=3, textured=True, texture_size=texture_size, angle=0.0)
    cameras = [scenes.fit_camera(size, size, 60.0, vertices, scenes.rotx(0.37) @ scenes.roty(0.23 + 2 * np.pi * k / views)) for k in range(views)]
    rs = np.random.RandomState(3)
    if basis:
        q, _ = np.linalg.qr(rs.randn(texture_size * texture_size * 3, 3))
        keywords.update(texture_basis=q.T.reshape(3, texture_size, texture_size, 3), coefficient_regu=0.05, sigmas=0.5 + rs.rand(3))
    f = mf.MeshTextureFitterMultiFrame(vertices, faces, s0.uv, faces, np.full((texture_size, texture_size, 3), 0.5), [-0.1, -0.5, -0.4], 0.6, cameras=cameras,
                                       clockwise=bool(s0.clockwise), device=device, pixel_dtype=torch.float64, **keywords)  # fmt: skip
    f.set_background_color(np.asarray(s0.background_color, dtype=np.float64))
    f.set_images(rs.rand(views, size, size, 3), weights=(rs.rand(views, size, size) > 0.1).astype(np.float64))
    return f


def camera(views=2, size=48, update=mf.CameraFitterMultiFrame.GROUPS, **keywords):
    p = scenes.calibration_scene(hand_v, views, size, arc=np.pi)["start"]
    colors = np.tile([0.8, 0.6, 0.5], (len(hand_v), 1))
    if not keywords.get("shared_intrinsics", True):
        p = dict(p, **{k: np.tile(p[k], (views, 1)) for k in ("focal", "center", "distortion")})
    f = mf.CameraFitterMultiFrame(hand_v, hand_f, p["quaternions"], p["translations"], p["focal"], p["center"], p["distortion"], colors=colors,
                                  light_directional=np.array([-0.3, -0.4, -0.6]), light_ambient=0.4, update=update, device=device, **keywords)  # fmt: skip
    f.set_background_color(np.array([0.1, 0.2, 0.3]))
    f.set_images(np.random.RandomState(9).rand(views, size, size, 3))
    return f


CONFIGURATIONS = [
    ("depth", lambda: depth()),
    ("depth weights", lambda: depth(weights=(np.random.RandomState(2).rand(100, 100) > 0.2).astype(np.float64))),
    ("depth subdivisions=1", lambda: depth(subdivisions=1)),
    ("depth shape_basis", lambda: depth(**shape_basis())),
    ("rgb directional", lambda: rgb()),
    ("rgb sh[9]", lambda: rgb(light_sh_init=sh((9,)))),
    ("rgb sh[9,3]", lambda: rgb(light_sh_init=sh((9, 3)))),
    ("rgb sh[9,3] vertex_albedo albedo_regu", lambda: rgb(light_sh_init=sh((9, 3)), vertex_albedo=True, albedo_regu=1.0)),
    ("rgb directional shape_basis", lambda: rgb(**shape_basis())),
    ("rgb sh[9] shape_basis", lambda: rgb(light_sh_init=sh((9,)), **shape_basis())),
    ("rgb directional update_lights=False", lambda: rgb(update_lights=False)),
    ("multi 3 views", lambda: rgb(views=3)),
    ("rgb pyramid_levels=3", lambda: rgb(pyramid_levels=3, pyramid_weights=[1.0, 0.5, 2.0, 0.25])),
    ("rgb ssim_weight=0.5", lambda: rgb(ssim_weight=0.5)),
    ("multi 3 views pyramid_levels=3", lambda: rgb(views=3, pyramid_levels=3)),
    ("multi 3 views ssim_weight=0.5", lambda: rgb(views=3, ssim_weight=0.5, ssim_data_range=2.0)),
    ("multi 3 views sh[9,3] vertex_albedo albedo_regu", lambda: rgb(views=3, light_sh_init=sh((9, 3)), vertex_albedo=True, albedo_regu=1.0)),
    ("texture", lambda: texture()),
    ("texture basis coefficient_regu", lambda: texture(basis=True)),
    ("texture step_max", lambda: texture(step_max=0.01)),
    ("texture basis step_max", lambda: texture(basis=True, step_max=0.01)),
    ("texture basis step_max=0", lambda: texture(basis=True, step_max=0)),
    ("camera shared", lambda: camera()),
    ("camera per-view intrinsics", lambda: camera(shared_intrinsics=False)),
    ("camera sigmas", lambda: camera(sigmas={"focal": 0.5, "translations": np.array([0.1, 0.1, 0.3]), "distortion": 0.01})),
    ("camera update=(extrinsic, focal)", lambda: camera(update=("extrinsic", "focal"))),
    ("camera pyramid_levels=2", lambda: camera(pyramid_levels=2)),
    ("camera ssim_weight=0.5", lambda: camera(ssim_weight=0.5)),
]  # fmt: skip


def state(f, energies):
    """{label: array} of what the digest covers, in a fixed order"""
    host = lambda t: t.detach().cpu().numpy().copy()
    out = {"energies": np.asarray(energies, dtype=np.float64)}
    for k in PARAMETERS:
        if torch.is_tensor(getattr(f, k, None)):
            out["parameter " + k] = host(getattr(f, k))
    for k in sorted(f.momentum.speed):
        out["speed " + k] = host(f.momentum.speed[k])
    return out


def report(name, arrays, dumped):
    h = hashlib.sha256()
    for k, a in arrays.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(a).tobytes())
        dumped[f"{name}|{k}"] = a
    print(f"{name:58s} {h.hexdigest()}  energy {arrays['energies'][0]:.17g} -> {arrays['energies'][-1]:.17g}", flush=True)


def run():
    dumped = {}
    only = arg("--only")
    for name, build in CONFIGURATIONS:
        if only is not None and only not in name:
            continue
        f = build()
        energies = [f.step()[0] for _ in range(STEPS)]
        report(name, state(f, energies), dumped)
        if not cpu and "--no-graph" not in sys.argv:
            f = build()
            # the deterministic mode keeps its integer shadows per stream and cannot allocate them under capture: one eager step on torch's capture stream
            if torch.cuda.graph.default_capture_stream is None:
                torch.cuda.graph.default_capture_stream = torch.cuda.Stream()
            capture_stream = torch.cuda.graph.default_capture_stream
            capture_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(capture_stream):
                f.step_device()
            torch.cuda.current_stream().wait_stream(capture_stream)
            g = mf.GraphedStep(f)
            energies = []
            for _ in range(REPLAYS):
                energies.append(float(g.step_device()[0].reshape(-1)[0]))
            report(name + " | graphed", state(f, energies), dumped)
    if arg("--dump"):
        np.savez(arg("--dump"), **dumped)


if cpu:
    import contextlib

    import cpu_raster, cpu_raster_texture
    from deodr_amd.scene3d import Scene3DDevice
    from oracle import api

    @contextlib.contextmanager
    def emulate():
        """the checker behind Scene3DDevice's rasterizer entries: the textured stand-in for textured renders, the plain one otherwise"""
        with cpu_raster.emulate(api.port()):
            plain, plain_l2 = Scene3DDevice._rasterize, Scene3DDevice._rasterize_l2

            def _rasterize(self, camera, ij, depths, colors, shade, textured, backface_culling, **given):
                return (cpu_raster_texture._rasterize if textured else plain)(self, camera, ij, depths, colors, shade, textured, backface_culling, **given)

            def _rasterize_l2(self, camera, ij, depths, colors, shade, textured, backface_culling, obs, **given):
                return (cpu_raster_texture._rasterize_l2 if textured else plain_l2)(self, camera, ij, depths, colors, shade, textured, backface_culling, obs, **given)

            Scene3DDevice._rasterize, Scene3DDevice._rasterize_l2 = _rasterize, _rasterize_l2
            yield  # (cpu_raster.emulate restores the entries of the product)

    with emulate():
        run()
else:
    from deodr_amd import hip_renderer

    hip_renderer.set_deterministic(True)
    run()
