"""GPU parity tests added in round 3 (through the C ABI, like the others):

* a fixed-seed slice of the randomised sweep (tests/fuzz_parity.py): 10 soups + 10 mesh views against the checker;
* the fit step with every tile class of the fused forward -- tiles with silhouette edges back-propagated in the forward launch,
  pairs of tiles sharing a wavefront, tiny frames -- against the two-call path and the checker;
* BASELINE configs[4] as a full-size 2-view textured batch (texture-gradient window path at scale) against the sum of per-view checker calls;
* rigid energy, vertex normals (index_add on ROCm) against the reference's fixtures; iteration-0 gradients of the float32 depth fit;
* the single-view CameraPytorch / Scene3DPytorch (reference shapes) on the device; two renders of one Scene3DDevice in one graph;
* residual-mode adjoint after another forward has used the workspace (stale generation stamp).
"""

import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from deodr_amd import scenes

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def checker(api, fixed=False):
    return api.ref(fixed=fixed) or api.port(fixed=fixed)


def fixture(name):
    return np.load(os.path.join(GOLDEN, name))


def hand():
    d = fixture("hand_mesh.npz")
    return d["vertices"], d["faces"].astype(np.int64)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def test_fixed_seed_slice_of_the_randomised_sweep(oracle_api, capsys):
    """what found round 2's only kernel defect, now in the driver's run: 10 random soups (sizes, flags, view counts, fill rules,
    pixel dtypes, textures) and 10 random mesh views (silhouette edges, 1-6 channels, antialiase_error, perspective-correct forward)"""
    import fuzz_parity

    assert fuzz_parity.main(10) == 0
    assert fuzz_parity.main_meshes(10) == 0
    out = capsys.readouterr().out
    assert "0 missed" in out


@pytest.mark.parametrize("size,nu,rings,n_views,dt", [(1024, 100, 100, 2, F32), (512, 60, 60, 3, F64), (520, 60, 60, 1, F32), (96, 20, 16, 2, F64)])
def test_fit_step_of_every_tile_class_equals_two_call_path_and_checker(oracle_api, size, nu, rings, n_views, dt):
    """1024 / 512: chunked grids (head of the work list with the fused edge adjoint, tile pairs in the rest); 520: an odd number of
    tile columns (65: no pairing); 96: a tiny frame (one class, the edge-capable instance walks everything)."""
    from test_hip_parity import compare_fit_step

    views = [scenes.sphere_scene(size=size, nu=nu, n_rings=rings, angle=a) for a in np.linspace(-0.4, 0.5, n_views)]
    compare_fit_step(oracle_api, views, 1.0, dt)
    compare_fit_step(oracle_api, views[:1], 2.5, dt)  # wider bands: more edges per tile
    compare_fit_step(oracle_api, views[:1], 0.0, dt)  # no edges at all: every non-empty tile may pair


def test_tile_pairs_cover_the_benchmark_frame(oracle_api):
    """the pairing really happens on the benchmark scene (otherwise the tests above would be comparing the single-tile path with
    itself): the fit step of a 1024^2 view lists fewer work entries than it has non-empty tiles"""
    from hip_util import device_scene
    from deodr_amd import hip_renderer as hr
    from deodr_amd.hip_renderer import HipRasterizer

    ds = device_scene(scenes.sphere_scene(size=1024), F32)
    r = HipRasterizer.for_scene(ds)
    obs = torch.zeros((1, 1024, 1024, 4), dtype=F32, device=ds.device)
    r.render_fit(ds, obs, 1.0, check_overflow=True, clear_grads=True)
    torch.cuda.synchronize()
    nonempty, edge_tiles = hr.tile_census(r, ds)
    words = r.workspace[:64].view(torch.int32).cpu().numpy()
    listed = int(words[13]) + int(words[14])  # WsHeader::work_count[0..1]
    assert edge_tiles > 0 and listed < nonempty and nonempty - listed > nonempty // 4, (nonempty, listed)


def test_config5_two_views_full_size_textured(oracle_api):
    """BASELINE configs[4] as a batch: 2 views of 2048^2, 100 352 triangles, 1024^2 texture; uv_b / texture_b summed over the views"""
    from test_hip_parity import compare_fit_step

    views = [scenes.sphere_scene(size=2048, nu=224, n_rings=224, nb_colors=3, textured=True, texture_size=1024, angle=a) for a in (-0.2, 0.3)]
    compare_fit_step(oracle_api, views, 1.0, F32)


def test_rigid_energy_and_normals_on_the_device():
    """index_add on ROCm tensors: vertex normals + their adjoint, the Laplacian rigid energy and gradient, against values produced
    by the reference (tests/golden/scene3d_helpers.npz, depth_hand_fit.npz)"""
    from deodr_amd.scene3d import LaplacianRigidEnergyDevice, MeshTopology

    d, h = fixture("depth_hand_fit.npz"), fixture("scene3d_helpers.npz")
    vertices, faces = hand()
    topo = MeshTopology(faces, 526, device="cuda")
    v = torch.tensor(vertices, device="cuda", requires_grad=True)
    normals = topo.vertex_normals(v)
    assert rel(normals.detach().cpu(), h["vertex_normals"]) < 1e-12
    lum = torch.relu(-(normals * torch.tensor(h["light"], device="cuda")).sum(-1)) + 0.3
    assert rel(lum.detach().cpu(), h["luminosity"]) < 1e-12
    (normals_b,) = torch.autograd.grad(lum, normals, torch.tensor(h["luminosity_b"], device="cuda"), retain_graph=True)
    assert rel(normals_b.cpu(), h["vertex_normals_b"]) < 1e-12
    e = LaplacianRigidEnergyDevice(topo, vertices, float(d["cregu"]))
    v0 = torch.tensor(vertices - vertices.mean(axis=0), device="cuda")
    energy, grad = e.evaluate(v0)  # (iteration 0 of the reference's fit: the energy of a pure translation, zero up to rounding)
    assert abs(float(energy) - float(d["it0_energy_rigid"])) <= 1e-10 * max(1.0, abs(float(d["it0_energy_rigid"])))
    assert float(grad.abs().max()) < 1e-9 and float(np.abs(d["it0_grad_rigid"]).max()) < 1e-9
    # a real deformation: the ROCm index_add against the same ops on CPU tensors (pinned on the reference by the CPU suite)
    bent = vertices + 0.05 * np.random.RandomState(3).randn(*vertices.shape) * np.std(vertices)
    e_cpu = LaplacianRigidEnergyDevice(MeshTopology(faces, 526, device="cpu"), vertices, float(d["cregu"]))
    en_d, g_d = e.evaluate(torch.tensor(bent, device="cuda"))
    en_c, g_c = e_cpu.evaluate(torch.tensor(bent))
    assert abs(float(en_d) - float(en_c)) < 1e-12 * float(en_c) and rel(g_d.cpu(), g_c) < 1e-12


def test_float32_depth_fit_first_step_gradients():
    """float32 pixel buffers: the gradients the FIRST step of the device depth fitter sees, through the speeds it leaves
    ((1 - damping)(1 - inertia) clamp(-factor gradient), mesh_fitter.py:160-196), against the reference's iteration-0 adjoints at 1e-4"""
    from deodr_amd.mesh_fitter import MeshDepthFitter

    d = fixture("depth_hand_fit.npz")
    depth = d["depth_raw_f32"].astype(np.float64)
    depth[depth == 0] = float(d["max_depth"])
    vertices, faces = hand()
    fitter = MeshDepthFitter(vertices, faces, d["euler_init"], d["translation_init"], cregu=1000, pixel_dtype=F32)
    fitter.set_image(depth / float(d["max_depth"]), focal=241, distortion=d["distortion"])
    fitter.set_max_depth(1)
    fitter.set_depth_scale(float(d["depth_scale"]))
    energy = fitter.step()[0]
    assert abs(energy - d["energies"][0]) <= 1e-6 * d["energies"][0]
    k, s = (1 - 0.05) * (1 - 0.96), fitter.momentum.speed
    assert rel(s["quaternion"][0].cpu(), k * np.clip(-0.00006 * d["it0_quaternion_b"], -0.1, 0.1)) < 1e-4
    assert rel(s["translation"][0].cpu(), k * np.clip(-0.00005 * d["it0_translation_b"], -0.1, 0.1)) < 1e-4
    assert rel(s["vertices"].cpu(), k * np.clip(-0.0005 * (d["it0_vertices_b"] + d["it0_grad_rigid"]), -1, 1)) < 1e-4


def test_single_view_classes_on_the_device(oracle_api):
    """CameraPytorch / Scene3DPytorch: the reference's shapes, results on the device of the inputs (CPU tensors in -> CPU tensors
    out, as the reference's fitters expect; ROCm tensors stay on the device), same numbers as the batched classes, gradients to
    mesh.vertices"""
    from deodr_amd.pytorch import CameraPytorch, DeviceCamera, DeviceMesh, Scene3DDevice, Scene3DPytorch

    vertices, faces = hand()
    rot = np.array([[1.0, 0, 0], [0, -1, 0], [0, 0, -1]])
    center = vertices.mean(axis=0) + np.array([0, 0, 9.0]) * np.max(np.std(vertices, axis=0))
    extrinsic, intrinsic = np.column_stack((rot, -rot.T.dot(center))), np.array([[300.0, 0, 80], [0, 300.0, 60], [0, 0, 1]])
    colors = np.random.RandomState(0).rand(len(vertices), 3)
    results = []
    for device in ("cpu", "cuda"):
        v = torch.tensor(vertices, device=device, requires_grad=True)
        cam = CameraPytorch(extrinsic, intrinsic, 120, 160, distortion=np.array([0.1, 0, 0, 0, 0]))
        ij, depths = cam.project_points(v)
        assert ij.shape == (526, 2) and depths.shape == (526,) and ij.device.type == device
        scene = Scene3DPytorch()
        scene.set_mesh(DeviceMesh(faces, v, colors=colors, device="cuda") if device == "cuda" else
                       type("Mesh", (), dict(faces=faces, vertices=v, vertices_colors=torch.tensor(colors), clockwise=False, uv=None, texture=None))())
        scene.set_light(np.array([-0.1, -0.5, -0.4]), 0.6)
        scene.set_background_color([0.5, 0.6, 0.7])
        image, z = scene.render(cam, return_z_buffer=True)
        assert image.shape == (120, 160, 3) and z.shape == (120, 160) and image.device.type == device
        (image**2).sum().backward()
        assert v.grad is not None and v.grad.device.type == device and float(v.grad.abs().max()) > 0
        results.append((image.detach().cpu().numpy(), v.grad.cpu().numpy()))
    assert np.abs(results[0][0] - results[1][0]).max() < 1e-12 and rel(results[0][1], results[1][1]) < 1e-9
    # the batched classes with n = 1 give the same frame
    batched = Scene3DDevice()
    batched.set_mesh(DeviceMesh(faces, vertices, colors=colors, device="cuda"))
    batched.set_light(np.array([-0.1, -0.5, -0.4]), 0.6)
    batched.set_background_color([0.5, 0.6, 0.7])
    image_b = batched.render(DeviceCamera(extrinsic, intrinsic, 120, 160, np.array([0.1, 0, 0, 0, 0])))
    assert image_b.shape == (1, 120, 160, 3) and np.abs(image_b[0].cpu().numpy() - results[1][0]).max() < 1e-12


def test_two_renders_of_one_scene3d_in_one_graph():
    """two cameras through ONE Scene3DDevice before one backward: the first render's adjoint must rebuild its forward state from ITS
    depths and silhouette flags (saved on the autograd context), not from the second render's.  Against separate graphs."""
    from deodr_amd.scene3d import DeviceCamera, DeviceMesh, Scene3DDevice

    vertices, faces = hand()
    rot = np.array([[1.0, 0, 0], [0, -1, 0], [0, 0, -1]])
    radius = np.max(np.std(vertices, axis=0))
    cams = []
    for shift in (np.array([0, 0, 9.0]), np.array([2.5, 1.0, 7.0])):
        center = vertices.mean(axis=0) + shift * radius
        cams.append(DeviceCamera(np.column_stack((rot, -rot.T.dot(center))), np.array([[260.0, 0, 64], [0, 260.0, 64], [0, 0, 1]]), 128, 128))
    colors = np.random.RandomState(1).rand(len(vertices), 3)

    def run(which):
        v = torch.tensor(vertices, device="cuda", requires_grad=True)
        scene = Scene3DDevice()
        scene.set_mesh(DeviceMesh(faces, v, colors=colors, device="cuda"))
        scene.set_background_color([0.2, 0.3, 0.4])
        loss = 0
        for i in which:
            loss = loss + (i + 1) * (scene.render(cams[i]) ** 2).sum()
        loss.backward()
        return v.grad.cpu().numpy()

    both, separate = run([0, 1]), run([0]) + run([1])
    assert rel(both, separate) < 1e-9


def test_residual_adjoint_with_a_stale_generation_stamp(oracle_api):
    """render_backward(residual_obs=..., generation=<stale>) after ANOTHER forward has used the workspace: the adjoint needs the
    frame of ITS forward (2 (image - obs) is formed inside the kernels), not the later one's"""
    from hip_util import device_scene, rel_err
    from deodr_amd.hip_renderer import HipRasterizer

    a, b = scenes.soup_scene(n_tri=40, width=96, height=80, seed=5, flat=False), scenes.soup_scene(n_tri=40, width=96, height=80, seed=6, flat=False)
    for s in (a, b):
        s.backface_culling = True
    da, db = device_scene(a, F64), device_scene(b, F64)
    r = HipRasterizer.for_scene(da)
    obs = torch.as_tensor(np.random.RandomState(2).rand(1, 80, 96, 3), device=da.device)
    image_a, _ = r.render(da, 1.0, check_overflow=True)
    image_a = image_a.clone()
    gen_a = r.generation
    r.render(db, 1.0)  # the workspace (and r._last) now belong to scene b
    g = r.render_backward(da, residual_obs=obs, generation=gen_a, sigma=1.0)
    torch.cuda.synchronize()
    ref = checker(oracle_api)
    im, z = ref.render(a, 1.0)
    g_ref = ref.grads(a, 1.0, im, z, 2 * (image_a[0].cpu().numpy() - obs[0].cpu().numpy()))
    for k in ("ij_b", "colors_b"):
        assert rel_err(g[k][0].cpu().numpy(), g_ref[k]) < 1e-8, k


def test_graphed_fit_steps_follow_the_reference_curves():
    """GraphedStep: one HIP-graph replay per iteration (parameters, momentum, camera, lighting, rasterizer, rigid energy: nothing
    leaves the device, nothing is launched from the host but the graph).  The depth fit replays onto the reference's 50-iteration
    curve (251.327...); the colour fit equals the eager fitter step for step."""
    from deodr_amd.mesh_fitter import GraphedStep, MeshDepthFitter, MeshRGBFitterWithPose

    d = fixture("depth_hand_fit.npz")
    depth = d["depth_raw_f32"].astype(np.float64)
    depth[depth == 0] = float(d["max_depth"])
    vertices, faces = hand()

    def depth_fitter():
        f = MeshDepthFitter(vertices, faces, d["euler_init"], d["translation_init"], cregu=1000)
        f.set_image(depth / float(d["max_depth"]), focal=241, distortion=d["distortion"])
        f.set_max_depth(1)
        f.set_depth_scale(float(d["depth_scale"]))
        return f

    f = depth_fitter()
    g = GraphedStep(f, warmup=3)  # 3 + 1 eager steps and 1 on the capture stream: iterations 0 .. 4 (capturing executes nothing)
    assert f.iter == 5
    energies = [float(g.step_device()[0]) for _ in range(45)]  # iterations 5 .. 49
    assert f.iter == 50
    golden = d["energies"]
    assert np.abs(np.array(energies) - golden[5:50]).max() <= 5e-4 * golden.max()
    # (the fit is sensitive: the reference's own test accepts these final energies, tests/test_depth_image_hand_fitting.py:18-42)
    possible = (251.32711113732933, 251.32711113730954, 251.3271111242092, 251.32711067513003, 251.31652686512888, 251.31652686495823)
    assert min(abs(energies[-1] - r) for r in possible) < 1e-4

    r = fixture("rgb_hand_fit.npz")
    image_obs = r["image_u8"].astype(np.float64) / 255

    def rgb_fitter():
        f = MeshRGBFitterWithPose(r["vertices_centered"], faces, np.zeros(3), r["translation_init"], r["default_color"], r["default_light_directional"],
                                  float(r["default_light_ambient"]), cregu=1000)  # fmt: skip
        f.set_image(image_obs)
        f.set_background_color(r["background_color"])
        return f

    eager = rgb_fitter()
    e_eager = [float(eager.step_device()[0]) for _ in range(12)]
    graphed = GraphedStep(rgb_fitter(), warmup=3)  # iterations 0 .. 4 as above
    e_graph = [float(graphed.step_device()[0]) for _ in range(7)]
    assert np.abs(np.array(e_graph) - np.array(e_eager[5:])).max() <= 1e-6 * e_eager[0]
    assert np.abs(np.array(e_eager[:10]) - r["energies"][:10]).max() <= 1e-6 * r["energies"][0]


def test_fused_front_half_kernels_equal_the_torch_formulas(monkeypatch):
    """rigid transform, projection (+ distortion), silhouette flags, momentum update: the kernels of dr_fronthalf.h (values and
    adjoints) against the torch formulas of scene3d.py / mesh_fitter.py they replace on float64 ROCm tensors"""
    from deodr_amd import fronthalf
    from deodr_amd.mesh_fitter import _Momentum, qrot
    from deodr_amd.scene3d import DeviceCamera, MeshTopology

    rs = np.random.RandomState(0)
    vertices, faces = hand()
    n, V = 3, len(vertices)
    dev = "cuda"
    # ---- rigid transform
    vc = torch.tensor(vertices - vertices.mean(axis=0), device=dev, requires_grad=True)
    q = torch.tensor(rs.randn(n, 4), device=dev)
    q = (q / q.norm(dim=-1, keepdim=True)).requires_grad_(True)
    t = torch.tensor(rs.randn(n, 3), device=dev, requires_grad=True)
    w = torch.tensor(rs.randn(n, V, 3), device=dev)
    out = fronthalf.RigidTransformFunc.apply(vc, q, t)
    ref = qrot(q, vc[None].expand(n, -1, -1)) + t[:, None, :]
    assert rel(out.detach().cpu(), ref.detach().cpu()) < 1e-14
    g = torch.autograd.grad((out * w).sum(), [vc, q, t])
    g_ref = torch.autograd.grad((ref * w).sum(), [vc, q, t])
    for a, b in zip(g, g_ref):
        assert rel(a.cpu(), b.cpu()) < 1e-12
    # ---- projection with distortion, against the torch path of the same class
    rot = np.array([[1.0, 0, 0], [0, -1, 0], [0, 0, -1]])
    ext = np.stack([np.column_stack((rot, -rot.T.dot(vertices.mean(axis=0) + np.array([0.3 * i, 0, 8.0 + i]) * np.std(vertices)))) for i in range(n)])
    K = np.stack([np.array([[250.0 + 10 * i, 0.3, 64], [0, 240.0, 48 + i], [0, 0, 1]]) for i in range(n)])
    dist = np.stack([np.array([0.1, -0.02, 0.003, -0.004, 0.01]) * (i + 1) for i in range(n)])
    for distortion in (None, dist):
        cam = DeviceCamera(ext, K, 96, 128, distortion, dev)
        pts = torch.tensor(vertices[None] + 0.01 * rs.randn(n, V, 3), device=dev, requires_grad=True)
        wi, wd = torch.tensor(rs.randn(n, V, 2), device=dev), torch.tensor(rs.randn(n, V), device=dev)
        ij, depths = cam.project_points(pts)  # fused
        (g,) = torch.autograd.grad((ij * wi).sum() + (depths * wd).sum(), [pts])
        with monkeypatch.context() as m:
            m.setattr(fronthalf, "usable", lambda *a: False)
            ij_r, depths_r = cam.project_points(pts)  # torch ops
            (g_r,) = torch.autograd.grad((ij_r * wi).sum() + (depths_r * wd).sum(), [pts])
        assert rel(ij.detach().cpu(), ij_r.detach().cpu()) < 1e-13 and rel(depths.detach().cpu(), depths_r.detach().cpu()) < 1e-14
        assert rel(g.cpu(), g_r.cpu()) < 1e-11
    # ---- silhouette flags (closed sphere, open hand mesh with a boundary at the wrist)
    for verts, fcs in ((vertices, faces), scenes.bumpy_sphere(30, 24)):
        topo = MeshTopology(fcs, len(verts), clockwise=False, device=dev)
        cams = DeviceCamera(ext, K, 96, 128, None, dev)
        ij, _ = cams.project_points(torch.tensor(np.asarray(verts, dtype=np.float64) * (1.0 if len(verts) == V else 0.2) + vertices.mean(axis=0), device=dev))
        fused = topo.edge_on_silhouette(ij)
        with monkeypatch.context() as m:
            m.setattr(fronthalf, "usable", lambda *a: False)
            plain = topo.edge_on_silhouette(ij)
        assert fused.dtype == torch.uint8 and torch.equal(fused, plain) and int(fused.sum()) > 0
    # ---- momentum update (clamp, second gradient, per-row renormalisation)
    mom_a, mom_b = _Momentum(0.96, 0.05), _Momentum(0.96, 0.05)
    x = [torch.tensor(rs.randn(V, 3), device=dev), torch.tensor(rs.randn(n, 4), device=dev), torch.tensor(rs.randn(1), device=dev)]
    for step in range(3):
        grads = [torch.tensor(rs.randn(*t_.shape) * 1e3, device=dev) for t_ in x]
        g2 = torch.tensor(rs.randn(V, 3), device=dev)
        entries = [("v", x[0], grads[0], g2, 0.0005, 0.5, 0), ("q", x[1], grads[1], None, 0.00006, 0.1, 4), ("a", x[2], grads[2], None, 0.0001, None, 0)]
        new = mom_a.update_all(entries)
        with monkeypatch.context() as m:
            m.setattr(fronthalf, "usable", lambda *a: False)
            new_r = mom_b.update_all([(nm, xr, gr, g2r, f, sm, rows) for (nm, _x, gr, g2r, f, sm, rows), xr in zip(entries, x)])
        for a, b in zip(new, new_r):
            assert rel(a.cpu(), b.cpu()) < 1e-14
        x = new


def test_fit_iteration_kernels_equal_the_torch_formulas(monkeypatch):
    """vertex normals + luminosity and the rigid energy as kernels (dr_fititer.h), values and adjoints, against the torch formulas of
    scene3d.py they replace on float64 ROCm tensors; bit-reproducible run to run (no atomics on values)"""
    from deodr_amd import fronthalf
    from deodr_amd.scene3d import DeviceMesh, LaplacianRigidEnergyDevice, Scene3DDevice

    rs = np.random.RandomState(1)
    vertices, faces = hand()
    n, V = 3, len(vertices)
    dev = "cuda"
    for clockwise in (False, True):
        mesh = DeviceMesh(faces, vertices, clockwise=clockwise, colors=np.zeros((V, 3)), device=dev)
        scene = Scene3DDevice()
        scene.set_mesh(mesh)
        light = torch.tensor([0.3, -0.5, 0.6], device=dev, dtype=torch.float64, requires_grad=True)
        amb = torch.tensor(0.25, device=dev, dtype=torch.float64, requires_grad=True)
        scene.light_directional, scene.light_ambient = light, amb
        posed = torch.tensor(vertices[None] + 0.02 * rs.randn(n, V, 3), device=dev, requires_grad=True)
        w = torch.tensor(rs.randn(n, V), device=dev)
        lum = scene.vertices_luminosity(posed)  # kernel
        assert type(lum.grad_fn).__name__.startswith("VertexLuminosityFunc")
        g = torch.autograd.grad((lum * w).sum(), [posed, light, amb])
        g2 = torch.autograd.grad((scene.vertices_luminosity(posed) * w).sum(), [posed, light, amb])
        with monkeypatch.context() as m:
            m.setattr(fronthalf, "usable", lambda *a: False)
            lum_r = scene.vertices_luminosity(posed)  # torch ops
            g_r = torch.autograd.grad((lum_r * w).sum(), [posed, light, amb])
        assert rel(lum.detach().cpu(), lum_r.detach().cpu()) < 1e-13
        assert float((lum.detach() > amb.detach()).double().mean()) > 0.2  # (lit and unlit vertices both present)
        for a, b, c in zip(g, g_r, g2):
            assert rel(a.cpu(), b.cpu()) < 1e-11
            assert torch.equal(a, c)  # deterministic
        # a single posed mesh [V,3] goes the same way
        assert rel(scene.vertices_luminosity(posed[0]).detach().cpu(), lum_r[0].detach().cpu()) < 1e-13
    # ---- a closed mesh whose poles have 30 faces around them (lists longer than the eight lanes that share one), one view
    sv, sf = scenes.bumpy_sphere(30, 24)
    sv = np.asarray(sv, dtype=np.float64)
    mesh = DeviceMesh(sf, sv, colors=np.zeros((len(sv), 3)), device=dev)
    scene = Scene3DDevice()
    scene.set_mesh(mesh)
    scene.light_directional = torch.tensor([0.1, 0.7, -0.4], device=dev, dtype=torch.float64, requires_grad=True)
    scene.light_ambient = torch.tensor(0.1, device=dev, dtype=torch.float64, requires_grad=True)
    posed = torch.tensor(sv[None] * (1 + 0.05 * rs.randn(1, len(sv), 1)), device=dev, requires_grad=True)
    w = torch.tensor(rs.randn(1, len(sv)), device=dev)
    g = torch.autograd.grad((scene.vertices_luminosity(posed) * w).sum(), [posed, scene.light_directional, scene.light_ambient])
    sphere_energy = LaplacianRigidEnergyDevice(mesh.topology, sv, 10.0)
    es, gs = sphere_energy.evaluate(posed[0].detach())
    with monkeypatch.context() as m:
        m.setattr(fronthalf, "usable", lambda *a: False)
        g_r = torch.autograd.grad((scene.vertices_luminosity(posed) * w).sum(), [posed, scene.light_directional, scene.light_ambient])
        es_r, gs_r = sphere_energy.evaluate(posed[0].detach())
    for a, b in zip(g, g_r):
        assert rel(a.cpu(), b.cpu()) < 1e-11
    assert abs(float(es) - float(es_r)) <= 1e-12 * abs(float(es_r)) and rel(gs.cpu(), gs_r.cpu()) < 1e-12
    # ---- rigid energy
    mesh = DeviceMesh(faces, vertices, device=dev)
    energy = LaplacianRigidEnergyDevice(mesh.topology, vertices, 1000.0)
    x = torch.tensor(vertices + 0.01 * rs.randn(V, 3), device=dev, requires_grad=True)
    e, grad = energy.evaluate(x)
    (ge,) = torch.autograd.grad(e, [x])
    with monkeypatch.context() as m:
        m.setattr(fronthalf, "usable", lambda *a: False)
        e_r, grad_r = energy.evaluate(x)
        (ge_r,) = torch.autograd.grad(e_r, [x])
    assert abs(float(e) - float(e_r)) <= 1e-12 * abs(float(e_r)) and rel(grad.cpu(), grad_r.detach().cpu()) < 1e-12 and rel(ge.cpu(), ge_r.cpu()) < 1e-12
    assert torch.equal(energy.evaluate(x)[0], e.detach()) or float(energy.evaluate(x)[0]) == float(e)


def test_fit_front_equals_its_three_kernels():
    """deodr_hip_fit_front -- silhouette flags, vertex colours and the rigid energy of a fit iteration in ONE launch -- against the three
    separate launches, bit for bit, with every subset of the parts; the total energy the momentum update adds up on the way"""
    from deodr_amd import fronthalf
    from deodr_amd.scene3d import DeviceMesh

    rs = np.random.RandomState(5)
    vertices, faces = hand()
    n, V, dev = 3, len(vertices), "cuda"
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), device=dev)
    for clockwise in (False, True):
        topo = DeviceMesh(faces, vertices, clockwise=clockwise, device=dev).topology
        T = topo.nb_faces
        posed, ij = t(vertices[None] + 0.02 * rs.randn(n, V, 3)), t(100 * rs.rand(n, V, 2))
        x, ref = t(vertices + 0.01 * rs.randn(V, 3)), t(vertices)
        light, amb, color = t([0.3, -0.5, 0.6]), t(0.25), t([0.7, 0.5, 0.4])
        scratch = fronthalf.fit_scratch(V, n, dev)
        flags_r = fronthalf.silhouette_flags(ij, topo._faces_u32, topo._edge_faces, clockwise)
        colors_r, lum_r = torch.zeros((n, V, 3), dtype=torch.float64, device=dev), torch.zeros((n, V), dtype=torch.float64, device=dev)
        fronthalf.vertex_shade(posed, topo, light, amb, color, luminosity=lum_r, colors=colors_r)
        grad_r, energy_r = torch.zeros((V, 3), dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)
        fronthalf.rigid_energy(x, ref, topo, 500.0, grad_r, energy_r, scratch)
        assert 0 < int(flags_r.sum()) < flags_r.numel() and float(energy_r[0]) > 0
        for want_flags, want_shade, want_rigid in [(1, 1, 1), (1, 0, 1), (0, 1, 1), (1, 1, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0)]:
            flags = torch.full((n, T, 3), 7, dtype=torch.uint8, device=dev)
            colors, lum = torch.full_like(colors_r, -1), torch.full_like(lum_r, -1)
            grad, energy = torch.full_like(grad_r, -1), torch.full_like(energy_r, -1)
            fronthalf.fit_front(topo, n, scratch, ij=ij, flags=flags if want_flags else None, posed=posed, light=light, ambient=amb, color=color,
                                luminosity=lum if want_shade else None, colors=colors if want_shade else None, vertices=x, vertices_ref=ref, cregu=500.0,
                                gradient=grad if want_rigid else None, energy=energy)  # fmt: skip
            assert torch.equal(flags, flags_r) if want_flags else bool((flags == 7).all())
            assert (torch.equal(colors, colors_r) and torch.equal(lum, lum_r)) if want_shade else bool((colors == -1).all())
            if want_rigid:
                assert torch.equal(grad, grad_r) and float(energy[0]) == float(energy_r[0]) and float(energy[1]) == -1
            else:
                assert bool((grad == -1).all()) and bool((energy == -1).all())
        # energy[1] = data_weight * data energy + energy[0], by the momentum update
        data = t([3.25])
        xs, speed, g = t(rs.randn(5, 3)), t(np.zeros((5, 3))), t(rs.randn(5, 3))
        fronthalf.momentum_update([(xs, speed, g, None, 0.1, None, 0)], 0.9, 0.05, energy=energy_r, data_energy=data, data_weight=0.5)
        assert float(energy_r[1]) == 0.5 * 3.25 + float(energy_r[0])


def test_direct_fit_iteration_equals_the_autograd_iteration():
    """The fitters' iteration as a fixed kernel sequence (_DirectIteration, the default on float64 ROCm tensors) against the same
    iteration through autograd (``direct = False``): energies and every parameter, step by step, for the three fitters (the multi-frame
    one with its per-view poses and the shared block of gradients)"""
    from deodr_amd.mesh_fitter import MeshDepthFitter, MeshRGBFitterWithPose, MeshRGBFitterWithPoseMultiFrame

    vertices, faces = hand()
    d = fixture("depth_hand_fit.npz")
    depth = d["depth_raw_f32"].astype(np.float64)
    depth[depth == 0] = float(d["max_depth"])
    r = fixture("rgb_hand_fit.npz")
    rs = np.random.RandomState(2)

    def depth_fitter():
        f = MeshDepthFitter(vertices, faces, d["euler_init"], d["translation_init"], cregu=1000)
        f.set_image(depth / float(d["max_depth"]), focal=241, distortion=d["distortion"])
        f.set_max_depth(1)
        f.set_depth_scale(float(d["depth_scale"]))
        return f, ("vertices", "transform_quaternion", "transform_translation")

    def rgb_fitter():
        f = MeshRGBFitterWithPose(r["vertices_centered"], faces, np.zeros(3), r["translation_init"], r["default_color"], r["default_light_directional"],
                                  float(r["default_light_ambient"]), cregu=1000)  # fmt: skip
        f.set_image(r["image_u8"].astype(np.float64) / 255)
        f.set_background_color(r["background_color"])
        return f, ("vertices", "transform_quaternion", "transform_translation", "mesh_color", "light_directional", "light_ambient")

    images = [np.clip(r["image_u8"].astype(np.float64) / 255 + 0.05 * rs.randn(*r["image_u8"].shape), 0, 1) for _ in range(3)]

    def multi_fitter():
        eul = np.stack([np.array([0, a, 0]) for a in (-0.2, 0.0, 0.2)])
        f = MeshRGBFitterWithPoseMultiFrame(r["vertices_centered"], faces, eul, np.tile(r["translation_init"], (3, 1)), r["default_color"],
                                            r["default_light_directional"], float(r["default_light_ambient"]), cregu=2000)  # fmt: skip
        f.set_images(images)
        f.set_background_color(r["background_color"])
        return f, ("vertices", "transform_quaternion", "transform_translation", "mesh_color", "light_directional", "light_ambient")

    for build in (depth_fitter, rgb_fitter, multi_fitter):
        (a, names), (b, _) = build(), build()
        b.direct = False
        for step in range(6):
            out_a, out_b = a.step_device(), b.step_device()
            assert a._direct_state is not None and b._direct_state is None
            ea, eb = float(out_a[0]), float(out_b[0])
            assert abs(ea - eb) <= 1e-9 * abs(eb), (build.__name__, step, ea, eb)
            assert rel(out_a[1].to(torch.float64).cpu(), out_b[1].to(torch.float64).cpu()) < 1e-9
            for name in names:
                pa, pb = getattr(a, name).detach().cpu(), getattr(b, name).detach().cpu()
                assert rel(pa, pb) < 1e-9, (build.__name__, step, name)
        assert a.iter == b.iter == 6


def test_l2_loss_kernel():
    """sum (image - obs)^2 of a frame batch in either pixel type, accumulated in double, deterministic"""
    from deodr_amd import fronthalf

    g = torch.Generator(device="cuda").manual_seed(0)
    scratch = fronthalf.fit_scratch(100, 1, "cuda")
    for dtype, shape in ((torch.float64, (2, 301, 517, 3)), (torch.float32, (8, 1024, 1024, 3)), (torch.float32, (1, 7, 5, 1))):
        a, b = torch.rand(shape, dtype=dtype, device="cuda", generator=g), torch.rand(shape, dtype=dtype, device="cuda", generator=g)
        out, again = torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
        fronthalf.l2_loss(a, b, out, scratch)
        fronthalf.l2_loss(a, b, again, scratch)
        ref = float(((a.double() - b.double()) ** 2).sum())
        assert abs(float(out) - ref) <= 1e-12 * ref and float(out) == float(again)


def test_depth_residual_kernel():
    """clamp, residual, loss and its adjoint of the depth fitter's data term in one kernel (deodr/mesh_fitter.py:108-123)"""
    from deodr_amd import fronthalf

    g = torch.Generator(device="cuda").manual_seed(1)
    scratch = fronthalf.fit_scratch(100, 1, "cuda")
    for dtype in (torch.float64, torch.float32):
        image = (torch.rand((1, 200, 213, 1), dtype=torch.float64, device="cuda", generator=g) * 1.4 - 0.2).to(dtype)  # some below 0, some above 1
        image[0, 0, 0, 0], image[0, 0, 1, 0] = 0.0, 1.0  # the ends of the clamp pass the gradient
        obs = torch.rand((200, 213), dtype=torch.float64, device="cuda", generator=g)
        depth, diff, image_b = torch.empty_like(obs), torch.empty_like(obs), torch.empty_like(image)
        loss = torch.zeros(1, dtype=torch.float64, device="cuda")
        fronthalf.depth_residual(image, obs, 1.0, depth, diff, image_b, loss, scratch)
        x = image.to(torch.float64).requires_grad_(True)
        d_ref = x.clamp(0, 1.0)[0, :, :, 0]
        diff_ref = (d_ref - obs) ** 2
        (g_ref,) = torch.autograd.grad(diff_ref.sum(), [x])
        assert torch.equal(depth, d_ref.detach()) and rel(diff.cpu(), diff_ref.detach().cpu()) < 1e-15
        assert abs(float(loss) - float(diff_ref.sum())) <= 1e-12 * float(diff_ref.sum())
        assert rel(image_b.double().cpu(), g_ref.to(dtype).double().cpu()) < 1e-15 and float((image_b == 0).double().mean()) > 0.1


def test_pose_project_adjoint_sums_views_and_colours(monkeypatch):
    """deodr_hip_fit_pose_project(_b) against autograd through the torch formulas (centring, renormalised quaternions, projection
    with distortion); the optional sum of per-vertex colour adjoints over the views (bench.py's shared-gradient reduction)"""
    from deodr_amd import fronthalf
    from deodr_amd.mesh_fitter import qrot
    from deodr_amd.scene3d import DeviceCamera

    rs = np.random.RandomState(3)
    vertices, _faces = hand()
    n, V, C = 4, len(vertices), 3
    dev = "cuda"
    rot = np.array([[1.0, 0, 0], [0, -1, 0], [0, 0, -1]])
    ext = np.stack([np.column_stack((rot, -rot.T.dot(vertices.mean(axis=0) + np.array([0.3 * i, 0, 8.0 + i]) * np.std(vertices)))) for i in range(n)])
    K = np.stack([np.array([[250.0 + 10 * i, 0.3, 64], [0, 240.0, 48 + i], [0, 0, 1]]) for i in range(n)])
    dist = np.stack([np.array([0.1, -0.02, 0.003, -0.004, 0.01]) * (i + 1) for i in range(n)])
    cam = DeviceCamera(ext, K, 96, 128, dist, dev)
    v0 = torch.tensor(vertices + 0.01, device=dev)
    q = torch.tensor(rs.randn(n, 4) * 0.1 + np.array([0, 0, 0, 1.0]), device=dev, requires_grad=True)  # raw: not unit
    t = torch.tensor(rs.randn(n, 3) * 0.05, device=dev, requires_grad=True)
    wi, wd, wp = torch.tensor(rs.randn(n, V, 2), device=dev), torch.tensor(rs.randn(n, V), device=dev), torch.tensor(rs.randn(n, V, 3), device=dev)
    colors_b = torch.tensor(rs.randn(n, V, C), device=dev)
    # torch formulation
    x = v0.clone().requires_grad_(True)
    with monkeypatch.context() as m:
        m.setattr(fronthalf, "usable", lambda *a: False)
        centred = x - x.mean(dim=0, keepdim=True)
        posed_r = qrot(q / q.norm(dim=-1, keepdim=True), centred[None].expand(n, -1, -1)) + t[:, None, :]
        ij_r, depths_r = cam.project_points(posed_r)
        g_r = torch.autograd.grad((ij_r * wi).sum() + (depths_r * wd).sum() * 0.7 + (posed_r * wp).sum(), [x, q, t])
    # kernels
    xk, mean = v0.clone(), v0.mean(dim=0)
    posed, ij, depths, dcol = torch.empty((n, V, 3), dtype=torch.float64, device=dev), torch.empty((n, V, 2), dtype=torch.float64, device=dev), torch.empty((n, V), dtype=torch.float64, device=dev), torch.empty((n, V), dtype=torch.float64, device=dev)  # fmt: skip
    fronthalf.fit_pose_project(xk, mean, q.detach(), t.detach(), cam, posed, ij, depths, depth_colors=dcol, depth_scale=2.5)
    assert rel(xk.cpu(), (v0 - mean).cpu()) < 1e-15 and rel(posed.cpu(), posed_r.detach().cpu()) < 1e-13
    assert rel(ij.cpu(), ij_r.detach().cpu()) < 1e-13 and rel(depths.cpu(), depths_r.detach().cpu()) < 1e-14 and rel(dcol.cpu(), 2.5 * depths.cpu()) < 1e-15
    vertices_b, out = torch.empty((V, 3), dtype=torch.float64, device=dev), torch.empty(3 + 7 * n, dtype=torch.float64, device=dev)
    colors_sum = torch.empty((V, C), dtype=torch.float64, device=dev)
    scratch = fronthalf.fit_scratch(V, n, dev)
    for _ in range(2):  # (twice: the scratch counters must come back to zero)
        fronthalf.fit_pose_project_b(xk, q.detach(), posed, cam, wp, wi, wd, vertices_b, out, scratch, depths_b_scale=0.7, colors_b=colors_b, colors_sum=colors_sum)
    # the torch gradient w.r.t. x went through the centring: the projection on zero-mean displacements
    assert rel((vertices_b - out[:3]).cpu(), g_r[0].cpu()) < 1e-11
    assert rel(out[3 : 3 + 4 * n].view(n, 4).cpu(), g_r[1].cpu()) < 1e-10 and rel(out[3 + 4 * n :].view(n, 3).cpu(), g_r[2].cpu()) < 1e-11
    assert rel(colors_sum.cpu(), colors_b.sum(dim=0).cpu()) < 1e-15
    assert int(scratch[:64].view(torch.int32).abs().sum()) == 0


def test_examples_run(capsys):
    """examples/: the reference's four examples on the device path, a few iterations each; the depth fit lands on the reference's curve"""
    import importlib
    import sys as _sys

    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    _sys.path.insert(0, ex)
    try:
        depth = importlib.import_module("depth_image_hand_fitting").main(iterations=10)  # iterations 5 .. 14 (GraphedStep ran 0 .. 4)
        golden = fixture("depth_hand_fit.npz")["energies"]
        assert np.abs(depth - golden[5:15]).max() <= 1e-6 * golden.max()
        rgb = importlib.import_module("rgb_image_hand_fitting").main(iterations=6)
        assert np.abs(rgb - fixture("rgb_hand_fit.npz")["energies"][5:11]).max() <= 1e-6 * rgb[0]
        multi = importlib.import_module("rgb_multiview_hand").main(iterations=6, graph=False)
        assert np.abs(multi - fixture("rgb_multiview_fit.npz")["energies"][:6]).max() <= 1e-6 * multi[0]
        soup = importlib.import_module("triangle_soup_fitting").main(iterations=8)
        assert soup[-1] < soup[0]
    finally:
        _sys.path.remove(ex)


def test_fit_step_loss_from_the_rasterizer_kernels():
    """deodr_hip_render_scene_fit_ex with a loss: sum (image - obs)^2 from the tile walkers + the background table, against the sum over the
    frame the same call stored -- every tile class (pairs, tiles with edges fused or left to the edge kernel, more than 16 edges, tiny
    frames, frames that are no multiple of the tile), both pixel types, background colour and image, several views, a second step with
    the same table, and the two fall-backs (more than 4 channels, no triangle at all)"""
    from hip_util import device_scene
    from deodr_amd.hip_renderer import HipRasterizer

    g = torch.Generator(device="cuda").manual_seed(5)

    def check(views, dt, sigma=1.0, tol=1e-12):
        ds = device_scene(views, dt)
        r = HipRasterizer.for_scene(ds)
        shape = (ds.n_views, ds.height, ds.width, ds.nb_colors)
        obs = torch.rand(shape, dtype=dt, device=ds.device, generator=g)
        loss = torch.zeros(1, dtype=torch.float64, device=ds.device)
        for step in range(2):
            image, _z, _grads = r.render_fit(ds, obs, sigma, check_overflow=step == 0, clear_grads=True, loss_out=loss)
            ref = float(((image.double() - obs.double()) ** 2).sum())
            assert abs(float(loss) - ref) <= tol * ref, (views[0].height, views[0].width, dt, sigma, step, float(loss), ref)
        # the gradients are those of the call without the loss
        g1 = r.render_fit(ds, obs, sigma, clear_grads=True, loss_out=loss)[2]
        g1 = {k: v.clone() for k, v in g1.items() if v is not None}
        g0 = r.render_fit(ds, obs, sigma, clear_grads=True)[2]
        for k, v in g1.items():
            assert rel(v.cpu(), g0[k].cpu()) < 1e-9, k
        # another observation: another table
        obs2 = torch.rand(shape, dtype=dt, device=ds.device, generator=g)
        image, _z, _grads = r.render_fit(ds, obs2, sigma, clear_grads=True, loss_out=loss)
        ref = float(((image.double() - obs2.double()) ** 2).sum())
        assert abs(float(loss) - ref) <= tol * ref

    sphere = lambda **kw: [scenes.sphere_scene(angle=a, **kw) for a in kw.pop("angles", (0.0,))]
    check([scenes.sphere_scene(size=1024, angle=a) for a in (-0.3, 0.4)], F32, tol=1e-9)  # (float32 frames: the residuals are exact, their sum is double)
    check([scenes.sphere_scene(size=512, nu=60, n_rings=60, angle=a) for a in (-0.3, 0.0, 0.4)], F64)
    check([scenes.sphere_scene(size=512, nu=60, n_rings=60)], F64, sigma=2.5)  # more edges per tile
    check([scenes.sphere_scene(size=520, nu=60, n_rings=60)], F32, tol=1e-9)  # 65 tile columns: no pairs
    check([scenes.sphere_scene(size=96, nu=20, n_rings=16)], F64)  # tiny frame: one class of walkers
    check([scenes.sphere_scene(size=512, nu=60, n_rings=60, nb_colors=3, textured=True, texture_size=64, angle=a) for a in (0.0, 0.3)], F64)  # edge tiles NOT fused
    check([scenes.soup_scene(n_tri=150, width=203, height=117, seed=s, textured_ratio=0.3) for s in (3,)], F64)  # background image, ragged frame, all edges flagged
    check([scenes.sphere_scene(size=256, nu=40, n_rings=40, nb_colors=6, depth_channel=False)], F64)  # un-staged kernels: one pass over the frame
    far = scenes.sphere_scene(size=128, nu=20, n_rings=16)
    far.ij = far.ij + 5000.0  # nothing on the screen
    check([far], F64)

    # ---- with a clamp: L = sum (clamp(image, lo, hi) - obs)^2 (the depth fitter's data term): loss and gradients against the two-call
    # path fed with the residual formed in torch, for the staged kernels (pairs, fused edge tiles, a textured scene) and the un-staged ones
    def check_clamped(views, dt, lo, hi):
        ds = device_scene(views, dt)
        r = HipRasterizer.for_scene(ds)
        obs = torch.rand((ds.n_views, ds.height, ds.width, ds.nb_colors), dtype=dt, device=ds.device, generator=g)
        loss = torch.zeros(1, dtype=torch.float64, device=ds.device)
        image, _z, grads = r.render_fit(ds, obs, 1.0, check_overflow=True, clear_grads=True, loss_out=loss, clamp=(lo, hi))
        grads = {k: v.clone() for k, v in grads.items() if v is not None}
        clamped = image.double().clamp(lo, hi)
        ref = float(((clamped - obs.double()) ** 2).sum())
        inside = float(((image >= lo) & (image <= hi)).double().mean())
        assert 0.02 < inside < 0.98, inside  # (the clamp is active somewhere and passes somewhere)
        assert abs(float(loss) - ref) <= 1e-9 * ref
        image2, _z2 = r.render(ds, 1.0)
        assert torch.equal(image2, image)
        image_b = (2 * (clamped - obs.double()) * ((image >= lo) & (image <= hi))).to(dt)
        g_ref = r.render_backward(ds, image_b=image_b)
        for k, v in grads.items():
            assert rel(v.cpu(), g_ref[k].cpu()) < (1e-9 if dt == F64 else 1e-5), k

    check_clamped([scenes.sphere_scene(size=512, nu=60, n_rings=60, angle=a) for a in (-0.3, 0.4)], F64, 0.35, 0.8)
    check_clamped([scenes.sphere_scene(size=1024)], F32, 0.35, 0.8)
    check_clamped([scenes.sphere_scene(size=256, nu=40, n_rings=40, nb_colors=3, textured=True, texture_size=64)], F64, 0.3, 0.7)
    check_clamped([scenes.sphere_scene(size=256, nu=40, n_rings=40, nb_colors=6, depth_channel=False)], F64, 0.3, 0.7)


def test_float32_vertex_arrays_equal_float64_vertex_arrays_of_the_same_values():
    """vertex_dtype float32 (ij, depths, colours, shade, uv and their adjoints stored in float32: SURVEY 8d's "fp32 device buffers"):
    on inputs that are exactly representable in float32 the frames are those of the float64 arrays bit for bit (all arithmetic is double
    either way), the gradients agree to float32 accumulation; untextured (fused fit step) and textured (five-launch fit step), two-call path"""
    import copy

    from hip_util import device_scene
    from deodr_amd.hip_renderer import HipRasterizer

    def rounded(view):
        v = copy.deepcopy(view)
        for name in ("ij", "depths", "colors", "shade", "uv"):
            setattr(v, name, np.asarray(getattr(v, name), dtype=np.float64).astype(np.float32).astype(np.float64))
        return v

    g = torch.Generator(device="cuda").manual_seed(7)
    for views in ([scenes.sphere_scene(size=512, nu=60, n_rings=60, angle=a) for a in (-0.3, 0.4)],
                  [scenes.sphere_scene(size=256, nu=40, n_rings=40, nb_colors=3, textured=True, texture_size=64)]):  # fmt: skip
        views = [rounded(v) for v in views]
        results = {}
        for vd in (torch.float64, torch.float32):
            ds = device_scene(views, torch.float64, vertex_dtype=vd)
            assert ds.ij.dtype == vd and ds.colors.dtype == vd
            r = HipRasterizer.for_scene(ds)
            obs = torch.rand((ds.n_views, ds.height, ds.width, ds.nb_colors), dtype=torch.float64, device=ds.device, generator=torch.Generator(device="cuda").manual_seed(11))
            image, z, grads = r.render_fit(ds, obs, 1.0, check_overflow=True, clear_grads=True)
            fit = {k: v.double().clone() for k, v in grads.items() if v is not None}
            image2, _z2 = r.render(ds, 1.0)
            two = {k: v.double() for k, v in r.render_backward(ds, residual_obs=obs).items() if v is not None}
            assert all(v.dtype == vd for k, v in grads.items() if v is not None and k != "texture_b")
            results[vd] = (image.clone(), z.clone(), image2, fit, two)
        a, b = results[torch.float64], results[torch.float32]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        for which in (3, 4):
            for k in a[which]:
                assert rel(b[which][k].cpu(), a[which][k].cpu()) < 2e-6, (which, k)


def _run_bench(*args):
    """plain `python bench.py ...` (for --gpus N > 1 bench.py becomes its own torch.distributed.run launcher) -> the parsed JSON line"""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    run = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + list(args), cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, run.stdout[-2000:]  # rank 0 alone prints
    return json.loads(lines[0])


def test_bench_two_ranks_on_one_gpu():
    """bench.py --gpus 2 started WITHOUT a launcher, as the driver's N = 1 command is (round 4: AssertionError) -- it re-executes itself under
    torch.distributed.run: one process per rank, views sharded, overlapped reduction of the shared gradient, MAX over the ranks' times, ONE
    JSON line from rank 0 -- with two ranks that share this box's GPU and all-reduce over gloo (`--test-backend gloo`: RCCL refuses two
    ranks on one device).  The line's own checks must hold: the timed launch against the unmodified reference, the all-reduced gradient
    against a synchronous reduction."""
    out = _run_bench("--gpus", "2", "--steps", "6", "--warmup", "2", "--size", "256", "--views", "2", "--test-backend", "gloo", "--full")
    assert out["n_gpus"] == 2 and out["steps"] == 6 and out["warmup"] == 2 and out["scaling"] == "weak" and out["value"] > 0
    assert out["config"]["global_views"] == 4 and out["config"]["views_per_gpu"] == 2
    assert any("NOT a measurement" in o for o in out["config"]["env_overrides"])
    assert out["parity_checked"] is True
    assert out["reduction_check"]["ok"] and out["reduction_check"]["ranks"] == 2
    assert "cpu_baseline" not in out  # rank 0 at N = 1 only


def test_bench_two_ranks_textured_batch_strong_scaling():
    """--config 4 (BASELINE configs[4]'s shape at a small frame: 100k triangles, 1024^2 texture) --scaling strong: 4 views in all, two per rank;
    texture_b and uv_b are part of the ONE all-reduced buffer (float32, 12.6 MB + the vertex sums), checked against a synchronous
    reduction of the re-rendered step; the timed launch against the unmodified reference."""
    out = _run_bench("--gpus", "2", "--config", "4", "--scaling", "strong", "--steps", "3", "--warmup", "1", "--size", "256", "--views", "4",
                     "--test-backend", "gloo", "--time-every", "0", "--full")  # fmt: skip
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["config"]["global_views"] == 4 and out["config"]["views_per_gpu"] == 2
    assert "strong_scaling_floor" in out["config"] and "configs[4]" in out["config"]["workload"]
    rc = out["reduction_check"]
    assert rc["ok"] and rc["ranks"] == 2 and rc["dtype"] == "float32" and rc["parts"].startswith("texture_b") and rc["bytes"] > 4 * 1024 * 1024 * 3
    assert out["parity_checked"] is True and out["parity"]["rel_err_shade_b"] < 1e-4
