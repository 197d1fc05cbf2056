"""The callers either side of the rasterizer: camera, lighting, silhouette flags, normals, rigid energy, fitters.

Pinned on fixtures produced by the REFERENCE's own fitters (tests/golden/make_golden.py -> depth_hand_fit.npz, rgb_hand_fit.npz:
deodr/examples/depth_image_hand_fitting.py and rgb_image_hand_fitting.py with ``dl_library="none"``, instrumented at iteration 0).

* CPU part (no GPU): everything that is plain tensor algebra in deodr_amd/scene3d.py runs on CPU tensors too -- projection
  with distortion forward + adjoint, silhouette flags, vertex normals, luminosity forward + adjoint, Laplacian energy;
  and the view-sharded fitter's all-reduce on a world_size-2 gloo group.
* GPU part: the NumPy-level ``Scene3D`` / ``Camera`` / ``ColoredTriMesh`` drop-ins against the reference's intermediates, the
  reference's fit loop (deodr/mesh_fitter.py:139-196) written against those drop-ins, and the device-resident fitters, all against
  the reference's 50-iteration energy curves (last value = the golden of the reference's tests/test_depth_image_hand_fitting.py).
"""

import os
import socket

import numpy as np
import pytest
import torch

from conftest import GOLDEN

F64 = torch.float64


def fixture(name):
    return np.load(os.path.join(GOLDEN, name))


def hand():
    d = fixture("hand_mesh.npz")
    return d["vertices"], d["faces"].astype(np.int64)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ------------------------------------------------------------------------------------------------------------ CPU part


def test_compat_camera_helpers_cpu():
    """fields of view, camera-to-world matrix, left_mul_intrinsic, repr of the drop-in Camera against the reference's own values
    (tests/golden/scene3d_helpers.npz); plain NumPy members, no device involved"""
    import deodr_amd as deodr

    d = fixture("scene3d_helpers.npz")
    vertices, _ = hand()
    camera = deodr.default_camera(96, 80, 70, vertices, d["rot"])
    assert abs(camera.xfov - float(d["xfov"])) < 1e-12 and abs(camera.yfov - float(d["yfov"])) < 1e-12
    assert rel(camera.camera_to_world_mtx_4x4(), d["camera_to_world"]) < 1e-13
    assert rel(camera.left_mul_intrinsic(d["points"]), d["left_mul_intrinsic"]) < 1e-13
    assert repr(camera) == str(d["repr"])
    assert np.array_equal(camera.column_stack((np.arange(3), np.ones(3))), np.column_stack((np.arange(3), np.ones(3))))
    off_centre = deodr.Camera(camera.extrinsic, camera.intrinsic + np.array([[0, 0, 1.0], [0, 0, 0], [0, 0, 0]]), 80, 96)
    with pytest.raises(AssertionError):
        off_centre.xfov


def test_projection_distortion_forward_and_adjoint_cpu():
    """DeviceCamera.project_points with OpenCV distortion (dr.py:341-395) and its adjoint (dr.py:397-438, here autograd)"""
    from deodr_amd.scene3d import DeviceCamera

    d = fixture("depth_hand_fit.npz")
    cam = DeviceCamera(d["camera_extrinsic"], d["camera_intrinsic"], 200, 200, d["distortion"], device="cpu")
    pts = torch.tensor(d["it0_vertices_transformed"], dtype=F64, requires_grad=True)
    ij, depths = cam.project_points(pts)
    assert rel(ij[0].detach(), d["it0_ij"]) < 1e-12 and rel(depths[0].detach(), d["it0_depths"]) < 1e-12
    # render_depth_backward: vertices_b = project_points_backward(ij_b, depths_b = colors_b * depth_scale)   (dr.py:1046-1051)
    depths_b = torch.tensor(d["it0_colors_b"][:, 0] * float(d["depth_scale"]))
    (g,) = torch.autograd.grad([ij, depths], [pts], [torch.tensor(d["it0_ij_b"])[None], depths_b[None]])
    assert rel(g, d["it0_vertices_transformed_b"]) < 1e-10
    cam2 = DeviceCamera(d["camera_extrinsic"], d["camera_intrinsic"], 200, 200, None, device="cpu")  # no distortion: plain pinhole
    ij2, _ = cam2.project_points(pts.detach())
    p = pts.detach().numpy() @ d["camera_extrinsic"][:, :3].T + d["camera_extrinsic"][:, 3]
    expect = (p[:, :2] / p[:, 2:]) @ d["camera_intrinsic"][:2, :2].T + d["camera_intrinsic"][:2, 2]
    assert rel(ij2[0], expect) < 1e-13


def duck_fixture():
    d = fixture("duck.npz")
    return d, d["texture_u8"] / 255


def test_reference_duck_test_front_half_cpu(oracle_api):
    """The scene of the reference's tests/test_render_mesh.py::test_render_mesh_duck (textured duck, camera with radial
    distortion, directional light, sigma = 1, 320 x 240; tests/golden/duck.npz): the device front half on CPU tensors -- projection
    with distortion, vertex normals, luminosity, silhouette flags -- assembled into the Scene2D the reference builds (dr.py:896-983)
    and rasterized by the CPU checker must give the reference's image, i.e. its stored test image deodr/data/test/duck.png."""
    from deodr_amd import Scene2D
    from deodr_amd.scene3d import DeviceCamera, DeviceMesh, Scene3DDevice

    d, texture = duck_fixture()
    mesh = DeviceMesh(d["faces"], d["vertices"], clockwise=False, uv=d["uv"], faces_uv=d["faces_uv"], texture=texture, device="cpu")
    cam = DeviceCamera(d["extrinsic"], d["intrinsic"], 240, 320, d["distortion"], device="cpu")
    scene = Scene3DDevice()
    scene.set_mesh(mesh)
    scene.set_light(0.3 * np.array([1.0, -1.0, 0.0]), 0.0)
    ij, depths = cam.project_points(mesh.vertices)
    shade = scene.vertices_luminosity(mesh.vertices)
    flags = mesh.topology.edge_on_silhouette(ij)
    T, V = len(d["faces"]), len(d["vertices"])
    s2 = Scene2D(
        faces=d["faces"].astype(np.uint32), faces_uv=d["faces_uv"].astype(np.uint32), ij=ij[0].numpy(), depths=depths[0].numpy(),
        textured=np.ones(T, dtype=bool), uv=d["uv"], shade=shade.numpy(), colors=np.zeros((V, 3)), shaded=np.ones(T, dtype=bool),
        edgeflags=flags[0].numpy().astype(bool), height=240, width=320, nb_colors=3, texture=texture, background_color=np.array([0.8, 0.8, 0.8]),
        clockwise=False, backface_culling=True,
    )  # fmt: skip
    image, _ = (oracle_api.ref() or oracle_api.port()).render(s2, 1.0)
    assert np.abs(image - d["image"]).max() < 1e-6  # the fixture keeps the reference's image in float32
    assert np.abs((image * 255).astype(np.uint8).astype(int) - d["stored_u8"].astype(int)).max() == 0  # the reference test's own assertion


def test_read_and_save_obj_cpu(tmp_path):
    """deodr_amd.read_obj / save_obj (deodr/obj.py): v / f records, corners with texture and normal indices, relative indices,
    a continued line; the reference's hand.obj (tests/golden/hand.obj) gives the arrays of tests/golden/hand_mesh.npz"""
    import deodr_amd as deodr

    path = tmp_path / "m.obj"
    path.write_text("# comment\nv 0 0 0\nv 1 0 0\nvt 0.5 0.5\nvn 0 0 1\nv 0 1 0\nv 0 0 1.5\nf 1/1/1 2/1/1 3/1/1\nf -1 -2 \\\n -4\nf 1//1 4//1 2//1\n")
    faces, vertices = deodr.read_obj(str(path))
    assert vertices.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]] and faces.tolist() == [[0, 1, 2], [3, 2, 0], [0, 3, 1]]
    v, f = hand()
    deodr.save_obj(str(tmp_path / "hand.obj"), v, f)
    f2, v2 = deodr.read_obj(str(tmp_path / "hand.obj"))
    assert np.array_equal(f2, f) and np.array_equal(v2, v)
    f3, v3 = deodr.read_obj(os.path.join(GOLDEN, "hand.obj"))
    assert np.array_equal(f3, f) and np.array_equal(v3, v)


def test_element_count_of_arrays_and_tensors_cpu():
    """np.size of a tensor is a bound method, not a number: the scene containers count elements through one helper (a texture given
    as a device tensor -- what Scene3DDevice passes for a textured mesh -- used to raise in DeviceScene)"""
    from deodr_amd.hip_renderer import _count

    assert _count(None) == 0 and _count(np.zeros((0, 0))) == 0 and _count(np.zeros((4, 4, 3))) == 48
    assert _count(torch.zeros(2, 3)) == 6 and _count(torch.zeros(0, 0, 3)) == 0


def test_silhouette_flags_cpu():
    """edge_on_silhouette (triangulated_mesh.py:153-166): exactly the reference's flags, also batched over views"""
    from deodr_amd.scene3d import MeshTopology

    _, faces = hand()
    for name in ("depth_hand_fit.npz", "rgb_hand_fit.npz"):
        d = fixture(name)
        topo = MeshTopology(faces, 526, clockwise=False, device="cpu")
        flags = topo.edge_on_silhouette(torch.tensor(d["it0_ij"]))
        assert np.array_equal(flags.numpy().astype(bool), d["it0_edgeflags"])
    both = torch.tensor(np.stack([fixture("depth_hand_fit.npz")["it0_ij"], fixture("rgb_hand_fit.npz")["it0_ij"]]))
    flags = topo.edge_on_silhouette(both)
    assert np.array_equal(flags[0].numpy().astype(bool), fixture("depth_hand_fit.npz")["it0_edgeflags"])
    assert np.array_equal(flags[1].numpy().astype(bool), fixture("rgb_hand_fit.npz")["it0_edgeflags"])
    assert topo.is_manifold and topo.n_components == 1


def test_normals_and_luminosity_forward_and_adjoint_cpu():
    """vertex normals (triangulated_mesh.py:113-151), colours = colour x (max(0, -n.l) + ambient) (dr.py:814-831) and the adjoint of
    the whole front half of Scene3D.render_backward (dr.py:985-999): vertices, light and colour gradients of iteration 0"""
    from deodr_amd.scene3d import DeviceCamera, DeviceMesh, Scene3DDevice

    d = fixture("rgb_hand_fit.npz")
    _, faces = hand()
    mesh = DeviceMesh(faces, d["it0_vertices_transformed"], colors=np.tile(d["default_color"], (526, 1)), device="cpu")
    v = mesh.vertices.clone().requires_grad_(True)
    col = mesh.vertices_colors.clone().requires_grad_(True)
    ldir = torch.tensor(d["default_light_directional"], requires_grad=True)
    lamb = torch.tensor(float(d["default_light_ambient"]), dtype=F64, requires_grad=True)
    normals = mesh.topology.vertex_normals(v)
    assert rel(normals.detach(), d["it0_vertex_normals"]) < 1e-12
    scene = Scene3DDevice()
    scene.set_mesh(mesh)
    scene.light_directional, scene.light_ambient = ldir, lamb
    colors = col * scene.vertices_luminosity(v)[:, None]
    assert rel(colors.detach(), d["it0_colors"]) < 1e-12
    cam = DeviceCamera(d["camera_extrinsic"], d["camera_intrinsic"], 199, 200, None, device="cpu")
    ij, depths = cam.project_points(v)
    assert rel(ij[0].detach(), d["it0_ij"]) < 1e-12
    g_v, g_col, g_dir, g_amb = torch.autograd.grad([ij, colors], [v, col, ldir, lamb], [torch.tensor(d["it0_ij_b"])[None], torch.tensor(d["it0_colors_b"])])
    assert rel(g_v, d["it0_vertices_transformed_b"]) < 1e-9
    assert rel(g_col.sum(0), d["it0_mesh_color_b"]) < 1e-10
    assert rel(g_dir, d["it0_light_directional_b"]) < 1e-10 and abs(float(g_amb) - float(d["it0_light_ambient_b"])) < 1e-9 * abs(float(d["it0_light_ambient_b"]))


def test_laplacian_rigid_energy_cpu():
    """0.5 c d^T (L^T L x I3) d and its gradient (laplacian_rigid_energy.py:31-41) at the vertices of iteration 0"""
    from deodr_amd.mesh_fitter import _Momentum  # noqa: F401  (import check)
    from deodr_amd.scene3d import LaplacianRigidEnergyDevice, MeshTopology

    d = fixture("depth_hand_fit.npz")
    vertices, faces = hand()
    topo = MeshTopology(faces, 526, device="cpu")
    e = LaplacianRigidEnergyDevice(topo, vertices, float(d["cregu"]))
    v0 = vertices - vertices.mean(axis=0)  # MeshDepthFitter.step centres the vertices first (mesh_fitter.py:140)
    energy, grad = e.evaluate(torch.tensor(v0))
    assert abs(float(energy) - float(d["it0_energy_rigid"])) <= 1e-10 * max(1.0, abs(float(d["it0_energy_rigid"])))
    assert rel(grad, d["it0_grad_rigid"]) < 1e-10
    v = torch.tensor(v0 + 0.01 * np.random.RandomState(0).randn(*v0.shape), requires_grad=True)
    energy, grad = e.evaluate(v)
    (auto,) = torch.autograd.grad(energy, v)
    assert rel(grad.detach(), auto) < 1e-12  # the returned gradient IS the derivative of the returned energy


def _fitter_worker(rank, world, port, out_dir):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from deodr_amd.mesh_fitter import MeshRGBFitterWithPoseMultiFrame

    vertices, faces = hand()
    n_views = 5
    f = MeshRGBFitterWithPoseMultiFrame(vertices, faces, np.zeros((n_views, 3)), np.tile(vertices.mean(0), (n_views, 1)), np.array([0.4, 0.3, 0.25]),
                                        -np.array([0.1, 0.5, 0.4]), 0.6, cregu=1000, device="cpu")  # fmt: skip
    rs = np.random.RandomState(0)
    per_view = [[rs.randn(526, 3), rs.randn(3), rs.randn(3), rs.randn(), rs.rand()] for _ in range(n_views)]
    mine = [torch.as_tensor(np.sum([np.asarray(per_view[i][k]) for i in f.my_views], axis=0)) for k in range(5)]
    total = f._reduce_shared(mine)
    ok = f.my_views == ([0, 1, 2] if rank == 0 else [3, 4]) and f.transform_quaternion.shape == (len(f.my_views), 4)
    for k in range(5):
        ok = ok and np.allclose(total[k].numpy(), np.sum([np.asarray(per_view[i][k]) for i in range(n_views)], axis=0))
    with open(os.path.join(out_dir, f"ok{rank}"), "w") as fh:
        fh.write(str(int(ok)))
    dist.destroy_process_group()


def test_multiview_fitter_shards_views_and_allreduces_gloo_world2(tmp_path):
    """N > 1: the views of MeshRGBFitterWithPoseMultiFrame shard across the ranks, the shared gradients (vertices, colour, lights)
    and the energy are summed with ONE packed all-reduce (CPU tensors + gloo here, ROCm tensors + RCCL on the GPUs)"""
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_fitter_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert [open(tmp_path / f"ok{r}").read() for r in range(2)] == ["1", "1"]


# --------------------------------------------------------------- CPU part: whole fits, the checker standing in for the rasterizer


def test_depth_fitter_on_cpu_tensors_reproduces_reference_energies(oracle_api):
    """deodr_amd.mesh_fitter.MeshDepthFitter with CPU tensors and the CPU checker as its rasterizer (tests/cpu_raster.py): the
    reference's 50-iteration energy curve, i.e. the golden of its tests/test_depth_image_hand_fitting.py -- everything of the fitter
    but the HIP kernels, without a GPU"""
    import cpu_raster
    from deodr_amd.mesh_fitter import MeshDepthFitter

    d, depth_image = depth_inputs()
    vertices, faces = hand()
    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        fitter = MeshDepthFitter(vertices, faces, d["euler_init"], d["translation_init"], cregu=1000, device="cpu")
        fitter.set_image(depth_image, focal=241, distortion=d["distortion"])
        fitter.set_max_depth(1)
        fitter.set_depth_scale(float(d["depth_scale"]))
        energies = [fitter.step()[0] for _ in range(50)]
    check_depth_fit_curve(energies, d["energies"])
    assert rel(fitter.transform_quaternion[0], d["final_quaternion"]) < 1e-3


def test_rgb_fitter_on_cpu_tensors_follows_reference_energies(oracle_api):
    """MeshRGBFitterWithPose the same way, 20 iterations of the reference's colour fit"""
    import cpu_raster
    from deodr_amd.mesh_fitter import MeshRGBFitterWithPose

    d = fixture("rgb_hand_fit.npz")
    _, faces = hand()
    image_obs = d["image_u8"].astype(np.float64) / 255
    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        fitter = MeshRGBFitterWithPose(d["vertices_centered"], faces, np.zeros(3), d["translation_init"], d["default_color"], d["default_light_directional"],
                                       float(d["default_light_ambient"]), cregu=1000, device="cpu")  # fmt: skip
        fitter.set_image(image_obs)
        fitter.set_background_color(d["background_color"])
        energies = np.array([fitter.step()[0] for _ in range(20)])
    assert np.abs(energies[:10] - d["energies"][:10]).max() <= 1e-6 * d["energies"][0]
    assert np.abs(energies - d["energies"][:20]).max() <= 2e-2 * d["energies"][0]


def check_multiview_equals_single_views(device):
    """MeshRGBFitterWithPoseMultiFrame renders the views of a process in one batch; its data term is weighted by 1 / number of views
    (mesh_fitter.py:535), so with every view showing the same pose and image -- and the camera and momentum constants of the
    single-view class -- energy, images and the first vertex step equal the single-view fitter's, and the fit proceeds"""
    from deodr_amd.mesh_fitter import MeshRGBFitterWithPose, MeshRGBFitterWithPoseMultiFrame

    d = fixture("rgb_hand_fit.npz")
    _, faces = hand()
    image_obs = d["image_u8"].astype(np.float64) / 255
    args = (d["default_color"], d["default_light_directional"], float(d["default_light_ambient"]))
    n = 3
    single = MeshRGBFitterWithPose(d["vertices_centered"], faces, np.zeros(3), d["translation_init"], *args, cregu=1000, device=device)
    single.set_background_color(d["background_color"])
    single.set_image(image_obs)
    multi = MeshRGBFitterWithPoseMultiFrame(d["vertices_centered"], faces, np.zeros((n, 3)), np.tile(d["translation_init"], (n, 1)), *args, cregu=1000,
                                            inertia=0.96, damping=0.05, device=device)  # fmt: skip
    assert rel(multi.camera_center, d["vertices_centered"].mean(axis=0) + np.array([0, 0, 6]) * np.max(np.std(d["vertices_centered"], axis=0))) < 1e-14
    multi.camera_center = single.camera_center  # (the multi-frame class has its own, nearer camera: mesh_fitter.py:416)
    multi.set_background_color(d["background_color"])
    multi.set_images([image_obs] * n)
    e_multi, images, _ = multi.step()
    e_single, image, _ = single.step()
    assert images.shape == (n,) + image.shape and np.abs(images - image[None]).max() < 1e-9
    assert abs(e_multi - e_single) < 1e-9 * e_multi  # rigid energy is 0 at the first iteration
    sm, ss = multi.momentum.speed["vertices"].cpu().numpy(), single.momentum.speed["vertices"].cpu().numpy()
    assert np.abs(sm - ss).max() < 1e-9 * np.abs(ss).max()
    e = [multi.step()[0] for _ in range(5)]
    assert e[-1] < e_multi


def check_multiview_fit_against_reference(device, iterations=30):
    """The reference's deodr/examples/rgb_multiview_hand.py (three photographs, one pose per view, shared shape / colour / lights)
    through MeshRGBFitterWithPoseMultiFrame against the energies of the reference's own class with its two defects repaired
    (tests/golden/make_golden.py::rgb_multiview_fit): iteration-0 gradients, the curve, the fitted parameters"""
    from deodr_amd.mesh_fitter import MeshRGBFitterWithPoseMultiFrame

    d = fixture("rgb_multiview_fit.npz")
    _, faces = hand()
    images = [im.astype(np.float64) / 255 for im in d["images_u8"]]
    fitter = MeshRGBFitterWithPoseMultiFrame(d["vertices_centered"], faces, d["euler_init"], d["translation_init"], d["default_color"],
                                             d["default_light_directional"], float(d["default_light_ambient"]), cregu=2000, device=device)  # fmt: skip
    fitter.set_images(images)
    fitter.set_background_color(np.zeros(3))
    assert rel(fitter.camera.extrinsic[0].cpu(), d["camera_extrinsic"]) < 1e-13 and rel(fitter.camera.intrinsic[0].cpu(), d["camera_intrinsic"]) < 1e-13
    energies = []
    for it in range(iterations):
        energies.append(fitter.step()[0])
        if it == 0:  # what the first step saw: the speeds are (1 - damping)(1 - inertia) clamp(-factor gradient)
            s = fitter.momentum.speed
            k = (1 - 0.15) * (1 - 0.97)
            assert rel(s["quaternion"].cpu(), k * np.clip(-0.00005 * d["it0_quaternion_b"], -0.05, 0.05)) < 1e-8
            assert rel(s["translation"].cpu(), k * np.clip(-0.00004 * d["it0_translation_b"], -0.1, 0.1)) < 1e-8
            assert rel(s["light_directional"].cpu(), k * -0.0001 * d["it0_light_directional_b"]) < 1e-8
            assert rel(s["mesh_color"].cpu(), k * -0.00001 * d["it0_mesh_color_b"]) < 1e-8
            assert abs(float(s["light_ambient"]) - k * -0.0001 * float(d["it0_light_ambient_b"])) < 1e-8 * abs(k * 0.0001 * float(d["it0_light_ambient_b"]))
    energies, golden = np.array(energies), d["energies"][:iterations]
    assert np.abs(energies[:10] - golden[:10]).max() <= 1e-6 * golden[0]
    # (the float64 atomics of the HIP adjoint sum in a run-dependent order: 1e-16 at the first step, amplified by the fit -- the same
    # head-tight / tail-loose comparison as for the single-view colour fit)
    assert np.abs(energies - golden).max() <= 2e-2 * golden[0]
    if iterations == 30:
        assert rel(fitter.transform_translation.cpu(), d["final_translation"]) < 5e-2 and rel(fitter.mesh_color.cpu(), d["final_mesh_color"]) < 5e-2


def check_torch_optimizer_depth_fit(device):
    """MeshDepthFitterEnergy / MeshDepthFitterPytorchOptim (deodr/pytorch/mesh_fitter_pytorch.py:34-170): the module's energy at the
    initial parameters is the reference fitter's first energy; L-BFGS steps through autograd bring it down"""
    from deodr_amd.pytorch import MeshDepthFitterPytorchOptim

    d, depth_image = depth_inputs()
    vertices, faces = hand()
    opt = MeshDepthFitterPytorchOptim(vertices, faces, d["euler_init"], d["translation_init"], cregu=1000, device=device)
    opt.set_image(depth_image, focal=241, distortion=d["distortion"])
    opt.set_max_depth(1)
    opt.set_depth_scale(float(d["depth_scale"]))
    assert [tuple(p.shape) for p in opt.energy.parameters()] == [(526, 3), (4,), (3,)]
    assert abs(float(opt.energy().detach()) - d["energies"][0]) < 1e-9 * d["energies"][0]
    energies = [float(opt.step()[0]) for _ in range(5)]
    energy, depth, diff_image = opt.step()
    assert depth.shape == (200, 200) and diff_image.shape == (200, 200) and float(energy) < 0.5 * energies[0]


def test_torch_optimizer_depth_fit_on_cpu_tensors(oracle_api):
    import cpu_raster

    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        check_torch_optimizer_depth_fit("cpu")


def test_multiview_fitter_on_cpu_tensors_equals_single_views(oracle_api):
    import cpu_raster

    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        check_multiview_equals_single_views("cpu")


def test_multiview_fitter_on_cpu_tensors_follows_the_repaired_reference(oracle_api):
    import cpu_raster

    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        check_multiview_fit_against_reference("cpu", iterations=12)


def _sharded_fit_worker(rank, world, port, out_dir):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import cpu_raster
    from deodr_amd.mesh_fitter import MeshRGBFitterWithPoseMultiFrame
    from oracle import api

    d = fixture("rgb_multiview_fit.npz")
    _, faces = hand()
    images = [im.astype(np.float64) / 255 for im in d["images_u8"]]
    with cpu_raster.emulate(api.ref() or api.port()):
        fitter = MeshRGBFitterWithPoseMultiFrame(d["vertices_centered"], faces, d["euler_init"], d["translation_init"], d["default_color"],
                                                 d["default_light_directional"], float(d["default_light_ambient"]), cregu=2000, device="cpu")  # fmt: skip
        fitter.set_images(images)
        fitter.set_background_color(np.zeros(3))
        energies = [fitter.step()[0] for _ in range(4)]
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), energies=np.array(energies), vertices=fitter.vertices.numpy(), views=np.array(fitter.my_views),
             translation=fitter.transform_translation.numpy(), color=fitter.mesh_color.numpy())  # fmt: skip
    dist.destroy_process_group()


def test_sharded_multiview_fit_on_two_gloo_ranks_equals_the_reference_curve(tmp_path):
    """N > 1 end to end: the three views of the reference's multi-view example sharded over TWO processes (views 0, 1 / view 2), each
    rank rendering its own views (checker as rasterizer, CPU tensors) and all-reducing the shared gradients over gloo: both ranks
    follow the (repaired) reference's energy curve and hold the same shape and colour; the poses stay with their rank"""
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_sharded_fit_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    golden = fixture("rgb_multiview_fit.npz")["energies"][:4]
    assert list(r0["views"]) == [0, 1] and list(r1["views"]) == [2]
    for r in (r0, r1):
        assert np.abs(r["energies"] - golden).max() <= 1e-6 * golden[0]
    assert np.abs(r0["vertices"] - r1["vertices"]).max() < 1e-12 and np.abs(r0["color"] - r1["color"]).max() < 1e-14
    assert r0["translation"].shape == (2, 3) and r1["translation"].shape == (1, 3)


# ------------------------------------------------------------------------------------------------------------ GPU part


# The reference's depth fit is sensitive: its own test accepts a SET of final energies (tests/test_depth_image_hand_fitting.py:18-24,
# 36-42: 251.3271... or 251.3165... depending on library and rounding).  Our gradient accumulators are float64 atomics whose
# summation order varies from run to run (1e-16 relative); the fit amplifies that to ~1e-5 by iteration 20 and, one run in six,
# into the reference's other basin.  So: the first iterations are compared tightly, the whole curve loosely, and the final energy
# against the reference's own list of possible results with the reference's own tolerance.
REFERENCE_POSSIBLE_RESULTS = [251.32711067513003, 251.31652686512888, 251.31652686495823, 251.32711113732933, 251.32711113730954, 251.3271111242092]


def check_depth_fit_curve(energies, golden):
    energies = np.asarray(energies)
    assert np.abs(energies[:8] - golden[:8]).max() <= 1e-9 * golden.max()
    assert np.abs(energies - golden).max() <= 5e-4 * golden.max()
    assert min(abs(energies[49] - r) for r in REFERENCE_POSSIBLE_RESULTS) < 1e-4


def depth_inputs():
    d = fixture("depth_hand_fit.npz")
    depth = d["depth_raw_f32"].astype(np.float64)
    depth[depth == 0] = float(d["max_depth"])
    return d, depth / float(d["max_depth"])


# the four helpers of deodr/tools.py the reference's fitters use (qrot :8-22, qrot_backward :25-35, normalize :38-41,
# normalize_backward :44-49), restated for the drop-in test below
def qrot(q, v):
    uv = np.cross(q[:3], v)
    return v + 2 * (q[3] * uv + np.cross(q[:3], uv))


def qrot_backward(q, v, vr_b):
    uv = np.cross(q[:3], v)
    uuv_b = 2 * vr_b
    uv_b = 2 * vr_b * q[3] + np.cross(uuv_b, q[:3])
    q_b = np.zeros(4)
    q_b[3] = 2 * np.sum(vr_b * uv)
    q_b[:3] = np.sum(np.cross(uv, uuv_b), axis=0) + np.sum(np.cross(v, uv_b), axis=0)
    return q_b, vr_b + np.cross(uv_b, q[:3])


def normalize(x):
    return x / np.sqrt(np.sum(x**2))


def normalize_backward(x, xn_b):
    inv_n = 1 / np.sqrt(np.sum(x**2))
    return (xn_b - x * np.sum(xn_b * x) * inv_n**2) * inv_n


def check_dropin_scene3d_depth_intermediates(device):
    """NumPy-level drop-ins (deodr_amd.Scene3D / Camera / ColoredTriMesh) on iteration 0 of the reference's depth fit: projected
    points, silhouette flags, depth image, and the vertex gradient of render_depth_backward"""
    from deodr_amd import Camera, ColoredTriMesh, Scene3D

    d, depth_image = depth_inputs()
    _, faces = hand()
    mesh = ColoredTriMesh(faces, vertices=d["it0_vertices_transformed"], colors=np.zeros((526, 0)), device=device)
    scene = Scene3D()
    scene.set_mesh(mesh)
    scene.set_background_color(np.array([1.0]))
    camera = Camera(extrinsic=d["camera_extrinsic"], intrinsic=d["camera_intrinsic"], distortion=d["distortion"], height=200, width=200)
    depth = scene.render_depth(camera, depth_scale=float(d["depth_scale"]))
    assert np.abs(depth - d["it0_depth_image"]).max() < 1e-9
    assert rel(scene.scene_2d.ij, d["it0_ij"]) < 1e-12 and np.array_equal(scene.scene_2d.edgeflags, d["it0_edgeflags"])
    clipped = np.clip(depth, 0, 1)
    depth_b = 2 * (clipped - depth_image[:, :, None])
    depth_b[depth < 0] = 0
    depth_b[depth > 1] = 0
    scene.clear_gradients()
    scene.render_depth_backward(depth_b)
    assert rel(scene.scene_2d.ij_b, d["it0_ij_b"]) < 1e-8 and rel(scene.scene_2d.colors_b, d["it0_colors_b"]) < 1e-8
    assert rel(mesh._vertices_b, d["it0_vertices_transformed_b"]) < 1e-8


def check_dropin_scene3d_rgb_intermediates(device):
    """Scene3D.render / render_backward with lights (iteration 0 of the reference's colour fit): image, vertex / light / colour
    gradients -- the result attributes the reference's fitters read (mesh_fitter.py:291-296)"""
    from deodr_amd import Camera, ColoredTriMesh, Scene3D

    d = fixture("rgb_hand_fit.npz")
    _, faces = hand()
    image_obs = d["image_u8"].astype(np.float64) / 255
    mesh = ColoredTriMesh(faces, vertices=d["it0_vertices_transformed"], nb_colors=3, device=device)
    mesh.set_vertices_colors(np.tile(d["default_color"], (526, 1)))
    scene = Scene3D()
    scene.set_mesh(mesh)
    scene.set_light(light_directional=d["default_light_directional"], light_ambient=float(d["default_light_ambient"]))
    scene.set_background_color(d["background_color"])
    camera = Camera(extrinsic=d["camera_extrinsic"], intrinsic=d["camera_intrinsic"], height=199, width=200)
    image = scene.render(camera)
    assert np.abs(image - d["it0_image"]).max() < 1e-9
    assert abs(np.sum((image - image_obs) ** 2) - (d["energies"][0] - 0.0)) < 1e-6 * d["energies"][0]  # E_rigid = 0 at iteration 0
    scene.clear_gradients()
    scene.render_backward(2 * (image - image_obs))
    assert rel(mesh._vertices_b, d["it0_vertices_transformed_b"]) < 1e-8
    assert rel(np.sum(mesh.vertices_colors_b, axis=0), d["it0_mesh_color_b"]) < 1e-8
    assert rel(scene.light_directional_b, d["it0_light_directional_b"]) < 1e-8
    assert abs(scene.light_ambient_b - float(d["it0_light_ambient_b"])) < 1e-8 * abs(float(d["it0_light_ambient_b"]))


def check_reference_fit_loop_runs_on_the_dropins(device):
    """The reference's MeshDepthFitter.step (deodr/mesh_fitter.py:139-196), restated here against deodr_amd's Scene3D / Camera /
    ColoredTriMesh / LaplacianRigidEnergy instead of DEODR's: 50 iterations reproduce the reference's own energy curve, whose
    last value is the golden of the reference's tests/test_depth_image_hand_fitting.py:36-42 (251.32711113...)."""
    from deodr_amd import Camera, ColoredTriMesh, LaplacianRigidEnergy, Scene3D

    d, depth_image = depth_inputs()
    vertices0, faces = hand()
    mesh = ColoredTriMesh(faces, vertices=vertices0, colors=np.zeros((526, 0)), device=device)
    scene = Scene3D()
    scene.set_mesh(mesh)
    scene.set_background_color(np.array([1.0]))
    rigid = LaplacianRigidEnergy(mesh, vertices0, 1000)
    camera = Camera(extrinsic=d["camera_extrinsic"], intrinsic=d["camera_intrinsic"], distortion=d["distortion"], height=200, width=200)
    vertices, q, t = vertices0.copy(), d["quaternion_init"].copy(), d["translation_init"].copy()
    speed_v, speed_q, speed_t = np.zeros_like(vertices), np.zeros(4), np.zeros(3)
    inertia, damping = 0.96, 0.05
    clamp = lambda x, a, lim: np.minimum(np.maximum(x * a, -lim), lim)
    energies = []
    for _ in range(50):
        vertices = vertices - vertices.mean(axis=0)[None, :]
        qn = normalize(q)
        mesh.set_vertices(qrot(qn, vertices) + t)
        depth_raw = scene.render_depth(camera, depth_scale=float(d["depth_scale"]))
        depth = np.clip(depth_raw, 0, 1)
        energy_data = np.sum((depth - depth_image[:, :, None]) ** 2)
        depth_b = 2 * (depth - depth_image[:, :, None])
        scene.clear_gradients()
        depth_b[depth_raw < 0] = 0
        depth_b[depth_raw > 1] = 0
        scene.render_depth_backward(depth_b)
        vt_b = scene.mesh._vertices_b
        t_b = np.sum(vt_b, axis=0)
        qn_b, v_b = qrot_backward(qn, vertices, vt_b)
        q_b = normalize_backward(q, qn_b)
        v_b = v_b - v_b.mean(axis=0)[None, :]
        energy_rigid, grad_rigid, _ = rigid.evaluate(vertices)
        energies.append(energy_data + energy_rigid)
        speed_v = (1 - damping) * (speed_v * inertia + (1 - inertia) * clamp(-(v_b + grad_rigid), 0.0005, 1))
        vertices = vertices + speed_v
        speed_q = (1 - damping) * (speed_q * inertia + (1 - inertia) * clamp(-q_b, 0.00006, 0.1))
        q = q + speed_q
        q = q / np.linalg.norm(q)
        speed_t = (1 - damping) * (speed_t * inertia + (1 - inertia) * clamp(-t_b, 0.00005, 0.1))
        t = t + speed_t
    check_depth_fit_curve(energies, d["energies"])


@pytest.mark.gpu
@pytest.mark.parametrize("pixel_dtype", [torch.float64, torch.float32])
def test_device_depth_fitter_reproduces_reference_energies(pixel_dtype):
    """deodr_amd.mesh_fitter.MeshDepthFitter (nothing leaves the device inside a step) against the reference's curve"""
    from deodr_amd.mesh_fitter import MeshDepthFitter

    d, depth_image = depth_inputs()
    vertices, faces = hand()
    fitter = MeshDepthFitter(vertices, faces, d["euler_init"], d["translation_init"], cregu=1000, pixel_dtype=pixel_dtype)
    fitter.set_image(depth_image, focal=241, distortion=d["distortion"])
    fitter.set_max_depth(1)
    fitter.set_depth_scale(float(d["depth_scale"]))
    assert rel(fitter.transform_quaternion_init[0].cpu(), d["quaternion_init"]) < 1e-14
    energies = [fitter.step()[0] for _ in range(50)]
    if pixel_dtype == torch.float64:
        check_depth_fit_curve(energies, d["energies"])
        assert rel(fitter.transform_quaternion[0].cpu(), d["final_quaternion"]) < 1e-3
    else:  # float32 frames: the rounding of the image feeds back into the trajectory from the first step on (the fit is
        # sensitive: the reference's own test accepts several final energies); same curve within 0.5 % of its range, same end
        # within 1 %, head of the curve tight
        e = np.array(energies)
        assert np.abs(e[:5] - d["energies"][:5]).max() <= 1e-6 * d["energies"][0]
        assert np.abs(e - d["energies"]).max() <= 5e-3 * d["energies"].max() and abs(e[49] - 251.32) < 2.5


@pytest.mark.gpu
def test_device_rgb_fitter_follows_reference_energies():
    """MeshRGBFitterWithPose on the device.  The reference calls this fit chaotic: the first iterations are compared
    tightly, the whole curve loosely, and the energy has to come down like the reference's."""
    from deodr_amd.mesh_fitter import MeshRGBFitterWithPose

    d = fixture("rgb_hand_fit.npz")
    _, faces = hand()
    image_obs = d["image_u8"].astype(np.float64) / 255
    fitter = MeshRGBFitterWithPose(d["vertices_centered"], faces, np.zeros(3), d["translation_init"], d["default_color"], d["default_light_directional"],
                                   float(d["default_light_ambient"]), cregu=1000)  # fmt: skip
    fitter.set_image(image_obs)
    fitter.set_background_color(d["background_color"])
    assert rel(fitter.camera.extrinsic[0].cpu(), d["camera_extrinsic"]) < 1e-13
    energies = np.array([fitter.step()[0] for _ in range(50)])
    assert np.abs(energies[:10] - d["energies"][:10]).max() <= 1e-6 * d["energies"][0]
    assert np.abs(energies - d["energies"]).max() <= 2e-2 * d["energies"][0]
    assert energies[49] < 0.6 * energies[0]


@pytest.mark.gpu
def test_silhouette_flags_and_projection_batched_on_device():
    """the device ops on ROCm tensors, 8 views in one call, against per-view NumPy restatements of the reference's formulas"""
    from deodr_amd import scenes
    from deodr_amd.scene3d import DeviceCamera, MeshTopology

    vertices, faces = scenes.bumpy_sphere(40, 40)
    cams = [scenes.fit_camera(256, 256, 60.0, vertices, scenes.rotx(0.37) @ scenes.roty(0.23 + a)) for a in np.linspace(-0.5, 0.5, 8)]
    cam = DeviceCamera(np.stack([c.extrinsic for c in cams]), np.stack([c.intrinsic for c in cams]), 256, 256)
    topo = MeshTopology(faces, len(vertices), clockwise=False)
    ij, depths = cam.project_points(torch.as_tensor(vertices, device="cuda"))
    flags = topo.edge_on_silhouette(ij).cpu().numpy().astype(bool)
    for i, c in enumerate(cams):
        ij_ref, d_ref = scenes.project(c, vertices)
        assert rel(ij[i].cpu(), ij_ref) < 1e-12 and rel(depths[i].cpu(), d_ref) < 1e-12
        assert np.array_equal(flags[i], scenes.silhouette_edgeflags(ij_ref, faces, False))


@pytest.mark.gpu
def test_dropin_scene3d_render_deferred():
    """Scene3D.render_deferred (dr.py:1053-1174) through the drop-ins: a 15-channel untextured soup render at sigma = 0 (the
    un-staged kernels: nb_colors > 4), every buffer against the reference's own output (tests/golden/deferred_hand.npz)"""
    import deodr_amd as deodr

    d = fixture("deferred_hand.npz")
    vertices, faces = hand()
    mesh = deodr.ColoredTriMesh(faces.copy(), vertices=vertices, nb_colors=3)
    mesh.set_vertices_colors(d["colors"])
    camera = deodr.default_camera(96, 80, 70, mesh.vertices, d["rot"])
    assert rel(camera.extrinsic, d["extrinsic"]) < 1e-13 and rel(camera.intrinsic, d["intrinsic"]) < 1e-13
    scene = deodr.Scene3D(sigma=0)
    scene.set_light(light_directional=np.array([-0.1, -0.5, -0.4]), light_ambient=0.3)
    scene.set_mesh(mesh)
    scene.set_background_color([0.2, 0.3, 0.4])
    buffers = scene.render_deferred(camera, depth_scale=0.5)
    assert list(buffers.keys()) == [str(k) for k in d["order"]]
    for k, v in buffers.items():
        ref = d["buf_" + k]
        assert v.shape == ref.shape, k
        assert np.abs(v - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), k
    # flat per triangle: the same owner at every pixel (the values carry the rounding of the plane coefficients, which depends on the
    # last bit of the projected vertices: the fused projection kernel and the reference's NumPy do not round identically)
    assert np.array_equal(np.round(buffers["face_id"]), np.round(d["buf_face_id"]))


@pytest.mark.gpu
def test_dropin_scene3d_luminosity_and_adjoint():
    """Scene3D.compute_vertices_luminosity / _backward (dr.py:814-850) against the reference's values on the hand mesh"""
    import deodr_amd as deodr

    d = fixture("scene3d_helpers.npz")
    vertices, faces = hand()
    mesh = deodr.ColoredTriMesh(faces.copy(), vertices=vertices, nb_colors=3)
    mesh.compute_vertex_normals()
    assert rel(mesh.vertex_normals, d["vertex_normals"]) < 1e-12
    scene = deodr.Scene3D(sigma=1)
    scene.set_light(light_directional=d["light"], light_ambient=0.3)
    scene.set_mesh(mesh)
    assert rel(scene.compute_vertices_luminosity(), d["luminosity"]) < 1e-12
    scene.compute_vertices_luminosity_backward(d["luminosity_b"])
    assert rel(scene.light_directional_b, d["light_directional_b"]) < 1e-12
    assert rel(scene.vertex_normals_b, d["vertex_normals_b"]) < 1e-12
    assert abs(scene.light_ambient_b - float(d["light_ambient_b"])) < 1e-10
    scene.set_light(light_directional=None, light_ambient=0.3)
    assert np.allclose(scene.compute_vertices_luminosity(), 0.3)
    scene.compute_vertices_luminosity_backward(d["luminosity_b"])
    assert abs(scene.light_ambient_b - d["luminosity_b"].sum()) < 1e-10


def check_reference_duck_test_through_the_dropins(device):
    """The reference's tests/test_render_mesh.py::test_render_mesh_duck through the drop-in classes and the rasterizer: the
    textured duck (ColoredTriMesh with uv / faces_uv / texture), `default_camera` + radial distortion, `Scene3D.render` -- compared
    with the image the reference renders and with its stored test image (exact in uint8, the reference test's assertion)."""
    import deodr_amd as deodr

    d, texture = duck_fixture()
    mesh = deodr.ColoredTriMesh(d["faces"], d["vertices"], clockwise=False, faces_uv=d["faces_uv"], uv=d["uv"], texture=texture, device=device)
    camera = deodr.default_camera(320, 240, 80, mesh.vertices, d["rot"])
    assert rel(camera.extrinsic, d["extrinsic"]) < 1e-13 and rel(camera.intrinsic, d["intrinsic"]) < 1e-13
    camera.distortion = np.array([-0.5, 0.5, 0, 0, 0])
    scene = deodr.Scene3D()
    scene.set_light(light_directional=0.3 * np.array([1, -1, 0]), light_ambient=0)
    scene.set_mesh(mesh)
    scene.set_background_color(np.array((0.8, 0.8, 0.8)))
    image = scene.render(camera)
    assert image.shape == (240, 320, 3)
    assert np.abs(image - d["image"]).max() < 1e-6
    different = (image * 255).astype(np.uint8).astype(int) - d["stored_u8"].astype(int)
    assert np.abs(different).max() <= 1 and np.count_nonzero(different) <= 3  # a value within 1e-13 of a grey-level boundary may round the other way


DROPIN_CHECKS = [check_dropin_scene3d_depth_intermediates, check_dropin_scene3d_rgb_intermediates, check_reference_fit_loop_runs_on_the_dropins,
                 check_reference_duck_test_through_the_dropins]  # fmt: skip


@pytest.mark.gpu
@pytest.mark.parametrize("check", DROPIN_CHECKS, ids=lambda f: f.__name__[6:])
def test_dropins_on_the_device(check):
    """the NumPy-level Scene3D / Camera / ColoredTriMesh / LaplacianRigidEnergy drop-ins over the HIP rasterizer"""
    check("cuda")


@pytest.mark.parametrize("check", DROPIN_CHECKS, ids=lambda f: f.__name__[6:])
def test_dropins_on_cpu_tensors(oracle_api, check):
    """the same checks in the CPU suite: CPU tensors, the checker as rasterizer (tests/cpu_raster.py)"""
    import cpu_raster

    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        check("cpu")


@pytest.mark.gpu
def test_multiview_fitter_one_batched_launch_equals_single_views():
    """MeshRGBFitterWithPoseMultiFrame on the device: see check_multiview_equals_single_views"""
    check_multiview_equals_single_views("cuda")


@pytest.mark.gpu
def test_torch_optimizer_depth_fit_on_the_device():
    check_torch_optimizer_depth_fit("cuda")


@pytest.mark.gpu
def test_multiview_fitter_follows_the_repaired_reference():
    """MeshRGBFitterWithPoseMultiFrame on the device: see check_multiview_fit_against_reference"""
    check_multiview_fit_against_reference("cuda")


def _sharded_direct_fit_worker(rank, world, port, out_dir):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)  # (two processes on the one GPU of the box: gloo moves ROCm tensors too)
    from deodr_amd.mesh_fitter import MeshRGBFitterWithPoseMultiFrame

    d = fixture("rgb_multiview_fit.npz")
    _, faces = hand()
    images = [im.astype(np.float64) / 255 for im in d["images_u8"]]
    fitter = MeshRGBFitterWithPoseMultiFrame(d["vertices_centered"], faces, d["euler_init"], d["translation_init"], d["default_color"],
                                             d["default_light_directional"], float(d["default_light_ambient"]), cregu=2000, device="cuda")  # fmt: skip
    fitter.set_images(images)
    fitter.set_background_color(np.zeros(3))
    energies = [fitter.step()[0] for _ in range(4)]
    assert fitter._direct_state is not None  # the fixed kernel sequence, its shared block all-reduced in place
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), energies=np.array(energies), vertices=fitter.vertices.cpu().numpy(), views=np.array(fitter.my_views),
             translation=fitter.transform_translation.cpu().numpy(), color=fitter.mesh_color.cpu().numpy())  # fmt: skip
    dist.destroy_process_group()


@pytest.mark.gpu
def test_sharded_multiview_fit_direct_iteration_two_ranks(tmp_path):
    """the same sharded fit on ROCm tensors: every rank runs the fitter's iteration as the fixed kernel sequence (no autograd graph) and
    the ONE all-reduce sums the contiguous shared block (light, ambient, colour, data energy, vertex gradient and its mean) in place"""
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_sharded_direct_fit_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    golden = fixture("rgb_multiview_fit.npz")["energies"][:4]
    assert list(r0["views"]) == [0, 1] and list(r1["views"]) == [2]
    for r in (r0, r1):
        assert np.abs(r["energies"] - golden).max() <= 1e-6 * golden[0]
    assert np.abs(r0["vertices"] - r1["vertices"]).max() < 1e-12 and np.abs(r0["color"] - r1["color"]).max() < 1e-14
