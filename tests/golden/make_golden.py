"""Generate tests/golden/*.npz from the REAL reference (its own Python + Cython build).

Run in the build container only (needs /root/reference):  python tests/golden/make_golden.py

The reference tree is copied to a temp dir, built there with its own setup.py
(`build_ext --inplace`), three import stubs are injected (trimesh.base.Trimesh is only a type
annotation in deodr/triangulated_mesh.py:10-13,369; cv2 / imageio are imported by the examples and
replaced by PIL), the reference's own drivers are run, and inputs + outputs are dumped as small
fixtures.  Nothing of the reference's source is written into this repository; the fixtures are data.

Fixtures
  soup30_cw{0,1}.npz   deodr/examples/triangle_soup_fitting.py `run()` set-up (np.random.seed(2),
                       create_example_scene(clockwise), perturbed scene_init): all Scene2D inputs,
                       the texture as uint8 (material = imread/255 is reproduced exactly), SHA-256 of
                       the float64 image / z_buffer of scene_gt and of scene_init for both
                       antialiase_error modes, every gradient array of the first
                       render_compare_and_backward, and the 50-iteration loss curves whose last values are
                       the goldens of tests/test_triangle_soup_fitting.py:29-108.
  hand_mesh.npz        vertices / faces of deodr/data/hand.obj read with deodr/obj.py (input data for
                       BASELINE configs 2 and 4).
  hand.obj             deodr/data/hand.obj itself (the mesh file the arrays of hand_mesh.npz were read from).
  hand_adjacency.npz   TriMeshAdjacencies of the hand mesh (deodr/triangulated_mesh.py): face normals, vertex normals and the
                       silhouette flags of the edges seen along z.
  depth_hand_fit.npz   deodr/examples/depth_image_hand_fitting.py `run(dl_library="none")`: the cropped depth image (float32 as
                       in deodr/data/depth.bin), the 50 energies of MeshDepthFitter.step (last one = the golden of the
                       reference's tests/test_depth_image_hand_fitting.py:36-42) and, for iteration 0, every intermediate of
                       the Scene3D front half: projected points (distortion camera), depths, silhouette edge flags, the
                       rendered depth image, the vertex / quaternion / translation gradients, the rigid energy and its gradient.
  deferred_hand.npz    Scene3D.render_deferred of the hand mesh (96 x 80): the depth / face_id / barycentric / normal / luminosity /
                       xyz / color buffers of one 15-channel soup render at sigma = 0.
  rgb_multiview_fit.npz  deodr/examples/rgb_multiview_hand.py with the reference's multi-frame fitter, two defects repaired (see
                       rgb_multiview_fit): the three photographs (uint8), 30 energies, iteration-0 gradients, final parameters.
  duck.npz             the scene of the reference's tests/test_render_mesh.py::test_render_mesh_duck: textured duck mesh (assembled as
                       ColoredTriMesh.from_trimesh does), distorted camera, the float image the reference renders and its stored
                       uint8 test image deodr/data/test/duck.png (equal, checked at generation).
  rgb_hand_fit.npz     deodr/examples/rgb_image_hand_fitting.py `run(dl_library="none")`: the image (uint8), background colour,
                       50 energies of MeshRGBFitterWithPose.step and the iteration-0 intermediates (vertex normals,
                       luminosity, rendered image, gradients of vertices, lights and colour).
"""

import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

REFERENCE = os.environ.get("DEODR_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))

STUBS = {
    "trimesh/__init__.py": "from . import base\n",
    "trimesh/base.py": "class Trimesh:\n    pass\n",
    "cv2.py": "def imshow(*a, **k):\n    pass\n\n\ndef waitKey(*a, **k):\n    return 0\n",
    "imageio/__init__.py": "from . import v3\n",
    "imageio/v3.py": (
        "import numpy as np\nfrom PIL import Image\n\n\n"
        "def imread(path):\n    return np.asarray(Image.open(path))\n\n\n"
        "def imwrite(path, arr):\n    Image.fromarray(np.asarray(arr)).save(path)\n"
    ),
}


def build_reference(tmp):
    for name in ("deodr", "C++", "setup.py", "readme.md"):
        src = os.path.join(REFERENCE, name)
        dst = os.path.join(tmp, name)
        shutil.copytree(src, dst) if os.path.isdir(src) else shutil.copy(src, dst)
    subprocess.run([sys.executable, "setup.py", "build_ext", "--inplace"], cwd=tmp, check=True, capture_output=True)
    stubs = os.path.join(tmp, "_stubs")
    for rel, text in STUBS.items():
        path = os.path.join(stubs, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    sys.path.insert(0, stubs)
    sys.path.insert(0, tmp)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def scene_inputs(s, prefix):
    keys = ["faces", "faces_uv", "ij", "depths", "textured", "uv", "shade", "colors", "shaded", "edgeflags"]
    return {prefix + k: np.asarray(getattr(s, k)) for k in keys}


def soup(clockwise):
    import copy

    import deodr
    from deodr import differentiable_renderer_cython as drc
    from deodr.examples.triangle_soup_fitting import create_example_scene, run
    from PIL import Image

    np.random.seed(2)
    scene_gt = create_example_scene(clockwise=clockwise)
    sigma = 1
    image_target = np.zeros((scene_gt.height, scene_gt.width, scene_gt.nb_colors))
    z_target = np.zeros((scene_gt.height, scene_gt.width))
    drc.renderSceneCpp(scene_gt, sigma, image_target, z_target)
    n_vertices = len(scene_gt.depths)
    scene_init = copy.deepcopy(scene_gt)  # as triangle_soup_fitting.py:131-136
    scene_init.ij = scene_gt.ij + np.random.randn(n_vertices, 2) * 10
    scene_init.uv = scene_gt.uv + np.random.randn(n_vertices, 2) * 0
    max_uv = np.array(scene_gt.texture.shape[:2]) - 1
    scene_init.uv = np.minimum(np.maximum(scene_init.uv, 0), max_uv)
    scene_init.colors = scene_gt.colors + np.random.randn(n_vertices, 3) * 0

    tex_u8 = np.asarray(Image.open(os.path.join(deodr.data_path, "trefle.jpg")))
    assert np.array_equal(tex_u8.astype(np.float64) / 255, scene_gt.texture)

    out = {}
    out.update(scene_inputs(scene_gt, "gt_"))
    out.update(scene_inputs(scene_init, "init_"))
    out["texture_u8"] = tex_u8
    out["background_rgb"] = np.array([0.3, 0.5, 0.7])
    out["height"], out["width"], out["clockwise"] = scene_gt.height, scene_gt.width, clockwise
    out["gt_image_sha256"], out["gt_z_sha256"] = sha(image_target), sha(z_target)
    out["gt_image_mean"] = image_target.mean()
    for aa in (False, True):
        sc = copy.deepcopy(scene_init)
        image, z, err_buffer, err = sc.render_compare_and_backward(sigma=sigma, antialiase_error=aa, obs=image_target)
        tag = f"aa{int(aa)}_"
        out[tag + "image_sha256"], out[tag + "z_sha256"], out[tag + "err_buffer_sha256"] = sha(image), sha(z), sha(err_buffer)
        out[tag + "loss"] = err
        for g in ("ij_b", "colors_b", "uv_b", "shade_b"):
            out[tag + g] = getattr(sc, g)
        out[tag + "texture_b_sha256"] = sha(sc.texture_b)  # stock reference: overwrite bug of H.h:621-624 included
        out[tag + "texture_b_sum"] = sc.texture_b.sum()
        losses, hashes = run(nb_max_iter=50, display=False, clockwise=clockwise, antialiase_error=aa)
        out[tag + "losses50"] = np.array(losses)
        out[tag + "hash_iter0"], out[tag + "hash_iter1"] = hashes[0], hashes[1]
        assert hashes[0] == out[tag + "image_sha256"]
    np.savez_compressed(os.path.join(OUT, f"soup30_cw{int(clockwise)}.npz"), **out)
    print(f"soup30_cw{int(clockwise)}: final losses", out["aa0_losses50"][-1], out["aa1_losses50"][-1])


def hand():
    import deodr
    from deodr.obj import read_obj

    faces, vertices = read_obj(os.path.join(deodr.data_path, "hand.obj"))
    np.savez_compressed(os.path.join(OUT, "hand_mesh.npz"), faces=np.asarray(faces, dtype=np.uint32), vertices=np.asarray(vertices, dtype=np.float64))
    print("hand mesh", np.shape(vertices), np.shape(faces))
    shutil.copy(os.path.join(deodr.data_path, "hand.obj"), os.path.join(OUT, "hand.obj"))


def hand_adjacency():
    from deodr.triangulated_mesh import TriMeshAdjacencies

    d = np.load(os.path.join(OUT, "hand_mesh.npz"))
    adjacency = TriMeshAdjacencies(d["faces"].astype(np.int64))
    face_normals = adjacency.compute_face_normals(d["vertices"])
    np.savez_compressed(
        os.path.join(OUT, "hand_adjacency.npz"), face_normals=face_normals, vertex_normals=adjacency.compute_vertex_normals(face_normals),
        edge_on_silhouette=np.asarray(adjacency.edge_on_silhouette(d["vertices"][:, :2]), dtype=bool),
    )  # fmt: skip
    print("hand adjacency: edges on the silhouette", int(np.sum(adjacency.edge_on_silhouette(d["vertices"][:, :2]))))


def depth_hand_fit():
    """deodr/examples/depth_image_hand_fitting.py:24-66 with dl_library="none", instrumented at iteration 0."""
    import deodr
    from deodr import ColoredTriMesh
    from deodr.mesh_fitter import MeshDepthFitter

    raw = np.fliplr(np.fromfile(os.path.join(deodr.data_path, "depth.bin"), dtype=np.float32).reshape(240, 320))[20:-20, 60:-60]
    depth_image = raw.astype(np.float64)
    max_depth = 450
    depth_image[depth_image == 0] = max_depth
    depth_image = depth_image / max_depth
    faces, vertices = deodr.read_obj(os.path.join(deodr.data_path, "hand.obj"))
    mesh = ColoredTriMesh(faces.copy(), vertices=vertices, nb_colors=0)
    euler_init, translation_init = np.array([0.1, 0.1, 0.1]), np.zeros(3)
    fitter = MeshDepthFitter(mesh.vertices, mesh.faces, euler_init, translation_init, cregu=1000)
    distortion = np.array([1, 0, 0, 0, 0])
    fitter.set_image(depth_image, focal=241, distortion=distortion)
    fitter.set_max_depth(1)
    fitter.set_depth_scale(110 / max_depth)
    out = dict(depth_raw_f32=np.ascontiguousarray(raw), max_depth=max_depth, focal=241.0, distortion=distortion.astype(np.float64),
               euler_init=euler_init, translation_init=translation_init, cregu=1000.0, depth_scale=110 / max_depth,
               quaternion_init=fitter.transform_quaternion_init, camera_extrinsic=fitter.camera.extrinsic,
               camera_intrinsic=fitter.camera.intrinsic)
    energies = []
    for it in range(50):
        energy, synthetic_depth, diff_image = fitter.step()
        energies.append(energy)
        if it == 0:
            s2 = fitter.scene.scene_2d
            out.update(it0_ij=np.array(s2.ij), it0_depths=np.array(s2.depths), it0_edgeflags=np.array(s2.edgeflags),
                       it0_depth_image=np.array(fitter.depth_not_clipped), it0_vertices_transformed_b=np.array(fitter.scene.mesh._vertices_b),
                       it0_vertices_b=np.array(fitter._vertices_b), it0_quaternion_b=np.array(fitter.transform_quaternion_b),
                       it0_translation_b=np.array(fitter.transform_translation_b), it0_ij_b=np.array(s2.ij_b),
                       it0_colors_b=np.array(s2.colors_b), it0_vertices_transformed=np.array(fitter.mesh.vertices))
            e_rigid, g_rigid, _ = fitter.rigid_energy.evaluate(fitter.vertices - fitter.speed_vertices)  # the vertices of iteration 0
            out.update(it0_energy_rigid=e_rigid, it0_grad_rigid=np.array(g_rigid))
    out["energies"] = np.array(energies)
    out["final_vertices"], out["final_quaternion"], out["final_translation"] = fitter.vertices, fitter.transform_quaternion, fitter.transform_translation
    np.savez_compressed(os.path.join(OUT, "depth_hand_fit.npz"), **out)
    print("depth hand fit: energies[0], [49] =", energies[0], energies[49])


def rgb_hand_fit():
    """deodr/examples/rgb_image_hand_fitting.py:27-100 with dl_library="none", instrumented at iteration 0."""
    import deodr
    from deodr import ColoredTriMesh, read_obj
    from deodr.mesh_fitter import MeshRGBFitterWithPose
    from PIL import Image

    img_u8 = np.asarray(Image.open(os.path.join(deodr.data_path, "hand.png")))
    hand_image = img_u8.astype(np.double) / 255
    faces, vertices = read_obj(os.path.join(deodr.data_path, "hand.obj"))
    mesh = ColoredTriMesh(faces.copy(), vertices=vertices, nb_colors=3)
    default_color = np.array([0.4, 0.3, 0.25])
    default_light_directional = -np.array([0.1, 0.5, 0.4])
    default_light_ambient = 0.6
    euler_init = np.array([0, 0, 0])
    translation_init = np.mean(mesh.vertices, axis=0)
    mesh.set_vertices(mesh.vertices - translation_init[None, :])
    fitter = MeshRGBFitterWithPose(mesh.vertices, mesh.faces, default_color=default_color, default_light_directional=default_light_directional,
                                   default_light_ambient=default_light_ambient, update_lights=True, update_color=True, euler_init=euler_init,
                                   translation_init=translation_init, cregu=1000)
    fitter.reset()
    background_color = np.median(np.vstack((hand_image[:10, :10, :].reshape(-1, 3), hand_image[-10:, :10, :].reshape(-1, 3),
                                            hand_image[-10:, -10:, :].reshape(-1, 3), hand_image[:10, -10:, :].reshape(-1, 3))), axis=0)
    background_color = np.asarray(background_color, dtype=np.float64)
    fitter.set_image(hand_image)
    fitter.set_background_color(background_color)
    out = dict(image_u8=img_u8, background_color=background_color, default_color=default_color,
               default_light_directional=default_light_directional, default_light_ambient=default_light_ambient,
               translation_init=translation_init, vertices_centered=np.array(mesh.vertices), cregu=1000.0,
               camera_extrinsic=fitter.camera.extrinsic, camera_intrinsic=fitter.camera.intrinsic)
    energies = []
    for it in range(50):
        energy, image, diff_image = fitter.step()
        energies.append(energy)
        if it == 0:
            s2 = fitter.scene.scene_2d
            out.update(it0_ij=np.array(s2.ij), it0_depths=np.array(s2.depths), it0_edgeflags=np.array(s2.edgeflags), it0_colors=np.array(s2.colors),
                       it0_image=np.array(image), it0_vertex_normals=np.array(fitter.mesh.vertex_normals),
                       it0_vertices_transformed_b=np.array(fitter.scene.mesh._vertices_b), it0_vertices_b=np.array(fitter._vertices_b),
                       it0_quaternion_b=np.array(fitter.transform_quaternion_b), it0_translation_b=np.array(fitter.transform_translation_b),
                       it0_light_directional_b=np.array(fitter.light_directional_b), it0_light_ambient_b=float(fitter.light_ambient_b),
                       it0_mesh_color_b=np.array(fitter.mesh_color_b), it0_ij_b=np.array(s2.ij_b), it0_colors_b=np.array(s2.colors_b),
                       it0_vertices_transformed=np.array(fitter.mesh.vertices))
    out["energies"] = np.array(energies)
    np.savez_compressed(os.path.join(OUT, "rgb_hand_fit.npz"), **out)
    print("rgb hand fit: energies[0], [49] =", energies[0], energies[49])


def deferred_hand():
    """Scene3D.render_deferred (dr.py:1053-1174) of the hand mesh, 96 x 80, every buffer: the stacked-channel (nb_colors = 15)
    untextured soup render at sigma = 0 that deferred shading uses."""
    import deodr
    from deodr import ColoredTriMesh, read_obj
    from deodr.differentiable_renderer import Scene3D, default_camera

    faces, vertices = read_obj(os.path.join(deodr.data_path, "hand.obj"))
    mesh = ColoredTriMesh(faces.copy(), vertices=vertices, nb_colors=3)
    mesh.set_vertices_colors(np.random.RandomState(0).rand(mesh.nb_vertices, 3))
    rot = np.array([[0.96, 0.0, 0.28], [0.0, -1.0, 0.0], [0.28, 0.0, -0.96]])
    camera = default_camera(96, 80, 70, mesh.vertices, rot)
    scene = Scene3D(sigma=0)
    scene.set_light(light_directional=np.array([-0.1, -0.5, -0.4]), light_ambient=0.3)
    scene.set_mesh(mesh)
    scene.set_background_color([0.2, 0.3, 0.4])
    buffers = scene.render_deferred(camera, depth_scale=0.5)
    out = {"buf_" + k: np.array(v) for k, v in buffers.items()}
    out.update(colors=np.array(mesh.vertices_colors), rot=rot, extrinsic=np.array(camera.extrinsic), intrinsic=np.array(camera.intrinsic),
               order=np.array(list(buffers.keys())))
    np.savez_compressed(os.path.join(OUT, "deferred_hand.npz"), **out)
    print("deferred hand:", {k: v.shape for k, v in buffers.items()})


def rgb_multiview_fit():
    """deodr/examples/rgb_multiview_hand.py:24-100 (three photographs of a hand, one mesh, one pose per view) with the reference's
    MeshRGBFitterWithPoseMultiFrame (mesh_fitter.py:378-632), TWO DEFECTS REPAIRED because as shipped the class does not fit the
    images it is given:
      M1  energy_data compares `image[idframe]` -- ROW idframe of the rendered image, broadcast -- with the target (:538-544);
          the rendered image of the frame is meant (`render` returns one image);
      M2  step renormalises the [n, 4] array of quaternions by its Frobenius norm (:595) instead of row by row.
    The repair is a subclass defined here (the data term restated with `image`, rows renormalised after every step); everything else
    -- hyper-parameters, momentum, camera, the 1 / nb_frames weight of the data term, rigid energy -- is the reference's code."""
    import glob

    import deodr
    from deodr import read_obj
    from deodr.mesh_fitter import MeshRGBFitterWithPoseMultiFrame
    from PIL import Image

    class Repaired(MeshRGBFitterWithPoseMultiFrame):
        def energy_data(self, vertices):
            self.vertices = vertices
            images, diff_images, total = [], [], 0.0
            self.clear_gradients()
            weight = self.cdata / self.nb_frames
            for k in range(self.nb_frames):
                image = self.render(idframe=k)
                residual = image - self.mesh_images[k]  # M1
                diff = np.sum(residual**2, axis=2)
                images.append(image)
                diff_images.append(diff)
                total += weight * np.sum(diff)
                self.render_backward(weight * 2 * residual)
            return float(total), images, diff_images

        def step(self, check_gradient=False):
            out = super().step(check_gradient)
            self.transform_quaternion = self.transform_quaternion / np.linalg.norm(self.transform_quaternion, axis=1, keepdims=True)  # M2
            return out

    files = sorted(glob.glob(os.path.join(deodr.data_path, "hand_multiview", "*.jpg")))
    images_u8 = np.stack([np.asarray(Image.open(f)) for f in files])
    hand_images = [im.astype(np.double) / 255 for im in images_u8]
    faces, vertices = read_obj(os.path.join(deodr.data_path, "hand.obj"))
    default_color = np.array([0.4, 0.3, 0.25]) * 1.5
    default_light_directional = -np.array([0.1, 0.5, 0.4])
    default_light_ambient = 0.6
    euler_init = np.vstack([np.array([0, yrot, 0]) for yrot in np.linspace(-0.5, 0.5, 3)])
    vertices = vertices - np.mean(vertices, axis=0)
    translation_init = np.tile(np.array([0, -0.2, 0.2])[None, :], [len(hand_images), 1])
    fitter = Repaired(vertices, faces, default_color=default_color, default_light_directional=default_light_directional,
                      default_light_ambient=default_light_ambient, update_lights=True, update_color=True, euler_init=euler_init,
                      translation_init=translation_init, cregu=2000)
    fitter.reset()
    fitter.set_images(hand_images)
    fitter.set_background_color(np.array([0, 0, 0]))
    energies, it0 = [], {}
    for it in range(30):
        energy, images, diff_images = fitter.step()
        energies.append(energy)
        if it == 0:
            it0 = dict(it0_vertices_b=np.array(fitter._vertices_b),
                       it0_quaternion_b=np.array(fitter.transform_quaternion_b), it0_translation_b=np.array(fitter.transform_translation_b),
                       it0_light_directional_b=np.array(fitter.light_directional_b), it0_light_ambient_b=float(fitter.light_ambient_b),
                       it0_mesh_color_b=np.array(fitter.mesh_color_b))
    np.savez_compressed(
        os.path.join(OUT, "rgb_multiview_fit.npz"), images_u8=images_u8, files=np.array([os.path.basename(f) for f in files]),
        vertices_centered=vertices, euler_init=euler_init, translation_init=translation_init, default_color=default_color,
        default_light_directional=default_light_directional, default_light_ambient=default_light_ambient, cregu=2000.0,
        camera_extrinsic=np.array(fitter.camera.extrinsic), camera_intrinsic=np.array(fitter.camera.intrinsic), energies=np.array(energies),
        final_vertices=np.array(fitter.vertices), final_quaternion=np.array(fitter.transform_quaternion),
        final_translation=np.array(fitter.transform_translation), final_light_directional=np.array(fitter.light_directional),
        final_light_ambient=float(fitter.light_ambient), final_mesh_color=np.array(fitter.mesh_color), **it0,
    )  # fmt: skip
    print("rgb multiview fit: energies[0], [29] =", energies[0], energies[29])


def read_textured_obj(path):
    """v / vt / f v/vt/vn records of a Wavefront file -> (vertices, uv in [0,1], per-corner vertex ids, per-corner uv ids)"""
    v, vt, fv, ft = [], [], [], []
    for line in open(path):
        p = line.split()
        if not p:
            continue
        if p[0] == "v":
            v.append([float(x) for x in p[1:4]])
        elif p[0] == "vt":
            vt.append([float(x) for x in p[1:3]])
        elif p[0] == "f":
            corners = [c.split("/") for c in p[1:]]
            assert len(corners) == 3
            fv.append([int(c[0]) - 1 for c in corners])
            ft.append([int(c[1]) - 1 for c in corners])
    return np.array(v), np.array(vt), np.array(fv), np.array(ft)


def duck():
    """The scene of the reference's tests/test_render_mesh.py::test_render_mesh_duck (deodr/examples/render_mesh.py:17-58 at
    320 x 240): textured duck, camera with radial distortion, directional light, sigma = 1.  The mesh is assembled here the way
    ColoredTriMesh.from_trimesh does (triangulated_mesh.py:369-438: texture / 255, uv = (u W, (1 - v) H) - 0.5, vertices merged
    with np.unique, faces_uv = the un-merged corner ids) -- trimesh itself is not installed, so the result is CHECKED against
    the reference's stored image deodr/data/test/duck.png before anything is written."""
    from PIL import Image
    from scipy.spatial.transform import Rotation

    import deodr
    from deodr import ColoredTriMesh
    from deodr.differentiable_renderer import Scene3D, default_camera

    v, vt, fv, ft = read_textured_obj(os.path.join(deodr.data_path, "duck.obj"))
    texture_u8 = np.asarray(Image.open(os.path.join(deodr.data_path, "duck.png")))[:, :, :3]
    texture = texture_u8 / 255
    uv = np.column_stack((vt[:, 0] * texture.shape[1], (1 - vt[:, 1]) * texture.shape[0])) - 0.5
    vertices, inverse = np.unique(v, axis=0, return_inverse=True)
    faces = inverse.reshape(-1)[fv].astype(np.uint32)
    mesh = ColoredTriMesh(faces, vertices, clockwise=False, faces_uv=ft.astype(np.uint32), uv=uv, texture=texture)
    width, height = 320, 240
    rot = Rotation.from_euler("xyz", [180, 0, 0], degrees=True).as_matrix()
    camera = default_camera(width, height, 80, mesh.vertices, rot)
    camera.distortion = np.array([-0.5, 0.5, 0, 0, 0])
    scene = Scene3D()
    scene.set_light(light_directional=0.3 * np.array([1, -1, 0]), light_ambient=0)
    scene.set_mesh(mesh)
    scene.set_background_color(np.array((0.8, 0.8, 0.8)))
    image = scene.render(camera)
    stored = np.asarray(Image.open(os.path.join(deodr.data_path, "test", "duck.png")))[:, :, :3]
    worst = int(np.abs(stored.astype(int) - (image * 255).astype(np.uint8).astype(int)).max())
    print("duck: largest difference with the reference's stored test image:", worst, "grey levels")
    assert worst == 0, "the mesh assembled here is not the one the reference's test renders"
    np.savez_compressed(
        os.path.join(OUT, "duck.npz"), vertices=vertices, faces=faces, uv=uv, faces_uv=ft.astype(np.uint32), texture_u8=texture_u8, rot=rot,
        extrinsic=np.array(camera.extrinsic), intrinsic=np.array(camera.intrinsic), distortion=np.array(camera.distortion),
        image=image.astype(np.float32), image_sha256=np.array(sha(image)), stored_u8=stored,
        ij=np.array(scene.scene_2d.ij) if getattr(scene, "scene_2d", None) is not None and hasattr(scene.scene_2d, "ij") else np.zeros(0),
    )  # fmt: skip


def scene3d_helpers():
    """The small public members of Camera / Scene3D around the render calls (dr.py:280-310, 443-451, 814-850): fields of view,
    camera-to-world matrix, left_mul_intrinsic, repr; compute_vertices_luminosity and its adjoint on the hand mesh."""
    import deodr
    from deodr import ColoredTriMesh, read_obj
    from deodr.differentiable_renderer import Scene3D, default_camera

    faces, vertices = read_obj(os.path.join(deodr.data_path, "hand.obj"))
    mesh = ColoredTriMesh(faces.copy(), vertices=vertices, nb_colors=3)
    rot = np.array([[0.96, 0.0, 0.28], [0.0, -1.0, 0.0], [0.28, 0.0, -0.96]])
    camera = default_camera(96, 80, 70, mesh.vertices, rot)
    rs = np.random.RandomState(3)
    points = rs.randn(7, 2)
    scene = Scene3D(sigma=1)
    light = np.array([-0.1, -0.5, -0.4])
    scene.set_light(light_directional=light, light_ambient=0.3)
    scene.set_mesh(mesh)
    mesh.compute_vertex_normals()
    scene.store_backward_current = {}
    luminosity = scene.compute_vertices_luminosity()
    luminosity_b = rs.randn(mesh.nb_vertices)
    scene.compute_vertices_luminosity_backward(luminosity_b)
    np.savez_compressed(
        os.path.join(OUT, "scene3d_helpers.npz"), rot=rot, xfov=camera.xfov, yfov=camera.yfov, camera_to_world=camera.camera_to_world_mtx_4x4(),
        points=points, left_mul_intrinsic=camera.left_mul_intrinsic(points), repr=np.array(repr(camera)), light=light,
        vertex_normals=np.array(mesh.vertex_normals), luminosity=luminosity, luminosity_b=luminosity_b,
        light_directional_b=np.array(scene.light_directional_b), vertex_normals_b=np.array(scene.vertex_normals_b), light_ambient_b=scene.light_ambient_b,
    )  # fmt: skip
    print("scene3d helpers: xfov, yfov =", camera.xfov, camera.yfov)


if __name__ == "__main__":
    only = sys.argv[1:]
    with tempfile.TemporaryDirectory() as tmp:
        build_reference(tmp)
        if not only or "soup" in only:
            soup(False)
            soup(True)
        if not only or "hand" in only:
            hand()
            hand_adjacency()
        if not only or "fits" in only:
            depth_hand_fit()
            rgb_hand_fit()
        if not only or "deferred" in only:
            deferred_hand()
        if not only or "helpers" in only:
            scene3d_helpers()
        if not only or "duck" in only:
            duck()
        if not only or "multiview" in only:
            rgb_multiview_fit()
