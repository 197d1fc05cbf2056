"""Fit the coefficients of an eigen-texture model, on the device (after the reference's deodr/examples/eigen_faces.py, with nothing downloaded):
the basis is a PCA of a few dozen smooth random textures synthesised here, the photographs are a textured bumpy sphere (planar UVs,
`deodr_amd.scenes`) rendered from known coefficients, and the fit recovers them from zero.  The texture is `mean + coefficients . basis`; one
iteration is `deodr_hip_basis_apply`, the rasterizer's one-call fit step, `deodr_hip_basis_apply_b` and one momentum update of the coefficients --
replayed as one HIP graph.

    python examples/eigen_texture_fitting.py [--iterations 200] [--eager] [--size 128] [--texture 64] [--modes 16] [--samples 48]
"""
import argparse

import numpy as np

from _common import run


def pca_of_smooth_textures(samples, modes, texture_size, seed=0):
    """-> (mean [Ht,Wt,3], components [modes,Ht,Wt,3] with orthonormal rows, standard deviation of every mode [modes])"""
    from deodr_amd import scenes

    textures = np.stack([scenes.smooth_texture(texture_size, texture_size, 3, seed=seed + i, passes=8) for i in range(samples)])
    mean = textures.mean(axis=0)
    _u, singular, vt = np.linalg.svd((textures - mean).reshape(samples, -1), full_matrices=False)
    return mean, vt[:modes].reshape(modes, *mean.shape), singular[:modes] / np.sqrt(samples - 1)


def main(iterations=200, graph=True, size=128, texture_size=64, modes=16, samples=48, views=4):
    import torch

    from deodr_amd import scenes
    from deodr_amd.mesh_fitter import GraphedStep, MeshTextureFitterMultiFrame
    from deodr_amd.scene3d import DeviceCamera, DeviceMesh, Scene3DDevice

    dev = torch.device("cuda", torch.cuda.current_device())
    vertices, faces = scenes.bumpy_sphere(60, 40)
    faces = faces.astype(np.int64)
    flat = scenes.sphere_scene(size, 60, 40, nb_colors=3, textured=True, texture_size=texture_size)  # (its planar UVs, winding flag and background)
    cameras = [scenes.fit_camera(size, size, 60.0, vertices, scenes.rotx(0.37) @ scenes.roty(0.23 + 2 * np.pi * k / views)) for k in range(views)]
    light, ambient, background = np.array([-0.1, -0.5, -0.4]), 0.6, np.asarray(flat.background_color)
    mean, components, sigmas = pca_of_smooth_textures(samples, modes, texture_size)
    truth = np.random.RandomState(1).randn(modes) * sigmas  # a texture of the model, drawn from its prior
    # the photographs: that texture through the same renderer
    mesh = DeviceMesh(faces, vertices, clockwise=bool(flat.clockwise), uv=flat.uv, faces_uv=faces, texture=mean + np.tensordot(truth, components, axes=1), device=dev)
    scene = Scene3DDevice(pixel_dtype=torch.float32)
    scene.set_mesh(mesh)
    scene.set_light(light, ambient)
    scene.set_background_color(background)
    photographs = scene.render(DeviceCamera.stack(cameras, dev)).cpu().numpy().astype(np.float64)

    fitter = MeshTextureFitterMultiFrame(vertices, faces, flat.uv, faces, mean, light, ambient, cameras=cameras, clockwise=bool(flat.clockwise), smoothness=0.0,
                                         device=dev, pixel_dtype=torch.float32, texture_basis=components, coefficient_regu=1e-3, sigmas=sigmas)  # fmt: skip
    fitter.set_background_color(background)
    fitter.set_images(photographs)
    stepper = GraphedStep(fitter) if graph else fitter
    values = run(lambda: stepper.step_device()[0][0], iterations, 1, f"eigen-texture fit, {modes} modes of {texture_size}^2 texels, {views} views of {size}^2")
    fitted = fitter.coefficients.cpu().numpy()
    print(f"coefficients: max |error| / sigma {np.abs((fitted - truth) / sigmas).max():.4f} (from zero: {np.abs(truth / sigmas).max():.4f})")
    return values


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--texture", type=int, default=64)
    ap.add_argument("--modes", type=int, default=16)
    ap.add_argument("--samples", type=int, default=48)
    a = ap.parse_args()
    main(a.iterations, not a.eager, a.size, a.texture, a.modes, a.samples)
