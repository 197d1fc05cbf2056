"""Recover the texture of a known shape from 8 calibrated views, on the device: a textured bumpy sphere (planar UVs, `deodr_amd.scenes`), a
ground-truth texture, 8 cameras around it, one view partly masked out (`weights=`), start from grey.  One iteration is the rasterizer's
one-call fit step, `deodr_hip_texture_smoothness` and `deodr_hip_texture_step` -- replayed as one HIP graph.

    python examples/texture_fitting.py [--iterations 300] [--eager] [--size 256] [--texture 128] [--out DIR]
"""
import argparse
import os

import numpy as np

from _common import run


def save(path, image):
    """an image [H,W,3] in 0..1 as PNG (Pillow) -- or as .npy where Pillow is missing"""
    try:
        from PIL import Image

        Image.fromarray((np.clip(image, 0, 1) * 255).astype(np.uint8)).save(path + ".png")
    except ImportError:
        np.save(path + ".npy", image)


def main(iterations=300, graph=True, size=256, texture_size=128, views=8, out=None):
    import torch

    from deodr_amd import scenes
    from deodr_amd.mesh_fitter import GraphedStep, MeshTextureFitterMultiFrame
    from deodr_amd.scene3d import DeviceCamera, DeviceMesh, Scene3DDevice

    dev = torch.device("cuda", torch.cuda.current_device())
    vertices, faces = scenes.bumpy_sphere(60, 40)
    faces = faces.astype(np.int64)
    flat = scenes.sphere_scene(size, 60, 40, nb_colors=3, textured=True, texture_size=texture_size)  # (its planar UVs, winding flag and background)
    truth = scenes.smooth_texture(texture_size, texture_size, 3, seed=7, passes=2)
    cameras = [scenes.fit_camera(size, size, 60.0, vertices, scenes.rotx(0.37) @ scenes.roty(0.23 + 2 * np.pi * k / views)) for k in range(views)]
    light, ambient, background = np.array([-0.1, -0.5, -0.4]), 0.6, np.asarray(flat.background_color)
    # the photographs: the ground truth through the same renderer
    mesh = DeviceMesh(faces, vertices, clockwise=bool(flat.clockwise), uv=flat.uv, faces_uv=faces, texture=truth, device=dev)
    scene = Scene3DDevice(pixel_dtype=torch.float32)
    scene.set_mesh(mesh)
    scene.set_light(light, ambient)
    scene.set_background_color(background)
    photographs = scene.render(DeviceCamera.stack(cameras, dev)).cpu().numpy().astype(np.float64)
    weights = np.ones((views, size, size))
    weights[0, :, : size // 2] = 0.0  # say, an occluder in front of the left half of the first photograph
    photographs[0, :, : size // 2] = 0.0

    grey = np.full((texture_size, texture_size, 3), 0.5)
    fitter = MeshTextureFitterMultiFrame(vertices, faces, flat.uv, faces, grey, light, ambient, cameras=cameras, clockwise=bool(flat.clockwise),
                                         smoothness=0.05, device=dev, pixel_dtype=torch.float32)  # fmt: skip
    fitter.set_background_color(background)
    fitter.set_images(photographs, weights=weights)
    before = fitter.step()[1]  # (one iteration: the images of the grey texture)
    stepper = GraphedStep(fitter) if graph else fitter
    values = run(lambda: stepper.step_device()[0][0], iterations, max(iterations // 10, 1), f"texture fit, {views} views of {size}^2, {texture_size}^2 texels")
    after = fitter.step()[1]
    error = np.abs(fitter.texture.cpu().numpy() - truth)
    print(f"texture: mean |error| {error.mean():.4f} (grey start: {np.abs(grey - truth).mean():.4f}); texels no view sees are in-painted by the smoothness term")
    if out:
        os.makedirs(out, exist_ok=True)
        save(os.path.join(out, "view1_before"), before[1])
        save(os.path.join(out, "view1_after"), after[1])
        save(os.path.join(out, "view1_photograph"), photographs[1])
        save(os.path.join(out, "texture_fitted"), fitter.texture.cpu().numpy())
        save(os.path.join(out, "texture_truth"), truth)
    return values


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--texture", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    main(a.iterations, not a.eager, a.size, a.texture, out=a.out)
