"""The cases tests/test_render_ops_host.py (CPU emulation: bit for bit) and tests/test_render_ops_gpu.py (the library: to its accumulation order) share:
the same computation through every route into deodr_amd/render_ops.py, and two forwards in one graph on one DeviceScene / workspace.

The scene is the smallest that has textured and untextured triangles and silhouette edges: two views of a 10-triangle soup on 32 x 32 pixels with an
8 x 8 texture, the second view shifted by 0.37 pixel.  Everything lands on the device ``hip_util.device_scene`` puts its scene on."""

import copy
from types import SimpleNamespace

import numpy as np
import torch

from deodr_amd import scenes
from deodr_amd.hip_renderer import HipRasterizer
from hip_util import device_scene


def soup_views():
    s0 = scenes.soup_scene(n_tri=10, width=32, height=32, seed=9, flat=False, textured_ratio=0.5, texture_size=8, min_area=20.0)
    s0.backface_culling = True
    s1 = copy.copy(s0)
    s1.ij = s0.ij + 0.37
    return [s0, s1]


def prepared(pixel_dtype):
    """-> (DeviceScene of the two views, its HipRasterizer, obs [2,32,32,3], weights [2,32,32], seed [2,32,32,3]) in the pixel dtype"""
    ds = device_scene(soup_views(), pixel_dtype)
    on = lambda a: torch.as_tensor(a).to(device=ds.device, dtype=pixel_dtype).contiguous()
    return ds, HipRasterizer.for_scene(ds), on(np.random.RandomState(2).rand(2, 32, 32, 3)), on(np.random.RandomState(5).rand(2, 32, 32)), on(np.random.RandomState(1).randn(2, 32, 32, 3))


def leaf(t):
    return t.detach().clone().requires_grad_()


def leaves(ds, shared, offset=0.0, flip_texture=False):
    """fresh differentiated inputs from the scene's own arrays: ij, colors, texture (and uv when ``shared`` names it)"""
    inputs = dict(ij=leaf(ds.ij + offset), colors=leaf(ds.colors), texture=leaf(1 - ds.texture if flip_texture else ds.texture))
    if "uv" in shared:
        inputs["uv"] = leaf(ds.uv)
    return inputs


def grads_of(inputs):
    return {k: t.grad for k, t in inputs.items()}


def render_routes(ds, r, seed, shared):
    """[(image, gradients) through the pytorch layer, the same through RenderViewsFunc given the scene's own shade / depths / edgeflags]"""
    from deodr_amd.pytorch import TorchDifferentiableRenderViews
    from deodr_amd.render_ops import RenderViewsFunc

    shade, depths, edgeflags = ds.shade.clone(), ds.depths.clone(), ds.edgeflags.clone()
    out = []
    for route in ("pytorch layer", "merged op"):
        x = leaves(ds, shared)
        if route == "pytorch layer":
            image = TorchDifferentiableRenderViews(x["ij"], x["colors"], ds, r, 1.0, texture=x["texture"], uv=x.get("uv"))
        else:
            image = RenderViewsFunc.apply(x["ij"], x["colors"], shade, depths, edgeflags, ds, r, 1.0, x["texture"], x.get("uv"))[0]
        image.backward(seed)
        out.append((image.detach(), grads_of(x)))
    return out


def l2_routes(ds, r, obs, weights, shared):
    """[(loss, image, gradients) through TorchRenderViewsL2Loss (loss from the frame), the same through RenderViewsL2Func(library_loss=True)]"""
    from deodr_amd.pytorch import TorchRenderViewsL2Loss
    from deodr_amd.render_ops import RenderViewsL2Func

    shade, depths, edgeflags = ds.shade.clone(), ds.depths.clone(), ds.edgeflags.clone()
    out = []
    for route in ("pytorch layer", "merged op"):
        x = leaves(ds, shared)
        if route == "pytorch layer":
            loss = TorchRenderViewsL2Loss(x["ij"], x["colors"], obs, ds, r, 1.0, weights=weights, texture=x["texture"], uv=x.get("uv"))
            image = r.last_fit[0]
        else:
            loss, image, _z = RenderViewsL2Func.apply(x["ij"], x["colors"], shade, depths, edgeflags, obs, ds, r, 1.0, weights, x["texture"], x.get("uv"), True)
        loss.backward()
        out.append((float(loss.detach()), image.detach().clone(), grads_of(x)))
    return out


def alone_and_together(forward, inputs_a, inputs_b, seed):
    """``forward(inputs) -> image``, all on ONE scene / workspace.  -> ([gradients of a, of b] each from its own forward + backward,
    the same from both forwards in one graph and one backward: the adjoint of the first finds the scene holding the second)"""
    fresh = lambda inputs: {k: leaf(t) for k, t in inputs.items()}
    alone = []
    for inputs in (inputs_a, inputs_b):
        x = fresh(inputs)
        forward(x).backward(seed)
        alone.append(grads_of(x))
    xa, xb = fresh(inputs_a), fresh(inputs_b)
    ((forward(xa) * seed).sum() + (forward(xb) * seed).sum()).backward()
    return alone, [grads_of(xa), grads_of(xb)]


def stale_views(ds, r, seed):
    from deodr_amd.pytorch import TorchDifferentiableRenderViews

    forward = lambda x: TorchDifferentiableRenderViews(x["ij"], x["colors"], ds, r, 1.0, texture=x["texture"])
    return alone_and_together(forward, leaves(ds, ("texture",)), leaves(ds, ("texture",), offset=0.25, flip_texture=True), seed)


def stale_2d():
    """TorchDifferentiableRender2D with the reference's CPU float64 tensors (no texture input: different ij only)"""
    from deodr_amd.pytorch import TorchDifferentiableRender2D

    s = soup_views()[0]
    holder = SimpleNamespace(scene_2d=s)
    forward = lambda x: TorchDifferentiableRender2D(x["ij"], x["colors"], holder)
    inputs = lambda offset: dict(ij=torch.as_tensor(s.ij + offset), colors=torch.as_tensor(s.colors))
    return alone_and_together(forward, inputs(0.0), inputs(0.3), torch.as_tensor(np.random.RandomState(1).randn(32, 32, 3)))


def stale_scene3d(pixel_dtype, device):
    """Scene3DDevice.render of a small textured sphere (two 48 x 48 views, 12 x 12 texture) with ``mesh.texture`` requiring grad: the two forwards
    differ in the vertices (hence in ij) and in the texture tensor the mesh holds"""
    import cpu_raster_texture as crt
    from deodr_amd.scene3d import DeviceCamera, DeviceMesh, Scene3DDevice

    v = crt.sphere_views(n_views=2, size=48, texture_size=12, nu=14, n_rings=10)
    mesh = DeviceMesh(v["faces"], v["vertices"], clockwise=v["clockwise"], uv=v["uv"], faces_uv=v["faces"], texture=v["texture"], device=device)
    scene = Scene3DDevice(pixel_dtype=pixel_dtype)
    scene.set_mesh(mesh)
    scene.set_light(v["light"], v["ambient"])
    scene.set_background_color(v["background"])
    camera = DeviceCamera.stack(v["cameras"], device)
    seed = torch.as_tensor(np.random.RandomState(3).randn(2, 48, 48, 3)).to(device=mesh.device, dtype=pixel_dtype)

    def forward(x):
        mesh.set_vertices(x["vertices"])
        mesh.texture = x["texture"]
        return scene.render(camera)

    vertices, texture = mesh.vertices.detach(), mesh.texture.detach()
    return alone_and_together(forward, dict(vertices=vertices, texture=texture), dict(vertices=vertices + 0.01, texture=1 - texture), seed)
