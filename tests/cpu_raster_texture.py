"""TEST harness, the textured companion of ``cpu_raster.py``: the CPU checker stands in for the HIP rasterizer behind
``Scene3DDevice._rasterize`` / ``_rasterize_l2`` and ALSO differentiates with respect to the texture and the texture coordinates.

The gradients are those of the REPAIRED reference (``oracle.api.port(fixed=True)``: DESIGN.md, D1 -- as shipped, the reference's ``texture_b`` of
a pixel under a silhouette edge is wrong), which is what the HIP library computes.  The stand-ins take the keyword arguments the product passes when
``mesh.texture`` / ``mesh.uv`` require grad (``texture=``, ``uv=``) and the ``weights=`` of a fit step, and record what they were given in
``calls``.  Nothing of this is reachable from the product."""

import contextlib

import numpy as np
import torch

from cpu_raster import _scene2d
from deodr_amd.scene3d import Scene3DDevice
from oracle import api


def checker():
    """the restatement with the adjoint defects repaired (the switch is process-wide and set by every call of ``api.port``: ask again before every use)"""
    return api.port(fixed=True)


class CheckerRenderViewsTextured(torch.autograd.Function):
    """(ij [n,V,2], colors [n,V,C], shade [n,V], texture [Ht,Wt,C], uv [Vuv,2]) -> (image [n,H,W,C], z [n,H,W]) through the checker, view by view;
    ``texture_b`` / ``uv_b`` are summed over the views, as the library delivers them"""

    @staticmethod
    def forward(ctx, ij, colors, shade, texture, uv, depths, flags, static, sigma):
        views, images, zs = [], [], []
        static = dict(static, texture=texture.detach().numpy().astype(np.float64), uv=uv.detach().numpy().astype(np.float64))
        for i in range(ij.shape[0]):
            bgi = static["background_image"]
            st = dict(static, background_image=None if bgi is None else (bgi[i] if bgi.ndim == 4 else bgi))
            s = _scene2d(st, ij[i].detach().numpy(), depths[i].detach().numpy(), colors[i].detach().numpy(), shade[i].detach().numpy(), flags[i].numpy())
            image, z = checker().render(s, sigma)
            views.append((s, image, z))
            images.append(image)
            zs.append(z)
        ctx.views, ctx.sigma, ctx.dtypes = views, sigma, (texture.dtype, uv.dtype)
        z = torch.as_tensor(np.stack(zs))
        ctx.mark_non_differentiable(z)
        return torch.as_tensor(np.stack(images)), z

    @staticmethod
    def backward(ctx, image_b, _z_b):
        g = [checker().grads(s, ctx.sigma, image, z, image_b[i].numpy().astype(np.float64)) for i, (s, image, z) in enumerate(ctx.views)]
        stack = lambda k: torch.as_tensor(np.stack([x[k] for x in g]))
        total = lambda k, dtype: torch.as_tensor(np.sum([x[k] for x in g], axis=0)).to(dtype)
        return stack("ij_b"), stack("colors_b"), stack("shade_b"), total("texture_b", ctx.dtypes[0]), total("uv_b", ctx.dtypes[1]), None, None, None, None


calls = []  # one dict per stand-in call: which optional keyword arguments it received


def _rasterize(self, camera, ij, depths, colors, shade, textured, backface_culling, **given):
    assert set(given) <= {"texture", "uv"}, given
    calls.append(dict(entry="_rasterize", given=sorted(given)))
    assert textured, "the textured stand-in serves textured renders only"
    if (self.background_image is None) == (self.background_color is None):
        raise BaseException("You need to provide either a background image or background color")
    m, n = self.mesh, camera.n_views
    flags = m.topology.edge_on_silhouette(ij) if self.sigma > 0 else torch.zeros((n, m.nb_faces, 3), dtype=torch.uint8)
    self.last = dict(ij=ij, depths=depths, edgeflags=flags, colors=colors, shade=shade)
    static = dict(
        faces=m.faces_np, faces_uv=m.faces_uv_np, textured=True, height=camera.height, width=camera.width,
        background_color=None if self.background_color is None else np.asarray(self.background_color, dtype=np.float64),
        background_image=None if self.background_image is None else np.asarray(self.background_image, dtype=np.float64), clockwise=m.clockwise,
        backface_culling=bool(backface_culling), perspective_correct=self.perspective_correct, integer_pixel_centers=self.integer_pixel_centers,
    )  # fmt: skip
    texture, uv = given.get("texture", m.texture.detach()), given.get("uv", m.uv.detach())  # (not given: the value the mesh holds at the call)
    return CheckerRenderViewsTextured.apply(ij, colors, shade, texture, uv, depths.detach(), flags, static, self.sigma)


def _rasterize_l2(self, camera, ij, depths, colors, shade, textured, backface_culling, obs, **given):
    assert set(given) <= {"texture", "uv", "weights"}, given
    weights = given.pop("weights", None)
    calls.append(dict(entry="_rasterize_l2", given=sorted(given), weights=weights is not None))
    image, _z = self._rasterize(camera, ij, depths, colors, shade, textured, backface_culling, **given)
    calls.pop()  # (the inner call is part of this one)
    r2 = (image.to(torch.float64) - obs.to(torch.float64)) ** 2
    if weights is not None:
        r2 = r2 * weights.to(torch.float64).expand(r2.shape[:3])[..., None]
    return r2.sum(), image.detach()


@contextlib.contextmanager
def emulate():
    """within the block Scene3DDevice rasterizes textured meshes with the repaired checker on CPU tensors"""
    saved = Scene3DDevice._rasterize, Scene3DDevice._rasterize_l2
    Scene3DDevice._rasterize, Scene3DDevice._rasterize_l2 = _rasterize, _rasterize_l2
    del calls[:]
    try:
        yield calls
    finally:
        Scene3DDevice._rasterize, Scene3DDevice._rasterize_l2 = saved


# ---- what the texture tests share: NumPy restatements of the two formulas, a multi-view textured scene, the oracle-driven fit loop ----------


def np_smoothness(t, weight):
    """-> (E, dE/dt) of E = 0.5 weight (sum of squared differences of x- and y-neighbours), free boundary, in float64 -- written with explicit
    neighbour sums (degree * t - sum of the neighbours), not the way the product's torch path writes it"""
    t = np.asarray(t, dtype=np.float64)
    dx, dy = t[:, 1:] - t[:, :-1], t[1:] - t[:-1]
    energy = 0.5 * weight * (np.sum(dx * dx) + np.sum(dy * dy))
    deg, nb = np.zeros(t.shape), np.zeros(t.shape)
    deg[:, 1:] += 1
    nb[:, 1:] += t[:, :-1]
    deg[:, :-1] += 1
    nb[:, :-1] += t[:, 1:]
    deg[1:] += 1
    nb[1:] += t[:-1]
    deg[:-1] += 1
    nb[:-1] += t[1:]
    return energy, weight * (deg * t - nb)


def np_step(t, s, g, factor, step_max=None, inertia=0.0, damping=0.0, clamp=None):
    """-> (new texture, new speed) in float64"""
    t, s, g = (np.asarray(a, dtype=np.float64) for a in (t, s, g))
    step = -factor * g
    if step_max is not None and step_max > 0:
        step = np.clip(step, -step_max, step_max)
    s = (1 - damping) * (inertia * s + (1 - inertia) * step)
    t = t + s
    if clamp is not None:
        out = (t < clamp[0]) | (t > clamp[1])
        t, s = np.clip(t, clamp[0], clamp[1]), np.where(out, 0.0, s)
    return t, s


def sphere_views(n_views=4, size=128, texture_size=64, nu=100, n_rings=100, nb_colors=3):
    """``scenes.sphere_scene(textured=True)`` seen from ``n_views`` angles, as the 3-D ingredients a fitter takes: the same mesh, planar UVs, light,
    background and cameras that ``sphere_scene(angle=...)`` assembles into one Scene2D per view"""
    from deodr_amd import scenes

    vertices, faces = scenes.bumpy_sphere(nu, n_rings)
    angles = [2 * np.pi * k / n_views for k in range(n_views)]
    views = [scenes.sphere_scene(size, nu, n_rings, nb_colors=nb_colors, textured=True, texture_size=texture_size, angle=a) for a in angles]
    assert len({bool(v.clockwise) for v in views}) == 1
    cameras = [scenes.fit_camera(size, size, 60.0, vertices, scenes.rotx(0.37) @ scenes.roty(0.23 + a)) for a in angles]
    return dict(vertices=vertices, faces=faces.astype(np.int64), uv=views[0].uv, texture=views[0].texture, cameras=cameras, clockwise=bool(views[0].clockwise),
                light=np.array([-0.1, -0.5, -0.4]), ambient=0.6, background=np.asarray(views[0].background_color, dtype=np.float64), scenes2d=views,
                size=size)  # fmt: skip


def view_scenes(views, faces, uv, texture, height, width, background, clockwise):
    """one Scene2D per view from the per-view arrays a fitter / Scene3DDevice computed (``ij`` [n,V,2], ``depths``, ``shade``, ``edgeflags``, as tensors)"""
    static = dict(faces=np.asarray(faces).astype(np.uint32), faces_uv=np.asarray(faces).astype(np.uint32), textured=True, uv=np.asarray(uv, dtype=np.float64),
                  texture=np.asarray(texture, dtype=np.float64), height=height, width=width, background_color=background, background_image=None,
                  clockwise=clockwise, backface_culling=True, perspective_correct=False, integer_pixel_centers=True)  # fmt: skip
    a = {k: v.detach().cpu().numpy() for k, v in views.items()}
    return [_scene2d(static, a["ij"][i].astype(np.float64), a["depths"][i].astype(np.float64), a["colors"][i].astype(np.float64),
                     a["shade"][i].astype(np.float64), a["edgeflags"][i]) for i in range(a["ij"].shape[0])]  # fmt: skip


def oracle_gradient(scenes2d, texture, obs, weights, sigma, renderer=None):
    """-> (sum over the views of sum w (image - obs)^2, its texture_b summed over the views, images) with ``texture`` in every Scene2D"""
    loss, texture_b, images = 0.0, np.zeros(np.shape(texture)), []
    for i, s in enumerate(scenes2d):
        s.texture = np.ascontiguousarray(texture, dtype=np.float64)
        image, z = (renderer or checker()).render(s, sigma)
        w = 1.0 if weights is None else np.asarray(weights, dtype=np.float64)[i][..., None]
        r = image - obs[i]
        loss += float(np.sum(w * r * r))
        texture_b += (renderer or checker()).grads(s, sigma, image, z, 2 * w * r)["texture_b"]
        images.append(image)
    return loss, texture_b, images


def oracle_fit(scenes2d, texture, obs, weights, sigma, iterations, smoothness, factor, step_max, inertia, damping, clamp, renderer=None, storage=np.float64):
    """the texture fit written out on the oracle -> (energies, per-iteration (texture before the step, texture_b incl. smoothness), final texture);
    ``storage``: the type texture, speed and gradient are rounded to between the steps (the pixel type of the run it is compared with)"""
    t, s = np.asarray(texture, dtype=storage), np.zeros(np.shape(texture), dtype=storage)
    energies, trajectory = [], []
    for _ in range(iterations):
        loss, texture_b, _images = oracle_gradient(scenes2d, t, obs, weights, sigma, renderer)
        e_smooth, g_smooth = np_smoothness(t, smoothness)
        texture_b = (texture_b.astype(storage).astype(np.float64) + g_smooth).astype(storage)
        energies.append(loss + e_smooth)
        trajectory.append((t.copy(), texture_b.copy()))
        t, s = (a.astype(storage) for a in np_step(t, s, texture_b, factor, step_max, inertia, damping, clamp))
    return np.array(energies), trajectory, t
