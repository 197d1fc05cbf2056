"""The rasterizer under autograd: the ONE implementation of its ``torch.autograd.Function``s, for the device layer (scene3d.py) and the pytorch layer.

Every op renders on a :class:`deodr_amd.hip_renderer.DeviceScene` and a :class:`deodr_amd.hip_renderer.HipRasterizer` that all renders of their owner share, so each of them follows the same
protocol, written once here as plain functions of ``ctx``:

* :func:`bind` -- forward: the inputs that are given are written into the scene, and their dtypes remembered;
* :func:`keep_forward` -- forward, after the launch: the rasterizer's generation stamp, the inputs, and what the scene read its texture / uv from when
  they are not inputs;
* :func:`restore` -- backward: when another forward has used the scene since (two cameras, or two vertex sets, in one loss) all of that is written back;
* :func:`gradients` -- backward: every gradient cast to the dtype of its input, ``None`` for everything else a forward takes.
"""

import torch

_VIEWS = ("ij", "colors", "shade", "depths", "edgeflags")
_DIFFERENTIATED = ("ij", "colors", "shade", "texture", "uv")


def _set_shared(device_scene, texture, uv):
    """the texture / texture coordinates a render is to read (None: what the scene holds)"""
    if texture is not None:
        device_scene.set_texture(texture)
    if uv is not None:
        device_scene.set_uv(uv)


def _set_views(device_scene, views):
    device_scene.set_views(**{name: t.detach() for name, t in zip(_VIEWS, views) if t is not None})


def bind(ctx, device_scene, views, texture=None, uv=None):
    """``views`` = (ij, colors, shade, depths, edgeflags), each a tensor or None, and ``texture`` / ``uv`` likewise: those given are what the next
    launch on ``device_scene`` reads; the others stay what the scene holds (and get no gradient: :func:`gradients`)."""
    _set_views(device_scene, views)
    _set_shared(device_scene, texture, uv)
    ctx.ds = device_scene
    inputs = dict(zip(_VIEWS + ("texture", "uv"), tuple(views) + (texture, uv)))
    ctx.dtypes = {name: inputs[name].dtype for name in _DIFFERENTIATED if inputs[name] is not None}


def keep_forward(ctx, rasterizer, sigma, views, texture=None, uv=None):
    """The workspace of ``rasterizer`` now holds the forward state of what :func:`bind` bound: stamp it, and save what :func:`restore` needs.  The
    per-view inputs that were None are NOT saved: a render that rebinds those arrays of the scene before this one's backward is not undone."""
    ctx.r, ctx.sigma, ctx.generation = rasterizer, sigma, rasterizer.generation
    ctx.given = tuple(t is not None for t in tuple(views) + (texture, uv))
    # what the scene read its texture and uv from when they are not inputs of this op (restored like the views)
    ctx.held = tuple(None if t is not None else source for t, source in zip((texture, uv), ctx.ds.shared_sources()))
    ctx.save_for_backward(*[t for t in tuple(views) + (texture, uv) if t is not None])


def restore(ctx):
    """If another forward has used the scene / workspace since this op's: write this one's inputs back (``render_backward`` then recomputes the
    forward state, told so by the stale ``generation``)."""
    if ctx.r.generation == ctx.generation:
        return
    saved = iter(ctx.saved_tensors)
    *views, texture, uv = (next(saved) if given else None for given in ctx.given)
    _set_views(ctx.ds, views)
    _set_shared(ctx.ds, ctx.held[0] if texture is None else texture, ctx.held[1] if uv is None else uv)


def gradients(ctx, g, arguments):
    """What a backward returns: one entry per argument of the forward, named in ``arguments`` -- ``g[name + "_b"]`` in the dtype of the input for the
    differentiated inputs that were given, None for every other argument."""
    return tuple(g[name + "_b"].to(ctx.dtypes[name]) if name in ctx.dtypes else None for name in arguments)


class RenderViewsFunc(torch.autograd.Function):
    """(ij [n,V,2], colors [n,V,C], shade [n,V][, texture [Ht,Wt,C], uv [Vuv,2]]) -> (image [n,H,W,C], z_buffer [n,H,W]): the HIP rasterizer, n views in
    one launch, with gradients for all of them.

    ``depths`` [n,V] and ``edgeflags`` [n,T,3] are inputs without gradient (dr.py:1017: the z buffer is not differentiated; the
    flags select which edges are antialiased).  ALL five per-view arrays are saved: the DeviceScene / workspace are shared by
    every render of a Scene3DDevice, and when another render has used them since (two cameras, or two vertex sets, in one loss)
    the adjoint rebuilds this forward's state from its own inputs, not from whatever the scene holds now.
    ``shade`` / ``depths`` / ``edgeflags`` may each be None (the pytorch layer's batched ops, on a prepared scene): the scene's own array is read, it
    has no gradient, and it is neither saved nor restored.
    ``texture`` / ``uv`` (optional, trailing): rendered with these values (``DeviceScene.set_texture`` / ``set_uv``) and differentiated -- their
    gradients are summed over the views, as the library delivers them.  Not given: the scene's own, no gradient, the same launches as ever."""

    ARGUMENTS = ("ij", "colors", "shade", "depths", "edgeflags", "device_scene", "rasterizer", "sigma", "texture", "uv")

    @staticmethod
    def forward(ctx, ij, colors, shade, depths, edgeflags, device_scene, rasterizer, sigma, texture=None, uv=None):
        views = (ij, colors, shade, depths, edgeflags)
        bind(ctx, device_scene, views, texture, uv)
        image, z = rasterizer.render(device_scene, sigma)
        keep_forward(ctx, rasterizer, sigma, views, texture, uv)
        ctx.mark_non_differentiable(z)
        return image, z

    @staticmethod
    def backward(ctx, image_b, _z_b):
        restore(ctx)
        g = ctx.r.render_backward(ctx.ds, image_b=image_b, generation=ctx.generation, sigma=ctx.sigma)
        return gradients(ctx, g, RenderViewsFunc.ARGUMENTS)


class RenderViewsL2Func(torch.autograd.Function):
    """(ij, colors, shade[, texture, uv]) -> (sum over the views of sum (image - obs)^2, image, z_buffer): ONE ``deodr_hip_render_scene_fit`` call renders
    and back-propagates the residual (the forward raster knows dL/dimage of a pixel the moment the pixel is resolved), so the backward
    of this op only scales the gradients the forward left.  What the reference's colour fitters write as render, subtract, square,
    sum, render_backward (deodr/mesh_fitter.py:296-318, 533-548; ``image = render(...); loss = ((image - obs) ** 2).sum(); loss.backward()`` in
    deodr/pytorch/mesh_fitter_pytorch.py) -- half the rasterizer time of the two-call path.
    ``shade`` / ``depths`` / ``edgeflags``: as in :class:`RenderViewsFunc`, None included.
    ``weights`` ([n,H,W] or [H,W], or None): the loss is ``sum(weights[..., None] * (image - obs)**2)``, see :meth:`HipRasterizer.render_fit`; not
    differentiated.  ``texture`` / ``uv`` (optional): as in :class:`RenderViewsFunc`.
    ``library_loss``: True -- the loss comes out of the fit step's own launches (no pass over the frame; a background table per observation tensor);
    False -- it is formed from the returned frame by torch ops in float64 (the pytorch layer: no table, its own rounding)."""

    ARGUMENTS = ("ij", "colors", "shade", "depths", "edgeflags", "obs", "device_scene", "rasterizer", "sigma", "weights", "texture", "uv", "library_loss")

    @staticmethod
    def forward(ctx, ij, colors, shade, depths, edgeflags, obs, device_scene, rasterizer, sigma, weights=None, texture=None, uv=None, library_loss=True):
        bind(ctx, device_scene, (ij, colors, shade, depths, edgeflags), texture, uv)
        if library_loss:
            out = torch.empty(1, dtype=torch.float64, device=ij.device)  # sum (image - obs)^2, from the same launches (no pass over the frame)
            image, z, g = rasterizer.render_fit(device_scene, obs, sigma, clear_grads=False, loss_out=out, weights=weights)
            loss = out[0]
        else:
            image, z, g = rasterizer.render_fit(device_scene, obs, sigma, clear_grads=False, weights=weights)
            r2 = (image.double() - obs.to(image.device).double()) ** 2
            if weights is not None:
                r2 = r2 * torch.as_tensor(weights).to(image.device).double()[..., None]
            loss = r2.sum()
        grads = gradients(ctx, g, RenderViewsL2Func.ARGUMENTS)
        ctx.differentiated = tuple(b is not None for b in grads)
        ctx.save_for_backward(*[b for b in grads if b is not None])
        ctx.mark_non_differentiable(image, z)
        return loss, image, z

    @staticmethod
    def backward(ctx, loss_b, _image_b, _z_b):
        saved = iter(ctx.saved_tensors)
        scaled = lambda b: loss_b.to(b.dtype) * b
        return tuple(scaled(next(saved)) if kept else None for kept in ctx.differentiated)
