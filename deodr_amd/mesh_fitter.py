"""Device-resident mesh fitters: deformable mesh + rigid pose (+ lights, colour) fitted to depth or colour images.

Same models, hyper-parameters, constructor arguments and ``step()`` protocol as the reference's fitters
(``MeshDepthFitter`` deodr/mesh_fitter.py:20-196, ``MeshRGBFitterWithPose`` :199-376, ``MeshRGBFitterWithPoseMultiFrame``
:378-632) -- but the whole iteration runs on the ROCm device: parameters, momentum, camera, lighting, silhouette flags,
rasterizer, rigid energy.  The reference chains hand-written adjoints on the host (and its PyTorch variants round-trip
through NumPy for every render); here one autograd graph per step ends in the HIP rasterizer's Function.  The multi-view
fitter renders all views of a rank in ONE batched launch and, under ``torch.distributed``, shards the views across ranks with a
single all-reduce of the shared gradients (the host ``+=`` of deodr/mesh_fitter.py:518-527).
"""

import numpy as np
import torch

from . import distributed as dd
from .fronthalf import usable as fronthalf_usable
from .scene3d import DeviceCamera, DeviceMesh, LaplacianRigidEnergyDevice, Scene3DDevice


def qrot(q, v):
    """rotate the points v [..., V, 3] by the unit quaternion(s) q [..., 4] = (x, y, z, w)   (deodr/tools.py:8-22)"""
    qv, qw = q[..., None, :3], q[..., None, 3:]
    uv = torch.cross(qv.expand_as(v), v, dim=-1)
    uuv = torch.cross(qv.expand_as(v), uv, dim=-1)
    return v + 2 * (qw * uv + uuv)


def _quat_from_euler_zyx(euler):
    import scipy.spatial.transform

    return scipy.spatial.transform.Rotation.from_euler("zyx", euler).as_quat()


# ---- what the fitters share: weights, default camera, raster state, prior, momentum, step() protocol ------------------------------------


def _weights_nhw(weights, shape, hint=" (one value per pixel)"):
    """``weights`` of a ``set_image(s)``: [H,W] (every view) or ``shape`` = [n,H,W], ``>= 0``, not checked for sign -> float64 NumPy [n,H,W]; None stays None"""
    if weights is None:
        return None
    n, height, width = shape
    w = np.asarray(weights.detach().cpu() if torch.is_tensor(weights) else weights, dtype=np.float64)
    if w.shape not in ((height, width), (n, height, width)):
        raise ValueError(f"weights must have shape [{height}, {width}] or [{n}, {height}, {width}]{hint}, not {list(w.shape)}")
    return np.array(np.broadcast_to(w, (n, height, width)))


def _pixel_weights(weights, shape, device, pixel_dtype):
    """:func:`_weights_nhw` on the device, cast to the pixel dtype at once (the texture and camera fitters, whose frame does not change after ``set_images``;
    the pose fitters keep float64 and cast lazily, :meth:`_PoseFitter._fit_weights`)"""
    w = _weights_nhw(weights, shape)
    return None if w is None else torch.as_tensor(w, device=device).to(pixel_dtype).contiguous()


def _image_term_keywords(fitter, pyramid_levels, pyramid_weights, ssim_weight, ssim_data_range, device):
    """the ``pyramid_levels=`` / ``pyramid_weights=`` and ``ssim_weight=`` / ``ssim_data_range=`` keywords of the colour and camera fitters -> the
    fitter's ``pyramid_levels``, ``pyramid_weights`` (a float64 tensor [levels+1] on ``device`` -- all ones when the keyword is None --, or None when
    the levels are 0), ``ssim_mix`` (the float64 tensor [1 - weight, weight] on ``device``, or None when the weight is 0) and ``ssim_data_range``
    (a float).  With both terms off the data term is the plain L2 of the fit step."""
    from . import pyramid

    levels, weight, real = pyramid_levels, ssim_weight, (int, float, np.integer, np.floating)
    if isinstance(levels, bool) or int(levels) != levels or not 0 <= int(levels) <= pyramid.MAX_LEVELS:
        raise ValueError(f"pyramid_levels must be an integer in 0 .. {pyramid.MAX_LEVELS}, not {levels!r}")
    levels = int(levels)
    if levels == 0 and pyramid_weights is not None:
        raise ValueError("pyramid_weights needs pyramid_levels > 0")
    w = np.ones(levels + 1) if pyramid_weights is None else np.array(pyramid_weights, dtype=np.float64)
    if w.shape != (levels + 1,):
        raise ValueError(f"pyramid_weights must have pyramid_levels + 1 = {levels + 1} entries, not shape {list(w.shape)}")
    if not np.all(w >= 0):  # (a NaN is refused as well)
        raise ValueError("pyramid_weights must be >= 0")
    if isinstance(weight, bool) or not isinstance(weight, real) or not 0 <= float(weight) <= 1:  # (a NaN is refused as well)
        raise ValueError(f"ssim_weight must be a real number in 0 .. 1, not {weight!r}")
    if isinstance(ssim_data_range, bool) or not isinstance(ssim_data_range, real) or not 0 < float(ssim_data_range) < np.inf:
        raise ValueError(f"ssim_data_range must be a finite real number > 0, not {ssim_data_range!r}")
    weight = float(weight)
    if weight > 0 and levels:
        raise ValueError("ssim_weight > 0 and pyramid_levels > 0 cannot be combined: composing the two data terms is not supported")
    fitter.pyramid_levels, fitter.pyramid_weights = levels, torch.as_tensor(w, device=device) if levels else None
    fitter.ssim_mix = torch.as_tensor([1.0 - weight, weight], dtype=torch.float64, device=device) if weight > 0 else None
    fitter.ssim_data_range = float(ssim_data_range)


def _neighbourhood_term(fitter):
    """whether the multi-scale or the structural data term is on: they are not the fit step's (the gradient of a pixel depends on its neighbours), so
    the iteration is render, the term's image_b, render_backward under autograd"""
    return bool(fitter.pyramid_levels) or fitter.ssim_mix is not None


def _render_data_term(fitter, camera, obs, weights):
    """-> (the data term that is switched on -- multi-scale, structural or the plain L2 -- of ``fitter.scene`` under ``camera``, the image)"""
    if fitter.pyramid_levels:
        return fitter.scene.render_pyramid_l2(camera, obs, fitter.pyramid_levels, weights=weights, level_weights=fitter.pyramid_weights)
    if fitter.ssim_mix is not None:
        return fitter.scene.render_ssim_l2(camera, obs, weights=weights, mix=fitter.ssim_mix, data_range=fitter.ssim_data_range)
    return fitter.scene.render_l2(camera, obs, weights=weights)


def _smoothing_keywords(smoothing, iterations):
    """the ``smoothing=`` / ``smoothing_iterations=`` keywords of the pose fitters -> (lambda as a float, 0: off; the steps of the solve)"""
    from . import smoothing as sm

    if isinstance(smoothing, bool) or not isinstance(smoothing, (int, float, np.integer, np.floating)) or not 0 <= float(smoothing) < np.inf:  # (a NaN is refused as well)
        raise ValueError(f"smoothing must be a finite real number >= 0, not {smoothing!r}")
    iterations = sm.DEFAULT_ITERATIONS if iterations is None else iterations
    if isinstance(iterations, bool) or int(iterations) != iterations or int(iterations) < 1:
        raise ValueError(f"smoothing_iterations must be an integer >= 1, not {iterations!r}")
    return float(smoothing), int(iterations)


def _kernel_clamp(step_max):
    """the kernels' convention for the clamp of a step: None or not positive means none"""
    return step_max if step_max is not None and step_max > 0 else None


def _default_camera(height, width, focal, camera_center):
    """-> (extrinsic [3,4], intrinsic [3,3]) of the camera of a fit: looking down -z from ``camera_center``, focal ``2 * width`` unless given, centred principal point"""
    focal = 2 * width if focal is None else focal
    rot = np.diag([1.0, -1.0, -1.0])
    intrinsic = np.array([[focal, 0, width / 2], [0, focal, height / 2], [0, 0, 1.0]])
    return np.column_stack((rot, -rot.T.dot(camera_center))), intrinsic


def _raster_state(scene, frame, textured, views):
    """Raster state of a fixed kernel sequence over ``frame`` = (n, H, W, C): -> (scene arrays with ``views`` bound -- no copies, the tensors are used as
    they are --, rasterizer, the (image, z) output pair in the pixel dtype).  The gradient buffers are the caller's."""
    if (scene.background_image is None) == (scene.background_color is None):
        raise BaseException("You need to provide either a background image or background color")
    n, height, width, nb_colors = frame
    ds, rasterizer = scene._rasterizer(n, height, width, nb_colors, textured, True)
    pd, dev = scene.pixel_dtype, views["ij"].device
    out = (torch.empty((n, height, width, nb_colors), dtype=pd, device=dev), torch.empty((n, height, width), dtype=pd, device=dev))
    ds.set_views(**views)
    return ds, rasterizer, out


class _GaussianPrior:
    """``regu * sum((c / sigmas)**2)`` on K coefficients (``sigmas`` [K] positive, None: ones): holds ``1 / sigmas**2``, gives energy and gradient"""

    def __init__(self, sigmas, K, regu, device):
        sig = np.ones(K) if sigmas is None else np.asarray(sigmas, dtype=np.float64)
        if sig.shape != (K,) or np.any(sig <= 0):
            raise ValueError(f"sigmas must be {K} positive numbers")
        self.regu, self.inv_sigma2 = float(regu), torch.as_tensor(1.0 / sig**2, device=device)

    def energy(self, c):
        return self.regu * (self.inv_sigma2 * c**2).sum()

    def gradient(self, c=None):
        return _prior_gradient(self.regu, self.inv_sigma2, c)


def _prior_gradient(regu, inv_sigma2, delta=None):
    """gradient of ``regu * sum(inv_sigma2 * delta**2)``; without ``delta``: the constant it is a multiple of ``delta`` by"""
    scale = 2.0 * regu * inv_sigma2
    return scale if delta is None else scale * delta


def _squared_difference(image, target):
    """squared difference per pixel [n,H,W] (what the reference's step returns for display, mesh_fitter.py:313-316)"""
    return ((image.to(torch.float64) - target) ** 2).sum(dim=-1)


def _to_host(energy, image, difference):
    """the ``step()`` protocol of the reference: a float and NumPy arrays (synchronises)"""
    return float(energy.detach()), image.to(torch.float64).cpu().numpy(), difference.cpu().numpy()


def _step_all_views(fitter):
    """-> (energy, images [n,H,W,C], squared difference per pixel [n,H,W]) as a float and NumPy arrays (synchronises): ``step()`` of the multi-view fitters"""
    energy, image = fitter.step_device()
    image = image.to(torch.float64)
    return _to_host(energy, image, _squared_difference(image, fitter.mesh_image))


class _Momentum:
    """x <- x + s,  s <- (1 - damping) (inertia s + (1 - inertia) clamp(-factor grad, +-step_max))   (mesh_fitter.py:153-190)"""

    def __init__(self, inertia, damping):
        self.inertia, self.damping, self.speed = inertia, damping, {}

    def speed_of(self, name, like):
        """the speed of this name, created as zeros of the shape of ``like`` when it is missing"""
        if name not in self.speed:
            self.speed[name] = torch.zeros_like(like, memory_format=torch.contiguous_format)
        return self.speed[name]

    def rule(self, speed, grad, factor, step_max=None):
        """-> the new speed (the rule, written once; ``step_max`` None: no clamp -- what 0 means is the caller's convention)"""
        step = grad * -factor
        if step_max is not None:
            step = step.clamp(-step_max, step_max)
        return (1 - self.damping) * (speed * self.inertia + (1 - self.inertia) * step)

    def update_all(self, entries):
        """The REBINDING update (autograd paths; ``GraphedStep`` finds the state by it).  entries: [(name, x, grad, grad2 | None, factor,
        step_max | None, normalize_rows)] -> the new x of every entry.  On float64 ROCm tensors: ONE kernel for all of them (in place on contiguous
        copies of x; ``step_max`` 0 or None: no clamp); otherwise the rule entry by entry (clamped whenever ``step_max`` is not None)."""
        from . import fronthalf

        if all(fronthalf.usable(e[1], e[2]) and (e[3] is None or fronthalf.usable(e[3])) for e in entries) and len(entries) <= 8:
            rows = [(x.contiguous().clone() if not x.is_contiguous() else x.clone(), self.speed_of(name, x), grad.contiguous(), None if grad2 is None else grad2.contiguous(),
                     factor, step_max, normalize_rows) for name, x, grad, grad2, factor, step_max, normalize_rows in entries]  # fmt: skip
            fronthalf.momentum_update(rows, self.inertia, self.damping)
            return [r[0] for r in rows]
        out = []
        for name, x, grad, grad2, factor, step_max, normalize_rows in entries:
            self.speed[name] = self.rule(self.speed_of(name, x), grad if grad2 is None else grad + grad2, factor, step_max)
            new = x + self.speed[name]
            out.append(new / new.norm(dim=-1, keepdim=True) if normalize_rows else new)
        return out

    def update_in_place(self, entries, **energy):
        """The IN-PLACE update (fixed kernel sequences: x and speed keep their storage).  entries: [(name, x, grad, grad2 | None, factor, step_max | None,
        normalize_rows, ...)] and ``energy`` as :func:`fronthalf.momentum_update` takes them: on float64 ROCm tensors that one launch; elsewhere the
        rule as torch ops, with the kernel's convention for the clamp (``step_max`` None or not positive: none)."""
        from . import fronthalf

        rows = [(x, self.speed_of(name, x)) + tuple(rest) for name, x, *rest in entries]
        if fronthalf.usable(*(r[0] for r in rows)):
            return fronthalf.momentum_update(rows, self.inertia, self.damping, **energy)
        assert not energy and all(len(r) == 7 for r in rows)
        for x, speed, grad, grad2, factor, step_max, normalize_rows in rows:
            speed.copy_(self.rule(speed, grad if grad2 is None else grad + grad2, factor, _kernel_clamp(step_max)))
            x += speed
            if normalize_rows:
                x /= x.norm(dim=-1, keepdim=True)


class GraphedStep:
    """``fitter.step_device`` captured once in a HIP graph and replayed: one graph launch per iteration instead of ~240 kernel
    launches (tools/fit_times.py: an iteration of any of the fitters takes 2.3 - 2.5 ms of host time issuing them, of which the
    rasterizer's kernels are 0.04 - 0.46 ms).

    A replay re-executes the captured kernels on the captured ADDRESSES, so the optimisation state has to live in fixed storage:
    the first (eager) call finds out which tensors a step rebinds -- parameters, momentum speeds -- gives each a persistent buffer,
    and the captured step ends by copying the new values into those buffers.  The tensors a step returns (energy, image, ...) are
    the graph's output buffers: overwritten by the next replay.  Everything the step reads besides its own state (target images,
    camera, hyper-parameters) is baked in at capture time: build a new GraphedStep after ``set_image`` or a change of constants."""

    def __init__(self, fitter, warmup=3):
        self.fitter = fitter
        self._owners = lambda: [("attr", fitter.__dict__), ("speed", fitter.momentum.speed)]
        for _ in range(warmup):  # sizes the workspace (spill pool check), creates the momentum speeds, warms the allocator
            fitter.step_device()
        before = {(kind, k): v for kind, d in self._owners() for k, v in d.items() if torch.is_tensor(v)}
        fitter.step_device()
        self.state = [(kind, k) for kind, d in self._owners() for k, v in d.items() if torch.is_tensor(v) and (kind, k) in before and before[(kind, k)] is not v]
        self.buffers = {}
        for kind, k in self.state:
            d = dict(self._owners())[kind]
            self.buffers[(kind, k)] = d[k].detach().clone().contiguous()
            d[k] = self.buffers[(kind, k)]
        self.graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=fitter.device)
        side.wait_stream(torch.cuda.current_stream(fitter.device))
        with torch.cuda.stream(side):
            self._captured_body()  # once more outside the graph, on the capture stream (allocator pools, lazy initialisations)
        torch.cuda.current_stream(fitter.device).wait_stream(side)
        it = fitter.iter
        with torch.cuda.graph(self.graph):
            self.outputs = self._captured_body()
        fitter.iter = it  # (capturing records the step without executing it)

    def _captured_body(self):
        out = self.fitter.step_device()
        for kind, k in self.state:  # the step rebound its state to fresh tensors: move the values into the persistent buffers
            d = dict(self._owners())[kind]
            self.buffers[(kind, k)].copy_(d[k])
            d[k] = self.buffers[(kind, k)]
        return tuple(o.detach() if torch.is_tensor(o) else o for o in out)

    def step_device(self):
        """one iteration = one graph launch; -> the (static) output tensors of ``fitter.step_device``.

        A spill-pool overflow (or invalid indices) inside a replay surfaces at a LATER call as an exception of ``poll_status``; by
        then the rasterizer has regrown -- i.e. freed -- the workspace whose address the graph holds, and the replays since the
        last poll (up to ``poll_every``) applied momentum updates computed from incomplete frames.  The graph is therefore
        dropped: every further call raises until the caller restores the fitter's state from its own checkpoint and builds a
        new ``GraphedStep`` (size the pool with headroom at capture time: ``HipRasterizer(pool_pairs=...)``)."""
        if self.graph is None:
            raise RuntimeError("GraphedStep: the captured graph was invalidated by a workspace overflow; restore the fitter's state and capture again")
        self.graph.replay()
        self.fitter.iter += 1
        r = self.fitter.scene._state[2] if self.fitter.scene._state is not None else None
        if r is not None:
            try:
                r.poll_status()  # (asynchronous: a spill-pool overflow inside a replay surfaces at a later call)
            except Exception:
                self.graph = None  # the workspace the graph writes to is gone: never replay it again
                raise
        return self.outputs


class _DirectIteration:
    """Buffers of a fitter iteration that runs as a FIXED KERNEL SEQUENCE (deodr_amd/csrc/dr_fititer.h) instead of an autograd graph:
    pose + projection, shading, silhouette flags, the rasterizer's fit step, the three adjoint kernels, the rigid energy and one momentum
    update of all parameters in place -- about a dozen launches, all sums deterministic.  (As torch ops, even with the fused front-half
    Functions, the colour fitter's iteration is ~155 launches of ~4 us: tools/fit_kernels.sh.)

    Layout of ``flat``: [light_b 3 | ambient_b 1 | colour_b C | data energy 1 | vertices_b 3V | mean of vertices_b 3 || quaternion_b 4n |
    translation_b 3n]: everything before the bar is shared by the views and is what ONE all-reduce sums over the ranks of a multi-GPU fit
    (no packing copies); the pose adjoints after it stay local.

    What ``step_device`` returns on this path (energy, image, ...) are views of these buffers: the next step overwrites them (``step()``
    converts them to a float and NumPy arrays at once, as the reference's protocol wants)."""

    def __init__(self, fitter, nb_colors, shaded, sh=None):
        """``sh`` = (shape of the SH coefficients, per-vertex albedo or not): the iteration of a fitter with spherical-harmonic lighting, whose shared
        block is [sh_b 9S | albedo_b (C or V C) | data energy 1 | vertices_b 3V | mean 3] instead"""
        from . import fronthalf

        f, topo, cam = fitter, fitter.mesh.topology, fitter.camera
        n, V, T, dev, C = cam.n_views, topo.nb_vertices, topo.nb_faces, fitter.device, nb_colors
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        self.posed, self.ij, self.depths, self.colors, self.shade = z(n, V, 3), z(n, V, 2), z(n, V), z(n, V, C), z(n, V)
        self.flags = torch.zeros((n, T, 3), dtype=torch.uint8, device=dev)
        self.posed_b = z(n, V, 3) if shaded else None
        self.scratch = fronthalf.fit_scratch(V, n, dev)
        head = 4 + C  # light_b 3 | ambient_b 1 | colour_b C
        if sh is not None:
            from . import hip_renderer as hr

            sh_shape, per_vertex = sh
            n_sh, n_albedo = int(np.prod(sh_shape)), (V * C if per_vertex else C)
            head = n_sh + n_albedo
            self.sh_scratch = hr.sh_scratch(V, n, C, dev)
            self.g_albedo = z(V, C) if per_vertex else None
            self.albedo_ref = z(V, C) if per_vertex else None  # the smoothness term is the Laplacian energy against zero
            self.energy3 = z(3)  # albedo smoothness, rigid + albedo smoothness, data_weight * data + both
        self.flat = z(head + 1 + 3 * V + 3 + 7 * n)
        self.shade_out, self.e_data = self.flat[:head], self.flat[head : head + 1]
        if sh is not None:
            self.sh_b = self.shade_out[:n_sh].view(sh_shape)
            self.albedo_b = self.shade_out[n_sh:].view((V, C) if per_vertex else (C,))
        self.vertices_b = self.flat[head + 1 : head + 1 + 3 * V].view(V, 3)
        self.pose_out = self.flat[head + 1 + 3 * V :]  # mean of vertices_b [3], quaternion adjoints [n,4], translation adjoints [n,3]
        self.shared = self.flat[: head + 1 + 3 * V + 3]
        self.g_rigid, self.energy, self.vmean = z(V, 3), z(2), z(3)  # energy: rigid, data_weight * data + rigid
        self.views = dict(ij=self.ij, depths=self.depths, colors=self.colors, shade=self.shade, edgeflags=self.flags)
        self.ds, self.rasterizer, (self.image, self.z) = _raster_state(f.scene, (n, cam.height, cam.width, C), False, self.views)
        assert self.ds.ij.data_ptr() == self.ij.data_ptr() and self.ds.colors.data_ptr() == self.colors.data_ptr()
        sizes = [("ij_b", (n, V, 2)), ("colors_b", (n, V, C)), ("shade_b", (n, V)), ("uv_b", tuple(self.ds.uv.shape))]
        self.grads_flat = z(sum(int(np.prod(shape)) for _, shape in sizes))  # one buffer: one fill clears all of them
        self.grads, at = {"texture_b": None}, 0
        for name, shape in sizes:
            self.grads[name] = self.grads_flat[at : at + int(np.prod(shape))].view(shape)
            at += int(np.prod(shape))
        self.bound = self.depth = self.diff = self.image_b = None

    def sync(self, fitter):
        """the kernels keep the column mean of the vertices up to date themselves; recompute it when the fitter's tensors were replaced"""
        now = (fitter.vertices, fitter.transform_quaternion, fitter.transform_translation)
        if self.bound is None or any(a is not b for a, b in zip(now, self.bound)):
            self.vmean.copy_(fitter.vertices.mean(dim=0))
            self.bound = now


class _PoseFitter:
    """deformable vertices + one rigid pose per view, shared machinery of the three fitters.

    ``subdivisions=k`` (0: off, every path as it is without the keyword): ``self.vertices`` [Vc,3] is the control cage of a Loop subdivision
    surface -- still the parameter, same ``step()`` protocol, and the Laplacian rigid energy acts on it --; ``self.mesh`` is the k-times subdivided
    mesh (faces, silhouette flags, normals, shading of the fine topology), ``self.control_mesh`` the cage.  The iteration then runs through autograd
    (the subdivision is one kernel forward, one backward: deodr_amd/subdivision.py); ``GraphedStep`` replays it as one graph launch.

    ``shape_basis`` (None: off, every path as it is without the keyword): a [K,V,3] array or a :class:`deodr_amd.basis.LinearBasis` of that shape --
    a morphable model.  The parameter is then ``self.coefficients`` [K] (float64, zeros after ``reset()``); the ``vertices`` argument is the mean and
    ``self.vertices = mean + coefficients . basis`` is derived, refreshed every step.  The energy is the data term + the Laplacian rigid energy of the
    derived vertices against the mean (same ``cregu``) + ``coefficient_regu sum((c / sigmas)**2)`` (``sigmas`` [K], None: ones).  The coefficient
    gradient is the basis adjoint (one kernel, deodr_amd/basis.py) of the total vertex gradient plus the prior's; the update is the momentum rule with
    ``step_factor_coefficients`` and the fourth entry of ``step_max``.  With ``subdivisions`` the two compose: basis, then cage, then subdivision.
    The iteration runs through autograd, as a subdivided fit does.

    ``skin`` (None: off, every path as it is without the keyword): a :class:`deodr_amd.skinning.Skin` of the mesh -- an articulated object.
    ``self.joint_quaternions`` [J,4] is one more parameter (identity after ``reset()``, or ``joint_quaternions_init``), one pose of the skeleton shared
    by all views.  What is rendered is ``qrot(q_view, skin.apply(vertices, joint_quaternions) - mean(vertices)) + t_view``: the skin acts in the frame
    the vertices and the joints were given in, then the mean of the rest vertices is subtracted (the vertices are then NOT re-centred between steps:
    they stay in the frame of the joints).  The rigid energy acts on the rest vertices as before; with ``shape_basis`` the basis comes first, the skin
    second.  The update is one more momentum entry with ``step_factor_joints``, rows renormalised; ``joint_regu >= 0`` adds the prior
    ``joint_regu sum |q - q_init|^2``.  The iteration runs through autograd; ``skin`` with ``subdivisions > 0`` is refused.

    ``smoothing`` (0: off, nothing is built and every path is as it is without the keyword) = lambda > 0: the vertices step in the metric
    ``I + lambda L`` of the graph Laplacian ``L`` (deodr_amd/smoothing.py).  The vertex entry of the momentum update receives
    ``u = (I + lambda L)^-1 (g_data + g_rigid)`` -- ``smoothing_iterations`` steps of conjugate gradients (None: ``smoothing.DEFAULT_ITERATIONS``), one
    launch on the device for a mesh of up to 1024 vertices -- in place of the sum of the two gradients (under ``torch.distributed`` after the
    all-reduce); the clamp and the momentum act on ``u``, the poses, lights, colours and joints are untouched.  A rough, sparse gradient becomes a
    smooth one of the same mean, so ``step_factor_vertices`` can be larger than without.  With ``subdivisions`` ``L`` is the cage's Laplacian and the
    cage gradient is smoothed, with ``skin`` the gradient of the rest vertices; with ``shape_basis`` the keyword is refused (the parameter is the
    coefficient vector).  ``self.smoothing_system`` is the :class:`deodr_amd.smoothing.SpdSystem` (``copy_`` the values of another lambda into its
    ``vals`` between steps, also under a ``GraphedStep``), ``self.smoothing_residual`` [3] the squared relative residual the last solve ended with,
    for display.  The iteration runs through autograd; ``GraphedStep`` replays it.

    ``rigidity``: "laplacian" (the default: the reference's ``0.5 cregu d^T (L^T L) d`` of the displacement ``d``, nothing else is built and every
    path is as it is without the keyword) or "arap": ``self.rigid_energy`` is a :class:`deodr_amd.arap.ArapEnergyDevice` -- the
    as-rigid-as-possible energy of Sorkine and Alexa, which does not charge a rotation of a part of the mesh (a finger that bends) as stretch --
    on the same vertices the Laplacian energy acts on (the cage with ``subdivisions``, the rest vertices with ``skin``, the derived vertices with
    ``shape_basis``), with ``arap_weights`` "uniform", "cotangent" (of the rest mesh, negative values clamped to 0) or an array per adjacency
    entry.  ``cregu`` keeps its name but NOT its scale: ``L^T L`` is a squared Laplacian (entries of order valence^2), the ARAP energy is first
    order in the edges, so the same ``cregu`` is a much softer regulariser under "arap" (examples/arap_hand_fitting.py says how one was chosen).
    ``smoothing`` composes unchanged.  The iteration runs through autograd; ``GraphedStep`` replays it."""

    direct = True  # run an iteration as the fixed kernel sequence of _DirectIteration when the tensors allow it (False: always autograd)
    # pose the vertices with the one kernel of fronthalf.RigidTransformFunc when the tensors allow it.  Its adjoint adds the pose gradients of the
    # wavefronts with double atomics, in no fixed order; False: the same formula as torch ops, whose reductions have one (MeshPointCloudFitter)
    fused_pose = True

    step_factor_vertices, step_factor_quaternion, step_factor_translation = 0.0005, 0.00006, 0.00005
    step_factor_coefficients = 0.0005  # (with an orthonormal basis a step of the coefficients moves the vertices as far as the same step of the vertices)
    # What the depth fits of the four-joint hand at 64 x 64 pixels are run with (tests/test_skinning_fit_host.py, first energy 3.4); the rig whose
    # first energy is 50 overshoots with it and converges with 1e-4.  The data gradient is a sum over the pixels: a step factor that suits one
    # image size scales with the inverse of the number of pixels.
    step_factor_joints = 0.0003

    def __init__(self, vertices, faces, euler_init, translation_init, cregu, inertia, damping, device, n_poses=1, clockwise=False, pixel_dtype=torch.float64,
                 subdivisions=0, shape_basis=None, coefficient_regu=0.0, sigmas=None, skin=None, joint_quaternions_init=None, joint_regu=0.0,
                 smoothing=0.0, smoothing_iterations=None, rigidity="laplacian", arap_weights="uniform"):  # fmt: skip
        self.device = torch.device(device)
        self.cregu, self.inertia, self.damping = cregu, inertia, damping
        v0 = np.asarray(vertices, dtype=np.float64)
        self.mesh = DeviceMesh(np.asarray(faces), v0, clockwise=clockwise, colors=np.zeros((v0.shape[0], 0)), device=self.device)
        # subdivisions = k > 0: `vertices` (the parameter) is the control cage of a Loop subdivision surface; what is posed, shaded and rendered is
        # the k-times subdivided mesh S vertices, and the rigid energy acts on the cage (deodr_amd/subdivision.py)
        self.subdivisions, self.control_mesh, self.subdivision = int(subdivisions), self.mesh, None
        if self.subdivisions < 0:
            raise ValueError("subdivisions must be >= 0")
        if self.subdivisions:
            with torch.no_grad():
                self.mesh = self.control_mesh.subdivise(self.subdivisions)
            self.subdivision = self.mesh.subdivision
        self.last_vertices = {}  # with subdivisions: the centred control vertices and S of them, as the last _transformed built them (in the graph)
        self.scene = Scene3DDevice(pixel_dtype=pixel_dtype)
        self.scene.set_mesh(self.mesh)
        if rigidity not in ("laplacian", "arap"):
            raise ValueError(f'rigidity must be "laplacian" or "arap", not {rigidity!r}')
        self.rigidity = rigidity
        if rigidity == "arap":
            from .arap import ArapEnergyDevice

            self.rigid_energy = ArapEnergyDevice(self.control_mesh.topology, v0, cregu, arap_weights)
        else:
            self.rigid_energy = LaplacianRigidEnergyDevice(self.control_mesh.topology, v0, cregu)
        self.vertices_init = torch.as_tensor(v0, device=self.device)
        self.shape_basis = None
        if shape_basis is not None:
            from .basis import LinearBasis

            basis = shape_basis if isinstance(shape_basis, LinearBasis) else LinearBasis(shape_basis, device=self.device, dtype=torch.float64)
            if basis.shape != tuple(v0.shape):
                raise ValueError(f"shape_basis must be [K, {v0.shape[0]}, 3] (one mode per row, of the shape of vertices), not {[basis.K, *basis.shape]}")
            if basis.mean is not None:
                raise ValueError("shape_basis: the `vertices` argument is the mean; give a LinearBasis without one")
            self.shape_basis = basis.with_mean(self.vertices_init)
            self.coefficient_regu = float(coefficient_regu)
            self._prior = _GaussianPrior(sigmas, self.shape_basis.K, self.coefficient_regu, self.device)
        self.skin = skin
        if skin is not None:
            self._init_skin(v0, joint_quaternions_init, joint_regu)
        self.smoothing, self.smoothing_iterations = _smoothing_keywords(smoothing, smoothing_iterations)
        self.smoothing_system = self.smoothing_residual = None
        if self.smoothing > 0:
            from .smoothing import laplacian_system

            if self.shape_basis is not None:
                raise ValueError("smoothing with shape_basis is not supported: the parameter is the coefficient vector, not the vertices")
            self.smoothing_system = laplacian_system(self.control_mesh.topology, self.smoothing)  # (with subdivisions: of the cage, the parameter)
        q0 = np.asarray([_quat_from_euler_zyx(e) for e in np.atleast_2d(euler_init)])
        t0 = np.atleast_2d(np.asarray(translation_init, dtype=np.float64))
        self.transform_quaternion_init = torch.as_tensor(np.broadcast_to(q0, (n_poses, 4)).copy(), device=self.device)
        self.transform_translation_init = torch.as_tensor(np.broadcast_to(t0, (n_poses, 3)).copy(), device=self.device)
        self.object_center, self.object_radius = v0.mean(axis=0), float(np.max(np.std(v0, axis=0)))
        self.reset()

    def _init_skin(self, v0, joint_quaternions_init, joint_regu):
        skin = self.skin
        if self.subdivisions:
            raise ValueError("skin with subdivisions > 0 is not supported (the skin of a subdivided cage is out of scope)")
        if skin.V != v0.shape[0]:
            raise ValueError(f"skin: a Skin of {skin.V} vertices for a mesh of {v0.shape[0]}")
        if skin.device != self.vertices_init.device:
            raise ValueError(f"skin: the Skin lives on {skin.device}, the fitter on {self.vertices_init.device}")
        if not joint_regu >= 0:
            raise ValueError("joint_regu must be >= 0")
        q = np.tile([0.0, 0.0, 0.0, 1.0], (skin.J, 1)) if joint_quaternions_init is None else np.array(joint_quaternions_init, dtype=np.float64)
        if q.shape != (skin.J, 4):
            raise ValueError(f"joint_quaternions_init must have shape [{skin.J}, 4], not {list(q.shape)}")
        self.joint_regu = float(joint_regu)
        self.joint_quaternions_init = torch.as_tensor(q / np.linalg.norm(q, axis=1, keepdims=True), device=self.device)

    def reset(self):
        self.vertices = self.vertices_init.clone()
        if self.shape_basis is not None:
            self.coefficients = torch.zeros(self.shape_basis.K, dtype=torch.float64, device=self.device)
        if self.skin is not None:
            self.joint_quaternions = self.joint_quaternions_init.clone()
        self.transform_quaternion = self.transform_quaternion_init.clone()
        self.transform_translation = self.transform_translation_init.clone()
        self.momentum = _Momentum(self.inertia, self.damping)
        self.iter = 0
        self._direct_state = None

    def _camera(self, height, width, focal, distortion, camera_center):
        return DeviceCamera(*_default_camera(height, width, focal, camera_center), height, width, distortion, self.device)

    def _transformed(self, vertices):
        """centred vertices moved by every pose: [n_poses, V, 3] (the centring is part of the graph: the data gradient comes out
        projected on zero-mean displacements, as the reference does by hand, mesh_fitter.py:140, 319)"""
        from . import fronthalf

        q = self.transform_quaternion_leaf / self.transform_quaternion_leaf.norm(dim=-1, keepdim=True)
        if self.skin is not None:  # (skinned in the frame of the joints, then moved by the mean of the rest vertices: one articulated pose for all views)
            centred = self.skin.apply(vertices, self.joint_quaternions_leaf) - vertices.mean(dim=0, keepdim=True)
        else:
            centred = vertices - vertices.mean(dim=0, keepdim=True)
        if self.subdivisions:  # (centring commutes with S: its rows sum to 1.  Centred first, the data gradient arrives on the cage projected on zero-mean displacements)
            control = centred
            centred = self.subdivision.apply(control)
            self.last_vertices = {"control": control, "fine": centred}
        if self.fused_pose and fronthalf.usable(centred, q, self.transform_translation_leaf):  # one kernel (two with its adjoint) instead of ~12 + ~25
            return fronthalf.RigidTransformFunc.apply(centred, q, self.transform_translation_leaf)
        return qrot(q, centred[None].expand(q.shape[0], -1, -1)) + self.transform_translation_leaf[:, None, :]

    def _leaves(self, extra=()):
        if self.shape_basis is not None:  # the vertices are derived: mean + coefficients . basis (not centred: _transformed does that in the graph)
            self.vertices = self.shape_basis.apply(self.coefficients)
        elif self.skin is None:  # (with a skin the vertices stay in the frame of the joints: _transformed subtracts their mean in the graph)
            self.vertices = self.vertices - self.vertices.mean(dim=0, keepdim=True)
        self.vertices_leaf = self.vertices.detach().requires_grad_(True)
        self.transform_quaternion_leaf = self.transform_quaternion.detach().requires_grad_(True)
        self.transform_translation_leaf = self.transform_translation.detach().requires_grad_(True)
        leaves = [self.vertices_leaf, self.transform_quaternion_leaf, self.transform_translation_leaf] + list(extra)
        if self.skin is not None:  # the last leaf: _without_joint_gradient takes its gradient off the list again
            self.joint_quaternions_leaf = self.joint_quaternions.detach().requires_grad_(True)
            leaves.append(self.joint_quaternions_leaf)
        return leaves

    def _without_joint_gradient(self, grads):
        """the gradients of :meth:`_leaves` without that of the joint quaternions, which is kept for :meth:`_update_pose_and_shape`"""
        grads = list(grads)
        self._g_joints = grads.pop() if self.skin is not None else None
        return grads

    def coefficients_gradient(self, g_vertices):
        """-> (basis adjoint of a vertex gradient [V,3], gradient of the prior ``coefficient_regu sum((c / sigmas)**2)``), both [K]"""
        return self.shape_basis.apply_b(g_vertices.detach()), self._prior.gradient(self.coefficients)

    def _energy_with_prior(self, energy):
        """``energy`` + the coefficient prior of a fit with ``shape_basis`` (of the parameters the gradients were taken at)"""
        if self.skin is not None and self.joint_regu:
            energy = energy + self.joint_regu * ((self.joint_quaternions - self.joint_quaternions_init) ** 2).sum()
        return energy if self.shape_basis is None else energy + self._prior.energy(self.coefficients)

    def _update_pose_and_shape(self, g_vertices, g_quaternion, g_translation, grad_rigidity, step_max, extra=()):
        """the rebinding momentum update of the shape (the vertices; with ``shape_basis`` the coefficients: the total vertex gradient goes through the
        basis adjoint), the poses and the ``extra`` entries -> the new values of the extras"""
        if self.smoothing_system is not None:  # the step in the metric I + lambda L: one solve of the total vertex gradient, then the same rule
            from .smoothing import spd_solve

            u, self.smoothing_residual = spd_solve(self.smoothing_system, (g_vertices + grad_rigidity).detach(), self.smoothing_iterations)
            shape = ("vertices", self.vertices, u, None, self.step_factor_vertices, step_max[0], 0)
        elif self.shape_basis is None:
            shape = ("vertices", self.vertices, g_vertices, grad_rigidity, self.step_factor_vertices, step_max[0], 0)
        else:
            g_c, g_prior = self.coefficients_gradient(g_vertices + grad_rigidity)
            shape = ("coefficients", self.coefficients, g_c, g_prior, self.step_factor_coefficients, step_max[3] if len(step_max) > 3 else None, 0)
        entries = [
            shape,
            ("quaternion", self.transform_quaternion, g_quaternion, None, self.step_factor_quaternion, step_max[1], 4),  # renormalised per view
            ("translation", self.transform_translation, g_translation, None, self.step_factor_translation, step_max[2], 0),
        ] + list(extra)
        if self.skin is not None:  # one pose of the skeleton, rows renormalised as the view quaternions are
            g_prior = _prior_gradient(self.joint_regu, 1.0, self.joint_quaternions - self.joint_quaternions_init) if self.joint_regu else None
            entries.append(("joint_quaternions", self.joint_quaternions, self._g_joints, g_prior, self.step_factor_joints, None, 4))
        new = self.momentum.update_all(entries)
        setattr(self, shape[0], new[0])
        self.transform_quaternion, self.transform_translation = new[1:3]
        if self.skin is not None:
            self.joint_quaternions = new.pop()
        self.iter += 1
        return new[3:]

    # ---- the iteration as a fixed kernel sequence (float64 ROCm tensors, manifold mesh) ------------------------------------------

    def _direct_iteration(self, nb_colors, shaded, sh=None):
        """-> the _DirectIteration of this fitter, or None when an iteration has to go through autograd (CPU tensors: the CPU suite;
        a non-manifold mesh: no static table for the silhouette flags; ``direct = False``; ``subdivisions > 0``: the kernels of the fixed
        sequence fold the centring and the gradient mean into passes keyed to the RENDERED vertex array, which is then not the parameter)"""
        from . import fronthalf

        if self.subdivisions or self.shape_basis is not None or self.skin is not None:  # (with a basis or a skin the rendered vertex array is not the parameter either)
            return None
        if _neighbourhood_term(self):
            return None
        if self.smoothing_system is not None:  # (the solve sits between the gradients and the momentum update, which the fixed sequence fuses with the energy)
            return None
        if self.rigidity != "laplacian":  # (the fixed sequence fuses the Laplacian energy into its first launch; the two launches of ARAP go through autograd)
            return None

        topo = self.mesh.topology
        params = (self.vertices, self.transform_quaternion, self.transform_translation)
        if not (self.direct and fronthalf.usable(*params) and all(p.is_contiguous() for p in params) and topo._edge_faces is not None
                and self.camera.n_views <= 64):  # (deodr_hip_fit_pose_project_b: at most 64 views per call)
            return None
        key = (id(self.camera), nb_colors, shaded, self.scene.pixel_dtype, id(self.scene.background_color), id(self.scene.background_image))
        if sh is not None:
            key += (sh,)
        if self._direct_state is None or self._direct_state[0] != key:
            self._direct_state = (key, _DirectIteration(self, nb_colors, shaded) if sh is None else _DirectIteration(self, nb_colors, shaded, sh))
        d = self._direct_state[1]
        d.sync(self)
        return d

    def _direct_forward(self, d, depth_colors=None, depth_scale=1.0, shade=None):
        """parameters -> posed vertices, image coordinates, depths (in the rasterizer's own arrays); then, in ONE launch, what depends on
        them but not on one another: silhouette flags, vertex colours (``shade`` = (light, ambient, colour)), rigid energy + gradient"""
        from . import fronthalf

        topo = self.mesh.topology
        d.ds.set_views(**d.views)  # (no copies; another render may have rebound them)
        fronthalf.fit_pose_project(self.vertices, d.vmean, self.transform_quaternion, self.transform_translation, self.camera, d.posed, d.ij, d.depths,
                                   depth_colors, depth_scale)  # fmt: skip
        light, ambient, color = shade if shade is not None else (None, None, None)
        fronthalf.fit_front(topo, d.posed.shape[0], d.scratch, ij=d.ij, flags=d.flags if self.scene.sigma > 0 else None, posed=d.posed, light=light,
                            ambient=ambient, color=color, colors=d.colors if shade is not None else None, vertices=self.vertices,
                            vertices_ref=self.rigid_energy.vertices_ref, cregu=self.cregu, gradient=d.g_rigid, energy=d.energy)  # fmt: skip

    def _direct_backward_and_update(self, d, depths_b, step_max, data_weight, extra=(), depths_b_scale=1.0, energy=None, views_sum=None):
        """adjoint of pose + projection, (all-reduce of the shared block,) momentum update of every parameter in place (which also adds the
        data energy to the rigid energy of :meth:`_direct_forward`)"""
        from . import fronthalf

        n = d.posed.shape[0]
        extra_sum = {} if views_sum is None else dict(colors_b=views_sum[0], colors_sum=views_sum[1])  # ([n,V,C] summed over the views -> [V,C])
        fronthalf.fit_pose_project_b(self.vertices, self.transform_quaternion, d.posed, self.camera, d.posed_b, d.grads["ij_b"], depths_b, d.vertices_b,
                                     d.pose_out, d.scratch, depths_b_scale, **extra_sum)  # fmt: skip
        self._allreduce_shared(d.shared)
        entries = [
            ("vertices", self.vertices, d.vertices_b, d.g_rigid, self.step_factor_vertices, step_max[0], 0, data_weight, d.pose_out[:3], d.vmean),
            ("quaternion", self.transform_quaternion, d.pose_out[3 : 3 + 4 * n], None, self.step_factor_quaternion, step_max[1], 4, data_weight, None, None),
            ("translation", self.transform_translation, d.pose_out[3 + 4 * n :], None, self.step_factor_translation, step_max[2], 0, data_weight, None, None),
        ] + [(name, x, g, g2, factor, None, 0, data_weight, None, None) for name, x, g, g2, factor in extra]  # fmt: skip
        energy = d.energy if energy is None else energy  # ([what the data energy is added to, the sum]; an extra entry may carry a second gradient)
        self.momentum.update_in_place(entries, scratch=d.scratch, energy=energy, data_energy=d.e_data, data_weight=data_weight)
        self.iter += 1
        return energy[1]

    def _allreduce_shared(self, shared):
        pass  # single process, every view local

    weights = None  # per-pixel weights of the data term [n,H,W] (float64, this fitter's device), or None: set_image(s)(..., weights=...)
    pyramid_levels, pyramid_weights = 0, None  # the colour fitters' multi-scale data term (their ``pyramid_levels=`` keyword); 0: off
    ssim_mix, ssim_data_range = None, 1.0  # the colour fitters' structural data term (their ``ssim_weight=`` keyword); None: off

    def _set_weights(self, w):
        """the :func:`_weights_nhw` of ``set_image`` / ``set_images`` (None: an unweighted fit), kept in float64: :meth:`_fit_weights` casts when a step needs them"""
        self._weights_key = None
        self.weights = None if w is None else torch.as_tensor(w, device=self.device)

    def _fit_weights(self):
        """the weights as the rasterizer's fit step takes them: [n,H,W] in its pixel dtype, converted once (None: no weights)"""
        if self.weights is None:
            return None
        if getattr(self, "_weights_key", None) is not self.weights:
            self._weights_key, self._weights_pix = self.weights, self.weights.to(self.scene.pixel_dtype).contiguous()
        return self._weights_pix


class MeshDepthFitter(_PoseFitter):
    """Fit a deformable mesh to a depth image (reference deodr/mesh_fitter.py:20-196)."""

    def __init__(self, vertices, faces, euler_init, translation_init, cregu=2000, inertia=0.96, damping=0.05, device="cuda", pixel_dtype=torch.float64,
                 subdivisions=0, shape_basis=None, coefficient_regu=0.0, sigmas=None, skin=None, joint_quaternions_init=None, joint_regu=0.0,
                 smoothing=0.0, smoothing_iterations=None, rigidity="laplacian", arap_weights="uniform"):  # fmt: skip
        super().__init__(vertices, faces, euler_init, translation_init, cregu, inertia, damping, device, pixel_dtype=pixel_dtype, subdivisions=subdivisions,
                         shape_basis=shape_basis, coefficient_regu=coefficient_regu, sigmas=sigmas, skin=skin,
                         joint_quaternions_init=joint_quaternions_init, joint_regu=joint_regu, smoothing=smoothing,
                         smoothing_iterations=smoothing_iterations, rigidity=rigidity, arap_weights=arap_weights)  # fmt: skip
        self.camera_center = self.object_center + np.array([-0.5, 0, 5]) * self.object_radius

    def set_max_depth(self, max_depth):
        self.max_depth = max_depth
        self.scene.set_background_color(np.array([max_depth], dtype=np.float64))

    def set_depth_scale(self, depth_scale):
        self.depthScale = depth_scale

    def set_image(self, mesh_image, focal=None, distortion=None, weights=None):
        """``weights`` [H,W], ``>= 0`` (or None): the data term becomes ``sum(weights * (clip(depth) - mesh_image)**2)`` -- 0 where the sensor
        returned no depth (a hole), so that whatever ``mesh_image`` holds there does not pull on the mesh.  Both the direct path (hence
        ``GraphedStep``) and the autograd path use them; the difference image a step returns for display stays un-weighted."""
        assert np.ndim(mesh_image) == 2
        self._set_weights(_weights_nhw(weights, (1, *np.shape(mesh_image))))
        self.height, self.width = mesh_image.shape
        self.mesh_image = torch.as_tensor(np.asarray(mesh_image, dtype=np.float64), device=self.device)
        self.camera = self._camera(self.height, self.width, focal, distortion, self.camera_center)
        self.iter = 0

    def energy(self):
        """-> (data energy, rigid energy, rigid gradient, clipped depth [H,W], squared difference [H,W]) as device tensors"""
        self.mesh.set_vertices(self._transformed(self.vertices_leaf))
        depth = self.scene.render_depth(self.camera, depth_scale=self.depthScale)[0]
        depth = depth.clamp(0, self.max_depth).to(torch.float64)
        diff_image = ((depth - self.mesh_image[:, :, None]) ** 2).sum(dim=2)
        e_rigid, g_rigid = self.rigid_energy.evaluate(self.vertices_leaf.detach())
        e_data = diff_image.sum() if self.weights is None else (self.weights[0] * diff_image).sum()
        return e_data, e_rigid, g_rigid, depth[:, :, 0], diff_image

    def _observation(self):
        """the target depth image as the rasterizer's fit step takes it: [1,H,W,1] in its pixel dtype, converted once"""
        if getattr(self, "_obs_key", None) is not self.mesh_image:
            self._obs_key, self._obs = self.mesh_image, self.mesh_image[None, :, :, None].to(self.scene.pixel_dtype).contiguous()
        return self._obs

    def _step_direct(self, d):
        from . import fronthalf

        self._direct_forward(d, d.colors, self.depthScale)  # the scaled depth of a vertex is its colour (dr.py:1001-1036)
        # the data term sum (clip(depth image, 0, max_depth) - target)^2, its gradients and its value from the rasterizer's one-call fit
        # step (four launches; render + residual + render_backward were nine)
        image, _z, _g = d.rasterizer.render_fit(d.ds, self._observation(), self.scene.sigma, grads=d.grads, out=(d.image, d.z), clear_grads=True,
                                                loss_out=d.e_data, clamp=(0.0, self.max_depth), weights=self._fit_weights())  # fmt: skip
        if d.depth is None:
            d.depth, d.diff, d.image_b = torch.empty_like(self.mesh_image), torch.empty_like(self.mesh_image), torch.empty_like(image)
            d.display_loss = torch.zeros(1, dtype=torch.float64, device=self.device)
        # (what a step returns for display: the clipped depth image and the squared difference per pixel)
        fronthalf.depth_residual(image, self.mesh_image, self.max_depth, d.depth, d.diff, d.image_b, d.display_loss, d.scratch)
        energy = self._direct_backward_and_update(d, d.grads["colors_b"], (1, 0.1, 0.1), 1.0, depths_b_scale=self.depthScale)
        return energy, d.depth, d.diff

    def step_device(self):
        """One iteration on the device -> (energy, image, difference image) as device tensors.

        OUTPUT LIFETIME: on the direct path (float64 ROCm tensors, manifold mesh: a fixed kernel sequence over persistent buffers,
        `_DirectIteration`) the returned tensors -- and ``self.vertices``, the pose, light and colour parameters -- are the SAME
        storage every step: they are updated in place, so a value kept across iterations (a trajectory, an energy history) must be
        ``.clone()``d by the caller.  The autograd path (CPU tensors, float32, non-manifold meshes) rebinds fresh tensors each step,
        as the reference does.  ``step()`` is safe either way: it converts to a float and NumPy arrays at once."""
        d = self._direct_iteration(1, False)
        if d is not None:
            return self._step_direct(d)
        leaves = self._leaves()
        e_data, e_rigid, g_rigid, depth, diff_image = self.energy()
        g_v, g_q, g_t = self._without_joint_gradient(torch.autograd.grad(e_data, leaves))
        energy = self._energy_with_prior(e_data + e_rigid)
        self._update_pose_and_shape(g_v, g_q, g_t, g_rigid, (1, 0.1, 0.1, 1))
        return energy, depth.detach(), diff_image.detach()

    def step(self):
        """-> (energy, synthetic depth [H,W], squared difference [H,W]) as a float and NumPy arrays, like the reference"""
        return _to_host(*self.step_device())


class MeshPointCloudFitter(_PoseFitter):
    """Fit a deformable mesh and one rigid pose per cloud to unorganised 3-D point sets: scans, LiDAR sweeps, back-projected depth images
    (:func:`deodr_amd.chamfer.depth_to_points`), the vertices of another mesh.  No camera and no render are involved.

    The energy is the closest-point term (:class:`deodr_amd.chamfer.PointCloudTerm`, include/deodr_hip_chamfer.h) of ``_transformed(vertices)``
    [n_poses,V,3] against one cloud per pose, summed over the poses, plus the rigid energy, plus the priors.  The iteration goes through autograd
    (the term is one op: :class:`deodr_amd.fronthalf.ChamferFunc`); ``GraphedStep`` replays it.  ``subdivisions``, ``shape_basis``, ``skin``,
    ``smoothing`` and ``rigidity`` compose through the shared machinery of :class:`_PoseFitter` (with ``subdivisions`` the fine vertices meet the
    cloud).  ``directions``, ``max_distance``, ``mix``, ``normalise``: the term's; ``self.term.params`` may be ``copy_``-ed into between steps, also
    under a ``GraphedStep`` (a ``max_distance`` that shrinks as the fit closes in).

    ``metric``: "vertex" (the default: the term above, every point against the VERTICES) or "surface": points -> mesh measures every point against
    the closest point of the closest TRIANGLE (:class:`deodr_amd.surface.PointSurfaceTerm`, include/deodr_hip_surface.h) of the mesh that meets the
    cloud -- what a cloud denser than the mesh needs: points that lie on a face then cost nothing and pull nothing.  mesh -> points is the same
    either way.  The step factors are the ones below for both metrics: a point's pull is spread over the three corners of its face with weights
    that sum to 1, so the gradients have the scale they have against the vertices (examples/point_surface_hand_fitting.py runs with them).

    ``search``: "brute" (the default) or "grid", ``cell_size``: the term's (``PointCloudTerm(search="grid")``, include/deodr_hip_chamfer_grid.h):
    the same neighbours found over a uniform grid, for clouds of 10^5 points and more; it needs a finite ``max_distance``, composes with every
    keyword the brute search composes with, and is refused together with ``metric="surface"``, whose own keyword is ``surface_search``.

    ``surface_search``: "brute" (the default) or "grid", only with ``metric="surface"``: the closest faces found over a uniform grid of the
    triangles and mesh -> points over the points' grid (``PointSurfaceTerm(search="grid")``, include_staged/deodr_hip_surface_grid.h), for the
    dense scans the surface metric is for -- a VGA depth frame against a mesh of 10^4 faces is beyond the brute-force operator's cap on F * P.
    It needs a finite ``max_distance``, takes ``cell_size``, and composes with every keyword the surface metric composes with.

    The step factors are this fitter's own, chosen on examples/point_cloud_hand_fitting.py with ``normalise=True`` (both terms are then mean squared
    distances, so the translation gradient is of the order of the offset whatever V and P are, and a vertex gradient of the order of offset / V):
    the largest powers of ten (times 1, 2 or 5) at which the hand's 60 iterations against 400 of its own posed vertices lower the energy
    monotonically after the first ten; ``step_factor_vertices`` is per vertex, multiplied by V here.  ``cregu`` is on the scale of the normalised
    term (a mean squared distance, not a sum over pixels): the default is the one value those fits were run with, not the result of a sweep."""

    step_factor_vertices, step_factor_quaternion, step_factor_translation = 0.2, 0.5, 1.0  # (vertices: times V, see above)
    step_factor_coefficients, step_factor_joints = 0.2, 0.5
    step_max = (None, None, None, None)  # no clamp: the gradients are bounded by the distances themselves
    # every other launch of this iteration adds in a fixed order (the term, the rigid energies, the momentum update): with the pose as torch ops an
    # iteration gives the same bits from run to run, and a GraphedStep the bits of the eager steps (tests/test_chamfer_gpu.py)
    fused_pose = False

    def __init__(self, vertices, faces, euler_init, translation_init, cregu=0.002, inertia=0.9, damping=0.05, device="cuda", n_poses=1,
                 directions="both", max_distance=float("inf"), mix=(1.0, 1.0), normalise=True, subdivisions=0, shape_basis=None, coefficient_regu=0.0,
                 sigmas=None, skin=None, joint_quaternions_init=None, joint_regu=0.0, smoothing=0.0, smoothing_iterations=None, rigidity="laplacian",
                 arap_weights="uniform", metric="vertex", search="brute", cell_size=None, surface_search="brute"):  # fmt: skip
        if metric not in ("vertex", "surface"):
            raise ValueError(f'metric must be "vertex" or "surface", not {metric!r}')
        if search not in ("brute", "grid"):
            raise ValueError(f'search must be "brute" or "grid", not {search!r}')
        if surface_search not in ("brute", "grid"):
            raise ValueError(f'surface_search must be "brute" or "grid", not {surface_search!r}')
        if search == "grid" and metric == "surface":
            raise ValueError('search="grid" finds nearest VERTICES: it does not go with metric="surface" (the grid over the triangles is surface_search="grid")')
        if surface_search != "brute" and metric != "surface":
            raise ValueError(f'surface_search="{surface_search}" belongs to metric="surface"')
        if cell_size is not None and search != "grid" and surface_search != "grid":
            raise ValueError('cell_size belongs to surface_search="grid"' if metric == "surface" else 'cell_size belongs to search="grid"')
        self.metric, self.search, self.surface_search = metric, search, surface_search
        super().__init__(vertices, faces, euler_init, translation_init, cregu, inertia, damping, device, n_poses=n_poses, subdivisions=subdivisions,
                         shape_basis=shape_basis, coefficient_regu=coefficient_regu, sigmas=sigmas, skin=skin,
                         joint_quaternions_init=joint_quaternions_init, joint_regu=joint_regu, smoothing=smoothing,
                         smoothing_iterations=smoothing_iterations, rigidity=rigidity, arap_weights=arap_weights)  # fmt: skip
        self.n_poses = int(n_poses)
        self.step_factor_vertices = type(self).step_factor_vertices * self.control_mesh.nb_vertices
        self._term_keywords = dict(directions=directions, max_distance=max_distance, mix=mix, normalise=normalise)
        if search == "grid":  # (its own refusals -- an infinite max_distance, a bad cell_size -- come from the term, in set_point_clouds)
            self._term_keywords.update(search=search, cell_size=cell_size)
        if surface_search == "grid":
            self._term_keywords.update(search=surface_search, cell_size=cell_size)
        self.term = None

    def set_point_clouds(self, points, weights=None, vertex_weights=None):
        """one cloud per pose: a list of [P_i,3] clouds (padded at weight 0) or [n_poses,P,3]; ``weights``: per point, ``>= 0``, of the same layout
        (None: ones); ``vertex_weights`` [V] of the vertices that meet the cloud (None: ones)"""
        if self.metric == "surface":  # the faces of the mesh that meets the cloud: the subdivided ones with subdivisions
            from .surface import PointSurfaceTerm

            term = PointSurfaceTerm(self.mesh.topology.faces, self.mesh.nb_vertices, points, weights, vertex_weights, device=self.device, **self._term_keywords)
        else:
            from .chamfer import PointCloudTerm

            term = PointCloudTerm(points, weights, vertex_weights, device=self.device, **self._term_keywords)
        if term.n != self.n_poses:
            raise ValueError(f"set_point_clouds: {term.n} clouds for a fitter of {self.n_poses} poses")
        self.term, self.iter = term, 0

    def set_point_cloud(self, points, weights=None, vertex_weights=None):
        """the cloud [P,3] of a fitter of one pose"""
        if np.ndim(points) != 2:
            raise ValueError(f"set_point_cloud: points must be [P, 3], not {list(np.shape(points))}")
        self.set_point_clouds([points], None if weights is None else [weights], vertex_weights)

    def energy(self):
        """-> (data energy, rigid energy, rigid gradient, terms [n_poses,2], posed vertices [n_poses,V,3]) as device tensors"""
        if self.term is None:
            raise RuntimeError("MeshPointCloudFitter: set_point_cloud(s) first")
        posed = self._transformed(self.vertices_leaf)
        loss, terms = self.term.evaluate(posed)
        e_rigid, g_rigid = self.rigid_energy.evaluate(self.vertices_leaf.detach())
        return loss.sum(), e_rigid, g_rigid, terms, posed

    def step_device(self):
        """One iteration on the device -> (energy, terms [n_poses,2], posed vertices [n_poses,V,3]) as device tensors"""
        leaves = self._leaves()
        e_data, e_rigid, g_rigid, terms, posed = self.energy()
        g_v, g_q, g_t = self._without_joint_gradient(torch.autograd.grad(e_data, leaves))
        energy = self._energy_with_prior(e_data + e_rigid)
        self._update_pose_and_shape(g_v, g_q, g_t, g_rigid, self.step_max)
        return energy.detach(), terms.detach(), posed.detach()

    def step(self):
        """-> (energy, terms [n_poses,2], posed vertices [n_poses,V,3]) as a float and NumPy arrays"""
        return _to_host(*self.step_device())


class MeshDepthFitterEnergy(torch.nn.Module):
    """The depth-fit energy as a module whose parameters are the vertices, the pose quaternion and the translation: ``forward()``
    renders and returns data + rigid energy, for any ``torch.optim`` optimizer (deodr/pytorch/mesh_fitter_pytorch.py:34-121).
    Same model as :class:`MeshDepthFitter` (the reference's module also reverses the winding of ``faces``, a leftover: not done here)."""

    def __init__(self, vertices, faces, euler_init, translation_init, cregu=2000, device="cuda", pixel_dtype=torch.float64):
        super().__init__()
        self._fit = MeshDepthFitter(vertices, faces, euler_init, translation_init, cregu=cregu, device=device, pixel_dtype=pixel_dtype)
        f = self._fit
        self._vertices = torch.nn.Parameter(f.vertices_init.clone())
        self.quaternion = torch.nn.Parameter(f.transform_quaternion_init[0].clone())
        self.translation = torch.nn.Parameter(f.transform_translation_init[0].clone())
        self.set_max_depth, self.set_depth_scale, self.set_image = f.set_max_depth, f.set_depth_scale, f.set_image

    def forward(self):
        f = self._fit
        f.vertices_leaf, f.transform_quaternion_leaf, f.transform_translation_leaf = self._vertices, self.quaternion[None], self.translation[None]
        e_data, _e_rigid, _g_rigid, depth, diff_image = f.energy()
        e_rigid, _ = f.rigid_energy.evaluate(self._vertices)  # differentiable: the optimizer needs its gradient through autograd
        self.depth, self.diff_image = depth.detach(), diff_image.detach()
        self.loss = e_data + e_rigid
        return self.loss


class MeshDepthFitterPytorchOptim:
    """L-BFGS (one inner iteration per step) on :class:`MeshDepthFitterEnergy` (deodr/pytorch/mesh_fitter_pytorch.py:124-170)"""

    def __init__(self, vertices, faces, euler_init, translation_init, cregu=2000, lr=0.8, device="cuda", pixel_dtype=torch.float64):
        self.energy = MeshDepthFitterEnergy(vertices, faces, euler_init, translation_init, cregu, device=device, pixel_dtype=pixel_dtype)
        self.optimizer = torch.optim.LBFGS(self.energy.parameters(), lr=lr, max_iter=1)

    def set_image(self, depth_image, focal=None, distortion=None, weights=None):
        self.energy.set_image(depth_image, focal=focal, distortion=distortion, weights=weights)

    def set_max_depth(self, max_depth):
        self.energy.set_max_depth(max_depth)

    def set_depth_scale(self, depth_scale):
        self.energy.set_depth_scale(depth_scale)

    def step(self):
        """-> (energy tensor, synthetic depth [H,W], squared difference [H,W] as NumPy)"""

        def closure():
            self.optimizer.zero_grad()
            loss = self.energy()
            loss.backward()
            return loss

        self.optimizer.step(closure)
        return self.energy.loss.detach(), self.energy.depth.cpu().numpy(), self.energy.diff_image.cpu().numpy()


class MeshRGBFitterWithPose(_PoseFitter):
    """Fit a deformable mesh, its pose, a directional + ambient light and one colour to a colour image (mesh_fitter.py:199-376).

    ``pyramid_levels`` (0: off, every path as it is without the keyword) = L in 1 .. 8: the data term becomes the multi-scale L2 of
    ``deodr_amd/pyramid.py``, ``data_weight * sum_l pyramid_weights[l] term_l`` -- the squared residual at full resolution and again after summing over
    2 x 2, ..., 2^L x 2^L cells --, which still pulls when the start is several pixels off.  ``self.pyramid_weights`` is a float64 device tensor [L+1]
    (from ``pyramid_weights``; None: all ones) that the kernels read when they run: ``copy_`` a new schedule into it between steps, also under a
    ``GraphedStep``.  The ``weights=`` of ``set_image(s)`` feed the term.  The iteration then runs through autograd (render, the term's ``image_b``,
    ``render_backward``): the one-call fit step cannot carry a term in which the gradient of a pixel depends on its neighbours.

    ``ssim_weight`` (0: off, every path as it is without the keyword) = lambda in (0, 1]: the data term becomes
    ``data_weight * ((1 - lambda) sum w (image - obs)^2 + lambda sum w (1 - SSIM))`` of ``deodr_amd/ssim.py`` -- the structural dissimilarity under an
    11 x 11 Gaussian window, which an exposure or shading the model does not explain moves far less than the pixel term --, with
    ``ssim_data_range`` the span of the intensities.  ``self.ssim_mix`` is the float64 device tensor ``[1 - lambda, lambda]`` that the kernels read
    when they run: ``copy_`` another mix into it between steps, also under a ``GraphedStep``.  The ``weights=`` of ``set_image(s)`` multiply the SSIM
    map (they do not enter its windows: dilate a mask by 5 pixels where that matters).  The iteration runs through autograd as with
    ``pyramid_levels``; the two keywords cannot be combined."""

    def __init__(self, vertices, faces, euler_init, translation_init, default_color, default_light_directional, default_light_ambient, cregu=2000,
                 inertia=0.96, damping=0.05, update_lights=True, update_color=True, device="cuda", pixel_dtype=torch.float64, n_poses=1,
                 subdivisions=0, shape_basis=None, coefficient_regu=0.0, sigmas=None, light_sh_init=None, vertex_albedo=False, albedo_regu=0.0,
                 skin=None, joint_quaternions_init=None, joint_regu=0.0, pyramid_levels=0, pyramid_weights=None, ssim_weight=0.0,
                 ssim_data_range=1.0, smoothing=0.0, smoothing_iterations=None, rigidity="laplacian", arap_weights="uniform"):  # fmt: skip
        _image_term_keywords(self, pyramid_levels, pyramid_weights, ssim_weight, ssim_data_range, torch.device(device))
        self.default_color = np.asarray(default_color, dtype=np.float64)
        self._init_lighting(light_sh_init, vertex_albedo, albedo_regu)
        self.default_light_directional = np.asarray(default_light_directional, dtype=np.float64)
        self.default_light_ambient = float(default_light_ambient)
        self.update_lights, self.update_color = update_lights, update_color
        super().__init__(vertices, faces, euler_init, translation_init, cregu, inertia, damping, device, n_poses=n_poses, pixel_dtype=pixel_dtype,
                         subdivisions=subdivisions, shape_basis=shape_basis, coefficient_regu=coefficient_regu, sigmas=sigmas, skin=skin,
                         joint_quaternions_init=joint_quaternions_init, joint_regu=joint_regu, smoothing=smoothing,
                         smoothing_iterations=smoothing_iterations, rigidity=rigidity, arap_weights=arap_weights)  # fmt: skip
        self.camera_center = self.object_center + np.atleast_2d(np.asarray(translation_init, dtype=np.float64))[0] + np.array([0, 0, 9]) * self.object_radius

    step_factor_light_sh, step_factor_albedo = 0.0001, 0.00001  # (those of the directional light and of the single colour)

    def _init_lighting(self, light_sh_init, vertex_albedo, albedo_regu):
        """``light_sh_init`` ([9] or [9,3]; None: off, every path as it is without the keyword): spherical-harmonic lighting of bands 0 - 2
        (deodr_amd/lighting.py) instead of the directional + ambient pair, which is then ignored for rendering; the parameter is ``self.light_sh``
        (``update_lights``).  ``vertex_albedo``: ``self.mesh_color`` is [V,3], initialised from ``default_color`` (``update_color``), and the energy
        gains ``0.5 albedo_regu sum_c a_c^T (L^T L) a_c`` over the Laplacian L of the rendered mesh."""
        self.light_sh_init = None if light_sh_init is None else np.asarray(light_sh_init, dtype=np.float64)
        if self.light_sh_init is not None and self.light_sh_init.shape not in ((9,), (9, 3)):
            raise ValueError(f"light_sh_init must have shape [9] or [9, 3], not {list(self.light_sh_init.shape)}")
        self.vertex_albedo, self.albedo_regu = bool(vertex_albedo), float(albedo_regu)
        if self.vertex_albedo and self.light_sh_init is None:
            raise ValueError("vertex_albedo needs light_sh_init (lighting.sh_from_directional gives the coefficients of a directional + ambient pair)")
        if self.vertex_albedo and self.albedo_regu and self.default_color.size != 3:
            raise ValueError(f"albedo_regu needs a colour of 3 channels (the smoothness term runs on [V,3] arrays), not {self.default_color.size}")
        self.light_sh = self._albedo_energy = None

    def reset(self):
        super().reset()
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=self.device)
        self.mesh_color, self.light_directional, self.light_ambient = t(self.default_color), t(self.default_light_directional), t(self.default_light_ambient)
        if self.light_sh_init is not None:
            self.light_sh = t(self.light_sh_init)
            if self.vertex_albedo:
                V = self.mesh.nb_vertices
                self.mesh_color = t(np.broadcast_to(self.default_color, (V, self.default_color.size)).copy())
                if self.albedo_regu and self._albedo_energy is None:
                    self._albedo_energy = LaplacianRigidEnergyDevice(self.mesh.topology, np.zeros((V, 3)), self.albedo_regu)

    def set_background_color(self, background_color):
        self.scene.set_background_color(background_color)

    def set_image(self, mesh_image, focal=None, distortion=None, weights=None):
        """``weights`` [H,W], ``>= 0`` (or None): the data term becomes ``sum(weights[..., None] * (image - mesh_image)**2)`` -- a foreground
        mask, an occluder to ignore, a confidence map.  Used by the direct path (hence ``GraphedStep``) and by the autograd path alike."""
        assert np.ndim(mesh_image) == 3
        self._set_weights(_weights_nhw(weights, (1, *np.shape(mesh_image)[:2])))
        self.height, self.width = mesh_image.shape[:2]
        self.mesh_image = torch.as_tensor(np.asarray(mesh_image, dtype=np.float64), device=self.device)[None]
        self.camera = self._camera(self.height, self.width, focal, distortion, self.camera_center)
        self.iter = 0

    def _appearance_leaves(self):
        self.mesh_color_leaf = self.mesh_color.detach().requires_grad_(True)
        if self.light_sh is not None:
            self.light_sh_leaf = self.light_sh.detach().requires_grad_(True)
            return [self.mesh_color_leaf, self.light_sh_leaf]
        self.light_directional_leaf = self.light_directional.detach().requires_grad_(True)
        self.light_ambient_leaf = self.light_ambient.detach().requires_grad_(True)
        return [self.mesh_color_leaf, self.light_directional_leaf, self.light_ambient_leaf]

    def _pose_scene(self):
        self.mesh.set_vertices(self._transformed(self.vertices_leaf))
        if self.light_sh is not None:  # one launch: albedo ([3] or [V,3]) times the SH irradiance (Scene3DDevice._vertex_inputs)
            self.scene.light_sh, self.scene.light_directional, self.scene.light_ambient = self.light_sh_leaf, None, 0.0
            self.mesh.set_vertices_colors(self.mesh_color_leaf)
            return
        self.scene.light_directional, self.scene.light_ambient = self.light_directional_leaf, self.light_ambient_leaf
        self.mesh.set_vertices_colors(self.mesh_color_leaf[None, :].expand(self.mesh.nb_vertices, -1))

    def render(self):
        """the image(s) of the current parameters [n,H,W,C] (mesh_fitter.py:270-285)"""
        self._leaves(self._appearance_leaves())
        self._pose_scene()
        return self.scene.render(self.camera).to(torch.float64).detach()

    data_weight = 1.0  # of sum (image - obs)^2 in the energy

    def _observation(self):
        """the target image(s) in the rasterizer's pixel dtype, converted once"""
        if getattr(self, "_obs_key", None) is not self.mesh_image:
            self._obs_key, self._obs = self.mesh_image, self.mesh_image.to(self.scene.pixel_dtype).contiguous()
        return self._obs

    def _data_energy(self):
        """-> (data energy, image [n,H,W,C]).  The data term of the colour fitters is exactly sum (image - obs)^2
        (mesh_fitter.py:296-318): rendered AND back-propagated by the one-call fit step (Scene3DDevice.render_l2)."""
        self._pose_scene()
        loss, image = _render_data_term(self, self.camera, self._observation(), self._fit_weights())
        return self.data_weight * loss, image

    def diff_image(self, image):
        """squared difference per pixel [n,H,W] (what the reference's step returns for display, mesh_fitter.py:313-316)"""
        return _squared_difference(image, self.mesh_image)

    def _reduce_shared(self, grads):
        return grads  # single process, every view local

    def _albedo_smoothness(self):
        """-> (0.5 albedo_regu sum_c a_c^T (L^T L) a_c, its gradient [V,3]) or (0, None) without the term"""
        if self._albedo_energy is None:
            return 0.0, None
        return self._albedo_energy.evaluate(self.mesh_color.detach())

    # The two lighting models -- the directional + ambient pair with one colour, and spherical harmonics (``light_sh``) with one colour or a per-vertex
    # albedo -- differ in four places: the leaves (:meth:`_appearance_leaves`), the appearance parameters a step updates with their step factors
    # (:meth:`_appearance_updates`), the shading launch and its adjoint on the direct path (:meth:`_step_direct`, :meth:`_direct_shade_b`), and the
    # albedo-smoothness energy, which only the second has.  One autograd step and one direct step serve both.

    def _appearance_updates(self, g_color, g_lights, g_albedo=None):
        """-> [(name, parameter, gradient, second gradient | None, step factor)] of what ``update_lights`` / ``update_color`` let move"""
        updates = []
        if self.update_lights and self.light_sh is not None:
            updates.append(("light_sh", self.light_sh, g_lights[0], None, self.step_factor_light_sh))
        elif self.update_lights:
            updates += [("light_directional", self.light_directional, g_lights[0], None, 0.0001), ("light_ambient", self.light_ambient, g_lights[1], None, 0.0001)]
        if self.update_color:
            updates.append(("mesh_color", self.mesh_color, g_color, g_albedo, self.step_factor_albedo if self.light_sh is not None else 0.00001))
        return updates

    def _direct_shade_b(self, d):
        """adjoint of the shading -> (appearance updates, [what the data energy is added to, the sum] | None, views_sum | None)"""
        from . import fronthalf
        from . import hip_renderer as hr

        topo = self.mesh.topology
        if self.light_sh is None:
            fronthalf.vertex_shade_b(d.posed, topo, self.light_directional, self.light_ambient, self.mesh_color, None, d.grads["colors_b"], d.posed_b,
                                     d.shade_out, d.scratch)  # fmt: skip
            return self._appearance_updates(d.shade_out[4:], (d.shade_out[:3], d.shade_out[3:4])), None, None
        # SH: two launches.  A per-vertex albedo under several views: sh_shade_b leaves the products colors_b E of every view in its scratch and their sum
        # over the views rides in fit_pose_project_b (its colors_sum), a launch the iteration has anyway
        views_sum = (hr.sh_products(d.sh_scratch, *d.posed.shape[1::-1], d.albedo_b.shape[-1]), d.albedo_b) if self.vertex_albedo and d.posed.shape[0] > 1 else None
        hr.sh_shade_b(d.posed, topo._faces_u32, topo._vf_offsets, topo._vf_corners, self.light_sh, self.mesh_color, colors_b=d.grads["colors_b"], posed_b=d.posed_b,
                      sh_b=d.sh_b, albedo_b=None if views_sum else d.albedo_b, scratch=d.sh_scratch, clockwise=topo.clockwise, want=(False, False, False))  # fmt: skip
        energy, g_albedo = None, None
        if self._albedo_energy is not None:
            # the albedo smoothness, one launch.  energy3 = [albedo smoothness, rigid energy + it, data_weight * data + both]: the kernel adds the rigid
            # energy of the front launch, the momentum update the data term
            fronthalf.rigid_energy(self.mesh_color, d.albedo_ref, topo, self.albedo_regu, d.g_albedo, d.energy3[:2], d.scratch, data_energy=d.energy[:1])
            energy, g_albedo = d.energy3[1:], d.g_albedo
        return self._appearance_updates(d.albedo_b, (d.sh_b,), g_albedo), energy, views_sum

    def _step_direct(self, d):
        """the iteration as a fixed kernel sequence: the front launch (with the directional shading, or followed by the SH shading), the rasterizer's fit
        step, the adjoint of the shading, the adjoint of pose + projection and one momentum update of every parameter"""
        if self.light_sh is None:  # (the directional shading rides in the front launch)
            self._direct_forward(d, shade=(self.light_directional, self.light_ambient, self.mesh_color))
        else:
            from . import hip_renderer as hr

            topo = self.mesh.topology
            self._direct_forward(d)
            hr.sh_shade(d.posed, topo._faces_u32, topo._vf_offsets, topo._vf_corners, self.light_sh, self.mesh_color, colors=d.colors, clockwise=topo.clockwise,
                        want_luminosity=False)  # fmt: skip
        # image, gradients AND the data energy from the rasterizer's four launches (the residual of every pixel is in the tile walkers'
        # registers; a separate pass over the 8-view frame was 73 us of a 350 us iteration)
        image, _z, _g = d.rasterizer.render_fit(d.ds, self._observation(), self.scene.sigma, grads=d.grads, out=(d.image, d.z), clear_grads=True,
                                                loss_out=d.e_data, weights=self._fit_weights())  # fmt: skip
        updates, energy, views_sum = self._direct_shade_b(d)
        return self._direct_backward_and_update(d, None, (0.5, 0.05, 0.1), self.data_weight, updates, energy=energy, views_sum=views_sum), image

    def _step_autograd(self):
        sh = self.light_sh is not None
        leaves = self._leaves(self._appearance_leaves())
        e_data, image = self._data_energy()
        e_rigid, g_rigid = self.rigid_energy.evaluate(self.vertices_leaf.detach())
        e_albedo, g_albedo = self._albedo_smoothness() if sh else (None, None)
        g_v, g_q, g_t, g_col, *g_lights = self._without_joint_gradient(torch.autograd.grad(e_data, leaves))
        if self.skin is None:
            g_v, g_col, *g_lights, e_data = self._reduce_shared([g_v, g_col, *g_lights, e_data.detach()])
        else:  # (the pose of the skeleton is shared by the views, as the vertices are)
            g_v, g_col, *g_lights, self._g_joints, e_data = self._reduce_shared([g_v, g_col, *g_lights, self._g_joints, e_data.detach()])
        updates = self._appearance_updates(g_col, g_lights, g_albedo)
        energy = self._energy_with_prior(e_data + e_rigid + e_albedo if sh else e_data + e_rigid)
        flat = lambda t: t.reshape(1) if t.dim() == 0 else t  # (``light_ambient`` is a scalar tensor: one row of one element for the update, () again after it)
        new = self._update_pose_and_shape(g_v, g_q, g_t, g_rigid, (0.5, 0.05, 0.1, 0.5),
                                          [(name, flat(x), flat(g), g2, factor, None, 0) for name, x, g, g2, factor in updates])  # fmt: skip
        for (name, x, *_), value in zip(updates, new):
            setattr(self, name, value.reshape(()) if x.dim() == 0 else value)
        return energy, image.detach()

    def step_device(self):
        """One iteration on the device -> (energy, image [n,H,W,C]) as device tensors.  OUTPUT LIFETIME: as :meth:`MeshDepthFitter.step_device` -- on the
        direct path the returned tensors and every parameter, light and colour included, are the same storage every step: ``.clone()`` what is kept."""
        if self.light_sh is not None:
            d = self._direct_iteration(int(self.mesh_color.shape[-1]), True, sh=(tuple(self.light_sh.shape), self.vertex_albedo))
            direct = d is not None and fronthalf_usable(self.mesh_color, self.light_sh) and self.light_sh.is_contiguous() and self.mesh_color.is_contiguous()
        else:
            d = None if self.light_directional is None else self._direct_iteration(int(self.mesh_color.numel()), True)
            direct = d is not None and fronthalf_usable(self.mesh_color, self.light_directional, self.light_ambient)
        return self._step_direct(d) if direct else self._step_autograd()

    def step(self):
        """-> (energy, image [H,W,C], squared difference [H,W]) as a float and NumPy arrays, the reference's protocol (synchronises;
        a loop that never needs them on the host calls step_device -- or a GraphedStep of it -- instead)"""
        energy, image = self.step_device()
        return _to_host(energy, image[0], self.diff_image(image)[0])


class MeshRGBFitterWithPoseMultiFrame(MeshRGBFitterWithPose):
    """One deformable mesh, lights and colour shared by ``n`` views, one pose per view (mesh_fitter.py:378-632).

    All views of this process are rendered by ONE batched launch.  Under ``torch.distributed`` (one process per GPU, RCCL) the
    views shard across the ranks (``deodr_amd.distributed.shard_views``): each rank holds the poses of its own views, the shared
    parameters are replicated, and the only communication per step is one all-reduce of the packed shared gradients + energy.

    Deliberate deviations from the reference's class (its trajectories are therefore NOT those of the unmodified reference; the
    golden this class is tested on, tests/golden/rgb_multiview_fit.npz, comes from a subclass with the first two repaired -- DESIGN.md
    section 6, divergence 6): (1) the data term compares the rendered image of frame ``idframe`` with that frame's photograph (the
    reference indexes ROW ``idframe`` of the image, mesh_fitter.py:538-544); (2) the quaternions are renormalised per view (the
    reference divides the whole [n, 4] array by its Frobenius norm, :595, which shrinks every rotation step by sqrt(n)); (3) the
    data gradient is always projected on zero-mean displacements (the reference stops doing so from iteration 500 on, :573);
    (4) ``update_lights`` / ``update_color`` switch the light and colour updates off (the reference stores the flags and updates
    anyway, :604-613)."""

    # the reference's multi-frame class has its own constants (mesh_fitter.py:391-416): smaller pose steps, more damping, a nearer
    # camera that does not follow translation_init, and a data term weighted by cdata / number of views
    step_factor_quaternion, step_factor_translation = 0.00005, 0.00004

    def __init__(self, vertices, faces, euler_init, translation_init, default_color, default_light_directional, default_light_ambient, cregu=2000,
                 cdata=1, inertia=0.97, damping=0.15, update_lights=True, update_color=True, device="cuda", pixel_dtype=torch.float64, group=None,
                 subdivisions=0, shape_basis=None, coefficient_regu=0.0, sigmas=None, light_sh_init=None, vertex_albedo=False, albedo_regu=0.0,
                 skin=None, joint_quaternions_init=None, joint_regu=0.0, pyramid_levels=0, pyramid_weights=None, ssim_weight=0.0,
                 ssim_data_range=1.0, smoothing=0.0, smoothing_iterations=None, rigidity="laplacian", arap_weights="uniform"):  # fmt: skip
        euler_init, translation_init = np.atleast_2d(euler_init), np.atleast_2d(translation_init)
        self.cdata = cdata
        self.n_views_total = max(len(euler_init), len(translation_init))
        import torch.distributed as dist

        self.group = group
        self.rank, self.world = (dist.get_rank(group), dist.get_world_size(group)) if dist.is_available() and dist.is_initialized() else (0, 1)
        self.my_views = list(dd.shard_views(self.n_views_total, self.rank, self.world))
        pick = lambda a: np.broadcast_to(a, (self.n_views_total, a.shape[1]))[self.my_views]
        super().__init__(vertices, faces, pick(euler_init), pick(translation_init), default_color, default_light_directional, default_light_ambient,
                         cregu, inertia, damping, update_lights, update_color, device, pixel_dtype, n_poses=len(self.my_views), subdivisions=subdivisions,
                         shape_basis=shape_basis, coefficient_regu=coefficient_regu, sigmas=sigmas, light_sh_init=light_sh_init,
                         vertex_albedo=vertex_albedo, albedo_regu=albedo_regu, skin=skin, joint_quaternions_init=joint_quaternions_init,
                         joint_regu=joint_regu, pyramid_levels=pyramid_levels, pyramid_weights=pyramid_weights, ssim_weight=ssim_weight,
                         ssim_data_range=ssim_data_range, smoothing=smoothing, smoothing_iterations=smoothing_iterations, rigidity=rigidity,
                         arap_weights=arap_weights)  # fmt: skip
        self.camera_center = self.object_center + np.array([0, 0, 6]) * self.object_radius
        self._packed = None

    # the data term: (cdata / number of views) * sum over THIS rank's views of the squared residual (mesh_fitter.py:533-548; the
    # reference compares row `idframe` of the rendered image with the target there -- a defect, the image of the frame is meant --
    # and is followed as repaired, see tests/golden/make_golden.py::rgb_multiview_fit)
    data_weight = property(lambda self: self.cdata / self.n_views_total)

    def set_images(self, mesh_images, focal=None, distortion=None, weights=None):
        """``mesh_images``: the images of ALL views (every rank keeps only its own).  ``weights``: [H,W] for every view or [n_views_total,H,W],
        of ALL views as well -- sharded with the images (``distributed.shard_views``) --, ``>= 0``: the data term of view v becomes
        ``sum(weights[v][..., None] * (image_v - mesh_images[v])**2)``; a view of weight 0 everywhere does not pull on the shared parameters."""
        imgs = np.stack([np.asarray(mesh_images[i], dtype=np.float64) for i in self.my_views])
        w = _weights_nhw(weights, (self.n_views_total, *imgs.shape[1:3]), hint="")
        self._set_weights(None if w is None else w[self.my_views])
        self.height, self.width = imgs.shape[1:3]
        self.mesh_image = torch.as_tensor(imgs, device=self.device)
        cam = self._camera(self.height, self.width, focal, distortion, self.camera_center)
        n = len(self.my_views)
        self.camera = DeviceCamera(cam.extrinsic.expand(n, -1, -1), cam.intrinsic.expand(n, -1, -1), self.height, self.width,
                                   None if cam.distortion is None else cam.distortion[0], self.device)  # fmt: skip
        self.iter = 0

    set_image = None  # (one image per view: use set_images)

    def _reduce_shared(self, grads):
        if self.world == 1:
            return grads
        if self._packed is None:
            self._packed = dd.PackedGradients([g.shape for g in grads], dtype=torch.float64, device=self.device)
        return dd.allreduce_shared_gradients(self._packed, grads, self.group)

    def _allreduce_shared(self, shared):
        if self.world > 1:
            import torch.distributed as dist

            dist.all_reduce(shared, op=dist.ReduceOp.SUM, group=self.group)  # (the shared gradients are contiguous by construction)

    step = _step_all_views


# ---- texture estimation -----------------------------------------------------------------------------------------------------------------


def texture_smoothness_torch(texture, gradient, weight):
    """``deodr_hip_texture_smoothness`` as torch ops, for tensors the library does not take (CPU tensors: the CPU suite): -> the energy
    ``0.5 weight (sum of the squared differences of x- and y-neighbours)`` of ``texture`` [Ht,Wt,C] (float64 scalar tensor); its gradient
    ``weight (deg t - sum of the neighbours)`` is accumulated into ``gradient`` in place.  Arithmetic in float64, one rounding to the storage type."""
    t = texture.detach().to(torch.float64)
    dx, dy = t[:, 1:] - t[:, :-1], t[1:] - t[:-1]
    g = torch.zeros_like(t)
    g[:, 1:] += dx
    g[:, :-1] -= dx
    g[1:] += dy
    g[:-1] -= dy
    gradient.copy_((gradient.to(torch.float64) + weight * g).to(gradient.dtype))
    return 0.5 * weight * ((dx * dx).sum() + (dy * dy).sum())


def texture_step_torch(texture, speed, gradient, factor, step_max=None, inertia=0.0, damping=0.0, clamp=None):
    """``deodr_hip_texture_step`` as torch ops (:meth:`_Momentum.rule` plus the clamp of the texture; ``step_max`` None or not positive: no clamp of the
    step), in place on ``texture`` and ``speed``; float64 arithmetic"""
    s = _Momentum(inertia, damping).rule(speed.to(torch.float64), gradient.to(torch.float64), factor, _kernel_clamp(step_max))
    t = texture.detach().to(torch.float64) + s
    if clamp is not None:
        clipped = (t < clamp[0]) | (t > clamp[1])
        t, s = t.clamp(clamp[0], clamp[1]), torch.where(clipped, torch.zeros_like(s), s)  # (the momentum does not keep pushing into the wall)
    texture.detach().copy_(t.to(texture.dtype))
    speed.copy_(s.to(speed.dtype))


class MeshTextureFitterMultiFrame:
    """Fit the TEXTURE of a mesh of known shape to ``n`` calibrated views: geometry, poses / cameras and light are given (for example by a
    :class:`MeshRGBFitterWithPoseMultiFrame` run), the unknown is ``texture`` [Ht,Wt,C].  With the geometry fixed the image is linear in the texels:
    the energy ``sum(weights * (image - observation)**2) + 0.5 smoothness (squared differences of neighbouring texels)`` is a linear least-squares
    problem, minimised by the momentum descent of the other fitters; texels no view sees are in-painted by the smoothness term.

    ``poses`` = (euler angles [n,3], translations [n,3]) of the mesh in front of the fitters' camera (the convention of
    :class:`MeshRGBFitterWithPoseMultiFrame`: the vertices are centred, rotated and moved), or ``cameras`` = a :class:`DeviceCamera` of ``n`` views (or a
    list of cameras) looking at the vertices as they are.

    Projection, silhouette flags and luminosity are computed ONCE, in :meth:`set_images`.  An iteration on the device is then a fixed sequence: the
    rasterizer's one-call fit step (image, data energy, ``texture_b``), ``deodr_hip_texture_smoothness`` into the same ``texture_b``,
    ``deodr_hip_texture_step`` in place -- no autograd graph, no tensor rebound, so ``GraphedStep(fitter)`` replays it as it is.  On CPU tensors the same
    two formulas run as torch ops around ``Scene3DDevice._rasterize_l2`` under autograd (which has no CPU implementation in the product: tests put a
    checker-backed stand-in there).

    ``texture_basis`` (None: off, every path as it is without the keyword): a [K,Ht,Wt,C] array or a :class:`deodr_amd.basis.LinearBasis` of that
    shape -- an eigen-texture model, the reference's deodr/examples/eigen_faces.py.  The parameter is then ``self.coefficients`` [K] (float64, zeros
    after ``reset()``), ``texture_init`` is the mean and ``self.texture = mean + coefficients . basis`` is written IN PLACE in the pixel dtype at the
    start of every iteration (the scene keeps reading the same tensor).  The energy is data + smoothness + ``coefficient_regu sum((c / sigmas)**2)``.
    One device iteration stays a fixed sequence: ``deodr_hip_basis_apply``, the fit step, the smoothness kernel when ``smoothness > 0``, one
    element-wise op that writes the prior's gradient into the coefficient gradient, ``deodr_hip_basis_apply_b`` accumulating onto it,
    ``deodr_hip_momentum_update`` of the coefficients (``step_factor_coefficients``, ``step_max``).  With a basis the texture is NOT clamped
    (``clamp`` is ignored), as in the reference's example: a clamp is not a linear function of the coefficients."""

    step_factor_texture = 0.5
    step_factor_coefficients = 0.5  # (for a basis of orthonormal rows: a step of the coefficients then moves the texture as far as the same step of the texels)

    def __init__(self, vertices, faces, uv, faces_uv, texture_init, light_directional, light_ambient, poses=None, cameras=None, smoothness=0.1,
                 inertia=0.9, damping=0.05, clamp=(0.0, 1.0), step_max=None, clockwise=False, sigma=1.0, device="cuda", pixel_dtype=torch.float32,
                 texture_basis=None, coefficient_regu=0.0, sigmas=None):  # fmt: skip
        if (poses is None) == (cameras is None):
            raise ValueError("MeshTextureFitterMultiFrame: give either poses = (euler [n,3], translations [n,3]) or cameras")
        self.device, self.pixel_dtype = torch.device(device), pixel_dtype
        self.smoothness, self.inertia, self.damping, self.clamp, self.step_max = float(smoothness), inertia, damping, clamp, step_max
        v0 = np.asarray(vertices, dtype=np.float64)
        self.texture_init = torch.as_tensor(np.asarray(texture_init, dtype=np.float64), device=self.device).to(pixel_dtype).contiguous()
        if self.texture_init.dim() != 3:
            raise ValueError("texture_init must have shape [Ht, Wt, C]")
        self.texture_basis = None
        if texture_basis is not None:
            from .basis import LinearBasis

            basis = texture_basis if isinstance(texture_basis, LinearBasis) else LinearBasis(texture_basis, device=self.device, dtype=pixel_dtype)
            if basis.shape != tuple(self.texture_init.shape):
                raise ValueError(f"texture_basis must be [K, {', '.join(str(int(v)) for v in self.texture_init.shape)}] (one mode per row, of the shape of "
                                 f"texture_init), not {[basis.K, *basis.shape]}")  # fmt: skip
            if basis.mean is not None:
                raise ValueError("texture_basis: `texture_init` is the mean; give a LinearBasis without one")
            self.texture_basis = basis.with_mean(np.asarray(texture_init, dtype=np.float64))
            self._prior = _GaussianPrior(sigmas, basis.K, coefficient_regu, self.device)
            self.coefficient_regu = self._prior.regu
            self._prior_scale = self._prior.gradient()  # gradient of the prior = this * coefficients (a constant: the fixed sequence multiplies in place)
        self.mesh = DeviceMesh(np.asarray(faces), v0, clockwise=clockwise, uv=uv, faces_uv=faces_uv, texture=None, device=self.device)
        self.scene = Scene3DDevice(sigma=sigma, pixel_dtype=pixel_dtype)
        self.scene.set_mesh(self.mesh)
        self.scene.set_light(light_directional, light_ambient)
        self.poses, self.cameras = poses, cameras
        self.object_center, self.object_radius = v0.mean(axis=0), float(np.max(np.std(v0, axis=0)))
        self.camera_center = self.object_center + np.array([0, 0, 6]) * self.object_radius  # (MeshRGBFitterWithPoseMultiFrame's)
        self.weights = self._views = None
        self.reset()

    def reset(self):
        self.texture = self.texture_init.clone()
        self.mesh.texture = self.texture  # (the scene renders the value this tensor has at every call; it is updated in place)
        self.momentum = _Momentum(self.inertia, self.damping)
        self.momentum.speed["texture"] = torch.zeros_like(self.texture)
        if self.texture_basis is not None:
            z = lambda: torch.zeros(self.texture_basis.K, dtype=torch.float64, device=self.device)
            self.coefficients, self.coefficients_b, self.momentum.speed["coefficients"] = z(), z(), z()
            self.e_prior, self._prior_terms = torch.zeros(1, dtype=torch.float64, device=self.device), z()
        self.iter = 0

    def set_background_color(self, background_color):
        self.scene.set_background_color(background_color)

    def set_images(self, images, focal=None, distortion=None, weights=None):
        """``images`` [n,H,W,C]: one photograph per view.  ``weights`` [H,W] or [n,H,W], ``>= 0`` (or None): per-pixel weights of the squared residual --
        a mask on what is not the object, a view to leave out (0 everywhere)."""
        from . import hip_renderer

        imgs = np.stack([np.asarray(im, dtype=np.float64) for im in images])
        n, height, width, nb_colors = imgs.shape
        if nb_colors != int(self.texture.shape[2]):
            raise ValueError(f"the images have {nb_colors} channels, the texture {int(self.texture.shape[2])}")
        dev, mesh = self.device, self.mesh
        if self.cameras is not None:
            cam = self.cameras if isinstance(self.cameras, DeviceCamera) else DeviceCamera.stack(list(self.cameras), dev)
            posed = mesh.vertices
        else:
            euler, translation = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in self.poses)
            extrinsic, intrinsic = _default_camera(height, width, focal, self.camera_center)
            cam = DeviceCamera(np.broadcast_to(extrinsic, (n, 3, 4)).copy(), np.broadcast_to(intrinsic, (n, 3, 3)).copy(), height, width, distortion, dev)
            q = torch.as_tensor(np.broadcast_to(np.asarray([_quat_from_euler_zyx(e) for e in euler]), (n, 4)).copy(), device=dev)
            t = torch.as_tensor(np.broadcast_to(translation, (n, 3)).copy(), device=dev)
            centred = mesh.vertices - mesh.vertices.mean(dim=0, keepdim=True)
            posed = qrot(q / q.norm(dim=-1, keepdim=True), centred[None].expand(n, -1, -1)) + t[:, None, :]
        if cam.n_views != n or (cam.height, cam.width) != (height, width):
            raise ValueError(f"{n} images of {height} x {width} for {cam.n_views} cameras of {cam.height} x {cam.width}")
        with torch.no_grad():  # the front half of an iteration, once: nothing in it depends on the texture
            ij, depths = cam.project_points(posed)
            lum = self.scene.vertices_luminosity(posed)
            lum = lum[None].expand(n, -1) if lum.dim() == 1 else lum
            flags = mesh.topology.edge_on_silhouette(ij) if self.scene.sigma > 0 else torch.zeros((n, mesh.nb_faces, 3), dtype=torch.uint8, device=dev)
        colors = torch.zeros((n, mesh.nb_vertices, nb_colors), dtype=torch.float64, device=dev)
        self.camera = cam
        self._views = dict(ij=ij.contiguous(), depths=depths.contiguous(), colors=colors, shade=lum.contiguous(), edgeflags=flags.contiguous())
        self.mesh_image = torch.as_tensor(imgs, device=dev)
        self._obs = self.mesh_image.to(self.pixel_dtype).contiguous()
        self.weights = _pixel_weights(weights, (n, height, width), dev, self.pixel_dtype)
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        self.e_data, self.e_smooth, self._energy = z(1), z(1), z(1)
        self._direct = None
        if self.device.type == "cuda":
            ds, r, out = _raster_state(self.scene, (n, height, width, nb_colors), True, self._views)
            ds.set_texture(self.texture)
            self._direct = (ds, r, ds.zero_grads(), out)
            self._scratch = hip_renderer.texture_scratch(dev)  # (its own: a captured step replays on the addresses it was captured with)
            if self.texture_basis is not None:
                self._basis_scratch = hip_renderer.basis_scratch(self.texture_basis.K, self.texture_basis.N, 1, dev)
        self.iter = 0

    def _gradient(self):
        """-> (texture_b = d (data + smoothness) / d texture, image [n,H,W,C]); the two energies land in ``self.e_data`` / ``self.e_smooth``"""
        from . import hip_renderer

        v = self._views
        if self._direct is not None:
            ds, r, grads, out = self._direct
            ds.set_views(**v)  # (no copies: the tensors are used as they are; another render of the scene may have rebound them)
            ds.set_texture(self.texture)
            image, _z, _g = r.render_fit(ds, self._obs, self.scene.sigma, grads=grads, out=out, clear_grads=True, loss_out=self.e_data, weights=self.weights)
            texture_b = grads["texture_b"]
            if self.texture_basis is None or self.smoothness > 0:
                hip_renderer.texture_smoothness(self.texture, texture_b, self.smoothness, self.e_smooth, scratch=self._scratch)
            return texture_b, image
        leaf = self.texture.detach().requires_grad_(True)
        extra = {} if self.weights is None else {"weights": self.weights}
        loss, image = self.scene._rasterize_l2(self.camera, v["ij"], v["depths"], v["colors"], v["shade"], True, True, self._obs, texture=leaf, **extra)
        (texture_b,) = torch.autograd.grad(loss, leaf)
        texture_b = texture_b.to(self.texture.dtype).contiguous()
        self.e_data.copy_(loss.detach().reshape(1))
        self.e_smooth.copy_(texture_smoothness_torch(self.texture, texture_b, self.smoothness).reshape(1))
        return texture_b, image.detach()

    def energy(self):
        """-> data energy + smoothness energy of the current texture (a device tensor of one element); nothing is updated"""
        assert self._views is not None, "call set_images first"
        if self.texture_basis is not None:
            self._texture_from_coefficients()
        self._gradient()
        energy = self.e_data + self.e_smooth
        return energy if self.texture_basis is None else energy + self._prior.energy(self.coefficients)

    def step_device(self):
        """One iteration on the device -> (energy BEFORE the update [1], image [n,H,W,C]).  ``self.texture`` and the momentum speed are updated in place,
        and the returned tensors are the same storage every step (clone what is to be kept); :meth:`step` converts at once."""
        from . import hip_renderer

        assert self._views is not None, "call set_images first"
        if self.texture_basis is not None:
            return self._step_basis()
        texture_b, image = self._gradient()
        speed = self.momentum.speed["texture"]
        update = hip_renderer.texture_step if self._direct is not None else texture_step_torch
        update(self.texture, speed, texture_b, self.step_factor_texture, self.step_max, self.inertia, self.damping, self.clamp)
        torch.add(self.e_data, self.e_smooth, out=self._energy)
        self.iter += 1
        return self._energy, image

    def _texture_from_coefficients(self):
        """``self.texture = mean + coefficients . basis`` in place, in the pixel dtype (one kernel on the device)"""
        B = self.texture_basis
        B.run(self.coefficients[None], out=self.texture.view(1, B.N))

    def _step_basis(self):
        """the iteration of a fit with ``texture_basis``: the same storage every step, no autograd graph on the device"""
        B, c, c_b = self.texture_basis, self.coefficients, self.coefficients_b
        self._texture_from_coefficients()
        texture_b, image = self._gradient()
        torch.mul(c, self._prior_scale, out=c_b)  # the prior's gradient 2 coefficient_regu c / sigmas^2; the data + smoothness gradient is added to it
        if self.coefficient_regu:
            torch.mul(c, c_b, out=self._prior_terms)
            torch.sum(self._prior_terms, dim=0, keepdim=True, out=self.e_prior)
            self.e_prior.mul_(0.5)
        if self._direct is not None:
            B.run_b(texture_b.view(1, B.N), out=c_b[None], accumulate=True, scratch=self._basis_scratch)
        else:
            c_b += B.run_b(texture_b.reshape(1, B.N))[0]
        self.momentum.update_in_place([("coefficients", c, c_b, None, self.step_factor_coefficients, self.step_max, 0)])
        torch.add(self.e_data, self.e_smooth, out=self._energy)
        self._energy += self.e_prior
        self.iter += 1
        return self._energy, image

    step = _step_all_views


# ---- camera calibration -----------------------------------------------------------------------------------------------------------------


class CameraFitterMultiFrame:
    """Fit the CAMERAS of ``n`` photographs of a known mesh: the world -> camera transform of every view (a quaternion (x, y, z, w) and a translation) and
    the focal lengths (fx, fy), the principal point (cx, cy) and OpenCV's distortion (k1, k2, p1, p2, k3) -- one physical camera shared by the views
    (``shared_intrinsics``, the default) or one per view.  The mesh is given as it is in the world: ``vertices``, ``faces`` and either per-vertex
    ``colors`` [V,C] or ``uv`` / ``faces_uv`` / ``texture``, plus a directional and an ambient light.  The energy is
    ``sum(weights * (image - photograph)**2)`` over all views.

    ``update`` chooses what moves -- any of "extrinsic", "focal", "center", "distortion"; what is not listed keeps its initial value to the bit.  That is
    how the gauge is fixed: a near-planar object cannot tell the focal length from its distance, a small one cannot tell the principal point from a
    rotation.  The update is the momentum rule of the other fitters with one ``step_factor_*`` / ``step_max_*`` per group (class attributes);
    quaternions are renormalised per view.  The factors are those of 4 views of 128 x 128; the gradients of the summed squared residual grow with the
    number of views and of pixels, so every factor is multiplied by ``step_scale`` -- None: ``min(1, 4 * 128**2 / (n * H * W))``, set in
    :meth:`set_images` -- while the clamps stay what they are.

    ``sigmas`` (None: no prior, every path as it is without the keyword): {parameter name: standard deviation(s)} for any of "quaternions",
    "translations", "focal", "center", "distortion" -- a number or an array that broadcasts to the parameter.  The energy gains
    ``sum(((parameter - its initial value) / sigma)**2)`` for each, which holds a weakly observed parameter near its prior calibration.

    The vertices, their luminosity and colours do not depend on the cameras: they are computed ONCE, in :meth:`set_images`.  An iteration on float64
    ROCm tensors is then a fixed kernel sequence over persistent buffers -- ``deodr_hip_camera_assemble``, ``deodr_hip_project_points``, silhouette
    flags, the rasterizer's one-call fit step, ``deodr_hip_camera_project_b`` (the 23 sums per view, deterministic), ``deodr_hip_camera_assemble_b``, one
    ``deodr_hip_momentum_update`` of all groups -- no autograd graph, no tensor rebound, so ``GraphedStep(fitter)`` replays it as it is.  On CPU
    tensors, or with ``direct = False``, the same iteration runs as autograd through ``DeviceCamera.from_pose`` and ``Scene3DDevice.render_l2``.

    ``pyramid_levels`` / ``pyramid_weights``: the multi-scale data term, as on :class:`MeshRGBFitterWithPose` (0: off, every path as it is without the
    keyword); with it the iteration is the autograd one, through ``Scene3DDevice.render_pyramid_l2``.  ``ssim_weight`` / ``ssim_data_range``: the
    structural data term, as on :class:`MeshRGBFitterWithPose` (0: off; ``self.ssim_mix`` the device tensor of the mix); the autograd iteration
    through ``Scene3DDevice.render_ssim_l2``; not together with ``pyramid_levels``."""

    direct = True
    GROUPS = ("extrinsic", "focal", "center", "distortion")
    # tuned on 2 - 4 views of 64 x 64 to 128 x 128 (tests/test_camera_fit_host.py, tests/test_camera_gpu.py); multiplied by ``step_scale`` (above)
    PARAMETERS = ("quaternions", "translations", "focal", "center", "distortion")
    step_factor_quaternion, step_factor_translation, step_factor_focal, step_factor_center, step_factor_distortion = 5e-6, 3e-5, 0.15, 0.005, 1e-4
    step_max_quaternion, step_max_translation, step_max_focal, step_max_center, step_max_distortion = 0.005, 0.02, 0.5, 1.0, 0.005

    def __init__(self, vertices, faces, quaternions_init, translations_init, focal_init, center_init, distortion_init=None, colors=None, uv=None,
                 faces_uv=None, texture=None, light_directional=None, light_ambient=1.0, update=GROUPS, shared_intrinsics=True, sigmas=None, sigma=1.0,
                 inertia=0.9, damping=0.05, step_scale=None, clockwise=False, device="cuda", pixel_dtype=torch.float64, pyramid_levels=0,
                 pyramid_weights=None, ssim_weight=0.0, ssim_data_range=1.0):  # fmt: skip
        _image_term_keywords(self, pyramid_levels, pyramid_weights, ssim_weight, ssim_data_range, torch.device(device))
        unknown = [g for g in update if g not in self.GROUPS]
        if unknown:
            raise ValueError(f"CameraFitterMultiFrame: update may list {self.GROUPS}, not {unknown}")
        if (colors is None) == (uv is None):
            raise ValueError("CameraFitterMultiFrame: give either per-vertex colors [V,C] or uv / faces_uv / texture")
        self.device, self.pixel_dtype = torch.device(device), pixel_dtype
        self.update, self.shared_intrinsics, self.inertia, self.damping = tuple(update), bool(shared_intrinsics), inertia, damping
        t = lambda a: torch.as_tensor(np.array(a, dtype=np.float64), device=self.device).contiguous()
        self.quaternions_init, self.translations_init = t(np.atleast_2d(quaternions_init)), t(np.atleast_2d(translations_init))
        n = self.n_views = int(self.quaternions_init.shape[0])
        if tuple(self.quaternions_init.shape) != (n, 4) or tuple(self.translations_init.shape) != (n, 3):
            raise ValueError("CameraFitterMultiFrame: quaternions_init must be [n,4] = (x, y, z, w) and translations_init [n,3]")
        if distortion_init is None and "distortion" in self.update:
            distortion_init = np.zeros(5)
        per_view = lambda a, width: a if self.shared_intrinsics else np.broadcast_to(np.asarray(a, dtype=np.float64), (n, width))
        self.focal_init, self.center_init = t(per_view(np.broadcast_to(focal_init, (2,)) if np.ndim(focal_init) == 0 else focal_init, 2)), t(per_view(center_init, 2))
        self.distortion_init = None if distortion_init is None else t(per_view(distortion_init, 5))
        width = lambda k: (k,) if self.shared_intrinsics else (n, k)
        for name, a, shape in (("focal_init", self.focal_init, width(2)), ("center_init", self.center_init, width(2)), ("distortion_init", self.distortion_init, width(5))):
            if a is not None and tuple(a.shape) != shape:
                raise ValueError(f"CameraFitterMultiFrame: {name} must have shape {list(shape)}, not {list(a.shape)}")
        v0 = np.asarray(vertices, dtype=np.float64)
        if uv is None:
            self.mesh = DeviceMesh(np.asarray(faces), v0, clockwise=clockwise, colors=np.asarray(colors, dtype=np.float64), device=self.device)
        else:
            tex = torch.as_tensor(np.asarray(texture, dtype=np.float64), device=self.device).to(pixel_dtype).contiguous()
            self.mesh = DeviceMesh(np.asarray(faces), v0, clockwise=clockwise, uv=uv, faces_uv=faces_uv, texture=None, device=self.device)
            self.mesh.texture = tex  # (in the pixel dtype, as the rasterizer reads it)
        self.scene = Scene3DDevice(sigma=sigma, pixel_dtype=pixel_dtype)
        self.scene.set_mesh(self.mesh)
        self.scene.set_light(light_directional, light_ambient)
        self.weights = self._views = self._direct = None
        self._step_scale_given, self.step_scale = step_scale, 1.0 if step_scale is None else float(step_scale)
        self._inv_sigma2 = {}  # parameter name -> 1 / sigma^2 of its prior, of the parameter's shape
        for name, sig in (sigmas or {}).items():
            init = getattr(self, name + "_init", None) if name in self.PARAMETERS else None
            if init is None:
                raise ValueError(f"CameraFitterMultiFrame: sigmas may name {self.PARAMETERS} (distortion only when the camera has one), not {name!r}")
            sig = np.asarray(sig, dtype=np.float64)
            if np.any(sig <= 0):
                raise ValueError(f"CameraFitterMultiFrame: sigmas[{name!r}] must be positive")
            self._inv_sigma2[name] = t(np.broadcast_to(1.0 / sig**2, tuple(init.shape)))
        self.reset()

    def reset(self):
        self.quaternions, self.translations = self.quaternions_init.clone(), self.translations_init.clone()
        self.focal, self.center = self.focal_init.clone(), self.center_init.clone()
        self.distortion = None if self.distortion_init is None else self.distortion_init.clone()
        self.momentum = _Momentum(self.inertia, self.damping)
        self.iter = 0

    def set_background_color(self, background_color):
        self.scene.set_background_color(background_color)

    def _parameters(self):
        """[(name, group, tensor, step factor, step_max, normalize_rows)] of the parameters that exist"""
        rows = [("quaternions", "extrinsic", self.quaternions, self.step_factor_quaternion, self.step_max_quaternion, 4),
                ("translations", "extrinsic", self.translations, self.step_factor_translation, self.step_max_translation, 0),
                ("focal", "focal", self.focal, self.step_factor_focal, self.step_max_focal, 0),
                ("center", "center", self.center, self.step_factor_center, self.step_max_center, 0),
                ("distortion", "distortion", self.distortion, self.step_factor_distortion, self.step_max_distortion, 0)]  # fmt: skip
        return [(name, group, x, self.step_scale * factor, step_max, rows_) for name, group, x, factor, step_max, rows_ in rows if x is not None]

    def _prior(self):
        """-> (sum(((parameter - initial value) / sigma)**2) over the parameters with a prior [1], {parameter name: its gradient}); (None, {}) without"""
        energy, grads = None, {}
        for name, inv in self._inv_sigma2.items():
            delta = getattr(self, name) - getattr(self, name + "_init")
            grads[name] = _prior_gradient(1.0, inv, delta)
            e = (inv * delta * delta).sum().reshape(1)  # (not _GaussianPrior.energy: (inv delta) delta rounds differently from inv delta**2)
            energy = e if energy is None else energy + e
        return energy, grads

    def set_images(self, images, weights=None):
        """``images`` [n,H,W,C]: one photograph per view.  ``weights`` [H,W] or [n,H,W], ``>= 0`` (or None): per-pixel weights of the squared residual,
        handed to the fit step (a mask on what is not the object, a view to leave out)."""
        from . import fronthalf, hip_renderer

        imgs = np.stack([np.asarray(im, dtype=np.float64) for im in images])
        n, height, width, nb_colors = imgs.shape
        if n != self.n_views:
            raise ValueError(f"{n} images for {self.n_views} cameras")
        dev, mesh = self.device, self.mesh
        self.height, self.width = height, width
        self.mesh_image = torch.as_tensor(imgs, device=dev)
        self._obs = self.mesh_image.to(self.pixel_dtype).contiguous()
        self.weights = _pixel_weights(weights, (n, height, width), dev, self.pixel_dtype)
        self.e_data, self._energy =torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
        if self._step_scale_given is None:
            self.step_scale = min(1.0, 4 * 128**2 / (n * height * width))
        self._direct = None
        topo = mesh.topology
        params = [p[2] for p in self._parameters()]
        if (self.direct and not _neighbourhood_term(self) and fronthalf.usable(mesh.vertices, *params) and topo._edge_faces is not None
                and n <= hip_renderer.CAMERA_MAX_VIEWS):  # fmt: skip
            self._direct = self._direct_buffers(n, height, width, nb_colors)
        self.iter = 0

    def _direct_buffers(self, n, height, width, nb_colors):
        """everything the fixed kernel sequence reads and writes, allocated once; the shading, which no camera parameter moves, computed once"""
        from types import SimpleNamespace

        from . import hip_renderer

        dev, mesh, V = self.device, self.mesh, self.mesh.nb_vertices
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        d = SimpleNamespace()
        d.points = mesh.vertices.detach()[None].expand(n, -1, -1).contiguous()  # the same world vertices for every view
        d.extrinsic, d.intrinsic = z(n, 3, 4), z(n, 3, 3)
        d.dist = None if self.distortion is None else z(n, 5)
        d.ij, d.depths = z(n, V, 2), z(n, V)
        d.flags = torch.zeros((n, mesh.nb_faces, 3), dtype=torch.uint8, device=dev)
        with torch.no_grad():
            lum = self.scene.vertices_luminosity(mesh.vertices)
            lum = lum[None].expand(n, -1).contiguous()
            textured = mesh.uv is not None
            if textured:
                colors, shade = z(n, V, nb_colors), lum
            else:
                colors, shade = (mesh.vertices_colors[None].expand(n, -1, -1) * lum[..., None]).contiguous(), z(n, V)
        if int(colors.shape[-1]) != nb_colors:
            raise ValueError(f"the images have {nb_colors} channels, the mesh {int(colors.shape[-1])}")
        d.views = dict(ij=d.ij, depths=d.depths, colors=colors, shade=shade, edgeflags=d.flags)
        d.ds, d.rasterizer, d.out = _raster_state(self.scene, (n, height, width, nb_colors), textured, d.views)
        d.grads = d.ds.zero_grads()
        d.extrinsic_b, d.intrinsic_b = z(n, 3, 4), z(n, 3, 3)
        d.dist_b = None if d.dist is None else z(n, 5)
        d.grad = {"quaternions": z(n, 4), "translations": z(n, 3), "focal": torch.zeros_like(self.focal), "center": torch.zeros_like(self.center),
                  "distortion": None if self.distortion is None else torch.zeros_like(self.distortion)}  # fmt: skip
        d.scratch = hip_renderer.camera_scratch(V, n, dev)  # (its own: a captured step replays on the addresses it was captured with)
        return d

    def _gradients_direct(self):
        """the fixed kernel sequence up to the gradients -> ({parameter name: gradient}, image); the data energy lands in ``self.e_data``"""
        from . import fronthalf, hip_renderer

        d, topo = self._direct, self.mesh.topology
        hip_renderer.camera_assemble(self.quaternions, self.translations, self.focal, self.center, self.distortion, shared=self.shared_intrinsics,
                                     out=(d.extrinsic, d.intrinsic, d.dist))  # fmt: skip
        fronthalf.project_points(d.points, d.extrinsic, d.intrinsic, d.dist, d.ij, d.depths)
        if self.scene.sigma > 0:
            fronthalf.silhouette_flags(d.ij, topo._faces_u32, topo._edge_faces, topo.clockwise, out=d.flags)
        d.ds.set_views(**d.views)  # (no copies: the tensors are used as they are; another render of the scene may have rebound them)
        if self.mesh.uv is not None:
            d.ds.set_texture(self.mesh.texture)
        image, _z, _g = d.rasterizer.render_fit(d.ds, self._obs, self.scene.sigma, grads=d.grads, out=d.out, clear_grads=True, loss_out=self.e_data,
                                                weights=self.weights)  # fmt: skip
        hip_renderer.camera_project_b(d.points, d.extrinsic, d.intrinsic, d.dist, d.grads["ij_b"], None, extrinsic_b=d.extrinsic_b, intrinsic_b=d.intrinsic_b,
                                      distortion_b=d.dist_b, scratch=d.scratch, want_points_b=False)  # fmt: skip
        g = d.grad
        hip_renderer.camera_assemble_b(self.quaternions, d.extrinsic_b, d.intrinsic_b, d.dist_b, shared=self.shared_intrinsics,
                                       out=(g["quaternions"], g["translations"], g["focal"], g["center"], g["distortion"]))  # fmt: skip
        return g, image

    def _gradients_autograd(self):
        """the same iteration under autograd -> ({parameter name: gradient}, image); the data energy lands in ``self.e_data``"""
        rows = self._parameters()
        leaves = {name: x.detach().requires_grad_(group in self.update) for name, group, x, *_ in rows}
        camera = DeviceCamera.from_pose(leaves["quaternions"], leaves["translations"], leaves["focal"], leaves["center"], self.height, self.width,
                                        leaves.get("distortion"), shared_intrinsics=self.shared_intrinsics, device=self.device)  # fmt: skip
        loss, image = _render_data_term(self, camera, self._obs, self.weights)
        wanted = [name for name, group, *_ in rows if group in self.update]
        grads = dict(zip(wanted, torch.autograd.grad(loss, [leaves[k] for k in wanted]))) if wanted else {}
        self.e_data.copy_(loss.detach().reshape(1))
        return grads, image.detach()

    def _data_gradients(self):
        return self._gradients_direct() if self._direct is not None else self._gradients_autograd()

    def _total_energy(self, e_prior):
        if e_prior is None:
            return self.e_data
        torch.add(self.e_data, e_prior, out=self._energy)
        return self._energy

    def gradients(self):
        """-> ({parameter name: d energy / d parameter}, image [n,H,W,C]) of the current parameters, prior included; nothing is updated"""
        assert self._obs is not None, "call set_images first"
        grads, image = self._data_gradients()
        _e, g_prior = self._prior()
        return {k: (g + g_prior[k] if k in g_prior else g) for k, g in grads.items()}, image

    def energy(self):
        """-> the energy of the current cameras, data term + prior (a device tensor of one element); nothing is updated"""
        self._data_gradients()
        return self._total_energy(self._prior()[0])

    def cameras(self):
        """the cameras of the current parameters, as a :class:`DeviceCamera` of ``n`` views (detached)"""
        with torch.no_grad():
            return DeviceCamera.from_pose(self.quaternions, self.translations, self.focal, self.center, self.height, self.width, self.distortion,
                                          shared_intrinsics=self.shared_intrinsics, device=self.device)  # fmt: skip

    def step_device(self):
        """One iteration on the device -> (energy BEFORE the update [1], image [n,H,W,C]).  On the direct path the parameters and the momentum speeds are
        updated in place and the returned tensors are the same storage every step (clone what is to be kept); :meth:`step` converts at once."""
        grads, image = self._data_gradients()
        e_prior, g_prior = self._prior()  # (of the parameters the gradients were taken at)
        entries = [(name, x, grads[name], g_prior.get(name), factor, step_max, normalize_rows)
                   for name, group, x, factor, step_max, normalize_rows in self._parameters() if group in self.update]  # fmt: skip
        if entries and self._direct is not None:
            self.momentum.update_in_place(entries)
        elif entries:
            for (name, *_), value in zip(entries, self.momentum.update_all(entries)):
                setattr(self, name, value)
        self.iter += 1
        return self._total_energy(e_prior), image

    step = _step_all_views
