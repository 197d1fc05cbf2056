"""Fused kernels for the O(V) algebra of a fit iteration (``deodr_amd/csrc/dr_fronthalf.h``, C ABI in ``include/deodr_hip.h``):
rigid transform, camera projection (+ distortion), silhouette flags and the momentum update, each one launch (two with its adjoint)
instead of the 10 - 50 torch kernels the same formulas take (``deodr_amd/scene3d.py`` keeps those formulas: they are what runs on
tensors that are not float64 ROCm tensors -- the CPU suite -- and what the kernels are tested against)."""

import ctypes as C

import torch

from . import hip_renderer as hr
from .hip_renderer import _dtype_tag, _launch, _ptr, lib


def usable(*tensors):
    """the kernels take contiguous float64 tensors on a ROCm device"""
    return all(t is not None and t.is_cuda and t.dtype == torch.float64 for t in tensors)


class RigidTransformFunc(torch.autograd.Function):
    """(vertices [V,3], unit quaternions [n,4] = (x, y, z, w), translations [n,3]) -> [n,V,3]: qrot(q, v) + t (deodr/tools.py:8-35)"""

    @staticmethod
    def forward(ctx, vertices, quaternions, translations):
        v, q, t = vertices.contiguous(), quaternions.contiguous(), translations.contiguous()
        n, V = q.shape[0], v.shape[0]
        out = torch.empty((n, V, 3), dtype=torch.float64, device=v.device)
        _launch(lib().deodr_hip_rigid_transform, v.device, _ptr(v), _ptr(q), _ptr(t), _ptr(out), V, n)
        ctx.save_for_backward(v, q)
        return out

    @staticmethod
    def backward(ctx, out_b):
        v, q = ctx.saved_tensors
        n, V = q.shape[0], v.shape[0]
        out_b = out_b.contiguous()
        v_b = torch.empty_like(v)
        pose_b = torch.empty(7 * n, dtype=torch.float64, device=v.device)
        _launch(lib().deodr_hip_rigid_transform_b, v.device, _ptr(v), _ptr(q), _ptr(out_b), _ptr(v_b), _ptr(pose_b), V, n)
        return v_b, pose_b[: 4 * n].view(n, 4), pose_b[4 * n :].view(n, 3)


def _check_cameras(n, extrinsic, intrinsic, distortion):
    """The kernels read `extrinsic[12 b + i]`, `intrinsic[9 b + i]`, `distortion[5 b + i]` of view b < n: one contiguous matrix PER VIEW
    (a camera shared by the views must have been expanded, as DeviceCamera does) -- anything else would be read out of bounds."""
    for name, a, shape in (("extrinsic", extrinsic, (3, 4)), ("intrinsic", intrinsic, (3, 3)), ("distortion", distortion, (5,))):
        if a is None:
            continue
        if tuple(a.shape) != (n,) + shape or not a.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous [{n}, {', '.join(map(str, shape))}] tensor (one per view), got {tuple(a.shape)}")


class ProjectPointsFunc(torch.autograd.Function):
    """(points [n,V,3]; extrinsic [n,3,4], intrinsic [n,3,3], distortion [n,5] | None: constants) -> (ij [n,V,2], depths [n,V]);
    Camera.project_points / project_points_backward (deodr/differentiable_renderer.py:341-438)"""

    @staticmethod
    def forward(ctx, points, extrinsic, intrinsic, distortion):
        pts = points.contiguous()
        n, V = pts.shape[0], pts.shape[1]
        _check_cameras(n, extrinsic, intrinsic, distortion)
        ij = torch.empty((n, V, 2), dtype=torch.float64, device=pts.device)
        depths = torch.empty((n, V), dtype=torch.float64, device=pts.device)
        project_points(pts, extrinsic, intrinsic, distortion, ij, depths)
        ctx.save_for_backward(pts, extrinsic, intrinsic)
        ctx.distortion = distortion
        return ij, depths

    @staticmethod
    def backward(ctx, ij_b, depths_b):
        pts, extrinsic, intrinsic = ctx.saved_tensors
        n, V = pts.shape[0], pts.shape[1]
        ij_b = ij_b.contiguous()
        depths_b = None if depths_b is None else depths_b.contiguous()
        if any(ctx.needs_input_grad[1:]):  # a camera tensor is being fitted: the full adjoint, every requested gradient from one launch
            if V > hr.CAMERA_MAX_VERTICES:
                raise RuntimeError(f"ProjectPointsFunc: the gradient of a camera is available for at most 2^24 vertices per view (include/deodr_hip_camera.h), "
                                   f"not {V}; detach extrinsic, intrinsic and distortion, or project the points in pieces")  # fmt: skip
            want = ctx.needs_input_grad[0]
            pts_b = torch.empty_like(pts) if want else None
            e_b, k_b = torch.empty_like(extrinsic), torch.empty_like(intrinsic)
            d_b = None if ctx.distortion is None else torch.empty_like(ctx.distortion)
            step = hr.CAMERA_MAX_VIEWS  # (the kernel takes at most 64 views per launch; the views are independent: more go in slices)
            for b in range(0, n, step):
                cut = lambda t: None if t is None else t[b : b + step]
                hr.camera_project_b(cut(pts), cut(extrinsic), cut(intrinsic), cut(ctx.distortion), cut(ij_b), cut(depths_b), points_b=cut(pts_b),
                                    extrinsic_b=cut(e_b), intrinsic_b=cut(k_b), distortion_b=cut(d_b), want_points_b=False,
                                    scratch=_camera_scratch(pts.device, V, min(step, n - b)))  # fmt: skip
            return pts_b, e_b if ctx.needs_input_grad[1] else None, k_b if ctx.needs_input_grad[2] else None, d_b if ctx.needs_input_grad[3] else None
        pts_b = torch.empty_like(pts)
        _launch(lib().deodr_hip_project_points_b, pts.device, _ptr(pts), _ptr(extrinsic), _ptr(intrinsic), _ptr(ctx.distortion), _ptr(ij_b),
                _ptr(depths_b), _ptr(pts_b), V, n)  # fmt: skip
        return pts_b, None, None, None


_camera_scratches = {}  # (device, V, n) -> the zero-filled scratch of camera_project_b for the autograd wrapper (kernels of one stream run in order)


def _camera_scratch(device, V, n):
    key = (device, int(V), int(n))
    if key not in _camera_scratches:
        _camera_scratches[key] = hr.camera_scratch(V, n, device)
    return _camera_scratches[key]


def camera_assemble_torch(quaternions, translations, focal, center, distortion, shared):
    """the formulas of ``deodr_hip_camera_assemble`` as torch ops (differentiable by autograd): what runs on tensors the kernels do not take"""
    n = quaternions.shape[0]
    q = quaternions / quaternions.norm(dim=1, keepdim=True)
    x, y, z, w = q.unbind(1)
    rot = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                       2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                       2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), dim=1).reshape(n, 3, 3)  # fmt: skip
    extrinsic = torch.cat((rot, translations[:, :, None]), dim=2)
    f, c = (focal[None].expand(n, 2), center[None].expand(n, 2)) if shared else (focal, center)
    zero, one = torch.zeros_like(f[:, 0]), torch.ones_like(f[:, 0])
    intrinsic = torch.stack((f[:, 0], zero, c[:, 0], zero, f[:, 1], c[:, 1], zero, zero, one), dim=1).reshape(n, 3, 3)
    if distortion is None:
        return extrinsic, intrinsic, None
    return extrinsic, intrinsic, (distortion[None].expand(n, 5) if shared else distortion).contiguous()


class CameraAssembleFunc(torch.autograd.Function):
    """(quaternions [n,4] raw, translations [n,3], focal, center [2] | [n,2], distortion [5] | [n,5] | None; shared) -> (extrinsic [n,3,4],
    intrinsic [n,3,3], distortion [n,5] | None): ``deodr_hip_camera_assemble`` and its adjoint, one launch each"""

    @staticmethod
    def forward(ctx, quaternions, translations, focal, center, distortion, shared):
        q, t, f, c = quaternions.contiguous(), translations.contiguous(), focal.contiguous(), center.contiguous()
        d = None if distortion is None else distortion.contiguous()
        e, k, dist = hr.camera_assemble(q, t, f, c, d, shared=shared)
        ctx.save_for_backward(q)
        ctx.shared, ctx.distorted = bool(shared), d is not None
        if dist is None:
            dist = q.new_zeros(0)  # (an autograd function returns tensors: the caller drops this one)
            ctx.mark_non_differentiable(dist)
        return e, k, dist

    @staticmethod
    def backward(ctx, e_b, k_b, d_b):
        (q,) = ctx.saved_tensors
        n = q.shape[0]
        e_b = q.new_zeros((n, 3, 4)) if e_b is None else e_b.contiguous()
        k_b = q.new_zeros((n, 3, 3)) if k_b is None else k_b.contiguous()
        if ctx.distorted:
            d_b = q.new_zeros((n, 5)) if d_b is None else d_b.contiguous()
        else:
            d_b = None
        q_b, t_b, f_b, c_b, din_b = hr.camera_assemble_b(q, e_b, k_b, d_b, shared=ctx.shared)
        return q_b, t_b, f_b, c_b, din_b, None


def camera_assemble(quaternions, translations, focal, center, distortion=None, shared=True):
    """-> (extrinsic, intrinsic, distortion | None) of the views, differentiable in all five inputs: the kernels on float64 ROCm tensors, the same
    formulas as torch ops otherwise (CPU tensors; more than the 64 views the kernels take per launch)"""
    tensors = [quaternions, translations, focal, center] + ([] if distortion is None else [distortion])
    if usable(*tensors) and quaternions.shape[0] <= hr.CAMERA_MAX_VIEWS:
        e, k, d = CameraAssembleFunc.apply(quaternions, translations, focal, center, distortion, bool(shared))
        return e, k, (None if distortion is None else d)
    return camera_assemble_torch(quaternions, translations, focal, center, distortion, shared)


def silhouette_flags(ij, faces_u32, edge_faces_u32, clockwise, out=None):
    """ij [n,V,2] -> uint8 [n,T,3] (TriMeshAdjacencies.edge_on_silhouette, deodr/triangulated_mesh.py:153-166); no gradient"""
    ij = ij.detach().contiguous()
    n, V, T = ij.shape[0], ij.shape[1], faces_u32.shape[0]
    flags = torch.empty((n, T, 3), dtype=torch.uint8, device=ij.device) if out is None else out
    _launch(lib().deodr_hip_silhouette_flags, ij.device, _ptr(ij), _ptr(faces_u32), _ptr(edge_faces_u32), _ptr(flags), T, V, n, int(bool(clockwise)))
    return flags


def project_points(points, extrinsic, intrinsic, distortion, ij, depths):
    """points [n,V,3] through the cameras of the views (one matrix per view, :func:`_check_cameras`; distortion [n,5] | None) into ``ij`` [n,V,2] and
    ``depths`` [n,V], both written in place: the plain launch, no checks, no gradient (:class:`ProjectPointsFunc` is the differentiable one)"""
    n, V = points.shape[0], points.shape[1]
    _launch(lib().deodr_hip_project_points, points.device, _ptr(points), _ptr(extrinsic), _ptr(intrinsic), _ptr(distortion), _ptr(ij), _ptr(depths), V, n)


def momentum_update(entries, inertia, damping, scratch=None, energy=None, data_energy=None, data_weight=1.0):
    """entries: [(x, speed, grad, grad2 | None, factor, step_max | None, normalize_rows[, grad_scale, grad_mean | None, mean_out | None])];
    x and speed are updated IN PLACE: s = (1 - damping)(inertia s + (1 - inertia) clamp(-factor (grad_scale (grad - grad_mean) + grad2))),
    x += s (deodr/mesh_fitter.py:153-190); mean_out [3] receives the column mean of the updated [.,3] tensor (needs ``scratch``);
    with ``energy`` [2] and ``data_energy`` [1]: energy[1] = data_weight * data_energy[0] + energy[0] on the way"""
    k = len(entries)
    assert 0 < k <= 8
    entries = [tuple(e) + (1.0, None, None)[len(e) - 7 :] for e in entries]
    ptrs = lambda j: (C.c_void_p * k)(*[None if e[j] is None else e[j].data_ptr() for e in entries])
    factor = (C.c_double * k)(*[float(e[4]) for e in entries])
    step_max = (C.c_double * k)(*[0.0 if e[5] is None else float(e[5]) for e in entries])
    count = (C.c_int * k)(*[int(e[0].numel()) for e in entries])
    rows = (C.c_int * k)(*[int(e[6]) for e in entries])
    scale = (C.c_double * k)(*[float(e[7]) for e in entries])
    for e in entries:
        assert e[0].is_contiguous() and e[1].is_contiguous() and e[2].is_contiguous() and (e[3] is None or e[3].is_contiguous())
    _launch(lib().deodr_hip_momentum_update, entries[0][0].device, k, ptrs(0), ptrs(1), ptrs(2), ptrs(3), factor, step_max, count, rows, float(inertia),
            float(damping), scale, ptrs(8), ptrs(9), _ptr(energy), _ptr(data_energy), float(data_weight), _ptr(scratch),
            0 if scratch is None else scratch.numel())  # fmt: skip


# ---- one fit iteration without an autograd graph (deodr_amd/csrc/dr_fititer.h) ----------------------------------------------------


def fit_scratch(V, n, device):
    """zero-filled scratch of the kernels below (their counter words stay zero between launches)"""
    return torch.zeros(int(lib().deodr_hip_fit_scratch_bytes(int(V), int(n))), dtype=torch.uint8, device=device)


def _topology_scratch(topology, n):
    """one scratch per (topology, number of views), for the autograd wrappers (the kernels of one stream run one after the other)"""
    cache = topology.__dict__.setdefault("_fit_scratch", {})
    if n not in cache:
        cache[n] = fit_scratch(topology.nb_vertices, n, topology.device)
    return cache[n]


def fit_pose_project(vertices, vertices_mean, quaternions, translations, camera, posed, ij, depths, depth_colors=None, depth_scale=1.0):
    """centre ``vertices`` [V,3] in place (when a mean [3] is given), pose them with every view's quaternion (normalised inside) and
    translation, project them with every view's camera -> posed [n,V,3], ij [n,V,2], depths [n,V] (all written)"""
    n, V = posed.shape[0], posed.shape[1]
    _check_cameras(n, camera.extrinsic, camera.intrinsic, camera.distortion)
    _launch(lib().deodr_hip_fit_pose_project, posed.device, _ptr(vertices), _ptr(vertices_mean), _ptr(quaternions), _ptr(translations),
            _ptr(camera.extrinsic), _ptr(camera.intrinsic), _ptr(camera.distortion), _ptr(posed), _ptr(ij), _ptr(depths), _ptr(depth_colors),
            float(depth_scale), V, n)  # fmt: skip


def fit_pose_project_b(vertices, quaternions, posed, camera, posed_b, ij_b, depths_b, vertices_b, out, scratch, depths_b_scale=1.0, colors_b=None,
                       colors_sum=None):
    """adjoint of :func:`fit_pose_project`: -> vertices_b [V,3]; out [3 + 7n] = mean of vertices_b over the vertices, quaternion adjoints
    [n,4] (raw quaternions), translation adjoints [n,3]; colors_sum [V,C] (optional) = colors_b [n,V,C] summed over the views"""
    n, V = posed.shape[0], posed.shape[1]
    _check_cameras(n, camera.extrinsic, camera.intrinsic, camera.distortion)
    _launch(lib().deodr_hip_fit_pose_project_b, posed.device, _ptr(vertices), _ptr(quaternions), _ptr(posed), _ptr(camera.extrinsic),
            _ptr(camera.intrinsic), _ptr(camera.distortion), _ptr(posed_b), _ptr(ij_b), _ptr(depths_b), float(depths_b_scale), _ptr(vertices_b),
            _ptr(out), _ptr(scratch), scratch.numel(), V, n, _ptr(colors_b), 0 if colors_b is None else int(colors_b.shape[-1]), _ptr(colors_sum))  # fmt: skip


def views_gradient_sum(posed, camera, ij_b, vertices_b, depths_b=None, depths_b_scale=1.0, colors_b=None, colors_sum=None, validate=True):
    """What the views of a multi-view fit share (mesh_fitter.py:518-527): vertices_b [V,3] (written) = the adjoint of every view's camera
    projection applied to ij_b [n,V,2] (and depths_b [n,V]), summed over the n views; colors_sum [V,C] (written, optional) = colors_b
    [n,V,C] summed over the views.  One wide launch -- the packed buffer a sharded fit all-reduces."""
    n, V = posed.shape[0], posed.shape[1]
    if validate:  # (validate=False: a caller that launches the same, already validated, tensors every step -- OverlappedViewsReduction)
        _validate_views_gradient_sum(posed, camera, ij_b, vertices_b, depths_b, colors_b, colors_sum)
    _launch(lib().deodr_hip_views_gradient_sum, posed.device, _ptr(posed), _ptr(camera.extrinsic), _ptr(camera.intrinsic), _ptr(camera.distortion),
            _ptr(ij_b), _ptr(depths_b), float(depths_b_scale), _ptr(vertices_b), V, n, _ptr(colors_b),
            0 if colors_b is None else int(colors_b.shape[-1]), _ptr(colors_sum))  # fmt: skip


def _validate_views_gradient_sum(posed, camera, ij_b, vertices_b, depths_b, colors_b, colors_sum):
    n, V = posed.shape[0], posed.shape[1]
    _check_cameras(n, camera.extrinsic, camera.intrinsic, camera.distortion)
    # the kernel reads every pointer as contiguous float64 of exactly these shapes: anything else (a float32 vertex_dtype, a strided
    # view) would be read out of bounds and go into the collective as garbage without an error
    expected = [("posed", posed, (n, V, 3)), ("ij_b", ij_b, (n, V, 2)), ("vertices_b", vertices_b, (V, 3))]
    if depths_b is not None:
        expected.append(("depths_b", depths_b, (n, V)))
    if colors_b is not None or colors_sum is not None:
        if colors_b is None or colors_sum is None:
            raise ValueError("views_gradient_sum: colors_b and colors_sum go together")
        expected += [("colors_b", colors_b, (n, V, int(colors_b.shape[-1]))), ("colors_sum", colors_sum, (V, int(colors_b.shape[-1])))]
    for name, t, shape in expected:
        if not usable(t) or not t.is_contiguous() or tuple(t.shape) != shape or t.device != posed.device:
            raise ValueError(f"views_gradient_sum: {name} must be a contiguous float64 ROCm tensor of shape {shape} on {posed.device}, got "
                             f"{tuple(t.shape)} {t.dtype} {t.device}{'' if t.is_contiguous() else ' (not contiguous)'}")


def vertex_shade(posed, topology, light, ambient, color=None, luminosity=None, colors=None):
    """luminosity [n,V] = max(0, -normal . light) + ambient and / or colors [n,V,C] = color [C] * luminosity (written)"""
    n, V = posed.shape[0], posed.shape[1]
    _launch(lib().deodr_hip_vertex_shade, posed.device, _ptr(posed), _ptr(topology._faces_u32), _ptr(topology._vf_offsets),
            _ptr(topology._vf_corners), _ptr(light), _ptr(ambient), _ptr(color), 0 if color is None else color.numel(), _ptr(luminosity),
            _ptr(colors), V, n, int(topology.clockwise))  # fmt: skip


def fit_front(topology, n, scratch, ij=None, flags=None, posed=None, light=None, ambient=None, color=None, luminosity=None, colors=None, vertices=None,
              vertices_ref=None, cregu=0.0, gradient=None, energy=None):
    """:func:`silhouette_flags` (``flags`` given), :func:`vertex_shade` (``luminosity`` or ``colors`` given) and :func:`rigid_energy`
    (``gradient`` given; energy[0] only) in ONE launch -- the three do not depend on one another.  Same results bit for bit."""
    off, cols, vals = topology._m_csr if gradient is not None else (None, None, None)
    _launch(lib().deodr_hip_fit_front, scratch.device, _ptr(ij), _ptr(topology._faces_u32), _ptr(topology._edge_faces), _ptr(flags), topology.nb_faces,
            _ptr(posed), _ptr(topology._vf_offsets), _ptr(topology._vf_corners), _ptr(light), _ptr(ambient), _ptr(color),
            0 if color is None else color.numel(), _ptr(luminosity), _ptr(colors), _ptr(vertices), _ptr(vertices_ref), _ptr(off), _ptr(cols),
            _ptr(vals), float(cregu), _ptr(gradient), _ptr(energy), _ptr(scratch), scratch.numel(), topology.nb_vertices, int(n),
            int(topology.clockwise))  # fmt: skip


def vertex_shade_b(posed, topology, light, ambient, color, luminosity_b, colors_b, posed_b, out, scratch):
    """adjoint of :func:`vertex_shade`: -> posed_b [n,V,3] (written), out [4 + C] = light_b, ambient_b, color_b"""
    n, V = posed.shape[0], posed.shape[1]
    _launch(lib().deodr_hip_vertex_shade_b, posed.device, _ptr(posed), _ptr(topology._faces_u32), _ptr(topology._vf_offsets),
            _ptr(topology._vf_corners), _ptr(light), _ptr(ambient), _ptr(color), 0 if color is None else color.numel(), _ptr(luminosity_b),
            _ptr(colors_b), _ptr(posed_b), _ptr(out), _ptr(scratch), scratch.numel(), V, n, int(topology.clockwise))  # fmt: skip


def rigid_energy(vertices, vertices_ref, topology, cregu, gradient, energy, scratch, data_energy=None, data_weight=1.0):
    """energy[0] = 0.5 c d^T (L^T L) d, gradient [V,3] = c (L^T L) d, d = vertices - vertices_ref (both written); with ``data_energy`` [1]
    also energy[1] = data_weight * data_energy[0] + energy[0]"""
    off, cols, vals = topology._m_csr
    _launch(lib().deodr_hip_rigid_energy, vertices.device, _ptr(vertices), _ptr(vertices_ref), _ptr(off), _ptr(cols), _ptr(vals), float(cregu),
            _ptr(gradient), _ptr(energy), _ptr(data_energy), float(data_weight), _ptr(scratch), scratch.numel(), vertices.shape[0])  # fmt: skip


def l2_loss(image, obs, out, scratch):
    """out[0] = sum (image - obs)^2, image and obs contiguous tensors of one pixel dtype (float32 / float64) and one shape"""
    assert image.dtype == obs.dtype and image.shape == obs.shape and image.is_contiguous() and obs.is_contiguous()
    _launch(lib().deodr_hip_l2_loss, image.device, _ptr(image), _ptr(obs), _dtype_tag(image), image.numel(), _ptr(out),
            _ptr(scratch), scratch.numel())  # fmt: skip


def depth_residual(image, obs, max_depth, depth, diff, image_b, loss, scratch):
    """the depth fitter's data term in one kernel: depth = clamp(image, 0, max_depth), diff = (depth - obs)^2 (both float64, written),
    image_b = d sum(diff) / d image in the pixel dtype, loss[0] = sum diff (deodr/mesh_fitter.py:108-123)"""
    assert obs.dtype == torch.float64 and depth.dtype == torch.float64 and diff.dtype == torch.float64 and image_b.dtype == image.dtype
    assert all(t.is_contiguous() and t.numel() == image.numel() for t in (image, obs, depth, diff, image_b))
    _launch(lib().deodr_hip_depth_residual, image.device, _ptr(image), _dtype_tag(image), _ptr(obs), float(max_depth),
            image.numel(), _ptr(depth), _ptr(diff), _ptr(image_b), _ptr(loss), _ptr(scratch), scratch.numel())  # fmt: skip


class VertexLuminosityFunc(torch.autograd.Function):
    """(posed [n,V,3], light [3], ambient []) -> luminosity [n,V]: vertex normals + max(0, -n.l) + ambient in one kernel, two for the adjoint
    (deodr/triangulated_mesh.py:113-151, deodr/differentiable_renderer.py:814-822)"""

    @staticmethod
    def forward(ctx, posed, light, ambient, topology):
        posed, light, ambient = posed.contiguous(), light.contiguous(), ambient.contiguous()
        lum = torch.empty(posed.shape[:2], dtype=torch.float64, device=posed.device)
        vertex_shade(posed, topology, light, ambient, luminosity=lum)
        ctx.save_for_backward(posed, light, ambient)
        ctx.topology = topology
        return lum

    @staticmethod
    def backward(ctx, lum_b):
        posed, light, ambient = ctx.saved_tensors
        posed_b = torch.empty_like(posed)
        out = torch.empty(4, dtype=torch.float64, device=posed.device)
        vertex_shade_b(posed, ctx.topology, light, ambient, None, lum_b.contiguous(), None, posed_b, out, _topology_scratch(ctx.topology, posed.shape[0]))
        return posed_b, out[:3], out[3].reshape(ambient.shape), None


class RigidEnergyFunc(torch.autograd.Function):
    """vertices [V,3] -> (energy, gradient [V,3]) of the Laplacian rigid energy (deodr/laplacian_rigid_energy.py:15-41) in one kernel;
    the energy is differentiable (its adjoint is the gradient the same launch produced)"""

    @staticmethod
    def forward(ctx, vertices, vertices_ref, topology, cregu):
        v = vertices.contiguous()
        grad, energy = torch.empty_like(v), torch.empty(1, dtype=torch.float64, device=v.device)
        rigid_energy(v, vertices_ref, topology, cregu, grad, energy, _topology_scratch(topology, 1))
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(grad)
        return energy[0], grad

    @staticmethod
    def backward(ctx, energy_b, _grad_b):
        (grad,) = ctx.saved_tensors
        return energy_b * grad, None, None, None


_sh_scratches = {}  # (device, stream) -> the zero-filled scratch of sh_shade_b for the autograd wrapper, grown to the largest shape asked for


def _sh_scratch(device, V, n, C):
    """one scratch per device and stream (the header: used by one stream at a time), kept at the largest size seen; a larger one than a call needs
    serves it (the layout is the call's, the counter words are zero between calls)"""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    need = int(lib().deodr_hip_sh_scratch_bytes(int(V), int(n), int(C)))
    if key not in _sh_scratches or _sh_scratches[key].numel() < need:
        _sh_scratches[key] = hr.sh_scratch(V, n, C, device)
    return _sh_scratches[key]


class SHShadeFunc(torch.autograd.Function):
    """(posed [n,V,3], sh [9] | [9,S], albedo None | [C] | [V,C]) -> luminosity [n,V] (no albedo) or colors [n,V,C]: spherical-harmonic lighting of
    the vertex normals times the albedo (``deodr_amd/lighting.py`` has the formulas) in one launch; the adjoint -- gradients to all three -- in two
    or three (``deodr_hip_sh_shade_b``).  More than the 64 views a launch takes go in slices, the sums over the views accumulated in slice order."""

    @staticmethod
    def forward(ctx, posed, sh, albedo, topology):
        posed, sh = posed.contiguous(), sh.contiguous()
        albedo = None if albedo is None else albedo.contiguous()
        n, V = posed.shape[0], posed.shape[1]
        out = torch.empty((n, V) if albedo is None else (n, V, albedo.shape[-1]), dtype=torch.float64, device=posed.device)
        step = hr.SH_MAX_VIEWS
        for b in range(0, n, step):
            hr.sh_shade(posed[b : b + step], topology._faces_u32, topology._vf_offsets, topology._vf_corners, sh, albedo,
                        luminosity=out[b : b + step] if albedo is None else None, colors=None if albedo is None else out[b : b + step],
                        clockwise=topology.clockwise)  # fmt: skip
        ctx.save_for_backward(posed, sh, *(() if albedo is None else (albedo,)))
        ctx.topology = topology
        return out

    @staticmethod
    def backward(ctx, out_b):
        posed, sh, *rest = ctx.saved_tensors
        albedo = rest[0] if rest else None
        topology, out_b = ctx.topology, out_b.contiguous()
        n, V = posed.shape[0], posed.shape[1]
        C = 1 if albedo is None else int(albedo.shape[-1])
        want = (ctx.needs_input_grad[0], True, albedo is not None)  # (the two sums come with the launch that everything else needs)
        posed_b = torch.empty_like(posed) if want[0] else None
        sh_b = torch.empty_like(sh)
        albedo_b = None if albedo is None else torch.empty_like(albedo)
        step = hr.SH_MAX_VIEWS
        for b in range(0, n, step):
            cut = lambda t: None if t is None else t[b : b + step]
            hr.sh_shade_b(posed[b : b + step], topology._faces_u32, topology._vf_offsets, topology._vf_corners, sh, albedo,
                          luminosity_b=cut(out_b) if albedo is None else None, colors_b=None if albedo is None else cut(out_b), posed_b=cut(posed_b),
                          sh_b=sh_b, albedo_b=albedo_b, accumulate=b > 0, scratch=_sh_scratch(posed.device, V, min(step, n - b), C),
                          clockwise=topology.clockwise, want=want)  # fmt: skip
        return posed_b, sh_b, albedo_b, None


def _skin_scratch(skin, n):
    """one scratch per (skin, number of poses), for the autograd wrapper (the kernels of one stream run one after the other)"""
    cache = skin.__dict__.setdefault("_skin_scratch", {})
    if n not in cache:
        cache[n] = hr.skin_scratch(skin.V, skin.J, skin.K, n, skin.device)
    return cache[n]


class SkinFunc(torch.autograd.Function):
    """(vertices [V,3], quaternions [n,J,4] raw, joints [J,3]; skin: a ``deodr_amd.skinning.Skin``) -> posed [n,V,3]: linear blend skinning
    (``deodr_amd/skinning.py`` has the formulas) in two launches; the adjoint -- gradients to all three -- in up to three (``deodr_hip_skin_apply_b``)."""

    @staticmethod
    def forward(ctx, vertices, quaternions, joints, skin):
        v, q, c = vertices.contiguous(), quaternions.contiguous(), joints.contiguous()
        world, posed = hr.skin_apply(v, c, skin.parents, q, skin.indices, skin.weights)
        ctx.save_for_backward(v, q, c, world)
        ctx.skin = skin
        return posed

    @staticmethod
    def backward(ctx, posed_b):
        v, q, c, world = ctx.saved_tensors
        skin = ctx.skin
        v_b, q_b, c_b = hr.skin_apply_b(v, c, skin.parents, q, skin.indices, skin.weights, world, posed_b.contiguous(), skin.joint_offsets,
                                        skin.joint_slots, scratch=_skin_scratch(skin, q.shape[0]), want=ctx.needs_input_grad[:3])  # fmt: skip
        return v_b, q_b, c_b, None


_image_term_scratches = {}  # (operator, device, n, H, W, C[, levels]) -> the scratch of the two classes below (the kernels of one stream run one after the other)


class _ImageTermFunc(torch.autograd.Function):
    """What the image data terms below share: (image [n,H,W,C]; obs, weights [n,H,W] | None, the term's float64 array on the device, its number:
    constants) -> the loss, a float64 scalar.  The forward call computes d loss / d image as well and keeps it; the backward multiplies it by the
    incoming scalar.  A term states ``operator(image, obs, weights, array, number, **how)``, its ``scratch`` maker and whether the number is one of
    that maker's dimensions (``sized_by_number``)."""

    @classmethod
    def forward(cls, ctx, image, obs, weights, array, number):
        key = (cls.operator, image.device, *(int(v) for v in image.shape), *((number,) if cls.sized_by_number else ()))
        if key not in _image_term_scratches:
            _image_term_scratches[key] = cls.scratch(*key[2:], image.device)
        want = ctx.needs_input_grad[0]
        _terms, loss, image_b = cls.operator(image, obs, weights, array, number, scratch=_image_term_scratches[key], want_gradient=want)
        if want:
            ctx.save_for_backward(image_b)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, loss_b):
        (image_b,) = ctx.saved_tensors
        return image_b * loss_b.to(image_b.dtype), None, None, None, None


class PyramidL2Func(_ImageTermFunc):
    """``apply(image, obs, weights, level_weights [levels+1], levels)`` -> the multi-scale L2 loss (``deodr_amd/pyramid.py`` has the formulas)"""

    scratch, sized_by_number = staticmethod(hr.pyramid_scratch), True
    operator = staticmethod(lambda image, obs, weights, level_weights, levels, **how: hr.pyramid_l2(image, obs, weights, levels, level_weights, **how))


class SSIML2Func(_ImageTermFunc):
    """``apply(image, obs, weights, mix [2], data_range)`` -> the mix of the pixel term and the structural term (``deodr_amd/ssim.py`` has the formulas)"""

    scratch, sized_by_number = staticmethod(hr.ssim_scratch), False
    operator = staticmethod(hr.ssim_l2)


class SpdSolveFunc(torch.autograd.Function):
    """(b [n,D]; system: a :class:`deodr_amd.smoothing.SpdSystem`, iterations, rel_tol: constants) -> (x, residual [D]) of
    ``deodr_amd.smoothing.spd_solve``, differentiable in ``b``.  ``A`` is symmetric, so the adjoint of ``b -> A^-1 b`` is the same solve of the
    incoming gradient.  With a truncated recurrence that is the adjoint of the CONVERGED operator, not of the ``iterations`` steps themselves (which
    are not linear in ``b``): exact only as far as the solve converges.  ``residual`` carries no gradient."""

    @staticmethod
    def forward(ctx, b, system, iterations, rel_tol):
        from . import smoothing

        ctx.system, ctx.iterations, ctx.rel_tol = system, iterations, rel_tol
        x, residual = smoothing.solve_no_grad(system, b, iterations, rel_tol)
        ctx.mark_non_differentiable(residual)
        return x, residual

    @staticmethod
    def backward(ctx, x_b, _residual_b):
        from . import smoothing

        return smoothing.spd_solve(ctx.system, x_b.contiguous(), ctx.iterations, ctx.rel_tol)[0], None, None, None


class ArapEnergyFunc(torch.autograd.Function):
    """(vertices [n,V,3]; energy: a :class:`deodr_amd.arap.ArapEnergyDevice`) -> (energy [n], gradient [n,V,3]) of the as-rigid-as-possible energy
    (include/deodr_hip_arap.h) in two launches; the energy is differentiable (its adjoint is the gradient the same call produced, exact wherever
    the rotations of the cells are unique), the gradient is not"""

    @staticmethod
    def forward(ctx, vertices, arap):
        energy, grad, _ = arap.evaluate_no_grad(vertices)
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(grad)
        return energy, grad

    @staticmethod
    def backward(ctx, energy_b, _grad_b):
        (grad,) = ctx.saved_tensors
        return energy_b[:, None, None] * grad, None


class ChamferFunc(torch.autograd.Function):
    """(vertices [n,V,3]; term: a :class:`deodr_amd.chamfer.PointCloudTerm`) -> (loss [n], terms [n,2]) of the closest-point energy
    (include/deodr_hip_chamfer.h); the loss is differentiable (its adjoint is the ``vertices_b`` the same call produced, exact wherever every nearest
    neighbour is unique), the terms are not: they are marked so, and torch refuses a gradient asked of them ("does not require grad").  The term
    chooses what runs: with ``search="grid"`` the call is ``deodr_hip_chamfer_grid`` (include/deodr_hip_chamfer_grid.h), and a
    :class:`deodr_amd.surface.PointSurfaceTerm` evaluates the point-to-surface energy (include/deodr_hip_surface.h: the envelope theorem, exact
    wherever every closest point is unique) -- ``SurfaceDistanceFunc`` is this class"""

    @staticmethod
    def forward(ctx, vertices, term):
        terms, loss, vertices_b = term.evaluate_no_grad(vertices)[:3]
        ctx.save_for_backward(vertices_b)
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, loss_b, _terms_b):
        (vertices_b,) = ctx.saved_tensors
        return loss_b[:, None, None] * vertices_b, None


SurfaceDistanceFunc = ChamferFunc


def sh_shade(posed, sh, albedo, topology):
    """-> luminosity [n,V] (``albedo`` None) or colors [n,V,C] of the posed vertices [n,V,3] (or [V,3]) under the SH lighting ``sh``, differentiable in
    all three: the kernels on float64 ROCm tensors, the same formulas as torch ops (``lighting.sh_shade_torch``) otherwise"""
    from . import lighting

    tensors = [posed, sh] + ([] if albedo is None else [albedo])
    n_columns = 1 if sh.dim() == 1 else int(sh.shape[1])
    channels = n_columns if albedo is None else int(albedo.shape[-1])
    fits = topology.nb_faces and posed.shape[-2] <= hr.SH_MAX_VERTICES and 1 <= channels <= 3 and n_columns in (1, channels)
    if usable(*tensors) and fits and (albedo is None or albedo.dim() in (1, 2)):
        out = SHShadeFunc.apply(posed if posed.dim() == 3 else posed[None], sh, albedo, topology)
        return out if posed.dim() == 3 else out[0]
    return lighting.sh_shade_torch(posed, topology, sh, albedo)
