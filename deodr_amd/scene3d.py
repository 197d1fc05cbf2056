"""Device-resident front half of the rasterizer: camera, lighting, silhouette flags, mesh normals, rigid energy.

The reference assembles the 2.5-D scene of every frame on the host with NumPy + SciPy (projection and distortion
``deodr/differentiable_renderer.py:341-438``, luminosity ``:814-850``, Scene2D assembly ``:896-983``, silhouette edge flags
``deodr/triangulated_mesh.py:153-166``, vertex normals ``:113-151``, Laplacian energy ``deodr/laplacian_rigid_energy.py``) and
its PyTorch layer round-trips through ``.numpy()`` (``deodr/pytorch/differentiable_renderer_pytorch.py:52-54``).  Once the
rasterizer takes tens of microseconds that glue is the whole iteration.  Here every array lives on the ROCm device from the
mesh vertices to the loss: the O(V) algebra is a handful of batched torch ops over ``n_views`` views (differentiated by
autograd), the rasterizer is the HIP library behind the autograd ops of render_ops.py, and nothing visits the host inside a fit loop.

Same math as the reference (float64 by default), not the same code: batched over views, index_add instead of SciPy sparse
products, adjacency as flat index arrays built once per topology.
"""

import numpy as np
import torch

from .hip_renderer import DeviceScene, HipRasterizer
from .render_ops import RenderViewsFunc, RenderViewsL2Func  # noqa: F401  (the rasterizer under autograd; re-exported)


def _t(a, device, dtype=torch.float64):
    return (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(device=device, dtype=dtype)


class DeviceCamera:
    """``n`` pinhole cameras with OpenCV's distortion model (k1, k2, p1, p2, k3), as device tensors.

    ``extrinsic`` [n,3,4] (or [3,4]) world -> camera, ``intrinsic`` [n,3,3] (or [3,3]), ``distortion`` [n,5] / [5] / None.
    Reference: ``Camera`` deodr/differentiable_renderer.py:250-438."""

    def __init__(self, extrinsic, intrinsic, height, width, distortion=None, device="cuda", dtype=torch.float64):
        self.device, self.dtype = torch.device(device), dtype
        e, k = _t(extrinsic, self.device, dtype), _t(intrinsic, self.device, dtype)
        self.extrinsic = e[None] if e.dim() == 2 else e
        self.intrinsic = k[None] if k.dim() == 2 else k
        # one camera matrix shared by n views (extrinsic [n,3,4] with one intrinsic [3,3], or the other way round): every array is
        # expanded to n views HERE -- the fused kernels index all three per view (`intrinsic[9 b + i]`, `extrinsic[12 b + i]`)
        self.n_views = max(int(self.extrinsic.shape[0]), int(self.intrinsic.shape[0]))
        for name in ("extrinsic", "intrinsic"):
            a = getattr(self, name)
            if a.shape[0] not in (1, self.n_views):
                raise ValueError(f"DeviceCamera: {name} has {a.shape[0]} views, expected 1 or {self.n_views}")
            setattr(self, name, a.expand(self.n_views, *a.shape[1:]))
        self.height, self.width = int(height), int(width)
        self.distortion = None
        if distortion is not None:
            d = _t(distortion, self.device, dtype)
            self.distortion = (d[None] if d.dim() == 1 else d).expand(self.n_views, 5).contiguous()
        self.extrinsic, self.intrinsic = self.extrinsic.contiguous(), self.intrinsic.contiguous()

    @classmethod
    def stack(cls, cameras, device="cuda", dtype=torch.float64):
        """One batched camera from a list of cameras with ``extrinsic`` / ``intrinsic`` / ``distortion`` / ``height`` / ``width``
        attributes (e.g. the reference's ``Camera`` objects or this module's NumPy-level mirror)."""
        c0 = cameras[0]
        dist = None
        if any(getattr(c, "distortion", None) is not None for c in cameras):
            dist = np.stack([np.zeros(5) if c.distortion is None else np.asarray(c.distortion, dtype=np.float64) for c in cameras])
        return cls(np.stack([np.asarray(c.extrinsic) for c in cameras]), np.stack([np.asarray(c.intrinsic) for c in cameras]), c0.height,
                   c0.width, dist, device, dtype)  # fmt: skip

    @classmethod
    def from_pose(cls, quaternions, translations, focal, center, height, width, distortion=None, shared_intrinsics=True, device="cuda", dtype=torch.float64):
        """``n`` cameras from what a calibration moves: quaternions [n,4] = (x, y, z, w) (normalised here) and translations [n,3] of the world ->
        camera transforms, focal = (fx, fy), center = (cx, cy) and distortion (k1, k2, p1, p2, k3) | None -- one set shared by the views ([2], [2],
        [5]) or per view ([n,2], [n,2], [n,5]).  Differentiable in all five (``deodr_hip_camera_assemble`` on float64 ROCm tensors)."""
        from . import fronthalf

        dev = torch.device(device)
        q, t, f, c = (_t(a, dev, dtype) for a in (quaternions, translations, focal, center))
        d = None if distortion is None else _t(distortion, dev, dtype)
        extrinsic, intrinsic, dist = fronthalf.camera_assemble(q, t, f, c, d, shared=shared_intrinsics)
        return cls(extrinsic, intrinsic, height, width, dist, device, dtype)

    def world_to_camera(self, points_3d):
        """[V,3] (shared by the views) or [n,V,3] -> [n,V,3]"""
        p = points_3d if points_3d.dim() == 3 else points_3d[None].expand(self.n_views, -1, -1)
        return p @ self.extrinsic[:, :, :3].transpose(1, 2) + self.extrinsic[:, None, :, 3]

    def project_points(self, points_3d):
        """-> (image coordinates [n,V,2] with x = column first, depths [n,V]); differentiable (dr.py:341-395)."""
        from . import fronthalf

        if points_3d.dtype != self.dtype:  # (a float32 mesh seen by a float64 camera: projected in the camera's arithmetic, its gradient cast back by autograd)
            points_3d = points_3d.to(self.dtype)
        batch_ok = points_3d.dim() == 2 or int(points_3d.shape[0]) == self.n_views  # (else: the torch path below broadcasts, or raises)
        if batch_ok and fronthalf.usable(points_3d, self.extrinsic, self.intrinsic) and (self.distortion is None or fronthalf.usable(self.distortion)):
            # one kernel (two with its adjoint) instead of ~15 + ~25 torch kernels
            p = points_3d if points_3d.dim() == 3 else points_3d[None].expand(self.n_views, -1, -1)
            return fronthalf.ProjectPointsFunc.apply(p, self.extrinsic, self.intrinsic, self.distortion)
        pc = self.world_to_camera(points_3d)
        depths = pc[..., 2]
        xy = pc[..., :2] / depths[..., None]
        if self.distortion is not None:
            k1, k2, p1, p2, k3 = (self.distortion[:, i, None] for i in range(5))
            x, y = xy[..., 0], xy[..., 1]
            x2, y2 = x * x, y * y
            r2 = x2 + y2
            r4 = r2 * r2
            radial = 1 + k1 * r2 + k2 * r4 + k3 * (r2 * r4)
            xd = x * radial + (2 * p1 * x * y + p2 * (r2 + 2 * x2))
            yd = y * radial + (p1 * (r2 + 2 * y2) + 2 * p2 * x * y)
            xy = torch.stack((xd, yd), dim=-1)
        ij = xy @ self.intrinsic[:, :2, :2].transpose(1, 2) + self.intrinsic[:, None, :2, 2]
        return ij, depths


class MeshTopology:
    """Static connectivity of a triangle mesh as flat device index arrays, built once on the host.

    ``face_edge`` [T,3]: id of the edge (v0,v1), (v1,v2), (v2,v0) of every face -- the same slot order as the rasterizer's
    ``edgeflags`` (reference ``TriMeshAdjacencies`` deodr/triangulated_mesh.py:17-110, which keeps SciPy sparse matrices)."""

    def __init__(self, faces, nb_vertices=None, clockwise=False, device="cuda"):
        f = np.asarray(faces).astype(np.int64)
        assert f.ndim == 2 and f.shape[1] == 3
        self.device = torch.device(device)
        self.clockwise = bool(clockwise)
        self.nb_faces = int(f.shape[0])
        self.nb_vertices = int(nb_vertices) if nb_vertices is not None else int(f.max()) + 1
        e = np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))  # slot-major: [3T,2]
        key = np.minimum(e[:, 0], e[:, 1]) * self.nb_vertices + np.maximum(e[:, 0], e[:, 1])
        _, edge_id, counts = np.unique(key, return_inverse=True, return_counts=True)
        self.nb_edges = int(edge_id.max()) + 1 if len(edge_id) else 0
        self.is_manifold = bool(np.all(counts <= 2))
        self.is_closed = bool(self.is_manifold and np.all(counts == 2))
        self.faces = torch.as_tensor(f, device=self.device)
        self.face_edge = torch.as_tensor(edge_id.reshape(3, -1).T.copy(), device=self.device)  # [T,3]
        # for the fused silhouette kernel (manifold meshes): the face across every edge slot, 0xffffffff on a boundary
        self._edge_faces = None
        if self.is_manifold and self.nb_faces:
            slot_face = np.tile(np.arange(self.nb_faces), 3)  # face of slot-major entry i of `e`
            order = np.argsort(edge_id, kind="stable")
            sorted_edge, sorted_face = edge_id[order], slot_face[order]
            other = np.full(3 * self.nb_faces, 0xFFFFFFFF, dtype=np.int64)
            same = sorted_edge[1:] == sorted_edge[:-1]  # (at most two slots per edge)
            other[order[:-1][same]] = sorted_face[1:][same]
            other[order[1:][same]] = sorted_face[:-1][same]
            self._edge_faces = torch.as_tensor(other.reshape(3, -1).T.astype(np.uint32).view(np.int32).copy(), device=self.device)
            self._faces_u32 = torch.as_tensor(f.astype(np.uint32).view(np.int32), device=self.device).contiguous()
        # graph Laplacian over "shares a face" adjacency, and M = L^T L as a COO list (dr: laplacian_rigid_energy.py:18-22)
        a = np.zeros((0, 2), dtype=np.int64)
        if self.nb_faces:
            pairs = np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]], f[:, [1, 0]], f[:, [2, 1]], f[:, [0, 2]]))
            a = np.unique(pairs, axis=0)
        import scipy.sparse as sp

        adj = sp.coo_matrix((np.ones(len(a)), (a[:, 0], a[:, 1])), shape=(self.nb_vertices, self.nb_vertices)).tocsr()
        lap = sp.diags(np.asarray(adj.sum(axis=1)).ravel()) - adj
        m = (lap.T @ lap).tocoo()
        u32 = lambda a: torch.as_tensor(np.ascontiguousarray(a).astype(np.uint32).view(np.int32), device=self.device)
        mc = m.tocsr()
        mc.sort_indices()
        self._m_csr = (u32(mc.indptr), u32(mc.indices), torch.as_tensor(mc.data.astype(np.float64), device=self.device))  # rows of L^T L
        # vertex -> the slots 3 f + corner it occupies in `faces` (the gathers of the shading adjoint, no atomics)
        corner_vertex = f.reshape(-1)
        self._vf_corners = u32(np.argsort(corner_vertex, kind="stable"))
        self._vf_offsets = u32(np.concatenate(([0], np.cumsum(np.bincount(corner_vertex, minlength=self.nb_vertices)))))
        if self._edge_faces is None and self.nb_faces:
            self._faces_u32 = u32(f)
        self._m_rows = torch.as_tensor(m.row.astype(np.int64), device=self.device)
        self._m_cols = torch.as_tensor(m.col.astype(np.int64), device=self.device)
        self._m_vals = torch.as_tensor(m.data.astype(np.float64), device=self.device)
        self.n_components = int(sp.csgraph.connected_components(adj, directed=False)[0]) if self.nb_vertices else 0

    # ---- differentiable geometry (batched: vertices [..., V, 3]) ---------------------------------------------------------

    def face_normals(self, vertices):
        tri = vertices[..., self.faces, :]  # [..., T, 3, 3]
        n = torch.cross(tri[..., 1, :] - tri[..., 0, :], tri[..., 2, :] - tri[..., 0, :], dim=-1)
        if self.clockwise:
            n = -n
        return n / n.norm(dim=-1, keepdim=True)

    def vertex_normals(self, vertices):
        """normalised sum of the unit normals of the faces around each vertex (triangulated_mesh.py:113-151)"""
        fn = self.face_normals(vertices)
        acc = torch.zeros_like(vertices)
        idx = self.faces.reshape(-1)
        acc = acc.index_add(-2, idx, fn.repeat_interleave(3, dim=-2))
        return acc / acc.norm(dim=-1, keepdim=True)

    def edge_on_silhouette(self, ij):
        """[..., V, 2] image coordinates -> uint8 [..., T, 3]: the edge has exactly one front-facing incident face in the image
        (triangulated_mesh.py:153-166).  No gradient (the flags select which edges are antialiased)."""
        from . import fronthalf

        if self._edge_faces is not None and ij.dim() == 3 and fronthalf.usable(ij):
            return fronthalf.silhouette_flags(ij, self._faces_u32, self._edge_faces, self.clockwise)  # one kernel instead of eight
        with torch.no_grad():
            tri = ij[..., self.faces, :]
            u, v = tri[..., 1, :] - tri[..., 0, :], tri[..., 2, :] - tri[..., 0, :]
            cr = u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]
            visible = (cr > 0) if self.clockwise else (cr < 0)  # [..., T]
            count = torch.zeros(ij.shape[:-2] + (self.nb_edges,), dtype=torch.int32, device=ij.device)
            count = count.index_add(-1, self.face_edge.reshape(-1), visible.to(torch.int32).repeat_interleave(3, dim=-1))
            return (count[..., self.face_edge] == 1).to(torch.uint8)

    def laplacian_quadratic(self, diff):
        """M diff with M = L^T L, diff [..., V, 3] (one index_add over the non-zeros of M)"""
        out = torch.zeros_like(diff)
        return out.index_add(-2, self._m_rows, self._m_vals[:, None] * diff[..., self._m_cols, :])


class LaplacianRigidEnergyDevice:
    """Laplacian rigid energy 0.5 c (V - V_ref)^T (L^T L x I3) (V - V_ref) and its gradient, on the device
    (reference deodr/laplacian_rigid_energy.py:15-41; its PyTorch twin falls back to SciPy on the host, :38-46).  A quadratic in the
    displacement: not invariant to rotations of a part of the mesh (``deodr_amd.arap.ArapEnergyDevice`` is)."""

    def __init__(self, topology, vertices_ref, cregu):
        if topology.n_components > 1:
            raise BaseException("You have more than one connected component in your mesh.")
        self.topology, self.cregu = topology, float(cregu)
        self.vertices_ref = _t(vertices_ref, topology.device).clone()

    def evaluate(self, vertices):
        """-> (energy, gradient [V,3]); the energy is differentiable too (autograd sees plain tensor ops)"""
        from . import fronthalf

        if fronthalf.usable(vertices, self.vertices_ref) and vertices.dim() == 2:
            return fronthalf.RigidEnergyFunc.apply(vertices, self.vertices_ref, self.topology, self.cregu)  # one kernel, deterministic
        diff = vertices - self.vertices_ref
        grad = self.cregu * self.topology.laplacian_quadratic(diff)
        return 0.5 * (diff * grad).sum(), grad


class DeviceMesh:
    """A coloured (or textured) triangle mesh on the device: topology + per-vertex attributes.

    The counterpart of the reference's ``ColoredTriMesh`` (deodr/triangulated_mesh.py:302-360) for the attributes the renderer
    consumes.  ``vertices`` may be a leaf tensor that requires grad."""

    def __init__(self, faces, vertices, clockwise=False, colors=None, uv=None, faces_uv=None, texture=None, device="cuda", dtype=torch.float64,
                 topology=None):  # fmt: skip
        self.device, self.dtype = torch.device(device), dtype
        self.topology = topology if topology is not None else MeshTopology(faces, int(np.shape(vertices)[-2]), clockwise, self.device)
        self.faces_np = np.asarray(faces).astype(np.uint32)
        self.clockwise = bool(clockwise)
        self.vertices = _t(vertices, self.device, dtype)
        self.vertices_colors = None if colors is None else _t(colors, self.device, dtype)
        self.uv = None if uv is None else _t(uv, self.device, dtype)
        self.faces_uv_np = None if faces_uv is None else np.asarray(faces_uv).astype(np.uint32)
        self.texture = None if texture is None else _t(texture, self.device, dtype)

    @property
    def nb_vertices(self):
        return self.topology.nb_vertices

    @property
    def nb_faces(self):
        return self.topology.nb_faces

    def set_vertices(self, vertices):
        self.vertices = vertices

    def set_vertices_colors(self, colors):
        self.vertices_colors = colors

    def subdivise(self, n_iter, subdivision=None):
        """-> a new DeviceMesh, ``n_iter`` times Loop-subdivided (deodr/triangulated_mesh.py:499-562): its ``vertices`` are ``S self.vertices``
        (differentiable: gradients reach the control vertices), its colours follow the reference's colour rule; ``mesh.subdivision`` keeps the
        :class:`deodr_amd.subdivision.LoopSubdivision` (pass it as ``subdivision`` to subdivide other vertices of the same connectivity)."""
        if not n_iter:
            return self
        if self.uv is not None:
            raise BaseException("Textured mesh not supported yet in subdivision.")
        from .subdivision import LoopSubdivision

        sub = subdivision or LoopSubdivision(self.faces_np, self.nb_vertices, n_iter, self.clockwise, self.device)
        colors = None if self.vertices_colors is None else sub.apply_colors(self.vertices_colors)
        fine = DeviceMesh(sub.faces_fine, sub.apply(self.vertices), clockwise=self.clockwise, colors=colors, device=self.device, dtype=self.dtype,
                          topology=sub.topology)  # fmt: skip
        fine.subdivision = sub
        return fine


class Scene3DDevice:
    """One mesh, one directional + one ambient light, ``n`` cameras: everything up to the image stays on the device.

    Mirrors what ``Scene3D.render`` / ``render_depth`` compute in the reference (dr.py:764-1051) with the per-view work
    batched: project -> silhouette flags -> vertex colours (or shade) -> rasterize.  Gradients reach ``mesh.vertices``,
    ``mesh.vertices_colors``, the light tensors and anything upstream through autograd."""

    def __init__(self, sigma=1.0, perspective_correct=False, integer_pixel_centers=True, pixel_dtype=torch.float64):
        self.sigma, self.perspective_correct, self.integer_pixel_centers = float(sigma), bool(perspective_correct), bool(integer_pixel_centers)
        self.pixel_dtype = pixel_dtype
        self.mesh = None
        self.light_directional, self.light_ambient = None, 0.0
        self.light_sh = None  # [9] | [9,S]: spherical-harmonic lighting instead of the directional + ambient pair (set_light_sh)
        self.background_color, self.background_image = None, None
        self._state = None  # (key, DeviceScene, HipRasterizer)
        self.last = {}

    def set_mesh(self, mesh):
        self.mesh = mesh

    def set_light(self, light_directional, light_ambient):
        self.light_directional = None if light_directional is None else _t(light_directional, self.mesh.device if self.mesh else "cuda")
        self.light_ambient = light_ambient
        self.light_sh = None

    def set_light_sh(self, sh):
        """Spherical-harmonic lighting of bands 0 - 2 (``deodr_amd/lighting.py``) in place of the directional + ambient pair: ``sh`` [9] (monochrome)
        or [9,C] (one column per colour channel), unclamped irradiance ``sum_k sh[k] Y_k(normal)``.  ``lighting.sh_from_directional`` gives the
        coefficients that approximate a directional + ambient pair."""
        self.light_sh = _t(sh, self.mesh.device if self.mesh else "cuda")
        self.light_directional, self.light_ambient = None, 0.0

    def set_background_color(self, background_color):
        if self.background_image is not None:
            raise BaseException("you cannot provide both background image and background color")
        self.background_color = np.asarray(background_color, dtype=np.float64).reshape(-1)

    def set_background_image(self, background_image):
        if self.background_color is not None:
            raise BaseException("you cannot provide both background image and background color")
        self.background_image = background_image

    # ---- pieces ------------------------------------------------------------------------------------------------------

    def vertices_luminosity(self, vertices):
        """max(0, -n . l) + ambient per vertex (dr.py:814-822); vertices [..., V, 3]"""
        if self.light_sh is not None:
            from . import fronthalf

            return fronthalf.sh_shade(vertices, self.light_sh, None, self.mesh.topology)  # (one column: a luminosity)
        amb = self.light_ambient
        if self.light_directional is None:
            return torch.zeros(vertices.shape[:-1], dtype=vertices.dtype, device=vertices.device) + amb
        from . import fronthalf

        light = self.light_directional
        if fronthalf.usable(vertices, light) and self.mesh.nb_faces and (not torch.is_tensor(amb) or fronthalf.usable(amb)):
            amb = amb if torch.is_tensor(amb) else torch.full((), float(amb), dtype=torch.float64, device=vertices.device)
            lum = fronthalf.VertexLuminosityFunc.apply(vertices if vertices.dim() == 3 else vertices[None], light, amb, self.mesh.topology)  # 1 kernel
            return lum if vertices.dim() == 3 else lum[0]
        normals = self.mesh.topology.vertex_normals(vertices)
        return torch.relu(-(normals * light).sum(-1)) + amb

    def _rasterizer(self, n_views, height, width, nb_colors, textured, backface_culling):
        m = self.mesh
        key = (id(m.topology), n_views, height, width, nb_colors, textured, backface_culling, self.perspective_correct, self.integer_pixel_centers,
               None if self.background_color is None else self.background_color.tobytes(), id(self.background_image),
               tuple(m.texture.shape) if textured else None)  # fmt: skip  (the texture's VALUE is set at every render: _shared_inputs)
        if self._state is None or self._state[0] != key:
            V, T = m.nb_vertices, m.nb_faces
            dev, vd = m.device, m.dtype
            zeros = lambda *s: torch.zeros(s, dtype=vd, device=dev)
            bgi = self.background_image
            if bgi is not None:
                bgi = _t(bgi, dev, self.pixel_dtype)
                bgi = bgi[None].expand(n_views, -1, -1, -1) if bgi.dim() == 3 else bgi
            ds = DeviceScene(
                m.faces_np, m.faces_uv_np if textured else m.faces_np, np.full(T, textured, dtype=np.uint8), np.full(T, textured, dtype=np.uint8),
                m.uv if textured else zeros(V, 2), zeros(n_views, V, 2), torch.ones(n_views, V, dtype=vd, device=dev), zeros(n_views, V, nb_colors),
                zeros(n_views, V), torch.zeros(n_views, T, 3, dtype=torch.uint8, device=dev), height, width,
                texture=m.texture if textured else None, background_color=self.background_color, background_image=bgi,
                clockwise=m.clockwise, backface_culling=backface_culling, strict_edge=True, perspective_correct=self.perspective_correct,
                integer_pixel_centers=self.integer_pixel_centers, vertex_dtype=vd, pixel_dtype=self.pixel_dtype, device=dev,
            )  # fmt: skip
            keep = self._state[2] if self._state is not None and self._state[2].dims == (T, height, width, nb_colors, n_views) else None
            self._state = (key, ds, keep or HipRasterizer.for_scene(ds))
        return self._state[1], self._state[2]

    def _shared_inputs(self, ds, textured, texture, uv):
        """A textured render reads the value ``mesh.texture`` / ``mesh.uv`` have at the call (an optimiser may have updated them in place, or rebound
        them); -> the extra inputs of the autograd function: those that are differentiated, and only those"""
        if textured and texture is None:
            ds.set_texture(self.mesh.texture)
        if textured and uv is None:
            ds.set_uv(self.mesh.uv)
        return () if texture is None and uv is None else (texture, uv)

    def _prepare(self, camera, ij, depths, colors, shade, textured, backface_culling, texture, uv):
        """What every rasterizer call starts with -> (DeviceScene, HipRasterizer, silhouette flags, the extra inputs of the autograd function)"""
        if (self.background_image is None) == (self.background_color is None):
            raise BaseException("You need to provide either a background image or background color")
        n = camera.n_views
        ds, r = self._rasterizer(n, camera.height, camera.width, int(colors.shape[-1]), textured, backface_culling)
        shared = self._shared_inputs(ds, textured, texture, uv)
        flags = self.mesh.topology.edge_on_silhouette(ij) if self.sigma > 0 else torch.zeros((n, self.mesh.nb_faces, 3), dtype=torch.uint8, device=ij.device)
        self.last = dict(ij=ij, depths=depths, edgeflags=flags, colors=colors, shade=shade)
        return ds, r, flags, shared

    def _rasterize(self, camera, ij, depths, colors, shade, textured, backface_culling, texture=None, uv=None):
        """``texture`` / ``uv``: given when they are to be differentiated (``mesh.texture`` / ``mesh.uv`` requiring grad), see :meth:`render`"""
        ds, r, flags, shared = self._prepare(camera, ij, depths, colors, shade, textured, backface_culling, texture, uv)
        return RenderViewsFunc.apply(ij, colors, shade, depths.detach(), flags, ds, r, self.sigma, *shared)

    def _rasterize_l2(self, camera, ij, depths, colors, shade, textured, backface_culling, obs, weights=None, texture=None, uv=None):
        """-> (sum (image - obs)^2 over all views -- times the per-pixel weights, if any --, image [n,H,W,C]) through the one-call fit step"""
        ds, r, flags, shared = self._prepare(camera, ij, depths, colors, shade, textured, backface_culling, texture, uv)
        return RenderViewsL2Func.apply(ij, colors, shade, depths.detach(), flags, obs, ds, r, self.sigma, weights, *shared)[:2]

    # ---- the reference's entry points, batched over the camera's views -----------------------------------------------

    def _vertex_inputs(self, camera):
        """-> (ij [n,V,2], depths [n,V], colors [n,V,C], shade [n,V], textured) of the mesh seen by ``camera``: a textured mesh is shaded by its
        luminosity and coloured by its texture, any other carries ``vertices_colors`` times the luminosity as its colours"""
        m = self.mesh
        assert m is not None, "You need to provide a mesh first."
        ij, depths = camera.project_points(m.vertices)
        n, V = ij.shape[0], m.nb_vertices
        if self.light_sh is not None and m.uv is None and m.vertices_colors.dim() in (1, 2):
            from . import fronthalf

            posed = m.vertices if m.vertices.dim() == 3 else m.vertices[None]  # (vertices shared by the views: shaded once)
            colors = fronthalf.sh_shade(posed, self.light_sh, m.vertices_colors, m.topology)  # one launch: albedo [C] | [V,C] times the irradiance
            return ij, depths, colors.expand(n, -1, -1), torch.zeros((n, V), dtype=m.dtype, device=m.device), False
        lum = self.vertices_luminosity(m.vertices)
        lum = lum[None].expand(n, -1) if lum.dim() == 1 else lum
        if m.uv is not None:
            assert m.texture is not None
            return ij, depths, torch.zeros((n, V, int(m.texture.shape[2])), dtype=m.dtype, device=m.device), lum, True
        vc = m.vertices_colors if m.vertices_colors.dim() == 3 else m.vertices_colors[None].expand(n, -1, -1)
        return ij, depths, vc * lum[..., None], torch.zeros((n, V), dtype=m.dtype, device=m.device), False

    def render_l2(self, camera, obs, backface_culling=True, weights=None):
        """-> (sum over views and pixels of (render(camera) - obs)^2 as a differentiable scalar, the rendered images [n,H,W,C]).
        ``obs`` [n,H,W,C] in the scene's pixel dtype, contiguous (anything else is converted at every call).
        ``weights`` [n,H,W] or [H,W] (same dtype, contiguous, to avoid a conversion): the sum becomes ``sum(weights[..., None] * (image - obs)**2)`` --
        a mask or a per-pixel confidence, ``>= 0``; the images are rendered everywhere.  No gradient flows to the weights."""
        ij, depths, colors, shade, textured = self._vertex_inputs(camera)
        n = ij.shape[0]
        obs = obs.to(device=ij.device, dtype=self.pixel_dtype)
        if weights is not None and tuple(weights.shape) not in ((n, camera.height, camera.width), (camera.height, camera.width)):
            raise ValueError(f"weights must have shape [{n}, {camera.height}, {camera.width}] or [{camera.height}, {camera.width}], not {list(weights.shape)}")
        extra = {} if weights is None else {"weights": weights}  # (only when given: a stand-in for _rasterize_l2 that knows no weights must fail, not ignore them)
        extra.update(self._differentiated_shared())  # (the same convention)
        return self._rasterize_l2(camera, ij, depths, colors, shade, textured, backface_culling, obs.expand(n, -1, -1, -1).contiguous(), **extra)

    def _rendered_frames(self, camera, obs, weights, backface_culling):
        """-> (``render(camera)`` [n,H,W,C], ``obs`` and ``weights`` (or None) as contiguous tensors of its views, dtype and device): what the image
        data terms below take"""
        image = self.render(camera, backface_culling=backface_culling)
        n = image.shape[0]
        obs = obs.to(device=image.device, dtype=image.dtype).expand(n, -1, -1, -1).contiguous()
        if weights is not None:
            if tuple(weights.shape) not in ((n, camera.height, camera.width), (camera.height, camera.width)):
                raise ValueError(f"weights must have shape [{n}, {camera.height}, {camera.width}] or [{camera.height}, {camera.width}], not {list(weights.shape)}")
            weights = weights.to(device=image.device, dtype=image.dtype).expand(n, -1, -1).contiguous()
        return image, obs, weights

    def render_pyramid_l2(self, camera, obs, levels, weights=None, level_weights=None, backface_culling=True):
        """-> (the multi-scale L2 loss of ``render(camera)`` against ``obs`` as a differentiable scalar, the rendered images [n,H,W,C]):
        :meth:`render` followed by :func:`deodr_amd.pyramid.pyramid_l2` (``levels`` coarse levels, ``level_weights`` [levels+1], None: ones), so the
        adjoint is that term's ``image_b`` through the rasterizer's ``render_backward``.  ``obs`` [n,H,W,C] and ``weights`` [n,H,W] or [H,W] (``>= 0``, or
        None) in the scene's pixel dtype (anything else is converted at every call).  The one-call fit step cannot carry this term: the gradient of
        a pixel depends on the residuals of its neighbours."""
        from . import pyramid

        image, obs, weights = self._rendered_frames(camera, obs, weights, backface_culling)
        return pyramid.pyramid_l2(image, obs, weights, levels, level_weights), image

    def render_ssim_l2(self, camera, obs, weights=None, mix=None, data_range=1.0, backface_culling=True):
        """-> (``mix[0] sum w (image - obs)^2 + mix[1] sum w (1 - SSIM)`` of ``render(camera)`` against ``obs`` as a differentiable scalar, the
        rendered images [n,H,W,C]): :meth:`render` followed by :func:`deodr_amd.ssim.ssim_l2` (``mix`` [2], None: (0, 1); ``data_range``: the span of
        the intensities), so the adjoint is that term's ``image_b`` through the rasterizer's ``render_backward``.  ``obs`` [n,H,W,C] and ``weights``
        [n,H,W] or [H,W] (``>= 0``, or None) in the scene's pixel dtype (anything else is converted at every call); the weights multiply the SSIM
        map and do not enter its windows.  The one-call fit step cannot carry this term: the gradient of a pixel depends on its 11 x 11
        neighbourhood."""
        from . import ssim

        image, obs, weights = self._rendered_frames(camera, obs, weights, backface_culling)
        return ssim.ssim_l2(image, obs, weights, mix, data_range), image

    def _differentiated_shared(self):
        """{"texture": mesh.texture, "uv": mesh.uv}, each only when it requires grad: the keyword arguments a textured render passes on"""
        m = self.mesh
        if m.uv is None:
            return {}
        return {k: t for k, t in (("texture", m.texture), ("uv", m.uv)) if torch.is_tensor(t) and t.requires_grad}

    def render(self, camera, return_z_buffer=False, backface_culling=True):
        """-> image [n,H,W,C] (and z_buffer [n,H,W]); dr.py:896-983.  A textured mesh is rendered with the value ``mesh.texture`` has at the call;
        when ``mesh.texture`` / ``mesh.uv`` require grad they receive their gradients (summed over the views)."""
        ij, depths, colors, shade, textured = self._vertex_inputs(camera)
        image, z = self._rasterize(camera, ij, depths, colors, shade, textured, backface_culling, **self._differentiated_shared())
        return (image, z) if return_z_buffer else image

    def render_depth(self, camera, depth_scale=1.0, backface_culling=True):
        """-> depth image [n,H,W,1]: the depth of every vertex rendered as its colour (dr.py:1001-1036)"""
        m = self.mesh
        ij, depths = camera.project_points(m.vertices)
        shade = torch.zeros_like(depths)
        image, _ = self._rasterize(camera, ij, depths, depths[..., None] * depth_scale, shade, False, backface_culling)
        return image
