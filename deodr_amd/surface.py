"""The point-to-surface data term on the device: a point set against the TRIANGLES of a mesh -- the closest point of the closest triangle, not the
closest vertex.  What a scan that is denser than the mesh needs: against the vertices, points that lie exactly on a large triangle are still far from
its corners, pay for it and pull on them; against the surface they pay nothing.

``loss = mix_0 sum_k w_k min(|p_k - q_k|^2, tau^2) + mix_1 sum_i u_i min(|v_i - p_k*(i)|^2, tau^2)`` with ``q_k`` the closest point of the mesh's
surface to ``p_k``; the second term is the mesh -> points side of :mod:`deodr_amd.chamfer`, unchanged (vertex to nearest point).  The gradient of
the first comes from the envelope theorem: corner ``c`` of the closest face receives ``bary_c`` times the pull ``2 w_k (q_k - p_k)``.
``include/deodr_hip_surface.h`` has the operation, rounded operation by operation -- ties between faces are the generic case (a closest point on a
shared vertex or edge), and the lowest face index wins --, ``deodr_amd/csrc/dr_surface.h`` the kernels: a brute-force tiled search over face
records, a face-major gather, no lists, no floating-point atomics, a fixed number of launches, the same bits from run to run.

:class:`PointSurfaceTerm` is a :class:`deodr_amd.chamfer.PointCloudTerm` (the same clouds, padding, weights and device-resident ``params``) that
also holds the faces and their transposed corner table; :func:`surface_distance_torch` is the same definition as torch ops, chunked over the
points -- what runs on tensors the kernels do not take and what the kernels are timed against; :func:`corner_table` builds the table.
``deodr_amd.pytorch.MeshPointCloudFitter(metric="surface")`` fits with it.

``PointSurfaceTerm(search="grid")`` finds the same faces over a uniform grid of hashed cells holding the triangles, one record per face
(``include_staged/deodr_hip_surface_grid.h``, ``deodr_amd/csrc/dr_surface_grid.h``): the cost grows with F + P instead of F * P and there is no cap
on F * P or V * P; it needs a finite ``max_distance``, and a point with no face within it has no correspondence (-1, barycentric zeros)."""

import numpy as np
import torch

from .chamfer import CHUNK_BYTES, PointCloudTerm, _array, _mesh_to_points, mask_beyond

LIVE_ARRAYS = 24  # [n, chunk, F] arrays alive at once in closest_point_torch, roughly: what a chunk is sized by


def corner_table(faces, nb_vertices):
    """-> (corner_offsets [V + 1], corners [3 F]) int32 NumPy arrays: for vertex ``i`` the entries ``3 f + c`` with ``faces[f][c] == i``, in increasing
    order, at ``corners[corner_offsets[i] : corner_offsets[i + 1]]``.  ``faces`` [F >= 1, 3] integers in ``[0, nb_vertices)``: checked."""
    f = np.asarray(_array(faces))
    V = int(nb_vertices)
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"corner_table: faces must be [F >= 1, 3] integers, not {list(f.shape)} {f.dtype}")
    if V < 1 or f.min() < 0 or f.max() >= V:
        raise ValueError(f"corner_table: the entries of faces must be in [0, {V})")
    if 3 * f.shape[0] > np.iinfo(np.int32).max:
        raise ValueError("corner_table: 3 F must fit an int32")
    flat = f.reshape(-1).astype(np.int64)
    corners = np.argsort(flat, kind="stable").astype(np.int32)  # (stable: increasing 3 f + c within a vertex)
    offsets = np.concatenate(([0], np.cumsum(np.bincount(flat, minlength=V)))).astype(np.int32)
    return offsets, corners


def sample_surface(vertices, faces, count, seed=0):
    """-> (points [count,3], face [count], barycentric [count,3]) NumPy: ``count`` points area-uniform on the triangles of a mesh (a synthetic scan)"""
    v, f = np.asarray(_array(vertices), dtype=np.float64), np.asarray(_array(faces))
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    rs = np.random.RandomState(seed)
    face = rs.choice(len(f), size=int(count), p=area / area.sum())
    s, t = rs.rand(int(count)), rs.rand(int(count))
    s, t = np.where(s + t > 1, 1 - s, s), np.where(s + t > 1, 1 - t, t)  # (the other half of the parallelogram folded back)
    bary = np.stack((1 - s - t, s, t), axis=1)
    return bary[:, 0:1] * a[face] + bary[:, 1:2] * b[face] + bary[:, 2:3] * c[face], face, bary


def check_corner_table(faces, nb_vertices, corner_offsets, corners):
    """raises ValueError unless (corner_offsets, corners) is :func:`corner_table` of ``faces``"""
    offsets, table = corner_table(faces, nb_vertices)
    o, c = np.asarray(_array(corner_offsets)), np.asarray(_array(corners))
    if o.shape != offsets.shape or c.shape != table.shape or not np.array_equal(o, offsets) or not np.array_equal(c, table):
        raise ValueError("corner table: corner_offsets / corners are not the transposed table of faces (deodr_amd.surface.corner_table)")


def closest_point_torch(p, a, b, c):
    """the sequence of ``include/deodr_hip_surface.h`` on broadcastable [..., 3] tensors -> (v, w, e [..., 3], d2): each torch op rounds once"""
    dot = lambda x, y: (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e_ab, e_ac, e_b, e_c = d1 - d3, d2 - d6, d4 - d3, d5 - d6
    e_bc, den = e_b + e_c, (va + vb) + vc
    A = (d1 <= 0) & (d2 <= 0)
    taken = A
    B = ~taken & (d3 >= 0) & (d4 <= d3)
    taken = taken | B
    AB = ~taken & (vc <= 0) & (d1 >= 0) & (d3 <= 0) & (e_ab > 0)
    taken = taken | AB
    C = ~taken & (d6 >= 0) & (d5 <= d6)
    taken = taken | C
    AC = ~taken & (vb <= 0) & (d2 >= 0) & (d6 <= 0) & (e_ac > 0)
    taken = taken | AC
    BC = ~taken & (va <= 0) & (e_b >= 0) & (e_c >= 0) & (e_bc > 0)
    inside = ~(taken | BC) & (den != 0)
    zero, one = torch.zeros_like(d1), torch.ones_like(d1)
    where = torch.where
    v_num, v_den = where(B, one, where(AB, d1, where(inside, vb, zero))), where(AB, e_ab, where(inside, den, one))
    w_num = where(C, one, where(AC, d2, where(BC, e_b, where(inside, vc, zero))))
    w_den = where(AC, e_ac, where(BC, e_bc, where(inside, den, one)))
    w = w_num / w_den
    v = where(BC, 1 - w, v_num / v_den)
    e = ((a + v[..., None] * ab) + w[..., None] * ac) - p
    return v, w, e, (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def _nearest_face(p, tri, chunk_bytes):
    """p [n,P,3], tri = (a, b, c) [n,F,3] -> (d2 [n,P], face [n,P] int64, v, w [n,P], e [n,P,3]) of the closest face, the lowest index of a tie"""
    n, P, F = int(p.shape[0]), int(p.shape[1]), int(tri[0].shape[1])
    chunk = max(1, int(chunk_bytes // (p.element_size() * F * n * LIVE_ARRAYS)))
    parts = []
    for at in range(0, P, chunk):
        q = p[:, at : at + chunk, None, :]
        v, w, e, d2 = closest_point_torch(q, *(t[:, None, :, :] for t in tri))
        best, face = d2.min(dim=2)  # (torch.min: the first minimal value)
        pick = lambda x: torch.gather(x, 2, face[..., None])[..., 0]
        parts.append((best, face, pick(v), pick(w), torch.stack([pick(e[..., x]) for x in range(3)], dim=-1)))
    return tuple(torch.cat(column, dim=1) for column in zip(*parts))


def surface_distance_torch(vertices, faces, points, params, point_weights=None, vertex_weights=None, directions=3, chunk_bytes=CHUNK_BYTES):
    """the operation of ``include/deodr_hip_surface.h`` as torch ops, in the dtype of ``vertices`` [n,V,3] -> (terms [n,2], loss [n], vertices_b
    [n,V,3], nearest_face [n,P] | None, barycentric [n,P,3] | None, nearest_point [n,V] | None; the indices int64).  ``faces`` [F,3] integers;
    ``params`` [3] = (mix_0, mix_1, max_distance), a tensor; about ``chunk_bytes`` of intermediate values exist at once.  The sums of the gradient
    are ``index_add_``'s, not in the kernels' order.  No autograd: see :class:`deodr_amd.fronthalf.SurfaceDistanceFunc`."""
    with torch.no_grad():
        v, p = vertices, points.to(vertices.dtype)
        n, P = int(v.shape[0]), int(p.shape[1])
        faces = torch.as_tensor(faces, device=v.device).long()
        params = params.to(v.dtype)
        mix0, mix1, tau2 = params[0], params[1], params[2] * params[2]
        terms, g = torch.zeros((n, 2), dtype=v.dtype, device=v.device), torch.zeros_like(v)
        nearest_face = barycentric = nearest_point = None
        if directions & 1:
            w = torch.ones((n, P), dtype=v.dtype, device=v.device) if point_weights is None else point_weights.to(v.dtype)
            d2, nearest_face, bv, bw, e = _nearest_face(p, tuple(v[:, faces[:, c], :] for c in range(3)), chunk_bytes)
            barycentric = torch.stack(((1 - bv) - bw, bv, bw), dim=-1)
            near = d2 <= tau2
            terms[:, 0] = (w * torch.where(near, d2, tau2)).sum(dim=1)
            pull = ((2 * w)[..., None] * barycentric)[..., None] * e[:, :, None, :]  # [n,P,3 corners,3]
            pull = torch.where(near[..., None, None], pull, torch.zeros_like(pull))
            corners = faces[nearest_face]  # [n,P,3]: the vertex of every corner
            for b in range(n):
                g[b].index_add_(0, corners[b].reshape(-1), mix0 * pull[b].reshape(-1, 3))
        if directions & 2:
            nearest_point = _mesh_to_points(v, p, vertex_weights, mix1, tau2, terms, g, chunk_bytes)
        loss = (mix0 * terms[:, 0] if directions & 1 else 0) + (mix1 * terms[:, 1] if directions & 2 else 0)
        return terms, loss, g, nearest_face, barycentric, nearest_point


class PointSurfaceTerm(PointCloudTerm):
    """The point-to-surface energy of posed vertices [n,V,3] with the triangles ``faces`` [F,3] against one point cloud per pose, on a device.

    ``faces``: integers in ``[0, nb_vertices)``, checked here; the transposed corner table the kernels need is built here too
    (:func:`corner_table`).  Everything else -- ``points``, the padding of clouds of unequal length (copies of the first point at weight 0),
    ``point_weights``, ``vertex_weights`` (of mesh -> points), ``directions``, ``max_distance``, ``mix``, ``normalise``, the device tensors
    ``self.params``, ``self.points`` and the weights that may be ``copy_``-ed into between calls and replays -- is :class:`PointCloudTerm`'s.

    ``search``: "brute" (the default: every (point, face) pair is visited, F * P is capped) or "grid": the same faces over a uniform grid of
    triangles (``deodr_hip_surface_grid``) and the nearest points of mesh -> points over the points' grid; the same barycentric coordinates, loss
    and terms, the gradient up to the order of its sums (on CPU tensors: the same bits), no cap on F * P or V * P.  The rules and messages are
    :class:`PointCloudTerm`'s: a finite ``max_distance`` -- refused here otherwise, and at a call when it was ``copy_``-ed into ``params`` where the
    host can see it --, ``cell_size`` finite and > 0 and only with the grid (None: :func:`deodr_amd.chamfer.default_cell_size` of the clouds; the
    kernels never use a cell below ``max_distance / 4`` or below the longest side of a face's bounding box), and :meth:`correspondences` gives -1
    and zero barycentric coordinates where there is no face within ``max_distance``."""

    def __init__(self, faces, nb_vertices, points, point_weights=None, vertex_weights=None, directions="both", max_distance=float("inf"), mix=(1.0, 1.0),
                 normalise=True, device="cuda", search="brute", cell_size=None):  # fmt: skip
        super().__init__(points, point_weights, vertex_weights, directions, max_distance, mix, normalise, device, search=search, cell_size=cell_size)
        offsets, corners = corner_table(faces, nb_vertices)
        self.nb_vertices, self.nb_faces = int(nb_vertices), int(len(corners) // 3)
        self.faces = torch.as_tensor(np.ascontiguousarray(np.asarray(_array(faces)), dtype=np.int32), device=self.device)
        self.corner_offsets, self.corners = torch.as_tensor(offsets, device=self.device), torch.as_tensor(corners, device=self.device)

    def _posed(self, vertices):
        vertices = super()._posed(vertices)
        if int(vertices.shape[1]) != self.nb_vertices:
            raise ValueError(f"PointSurfaceTerm: the faces are those of {self.nb_vertices} vertices, not of {int(vertices.shape[1])}")
        return vertices

    # :meth:`evaluate_no_grad` is PointCloudTerm's with these two: -> (terms [n,2], loss [n], vertices_b [n,V,3], nearest_face [n,P] | None, barycentric
    # [n,P,3] | None, nearest_point [n,V] | None), ``deodr_hip_surface_distance`` on float64 ROCm tensors, :func:`surface_distance_torch` elsewhere (the
    # indices int64 either way); :meth:`evaluate` is PointCloudTerm's as it stands (the adjoint of the loss is the ``vertices_b`` of the same call)
    def _torch(self, v, u, want_nearest):
        to = lambda t: None if t is None else t.to(v.device)
        faces, points, params = to(self.faces), to(self.points), to(self.params)
        out = surface_distance_torch(v, faces, points, params, to(self.point_weights), to(u), self.directions)
        if not want_nearest:
            return out[:3] + (None, None, None)
        if self.search == "grid":  # the same values; the correspondences beyond max_distance are none
            p, face, bary, nearest_point = points.to(v.dtype), out[3], out[4], out[5]
            if face is not None:
                a, b, c = (torch.gather(v, 1, faces.long()[face][..., k, None].expand(-1, -1, 3)) for k in range(3))
                e = ((a + bary[..., 1:2] * (b - a)) + bary[..., 2:3] * (c - a)) - p  # the header's closest point, operation by operation
                tau2 = params[2].to(v.dtype) * params[2].to(v.dtype)
                near = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2] <= tau2
                face, bary = torch.where(near, face, torch.full_like(face, -1)), torch.where(near[..., None], bary, torch.zeros_like(bary))
            out = out[:3] + (face, bary, None if nearest_point is None else mask_beyond(v, p, nearest_point, params))
        return out

    def _kernel(self, hr, V):
        mesh = (self.faces, self.corner_offsets, self.corners)
        if self.search == "grid":
            return hr.surface_grid_scratch, (V, self.nb_faces, self.nb_points, self.n), hr.surface_grid, mesh + (self.points, self.params, self.cell_size)
        return hr.surface_scratch, (V, self.nb_faces, self.nb_points, self.n), hr.surface_distance, mesh + (self.points, self.params)

    def correspondences(self, vertices):
        """-> (nearest_face [n,P] | None, barycentric [n,P,3] | None, nearest_point [n,V] | None): the closest face of every point and the
        barycentric coordinates of its closest point on it (None without points -> mesh; a padded point has those of its cloud's first point), the
        nearest point of every vertex (None without mesh -> points); the indices int64"""
        return self.evaluate_no_grad(vertices, want_nearest=True)[3:]
