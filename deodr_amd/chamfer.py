"""The closest-point (ICP / Chamfer) data term on the device: a mesh against an unorganised 3-D point set -- a fused scan, a LiDAR sweep, a depth
image back-projected with somebody else's camera model, the vertices of another mesh.

``loss = mix_0 sum_k w_k min(|p_k - v_j*(k)|^2, tau^2) + mix_1 sum_i u_i min(|v_i - p_k*(i)|^2, tau^2)``: every point pulls its nearest vertex
(points -> mesh: what a partial scan needs), every vertex is pulled to its nearest point (mesh -> points), pairs further apart than
``max_distance`` pay a constant and pull nothing (the truncated ICP rule).  ``include/deodr_hip_chamfer.h`` has the operation,
``deodr_amd/csrc/dr_chamfer.h`` the kernels: a brute-force tiled nearest-neighbour search both ways and the gradient gathered in the same walk,
without lists and without floating-point atomics -- a fixed number of launches, nothing read back, the same bits from run to run, so it runs
inside a captured graph.

:class:`PointCloudTerm` holds the clouds, the weights and the device-resident ``params`` and evaluates, differentiably; :func:`chamfer_torch` is
the same definition as torch ops, chunked over the queries -- what runs on tensors the kernels do not take (CPU tensors, other dtypes) and what
the kernels are timed against; :func:`depth_to_points` back-projects a depth image.  ``deodr_amd.pytorch.MeshPointCloudFitter`` fits with it.

``PointCloudTerm(search="grid")`` finds the same neighbours over a uniform grid of hashed cells (``include/deodr_hip_chamfer_grid.h``,
``deodr_amd/csrc/dr_chamfer_grid.h``): the cost grows with V + P instead of V * P and there is no cap on V * P; it needs a finite
``max_distance``, and a query with nothing within it has no correspondence (-1)."""

import math

import numpy as np
import torch

DIRECTIONS = {"points_to_mesh": 1, "mesh_to_points": 2, "both": 3}
SEARCHES = ("brute", "grid")
CHUNK_BYTES = 64 << 20  # of distances that exist at once in chamfer_torch


def _d2(a, b):
    """[n,A,1,3] x [n,1,B,3] -> [n,A,B]: the expression of the header, each operation rounded"""
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _nearest(queries, refs, chunk_bytes):
    """-> (d2 [n,Q], index [n,Q] int64) of the nearest reference of every query, the lowest index of a tie, chunked over the queries"""
    n, Q, R = int(queries.shape[0]), int(queries.shape[1]), int(refs.shape[1])
    chunk = max(1, int(chunk_bytes // (queries.element_size() * R * n)))
    best, arg = [], []
    for at in range(0, Q, chunk):
        d2, idx = _d2(queries[:, at : at + chunk, None, :], refs[:, None, :, :]).min(dim=2)  # (torch.min: the first minimal value)
        best.append(d2), arg.append(idx)
    return torch.cat(best, dim=1), torch.cat(arg, dim=1)


def _mesh_to_points(v, p, vertex_weights, mix1, tau2, terms, g, chunk_bytes):
    """mesh -> points of :func:`chamfer_torch` and :func:`deodr_amd.surface.surface_distance_torch`: term_1 -> ``terms[:, 1]``, its gradient added
    to ``g``; -> nearest_point [n,V]"""
    u = torch.ones(int(v.shape[1]), dtype=v.dtype, device=v.device) if vertex_weights is None else vertex_weights.to(v.dtype)
    d2, nearest_point = _nearest(v, p, chunk_bytes)
    near = d2 <= tau2
    terms[:, 1] = (u[None] * torch.where(near, d2, tau2)).sum(dim=1)
    g += mix1 * ((2 * u[None] * near)[..., None] * (v - torch.gather(p, 1, nearest_point[..., None].expand(-1, -1, 3))))
    return nearest_point


def chamfer_torch(vertices, points, params, point_weights=None, vertex_weights=None, directions=3, chunk_bytes=CHUNK_BYTES):
    """the operation of ``include/deodr_hip_chamfer.h`` as torch ops, in the dtype of ``vertices`` [n,V,3] -> (terms [n,2], loss [n], vertices_b
    [n,V,3], nearest_vertex [n,P] | None, nearest_point [n,V] | None, int64).  ``params`` [3] = (mix_0, mix_1, max_distance), a tensor; no more
    than about ``chunk_bytes`` of distances exist at once.  No autograd: see :class:`deodr_amd.fronthalf.ChamferFunc`."""
    with torch.no_grad():
        v, p = vertices, points.to(vertices.dtype)
        n, P = int(v.shape[0]), int(p.shape[1])
        params = params.to(v.dtype)
        mix0, mix1, tau2 = params[0], params[1], params[2] * params[2]
        terms, g = torch.zeros((n, 2), dtype=v.dtype, device=v.device), torch.zeros_like(v)
        nearest_vertex = nearest_point = None
        if directions & 1:
            w = torch.ones((n, P), dtype=v.dtype, device=v.device) if point_weights is None else point_weights.to(v.dtype)
            d2, nearest_vertex = _nearest(p, v, chunk_bytes)
            near = d2 <= tau2
            terms[:, 0] = (w * torch.where(near, d2, tau2)).sum(dim=1)
            pull = (2 * w * near)[..., None] * (torch.gather(v, 1, nearest_vertex[..., None].expand(-1, -1, 3)) - p)
            g += mix0 * torch.zeros_like(v).scatter_add_(1, nearest_vertex[..., None].expand(-1, -1, 3), pull)
        if directions & 2:
            nearest_point = _mesh_to_points(v, p, vertex_weights, mix1, tau2, terms, g, chunk_bytes)
        loss = (mix0 * terms[:, 0] if directions & 1 else 0) + (mix1 * terms[:, 1] if directions & 2 else 0)
        return terms, loss, g, nearest_vertex, nearest_point


def mask_beyond(queries, refs, nearest, params):
    """``nearest`` [n,Q] (int64, into ``refs`` [n,R,3]) with -1 where the header's d2 of the pair is above ``params[2] ** 2``: what the grid search
    reports for a query with no neighbour within ``max_distance``"""
    tau2 = params[2].to(queries.dtype) * params[2].to(queries.dtype)
    d = queries - torch.gather(refs, 1, nearest[..., None].expand(-1, -1, 3))
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return torch.where(d2 <= tau2, nearest, torch.full_like(nearest, -1))


def default_cell_size(clouds):
    """the cell size of ``search="grid"`` when none is given, from the clouds alone (nothing that moves): twice the spacing the points of a cloud
    would have if they covered half the surface of its bounding box evenly, ``2 sqrt((e0 e1 + e1 e2 + e0 e2) / P)`` with e the extents of the box
    -- a cell then holds a handful of the points of a scanned surface --, the largest over the clouds; 1 for clouds without extent.  Reasoned,
    not swept; the kernels never use a cell below ``max_distance / 4`` whatever this gives."""
    sizes = []
    for c in clouds:
        e = c.max(axis=0) - c.min(axis=0)
        sizes.append(2.0 * math.sqrt(float(e[0] * e[1] + e[1] * e[2] + e[0] * e[2]) / len(c)))
    size = max(sizes)
    return size if size > 0 and math.isfinite(size) else 1.0


def _array(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


class PointCloudTerm:
    """The closest-point energy of posed vertices [n,V,3] against one point cloud per pose, on a device.

    ``points``: a [P,3] cloud (n = 1), [n,P,3] clouds, or a list of n clouds of different lengths -- those are padded to the longest with copies of
    their first point at weight 0 (a copy never wins the nearest-point search: the lowest index does).  ``point_weights``: per point, of the shape
    of ``points`` without its last axis (a list for a list), ``>= 0``, None: ones.  ``vertex_weights`` [V] ``>= 0``, shared by the poses, None: ones.
    ``directions``: "both", "points_to_mesh" (a partial scan: half the work) or "mesh_to_points".  ``max_distance > 0`` (inf: no truncation),
    ``mix`` = (mix_0, mix_1).  ``normalise``: every weight vector is divided by its sum, so both terms are weighted mean squared distances.
    Checked here, on the host, because the kernels cannot: finite coordinates, finite weights ``>= 0`` with a positive sum, ``max_distance``,
    ``mix``.  ``self.params`` [3] = (mix_0, mix_1, max_distance), ``self.points`` and the weights are device tensors read when the kernels run:
    ``copy_`` other values into them between calls, also between replays of a captured graph (they are not checked again).

    ``search``: "brute" (the default: every pair is visited, V * P is capped) or "grid": the same neighbours over a uniform grid of cells
    (``deodr_hip_chamfer_grid``); the same loss, terms and gradient up to the order of the sums (on CPU tensors: the same bits), no cap on V * P.
    The grid needs a finite ``max_distance`` -- an infinite one is refused here, and at a call when it was ``copy_``-ed into ``params`` where the
    host can see it (CPU tensors) --, and :meth:`correspondences` gives -1 for a query with nothing within ``max_distance``.  ``cell_size`` > 0:
    the cells' edge (the kernels use ``max(cell_size, max_distance / 4)``); None: :func:`default_cell_size` of the clouds, evaluated once here."""

    def __init__(self, points, point_weights=None, vertex_weights=None, directions="both", max_distance=math.inf, mix=(1.0, 1.0), normalise=True, device="cuda",
                 search="brute", cell_size=None):  # fmt: skip
        what = "PointCloudTerm"
        if directions not in DIRECTIONS:
            raise ValueError(f'{what}: directions must be "both", "points_to_mesh" or "mesh_to_points", not {directions!r}')
        if search not in SEARCHES:
            raise ValueError(f'{what}: search must be "brute" or "grid", not {search!r}')
        if cell_size is not None and search != "grid":
            raise ValueError(f'{what}: cell_size belongs to search="grid"')
        if cell_size is not None and not (float(cell_size) > 0 and math.isfinite(float(cell_size))):
            raise ValueError(f"{what}: cell_size must be finite and > 0, not {cell_size}")
        self.search = search
        self.device, self.directions, self.normalise = torch.device(device), DIRECTIONS[directions], bool(normalise)
        max_distance, mix = float(max_distance), tuple(float(m) for m in mix)
        if not max_distance > 0:  # (a NaN is refused as well)
            raise ValueError(f"{what}: max_distance must be > 0 (inf: no truncation), not {max_distance}")
        if search == "grid" and not math.isfinite(max_distance):
            raise ValueError(f'{what}: search="grid" needs a finite max_distance (only neighbours within it are looked for), not {max_distance}')
        if len(mix) != 2 or not all(math.isfinite(m) for m in mix):
            raise ValueError(f"{what}: mix must be two finite values, not {mix}")
        if isinstance(points, (list, tuple)):
            clouds = [np.asarray(_array(c), dtype=np.float64) for c in points]
            weights = [None] * len(clouds) if point_weights is None else list(point_weights)
            if len(weights) != len(clouds):
                raise ValueError(f"{what}: {len(weights)} weight vectors for {len(clouds)} clouds")
        else:
            clouds = np.asarray(_array(points), dtype=np.float64)
            clouds = [clouds] if clouds.ndim == 2 else list(clouds) if clouds.ndim == 3 else [np.zeros((0,))]
            w = None if point_weights is None else np.asarray(_array(point_weights), dtype=np.float64)
            weights = [None] * len(clouds) if w is None else [w] if w.ndim == 1 else list(w)
            if len(weights) != len(clouds):
                raise ValueError(f"{what}: point_weights must have the shape of points without its last axis")
        if not clouds or any(c.ndim != 2 or c.shape[1] != 3 or c.shape[0] < 1 for c in clouds):
            raise ValueError(f"{what}: points must be [P >= 1, 3], [n >= 1, P >= 1, 3] or a list of [P_i >= 1, 3] clouds")
        self.n, self.lengths = len(clouds), [len(c) for c in clouds]
        P = max(self.lengths)
        pts, w = np.empty((self.n, P, 3)), np.zeros((self.n, P))
        for b, (c, cw) in enumerate(zip(clouds, weights)):
            if not np.all(np.isfinite(c)):
                raise ValueError(f"{what}: the coordinates of the points must be finite")
            cw = np.ones(len(c)) if cw is None else np.asarray(_array(cw), dtype=np.float64)
            if cw.shape != (len(c),):
                raise ValueError(f"{what}: cloud {b} has {len(c)} points and weights of shape {list(cw.shape)}")
            w[b, : len(c)] = self._weights(cw, "point_weights")
            pts[b, : len(c)], pts[b, len(c) :] = c, c[0]
        self.nb_points = P
        self.cell_size = None if search != "grid" else float(cell_size) if cell_size is not None else default_cell_size(clouds)
        self.points, self.point_weights = torch.as_tensor(pts, device=self.device), torch.as_tensor(w, device=self.device)
        self.vertex_weights = None
        if vertex_weights is not None:
            u = np.asarray(_array(vertex_weights), dtype=np.float64)
            if u.ndim != 1:
                raise ValueError(f"{what}: vertex_weights must be [V], not {list(u.shape)}")
            self.vertex_weights = torch.as_tensor(self._weights(u, "vertex_weights"), device=self.device)
        self.params = torch.tensor([mix[0], mix[1], max_distance], dtype=torch.float64, device=self.device)
        self._scratch = {}  # (n, V) -> the kernels' scratch.  Per shape, not per stream: a captured step has to find the one the eager steps made

    def _weights(self, w, name):
        if not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError(f"PointCloudTerm: {name} must be finite and >= 0")
        if self.normalise:
            if not w.sum() > 0:
                raise ValueError(f"PointCloudTerm: {name} sum to 0, they cannot be normalised")
            w = w / w.sum()
        return w

    def _vertex_weights(self, V):
        """[V] (None: ones in the kernels); with ``normalise`` and no weights given, 1 / V -- made at the first call (not inside a graph capture)"""
        if self.vertex_weights is None and self.normalise:
            self.vertex_weights = torch.full((V,), 1.0 / V, dtype=torch.float64, device=self.device)
        if self.vertex_weights is not None and int(self.vertex_weights.shape[0]) != V:
            raise ValueError(f"PointCloudTerm: {int(self.vertex_weights.shape[0])} vertex weights for {V} vertices")
        return self.vertex_weights

    def uses_kernel(self, vertices):
        """does :meth:`evaluate` run the kernels on these vertices (a float64 ROCm tensor on this term's device)?"""
        return torch.is_tensor(vertices) and vertices.is_cuda and vertices.dtype == torch.float64 and vertices.device == self.points.device

    def _posed(self, vertices):
        if vertices.dim() == 2:  # one mesh against every cloud
            vertices = vertices[None].expand(self.n, -1, -1)
        if vertices.dim() != 3 or int(vertices.shape[0]) != self.n or vertices.shape[1] < 1 or vertices.shape[2] != 3:
            raise ValueError(f"PointCloudTerm: vertices must be [V, 3] or [{self.n}, V, 3] (one pose per cloud), not {list(vertices.shape)}")
        return vertices

    def _torch(self, v, u, want_nearest):
        """:meth:`evaluate_no_grad` on tensors the kernels do not take"""
        to = lambda t: None if t is None else t.to(v.device)
        points, params = to(self.points), to(self.params)
        out = chamfer_torch(v, points, params, to(self.point_weights), to(u), self.directions)
        if not want_nearest:
            return out[:3] + (None, None)
        if self.search == "grid":  # the same values; the correspondences beyond max_distance are none
            p = points.to(v.dtype)
            out = out[:3] + (None if out[3] is None else mask_beyond(p, v, out[3], params), None if out[4] is None else mask_beyond(v, p, out[4], params))
        return out

    def _kernel(self, hr, V):
        """-> (the function that makes the scratch, its dimensions, the operator, its arguments between the vertices and the weights)"""
        if self.search == "grid":
            return hr.chamfer_grid_scratch, (V, self.nb_points, self.n), hr.chamfer_grid, (self.points, self.params, self.cell_size)
        return hr.chamfer_scratch, (V, self.nb_points, self.n), hr.chamfer, (self.points, self.params)

    def evaluate_no_grad(self, vertices, want_nearest=False):
        """(terms [n,2], loss [n], vertices_b [n,V,3], nearest_vertex [n,P] | None, nearest_point [n,V] | None) without autograd:
        ``deodr_hip_chamfer`` on float64 ROCm tensors, :func:`chamfer_torch` elsewhere (the indices int64 either way)"""
        v = self._posed(vertices).detach().contiguous()
        V = int(v.shape[1])
        u = self._vertex_weights(V)
        grid = self.search == "grid"
        if grid and not self.params.is_cuda and not math.isfinite(float(self.params[2])):
            raise ValueError('PointCloudTerm: search="grid" needs a finite max_distance, params[2] is not')
        if not self.uses_kernel(v):
            return self._torch(v, u, want_nearest)
        from . import hip_renderer as hr

        key = ("grid", self.n, V) if grid else (self.n, V)
        make_scratch, dims, operator, args = self._kernel(hr, V)
        if key not in self._scratch:
            self._scratch[key] = make_scratch(*dims, v.device)
        out = operator(v, *args, self.point_weights, u, self.directions, scratch=self._scratch[key], want_nearest=want_nearest)
        # the indices: below 2^31, the bit patterns are the values; NONE of the grid, all bits set, is -1
        return tuple(t.long() if t is not None and t.dtype == torch.int32 else t for t in out)

    def evaluate(self, vertices):
        """-> (loss [n], terms [n,2]) of ``vertices`` [n,V,3] (or [V,3]: the same mesh against every cloud).  The loss is differentiable in the
        vertices (its adjoint is the ``vertices_b`` the same call produced: exact wherever every nearest neighbour is unique and no pair sits at
        ``max_distance``); the terms are returned for display and marked non-differentiable -- asking autograd for their gradient is refused by
        torch ("does not require grad").  Calls of one shape must not run on two streams at once (they share a scratch)."""
        from . import fronthalf

        return fronthalf.ChamferFunc.apply(self._posed(vertices), self)

    def correspondences(self, vertices):
        """-> (nearest_vertex [n,P] | None, nearest_point [n,V] | None), int64: the index of the nearest vertex of every point (None without points ->
        mesh; a padded point has the one of its cloud's first point) and of the nearest point of every vertex (None without mesh -> points); with
        ``search="grid"`` -1 where nothing lies within ``max_distance``"""
        return self.evaluate_no_grad(vertices, want_nearest=True)[3:]


def depth_to_points(depth, camera, mask=None, integer_pixel_centers=True):
    """Back-project a depth image (the z coordinate in the camera's frame, as ``DeviceCamera.project_points`` returns it) of a distortion-free
    :class:`deodr_amd.scene3d.DeviceCamera` into world coordinates.  ``depth`` [H,W] with a camera of one view -> [P,3]; [n,H,W] -> a list of n
    clouds.  ``mask`` (the shape of ``depth``, bool; None: where the depth is finite and > 0) selects the pixels.  The centre of pixel (row r,
    column c) is (x, y) = (c, r) (``integer_pixel_centers``, the rasterizer's default) or (c + 0.5, r + 0.5).  A camera with distortion is
    refused: its projection has no closed-form inverse."""
    if camera.distortion is not None and bool((camera.distortion != 0).any()):
        raise ValueError("depth_to_points: the camera has distortion; undistort the depth image first")
    d = torch.as_tensor(_array(depth), dtype=camera.dtype, device=camera.device)
    single = d.dim() == 2
    d = d[None] if single else d
    if d.dim() != 3 or tuple(d.shape) != (camera.n_views, camera.height, camera.width):
        raise ValueError(f"depth_to_points: depth must be [{camera.height}, {camera.width}] per view of the camera ({camera.n_views}), not {list(d.shape)}")
    keep = (torch.isfinite(d) & (d > 0)) if mask is None else torch.as_tensor(_array(mask), device=camera.device).bool().reshape(d.shape)
    offset = 0.0 if integer_pixel_centers else 0.5
    rows, cols = torch.meshgrid(torch.arange(camera.height, dtype=camera.dtype, device=camera.device) + offset,
                                torch.arange(camera.width, dtype=camera.dtype, device=camera.device) + offset, indexing="ij")  # fmt: skip
    pixels = torch.stack((cols, rows, torch.ones_like(rows)), dim=-1).reshape(-1, 3)  # (x = column first)
    clouds = []
    for b in range(camera.n_views):
        rays = pixels @ torch.linalg.inv(camera.intrinsic[b]).T  # z = 1
        in_camera = rays * d[b].reshape(-1, 1)
        world = (in_camera - camera.extrinsic[b, :, 3]) @ camera.extrinsic[b, :, :3]  # R^T (x - t)
        clouds.append(world[keep[b].reshape(-1)])
    return clouds[0] if single else clouds
