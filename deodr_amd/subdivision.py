"""Loop subdivision as a linear map on the device: fine vertices = ``S control``, adjoint = ``S^T gradient``.

The reference subdivides a mesh on the host with SciPy products, one level per call (``loop_subdivision``,
deodr/triangulated_mesh.py:499-562).  The connectivity never changes during a fit, so here the ``k`` levels are composed ONCE, on the host,
into one sparse matrix ``S = S_k ... S_1`` [Vf, Vc]; on the device a subdivision, whatever ``k``, is one launch of ``deodr_hip_subdiv_apply``
with the rows of ``S`` and its adjoint one launch with the rows of ``S^T`` (include/deodr_hip_subdiv.h, kernel in csrc/dr_subdiv.h).
That makes the control cage of a subdivision surface a parameter the fitters can optimise (``subdivisions=k``, deodr_amd/mesh_fitter.py).

Vertex and face order are the reference's: new vertices = [moved old vertices ; edge points in edge-id order] (the edge numbering of
:class:`MeshTopology` is the reference's ``id_edge``), faces = the four stacked blocks of triangulated_mesh.py:521-549.

Rules.  Closed manifold meshes: the reference's -- even vertex ``5/8 v + (3/8)/deg sum(neighbours)``, edge point ``3/8 (a + b) + 1/8 (c + d)``.
Manifold meshes with a boundary: the STANDARD boundary rules, edge point ``1/2 (a + b)``, boundary vertex ``3/4 v + 1/8 (previous + next along
the boundary)`` -- the reference's formula gives a boundary edge point the weights 2/8, 2/8, 1/8, which sum to 5/8: not an affine map (DESIGN.md
section 6).  Refused: an edge with more than two faces, a vertex on more than two boundary edges, a vertex no face references.
Colours follow the reference (:552-554): old colours kept, an edge point gets the mean of its two ends (not Loop-smoothed).
"""

import numpy as np
import scipy.sparse as sp
import torch


def _edges(faces, nb_vertices):
    """-> (edge end points [E,2] with a < b, edge id of every face slot [T,3] in the slot order (v0,v1), (v1,v2), (v2,v0), faces per edge [E]);
    the numbering of MeshTopology and of the reference's ``id_edge`` (triangulated_mesh.py:104-111): np.unique of min * V + max"""
    e = np.concatenate((faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]))  # slot-major [3T,2]
    key = np.minimum(e[:, 0], e[:, 1]) * nb_vertices + np.maximum(e[:, 0], e[:, 1])
    keys, edge_id, counts = np.unique(key, return_inverse=True, return_counts=True)
    return np.column_stack((keys // nb_vertices, keys % nb_vertices)), edge_id.reshape(3, -1).T, counts


def loop_subdivision_level(faces, nb_vertices):
    """One level: -> (S [V + E, V] CSR, colours matrix [V + E, V] CSR, fine faces [4T,3]) of a manifold mesh, with or without a boundary."""
    f = np.asarray(faces).astype(np.int64)
    if f.ndim != 2 or f.shape[1] != 3 or len(f) == 0:
        raise ValueError("loop subdivision: faces must be a non-empty [T,3] array")
    V, T = int(nb_vertices), len(f)
    if f.min() < 0 or f.max() >= V:
        raise ValueError("loop subdivision: a face refers to a vertex that does not exist")
    edges, face_edge, counts = _edges(f, V)
    E = len(edges)
    if np.any(counts > 2):
        raise ValueError(f"loop subdivision: edge {tuple(edges[np.argmax(counts > 2)])} belongs to more than two faces (not a manifold mesh)")
    referenced = np.zeros(V, dtype=bool)
    referenced[f.reshape(-1)] = True
    if not referenced.all():
        raise ValueError(f"loop subdivision: vertex {int(np.argmin(referenced))} is referenced by no face")
    boundary_edge = counts == 1
    nb_boundary = np.bincount(edges[boundary_edge].reshape(-1), minlength=V)
    if np.any(nb_boundary > 2):
        raise ValueError(f"loop subdivision: vertex {int(np.argmax(nb_boundary > 2))} lies on more than two boundary edges (not a manifold mesh)")
    # (a vertex on exactly one boundary edge cannot exist: the boundary edges of a union of triangles form closed loops)
    boundary_vertex = nb_boundary > 0
    a, b = edges[:, 0], edges[:, 1]
    degree = np.bincount(edges.reshape(-1), minlength=V)  # number of neighbours (the reference's degree_v_e)
    rows, cols, vals = [], [], []

    def add(r, c, v):
        rows.append(np.asarray(r)), cols.append(np.asarray(c)), vals.append(np.broadcast_to(np.asarray(v, dtype=np.float64), np.shape(r)))

    # even (old) vertices
    inner = np.flatnonzero(~boundary_vertex)
    add(inner, inner, 5 / 8)
    beta = (3 / 8) * (1 / degree)
    for p, q in ((a, b), (b, a)):  # every neighbour q of p, once per edge
        keep = ~boundary_vertex[p]
        add(p[keep], q[keep], beta[p[keep]])
        keep = boundary_vertex[p] & boundary_edge  # a boundary vertex sees its two neighbours along the boundary only
        add(p[keep], q[keep], 1 / 8)
    rim = np.flatnonzero(boundary_vertex)
    add(rim, rim, 3 / 4)
    # odd vertices (edge points)
    ie = np.flatnonzero(~boundary_edge)
    add(V + ie, a[ie], 1 / 8), add(V + ie, b[ie], 1 / 8)  # 1/8 (a + b), and 1/8 of the three corners of each of the two faces: 3/8 (a + b) + 1/8 (c + d)
    slot_inner = ~boundary_edge[face_edge]  # [T,3]
    for s in range(3):
        t = np.flatnonzero(slot_inner[:, s])
        for corner in range(3):
            add(V + face_edge[t, s], f[t, corner], 1 / 8)
    be = np.flatnonzero(boundary_edge)
    add(V + be, a[be], 1 / 2), add(V + be, b[be], 1 / 2)
    S = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(V + E, V)).tocsr()  # (duplicates are summed)
    every = np.arange(E)
    colors = sp.coo_matrix((np.concatenate((np.ones(V), np.full(2 * E, 0.5))), (np.concatenate((np.arange(V), V + every, V + every)),
                                                                                np.concatenate((np.arange(V), a, b)))), shape=(V + E, V)).tocsr()  # fmt: skip
    fe = face_edge + V
    fine = np.vstack((np.column_stack((f[:, 0], fe[:, 0], fe[:, 2])), np.column_stack((f[:, 1], fe[:, 1], fe[:, 0])),
                      np.column_stack((f[:, 2], fe[:, 2], fe[:, 1])), np.column_stack((fe[:, 0], fe[:, 1], fe[:, 2]))))  # fmt: skip
    assert fine.shape == (4 * T, 3)
    return S, colors, fine


def _checked_csr(m):
    """a SciPy matrix as CSR with sorted columns, its tables checked as ``deodr_hip_subdiv_apply`` expects them (it cannot check device memory)"""
    m = sp.csr_matrix(m)
    m.sum_duplicates()
    m.sort_indices()
    if m.nnz == 0 or m.nnz >= 2**32 or m.indptr[0] != 0 or m.indptr[-1] != m.nnz or np.any(np.diff(m.indptr) < 0):
        raise ValueError("sparse operator: row offsets are not a non-decreasing sequence from 0 to nnz")
    if m.indices.min() < 0 or m.indices.max() >= m.shape[1]:
        raise ValueError("sparse operator: a column index is out of range")
    return m


class SparseOperator:
    """A fixed sparse matrix ``A`` [rows, columns] as a differentiable map ``x [..., columns, D] -> A x [..., rows, D]`` (leading dimensions are
    a batch).  On float32 / float64 ROCm tensors: ``deodr_hip_subdiv_apply`` with the rows of ``A``, and with the rows of ``A^T`` in the backward
    pass.  On anything else (CPU tensors: the CPU suite; other dtypes) the same map as torch ops over the COO triplets."""

    def __init__(self, matrix, device):
        self.matrix = _checked_csr(matrix)
        self.transposed = _checked_csr(self.matrix.T)
        self.device = torch.device(device)
        self._csr, self._coo = {}, {}

    def _of(self, transposed):
        return self.transposed if transposed else self.matrix

    def csr_tables(self, transposed=False, device=None):
        """-> (offsets u32 [rows + 1], cols u32 [nnz], vals f64 [nnz]) on the device (uint32 bit patterns in int32 tensors, as MeshTopology's)"""
        device = self.device if device is None else torch.device(device)
        if (transposed, device) not in self._csr:
            m = self._of(transposed)
            u32 = lambda a: torch.as_tensor(np.ascontiguousarray(a).astype(np.uint32).view(np.int32), device=device)
            self._csr[(transposed, device)] = (u32(m.indptr), u32(m.indices), torch.as_tensor(m.data.astype(np.float64), device=device))
        return self._csr[(transposed, device)]

    def coo_tables(self, transposed, device):
        key = (transposed, torch.device(device))
        if key not in self._coo:
            m = self._of(transposed).tocoo()
            self._coo[key] = tuple(torch.as_tensor(np.ascontiguousarray(a), device=device) for a in (m.row.astype(np.int64), m.col.astype(np.int64), m.data.astype(np.float64)))
        return self._coo[key]

    def uses_kernel(self, x):
        from . import hip_renderer

        return x.is_cuda and x.dtype in (torch.float32, torch.float64) and 1 <= x.shape[-1] <= hip_renderer.MAX_COLORS

    def lanes(self, transposed=False):
        """the kernel instance (lanes per row) the library runs for this matrix / its transpose"""
        from . import hip_renderer

        m = self._of(transposed)
        return hip_renderer.sparse_rows_lanes(m.shape[0], m.nnz)

    def run(self, x, transposed=False):
        """``A x`` (or ``A^T x``), no autograd"""
        m = self._of(transposed)
        if x.dim() < 2 or int(x.shape[-2]) != m.shape[1]:
            raise ValueError(f"sparse operator: expected [..., {m.shape[1]}, D], got {list(x.shape)}")
        if x.numel() and self.uses_kernel(x):
            from . import hip_renderer

            lead = x.shape[:-2]
            out = hip_renderer.sparse_rows_apply(*self.csr_tables(transposed, x.device), x.reshape(-1, m.shape[1], x.shape[-1]).contiguous())
            return out.reshape(*lead, m.shape[0], x.shape[-1])
        rows, cols, vals = self.coo_tables(transposed, x.device)
        out = torch.zeros(x.shape[:-2] + (m.shape[0], x.shape[-1]), dtype=x.dtype, device=x.device)
        return out.index_add_(-2, rows, vals.to(x.dtype)[:, None] * x.index_select(-2, cols))

    def apply(self, x, transposed=False):
        return _SparseApply.apply(x, self, transposed)


class _SparseApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, operator, transposed):
        ctx.operator, ctx.transposed = operator, transposed
        return operator.run(x, transposed)

    @staticmethod
    def backward(ctx, y_b):
        return _SparseApply.apply(y_b, ctx.operator, not ctx.transposed), None, None  # (linear: differentiable any number of times)


class LoopSubdivision:
    """``n_iter`` levels of Loop subdivision of the connectivity ``faces`` [T,3], composed into one matrix.

    ``faces_fine`` [4^n_iter T, 3] and ``nb_vertices_fine`` in the reference's order; ``matrix`` / ``colors_matrix``: SciPy CSR [Vf, Vc], columns
    sorted within a row; :meth:`apply` / :meth:`apply_colors`: the differentiable maps; ``topology``: the :class:`MeshTopology` of the fine mesh
    (built at first use)."""

    def __init__(self, faces, nb_vertices=None, n_iter=1, clockwise=False, device="cuda"):
        if int(n_iter) < 1:
            raise ValueError("LoopSubdivision: n_iter must be at least 1")
        f = np.asarray(faces).astype(np.int64)
        self.n_iter, self.clockwise, self.device = int(n_iter), bool(clockwise), torch.device(device)
        self.faces = f
        self.nb_vertices = int(nb_vertices) if nb_vertices is not None else int(f.max()) + 1
        S = C = None
        V = self.nb_vertices
        for _ in range(self.n_iter):
            s, c, f = loop_subdivision_level(f, V)
            S, C = (s, c) if S is None else (s @ S, c @ C)
            V = s.shape[0]
        self.faces_fine, self.nb_vertices_fine = f, V
        self._vertices, self._colors = SparseOperator(S, self.device), SparseOperator(C, self.device)
        self.matrix, self.colors_matrix = self._vertices.matrix, self._colors.matrix
        self._topology = None

    @property
    def topology(self):
        if self._topology is None:
            from .scene3d import MeshTopology

            self._topology = MeshTopology(self.faces_fine, self.nb_vertices_fine, self.clockwise, self.device)
        return self._topology

    def tables(self, transposed=False, colors=False):
        """(offsets u32 [rows + 1], cols u32, vals f64) of ``matrix`` (or ``colors_matrix``), or of its transpose, on the device"""
        return (self._colors if colors else self._vertices).csr_tables(transposed)

    def lanes(self, transposed=False, colors=False):
        return (self._colors if colors else self._vertices).lanes(transposed)

    def apply(self, x):
        """control values [..., Vc, D] -> fine values [..., Vf, D] by the Loop rules; differentiable"""
        return self._vertices.apply(x)

    def apply_colors(self, x):
        """colours [..., Vc, D] -> [..., Vf, D]: old ones kept, an edge point gets the mean of its ends; differentiable"""
        return self._colors.apply(x)
