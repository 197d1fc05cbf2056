"""The as-rigid-as-possible energy of Sorkine and Alexa (*As-Rigid-As-Possible Surface Modeling*, 2007) on the device.

Every vertex carries the rotation ``R_i`` that best maps its rest one-ring onto its current one, and only what that rotation cannot explain is
charged: ``E = 1/2 c sum_i sum_j w_ij |(p_i - p_j) - R_i (q_i - q_j)|^2``.  Unlike the Laplacian energy of the reference
(``LaplacianRigidEnergyDevice``: a quadratic in the displacement), it is invariant to rotations of a PART of the mesh -- a finger that bends costs
what its knuckle stretches, not what the whole finger moved.  ``include/deodr_hip_arap.h`` has the operation, ``deodr_amd/csrc/dr_arap.h`` the two
kernels (a 3 x 3 polar decomposition per vertex by Jacobi sweeps on Horn's 4 x 4 matrix, then the gradient with the neighbours' rotations): a fixed
number of launches, nothing read back, so it runs inside a captured graph.

:class:`ArapEnergyDevice` holds the adjacency, the weights and the rest vertices of a mesh and evaluates, differentiably;
:func:`arap_energy_torch` is the same definition as torch ops (batched ``torch.linalg.svd``) -- what runs on tensors the kernels do not take (CPU
tensors, other dtypes) and what the kernels are compared with; :class:`ArapEnergy` has the NumPy interface of the reference's
``LaplacianRigidEnergy``.  The mesh fitters take ``rigidity="arap"`` (``deodr_amd/mesh_fitter.py``)."""

import numpy as np
import scipy.sparse as sp
import torch

from .smoothing import _host, graph_laplacian


def cotangent_weights(faces, vertices, nb_vertices=None):
    """``w_ij = 1/2 (cot a_ij + cot b_ij)``, the angles opposite the edge in its one or two faces, of the REST mesh -> SciPy CSR [V,V], symmetric, no
    diagonal.  A negative weight (an edge opposite obtuse angles) is clamped to 0: the energy needs ``w >= 0`` to be bounded below, and the edge
    then simply does not count.  An edge keeps its place in the pattern at weight 0."""
    f, v = np.asarray(faces).astype(np.int64).reshape(-1, 3), np.asarray(vertices, dtype=np.float64)
    V = int(nb_vertices) if nb_vertices is not None else len(v)
    rows, cols, vals = [], [], []
    for k in range(3):  # the angle at corner k is opposite the edge (k + 1, k + 2)
        o, a, b = f[:, k], f[:, (k + 1) % 3], f[:, (k + 2) % 3]
        u, w = v[a] - v[o], v[b] - v[o]
        cot = (u * w).sum(axis=1) / np.maximum(np.linalg.norm(np.cross(u, w), axis=1), 1e-300)
        rows += [a, b]
        cols += [b, a]
        vals += [0.5 * cot, 0.5 * cot]
    if not len(f):
        return sp.csr_matrix((V, V))
    m = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(V, V)).tocsr()
    m.sum_duplicates()
    m.data = np.maximum(m.data, 0.0)  # (explicit zeros stay in the pattern)
    m.sort_indices()
    return m


def _rotations_to_quaternions(R):
    """R [...,3,3] -> unit quaternions (x, y, z, w) [...,4] with w >= 0 (the largest of the four candidates, for accuracy at any angle)"""
    m = lambda a, b: R[..., a, b]
    tr = m(0, 0) + m(1, 1) + m(2, 2)
    cand = torch.stack((
        torch.stack((m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1), 1 + tr), -1),
        torch.stack((1 + m(0, 0) - m(1, 1) - m(2, 2), m(0, 1) + m(1, 0), m(0, 2) + m(2, 0), m(2, 1) - m(1, 2)), -1),
        torch.stack((m(0, 1) + m(1, 0), 1 - m(0, 0) + m(1, 1) - m(2, 2), m(1, 2) + m(2, 1), m(0, 2) - m(2, 0)), -1),
        torch.stack((m(0, 2) + m(2, 0), m(1, 2) + m(2, 1), 1 - m(0, 0) - m(1, 1) + m(2, 2), m(1, 0) - m(0, 1)), -1),
    ), -2)  # fmt: skip
    pivot = torch.stack((1 + tr, 1 + m(0, 0) - m(1, 1) - m(2, 2), 1 - m(0, 0) + m(1, 1) - m(2, 2), 1 - m(0, 0) - m(1, 1) + m(2, 2)), -1)
    q = torch.gather(cand, -2, pivot.argmax(-1)[..., None, None].expand(*pivot.shape[:-1], 1, 4))[..., 0, :]
    q = q / q.norm(dim=-1, keepdim=True)
    return torch.where(q[..., 3:] < 0, -q, q)


def arap_energy_torch(rows, cols, weights, vertices_ref, vertices, cregu, want_rotations=False):
    """the operation of ``include/deodr_hip_arap.h`` as torch ops, in the dtype of ``vertices`` [n,V,3]: ``rows`` / ``cols`` [nnz] the row and column
    of every stored entry (int64), ``weights`` [nnz] -> (energy [n], gradient [n,V,3], rotations [n,V,4] or None).  The rotations by batched SVD
    (Kabsch), ``R = U diag(1, 1, det(U V^T)) V^T``; the two exact cases of the contract by selects: a cell with ``S = 0`` and every cell of a pose
    bit-equal to ``vertices_ref`` have ``R = identity``, so that pose has energy and gradient 0.0 exactly.  No autograd: see
    :class:`deodr_amd.fronthalf.ArapEnergyFunc`."""
    with torch.no_grad():
        p, q, w = vertices, vertices_ref.to(vertices.dtype), weights.to(vertices.dtype)
        n, V = int(p.shape[0]), int(p.shape[1])
        ep, eq = p[:, rows] - p[:, cols], q[rows] - q[cols]  # [n,nnz,3], [nnz,3]
        S = torch.zeros((n, V, 3, 3), dtype=p.dtype, device=p.device).index_add_(1, rows, w[:, None, None] * (ep[..., :, None] * eq[None, :, None, :]))
        U, _, Vh = torch.linalg.svd(S)
        D = torch.ones((n, V, 3), dtype=p.dtype, device=p.device)
        D[..., 2] = torch.where(torch.linalg.det(U @ Vh) < 0, -1.0, 1.0).to(p.dtype)
        R = (U * D[..., None, :]) @ Vh
        identity = (S == 0).all(dim=-1).all(dim=-1) | (p == q).all(dim=-1).all(dim=-1)[:, None]
        R = torch.where(identity[..., None, None], torch.eye(3, dtype=p.dtype, device=p.device), R)
        d = ep - (R[:, rows] @ eq[None, :, :, None])[..., 0]
        dj = ep - (R[:, cols] @ eq[None, :, :, None])[..., 0]
        cell = torch.zeros((n, V), dtype=p.dtype, device=p.device).index_add_(1, rows, w * (d * d).sum(dim=-1))
        g = torch.zeros_like(p).index_add_(1, rows, w[:, None] * (d + dj))
        return (0.5 * cregu) * cell.sum(dim=1), cregu * g, (_rotations_to_quaternions(R) if want_rotations else None)


class ArapEnergyDevice:
    """The as-rigid-as-possible energy of a mesh against its rest vertices, on a device.

    ``topology``: a :class:`deodr_amd.scene3d.MeshTopology` (its device is used) or a ``faces`` [T,3] array (``device``, "cuda" by default).
    ``vertices_ref`` [V,3]: the rest vertices (``self.vertices_ref``, a float64 device tensor the kernels read when they run).  ``cregu >= 0``.
    ``weights``: "uniform" (1 per edge), "cotangent" (:func:`cotangent_weights` of the rest mesh, negative values clamped to 0), or an array
    with one value per stored entry of the adjacency -- the pairs (i, j) that share an edge of a face, sorted by i, then j
    (``self.rows`` / ``self.columns``).  Checked here, on the host, because the kernels cannot: offsets monotone from 0 to nnz, columns < V, no
    diagonal, the pattern symmetric, the weights symmetric, finite and >= 0.  ``self.weights`` is read when the kernels run: ``copy_`` other
    values into it between calls, also between replays of a captured graph (they are not checked again).

    A mesh of several components is fine (the Laplacian energy refuses one); a vertex without neighbours contributes nothing.
    ``cregu`` does not have the scale of ``LaplacianRigidEnergyDevice``'s: that energy squares the Laplacian (``L^T L``, entries of order valence^2),
    this one is first order in it -- ONE displaced vertex of valence ``v`` costs ``0.5 c (v^2 + v) |d|^2`` there and ``c v |d|^2`` here (the
    rotations held), so the same stiffness against it needs a ``cregu`` that is ``(v + 1) / 2`` = 3.5 times larger at valence 6."""

    def __init__(self, topology, vertices_ref, cregu, weights="uniform", device=None):
        if hasattr(topology, "face_edge"):  # a MeshTopology
            faces, V, device = _host(topology.faces), topology.nb_vertices, (topology.device if device is None else device)
        else:
            faces, V, device = np.asarray(topology), int(np.shape(vertices_ref)[-2]), ("cuda" if device is None else device)
        self.device, self.cregu = torch.device(device), float(cregu)
        if not self.cregu >= 0:  # (a NaN is refused as well)
            raise ValueError(f"ArapEnergyDevice: cregu must be >= 0, not {cregu!r}")
        v_ref = _host(vertices_ref).astype(np.float64)
        if v_ref.shape != (V, 3):
            raise ValueError(f"ArapEnergyDevice: vertices_ref must be [{V}, 3], not {list(v_ref.shape)}")
        adj = -graph_laplacian(faces, V)
        adj.setdiag(0)
        adj.eliminate_zeros()
        adj.sort_indices()
        offsets, cols = adj.indptr.astype(np.int64), adj.indices.astype(np.int64)
        rows = np.repeat(np.arange(V), np.diff(offsets))
        if isinstance(weights, str):
            if weights == "uniform":
                w = np.ones(len(cols))
            elif weights == "cotangent":
                w = np.asarray(cotangent_weights(faces, v_ref, V)[rows, cols]).ravel() if len(cols) else np.zeros(0)
            else:
                raise ValueError(f'ArapEnergyDevice: weights must be "uniform", "cotangent" or an array, not {weights!r}')
        else:
            w = _host(weights).astype(np.float64)
        self._check(offsets, cols, w, V)
        self.nb_vertices, self.nnz = V, len(cols)
        u32 = lambda a: torch.as_tensor(np.ascontiguousarray(a).astype(np.uint32).view(np.int32), device=self.device)
        self.offsets, self.cols = u32(offsets), u32(cols)  # (uint32 bit patterns in int32 tensors, as MeshTopology's)
        self.weights = torch.as_tensor(w, device=self.device)
        self.rows, self.columns = torch.as_tensor(rows, device=self.device), torch.as_tensor(cols, device=self.device)
        self.vertices_ref = torch.as_tensor(v_ref, device=self.device)
        self._scratch = {}  # n -> the kernels' scratch.  Per shape, not per stream: a captured step has to find the one the eager steps made

    @staticmethod
    def _check(offsets, cols, w, V):
        nnz = len(cols)
        if len(offsets) != V + 1 or offsets[0] != 0 or offsets[-1] != nnz or np.any(np.diff(offsets) < 0) or nnz >= 2**32:
            raise ValueError("ArapEnergyDevice: offsets are not a non-decreasing sequence from 0 to nnz")
        if w.shape != (nnz,):
            raise ValueError(f"ArapEnergyDevice: weights must have one value per stored entry ({nnz}), not shape {list(w.shape)}")
        if nnz and (cols.min() < 0 or cols.max() >= V):
            raise ValueError("ArapEnergyDevice: a column index is out of range")
        rows = np.repeat(np.arange(V), np.diff(offsets))
        if np.any(rows == cols):
            raise ValueError("ArapEnergyDevice: the adjacency must not have a diagonal entry")
        if not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError("ArapEnergyDevice: the weights must be finite and >= 0")
        m = sp.csr_matrix((w + 1.0, cols, offsets), shape=(V, V))  # (+ 1: an entry of weight 0 still counts for the pattern)
        asym = abs(m - m.T)
        if asym.nnz and asym.max() > 1e-12 * (1.0 + (w.max() if nnz else 0.0)):
            raise ValueError("ArapEnergyDevice: the pattern and the weights must be symmetric")

    def uses_kernel(self, vertices):
        """does :meth:`evaluate` run the kernels on these vertices (a float64 ROCm tensor on this energy's device)?"""
        return torch.is_tensor(vertices) and vertices.is_cuda and vertices.dtype == torch.float64 and vertices.device == self.vertices_ref.device

    def evaluate_no_grad(self, vertices, want_rotations=False):
        """(energy [n], gradient [n,V,3], rotations [n,V,4] or None) of ``vertices`` [n,V,3] without autograd: ``deodr_hip_arap_energy`` on float64
        ROCm tensors, :func:`arap_energy_torch` elsewhere"""
        if vertices.dim() != 3 or tuple(vertices.shape[1:]) != (self.nb_vertices, 3) or vertices.shape[0] < 1:
            raise ValueError(f"ArapEnergyDevice: vertices must be [{self.nb_vertices}, 3] or [n, {self.nb_vertices}, 3], not {list(vertices.shape)}")
        v = vertices.detach().contiguous()
        if not self.uses_kernel(v):
            to = lambda t: t.to(v.device)
            return arap_energy_torch(to(self.rows), to(self.columns), to(self.weights), to(self.vertices_ref), v, self.cregu, want_rotations)
        from . import hip_renderer as hr

        n = int(v.shape[0])
        if n not in self._scratch:
            self._scratch[n] = hr.arap_scratch(self.nb_vertices, n, v.device)
        return hr.arap_energy(self.offsets, self.cols, self.weights, self.vertices_ref, v, self.cregu, scratch=self._scratch[n], want_rotations=want_rotations)

    def evaluate(self, vertices):
        """-> (energy, gradient): of ``vertices`` [V,3] a scalar and [V,3], of [n,V,3] an energy per pose [n] and [n,V,3].  The energy is
        differentiable (its adjoint is the gradient the same call produced: exact wherever the rotations are unique); the gradient is returned
        for the fitters' update rule and marked non-differentiable.  On float64 ROCm tensors the kernels (two launches, deterministic); elsewhere
        the torch ops.  Calls of one shape must not run on two streams at once (they share a scratch)."""
        from . import fronthalf

        single = vertices.dim() == 2
        energy, gradient = fronthalf.ArapEnergyFunc.apply(vertices[None] if single else vertices, self)
        return (energy[0], gradient[0]) if single else (energy, gradient)

    def rotations(self, vertices):
        """the rotations of the cells as unit quaternions (x, y, z, w), w >= 0: [V,4] of ``vertices`` [V,3], [n,V,4] of [n,V,3]"""
        single = vertices.dim() == 2
        quats = self.evaluate_no_grad(vertices[None] if single else vertices, want_rotations=True)[2]
        return quats[0] if single else quats

    def laplacian(self):
        """the weighted graph Laplacian ``L_w = diag(sum_j w_ij) - W`` with the values ``self.weights`` holds now -> SciPy CSR (synchronises)"""
        W = sp.csr_matrix((_host(self.weights), (_host(self.rows), _host(self.columns))), shape=(self.nb_vertices,) * 2)
        return (sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W).tocsr()


class ArapEnergy:
    """``evaluate(vertices, return_grad, return_hessian)`` with the reference's ``LaplacianRigidEnergy`` interface
    (deodr/laplacian_rigid_energy.py:15-41) for the as-rigid-as-possible energy of ``mesh`` against its own vertices.  The approximate Hessian is
    that of the energy with the rotations held fixed, ``2 cregu L_w kron I3`` (``L_w`` the weighted graph Laplacian), built once on the host."""

    def __init__(self, mesh, cregu, weights="uniform", vertices=None):
        self.mesh, self.cregu = mesh, cregu
        self.vertices_ref = np.array(mesh.vertices if vertices is None else vertices, dtype=np.float64)
        self._dev = ArapEnergyDevice(mesh.adjacencies.topology, self.vertices_ref, cregu, weights)
        self.approx_hessian = (2.0 * float(cregu) * sp.kron(self._dev.laplacian(), sp.eye(3))).tocsr()

    def evaluate(self, vertices, return_grad=True, return_hessian=True):
        v = torch.as_tensor(np.array(vertices, dtype=np.float64), device=self._dev.device)
        energy, grad, _ = self._dev.evaluate_no_grad(v[None])
        out = (float(energy[0]),) + ((grad[0].cpu().numpy(),) if return_grad else ()) + ((self.approx_hessian,) if return_hessian else ())
        return out if len(out) > 1 else out[0]
