"""Smoothed steps: ``u = (I + lambda L)^-1 g``, a sparse symmetric positive definite solve on the device.

A rasterizer's vertex gradient ``g`` is sparse and rough -- the vertices on silhouettes and shading edges receive most of it.  Taking the step in
the metric ``I + lambda L`` of the mesh Laplacian ``L`` (Nicolet, Jacobson, Jakob, *Large Steps in Inverse Rendering*, 2021) spreads it over the
neighbourhood before the update rule sees it.  The solve is ``iterations`` steps of conjugate gradients from ``x = 0``, the columns independently
(``include/deodr_hip_solve.h`` has the recurrence, ``deodr_amd/csrc/dr_solve.h`` the kernels): a fixed number of launches, nothing read back, so it
runs inside a captured graph.  A truncated run is still a descent direction (``g^T u = u^T A u >= 0``), and since the rows of ``I + lambda L`` sum
to 1 a zero-mean ``g`` gives a zero-mean ``u``.

:func:`laplacian_system` builds ``I + lambda L`` of a mesh, :class:`SpdSystem` wraps a caller's own matrix (cotangent weights, ``(I + lambda L)^2``),
:func:`spd_solve` solves, differentiably in ``b``; :func:`spd_solve_torch` is the same recurrence as torch ops -- what runs on tensors the kernels do
not take (CPU tensors: the CPU suite) and what the kernels are tested against.  The mesh fitters take ``smoothing=lambda``
(``deodr_amd/mesh_fitter.py``).
"""

import numpy as np
import scipy.sparse as sp
import torch

# Steps of a smoothed fitter step and of :func:`spd_solve` by default.  Measured on the hand mesh (526 vertices), random zero-mean right-hand sides,
# squared relative residual after 8 / 16 / 32 steps: lambda = 4: 5.9e-3 / 3.3e-5 / 7.4e-10; 16: 3.6e-2 / 1.8e-3 / 2.5e-6; 64: 6.6e-2 / 8.8e-3 / 6.1e-5
# (DESIGN.md 4k).  16 steps leave 0.6 % to 9 % of the right-hand side's norm over that range: a smoothed direction does not need more, any truncation
# is a descent direction, and another 16 steps would cost the one-workgroup kernel another 53 us per iteration.
DEFAULT_ITERATIONS = 16


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


class SpdSystem:
    """A symmetric positive definite matrix in compressed rows, on a device, as :func:`spd_solve` takes it.  ``offsets`` [n + 1], ``cols`` [nnz],
    ``vals`` [nnz] (arrays or tensors; the diagonal stored like any other entry).  Checked here, on the host, because the kernels cannot: offsets
    non-decreasing from 0 to nnz, columns < n, the pattern and the values symmetric, a positive diagonal (positive definiteness itself is the
    caller's).  ``self.vals`` is a float64 device tensor that the kernels read when they run: ``copy_`` other values of the SAME pattern into it
    between calls, also between replays of a captured graph (they are not checked again)."""

    def __init__(self, offsets, cols, vals, device="cuda"):
        offsets, cols, vals = _host(offsets).astype(np.int64), _host(cols).astype(np.int64), _host(vals).astype(np.float64)
        if offsets.ndim != 1 or cols.ndim != 1 or vals.shape != cols.shape or len(offsets) < 2:
            raise ValueError("SpdSystem: offsets [n + 1], cols [nnz] and vals [nnz] must be one-dimensional, n >= 1")
        n, nnz = len(offsets) - 1, len(cols)
        if offsets[0] != 0 or offsets[-1] != nnz or np.any(np.diff(offsets) < 0) or nnz >= 2**32:
            raise ValueError("SpdSystem: offsets are not a non-decreasing sequence from 0 to nnz")
        if nnz and (cols.min() < 0 or cols.max() >= n):
            raise ValueError("SpdSystem: a column index is out of range")
        if not np.all(np.isfinite(vals)):
            raise ValueError("SpdSystem: vals must be finite")
        m = sp.csr_matrix((vals, cols, offsets), shape=(n, n))
        asym = abs(m - m.T)
        if asym.nnz and asym.max() > 1e-12 * max(abs(vals).max(), 1e-300):
            raise ValueError("SpdSystem: the matrix is not symmetric")
        if np.any(m.diagonal() <= 0):
            raise ValueError("SpdSystem: the diagonal must be positive (the matrix is not positive definite)")
        self.n, self.nnz, self.device = n, nnz, torch.device(device)
        u32 = lambda a: torch.as_tensor(np.ascontiguousarray(a).astype(np.uint32).view(np.int32), device=self.device)
        self.offsets, self.cols = u32(offsets), u32(cols)  # (uint32 bit patterns in int32 tensors, as MeshTopology's)
        self.vals = torch.as_tensor(vals, device=self.device)
        # the COO rows and columns of the entries, for the torch recurrence
        self._rows = torch.as_tensor(np.repeat(np.arange(n), np.diff(offsets)), device=self.device)
        self._cols = torch.as_tensor(cols, device=self.device)

    @classmethod
    def from_scipy(cls, matrix, device="cuda"):
        m = sp.csr_matrix(matrix)
        m.sum_duplicates()
        m.sort_indices()
        if m.shape[0] != m.shape[1]:
            raise ValueError("SpdSystem: the matrix must be square")
        return cls(m.indptr, m.indices, m.data, device)

    def to_scipy(self):
        """the matrix as SciPy CSR, with the values ``self.vals`` holds now (synchronises)"""
        return sp.csr_matrix((_host(self.vals), _host(self._cols), np.concatenate(([0], np.cumsum(np.bincount(_host(self._rows), minlength=self.n))))),
                             shape=(self.n, self.n))  # fmt: skip

    def matvec(self, p):
        """``A p`` for ``p`` [n, D] as torch ops (one index_add over the entries)"""
        return torch.zeros_like(p).index_add_(0, self._rows, self.vals.to(p.dtype)[:, None] * p.index_select(0, self._cols))


def graph_laplacian(faces, nb_vertices=None):
    """the graph Laplacian ``deg - adjacency`` over "shares an edge of a face", the one :class:`deodr_amd.scene3d.MeshTopology` builds -> SciPy CSR"""
    f = np.asarray(faces).astype(np.int64)
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("graph_laplacian: faces must be a [T,3] array")
    V = int(nb_vertices) if nb_vertices is not None else int(f.max()) + 1
    if len(f) and (f.min() < 0 or f.max() >= V):
        raise ValueError("graph_laplacian: a face refers to a vertex that does not exist")
    a = np.zeros((0, 2), dtype=np.int64)
    if len(f):
        a = np.unique(np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]], f[:, [1, 0]], f[:, [2, 1]], f[:, [0, 2]])), axis=0)
    adj = sp.coo_matrix((np.ones(len(a)), (a[:, 0], a[:, 1])), shape=(V, V)).tocsr()
    return (sp.diags(np.asarray(adj.sum(axis=1)).ravel()) - adj).tocsr()


def laplacian_system(topology_or_faces, lam, nb_vertices=None, device=None):
    """-> the :class:`SpdSystem` of ``I + lam L``, ``L`` the graph Laplacian of a :class:`MeshTopology` (on its device unless ``device`` is given) or
    of a ``faces`` [T,3] array (``device`` "cuda" by default).  ``lam >= 0``.  The values for another ``lam`` have the same pattern:
    ``system.vals.copy_(laplacian_system(faces, other, device="cpu").vals)``."""
    lam = float(lam)
    if not 0 <= lam < np.inf:  # (a NaN is refused as well)
        raise ValueError(f"laplacian_system: lam must be a finite real number >= 0, not {lam!r}")
    if hasattr(topology_or_faces, "face_edge"):  # a MeshTopology
        topo = topology_or_faces
        faces, nb_vertices, device = _host(topo.faces), topo.nb_vertices, (topo.device if device is None else device)
    else:
        faces, device = topology_or_faces, ("cuda" if device is None else device)
    lap = graph_laplacian(faces, nb_vertices).tocoo()
    n, off = lap.shape[0], lap.row != lap.col
    # every row gets its diagonal, also that of a vertex without neighbours, and an entry whose value is 0 (lam = 0) stays in the pattern: the
    # tables are put together by hand, SciPy's sums drop explicit zeros
    rows, cols = np.concatenate((lap.row[off], np.arange(n))), np.concatenate((lap.col[off], np.arange(n)))
    vals = np.concatenate((lam * lap.data[off], 1.0 + lam * lap.diagonal()))
    order = np.lexsort((cols, rows))
    offsets = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n))))
    return SpdSystem(offsets, cols[order], vals[order], device)


def spd_solve_torch(system, b, iterations=DEFAULT_ITERATIONS, rel_tol=0.0):
    """the recurrence of ``include/deodr_hip_solve.h`` as torch ops, in the dtype of ``b`` [n, D] -> (x [n, D], residual [D]).  The same algorithm as
    the kernels: a CPU fit and a GPU fit take the same steps up to rounding."""
    if b.dim() != 2 or int(b.shape[0]) != system.n:
        raise ValueError(f"spd_solve: b must have shape [{system.n}, D], not {list(b.shape)}")
    if int(iterations) < 1 or not float(rel_tol) >= 0:
        raise ValueError("spd_solve: iterations must be >= 1 and rel_tol >= 0")
    b = b.detach()
    zero, one = torch.zeros((), dtype=b.dtype, device=b.device), torch.ones((), dtype=b.dtype, device=b.device)
    x, r, p = torch.zeros_like(b), b.clone(), b.clone()
    rho = (r * r).sum(dim=0)
    rho_b, tol2 = rho.clone(), float(rel_tol) ** 2
    for _ in range(int(iterations)):
        q = system.matvec(p)
        sigma = (p * q).sum(dim=0)
        active = (rho > tol2 * rho_b) & (sigma > 0)
        alpha = torch.where(active, rho / torch.where(active, sigma, one), zero)
        x, r = x + alpha * p, r - alpha * q
        rho_new = (r * r).sum(dim=0)
        beta = torch.where(active, rho_new / torch.where(active, rho, one), zero)
        rho = torch.where(active, rho_new, rho)
        p = r + beta * p
    return x, torch.where(rho_b > 0, rho / torch.where(rho_b > 0, rho_b, one), zero)


# (device, n, D) -> the scratch of the kernels.  Per shape, NOT per stream: a captured step has to find the scratch of the eager steps before it, and a
# capture runs on a stream of its own.  Hence the restriction in the docstring of spd_solve: solves of one shape run on one stream at a time.
_scratches = {}


def uses_kernel(system, b):
    """does :func:`spd_solve` run the kernels on this right-hand side (a float64 ROCm tensor [n, D <= 4] on the system's device)?"""
    return torch.is_tensor(b) and b.is_cuda and b.dtype == torch.float64 and b.dim() == 2 and 1 <= b.shape[1] <= 4 and b.device == system.vals.device


def solve_no_grad(system, b, iterations, rel_tol):
    """(x, residual) without autograd: ``deodr_hip_spd_solve`` on float64 ROCm tensors, :func:`spd_solve_torch` elsewhere"""
    if not uses_kernel(system, b):
        return spd_solve_torch(system, b, iterations, rel_tol)
    from . import hip_renderer as hr

    if int(b.shape[0]) != system.n:
        raise ValueError(f"spd_solve: b must have shape [{system.n}, D], not {list(b.shape)}")
    key = (b.device, system.n, int(b.shape[1]))
    if key not in _scratches:
        _scratches[key] = hr.spd_scratch(system.n, key[2], b.device)
    return hr.spd_solve(system.offsets, system.cols, system.vals, b.detach().contiguous(), iterations, rel_tol, scratch=_scratches[key])


def spd_solve(system, b, iterations=DEFAULT_ITERATIONS, rel_tol=0.0):
    """``iterations`` steps of conjugate gradients on ``system x = b`` from ``x = 0``, the columns of ``b`` [n, D] independently -> (x, residual [D]:
    the squared relative residual the recurrence ends with, for display).  A column stops changing once its residual is below ``rel_tol``
    (relative, not squared).  On float64 ROCm tensors with ``D <= 4`` the kernels; elsewhere the torch recurrence.  The kernels' scratch is kept per
    (device, n, D), not per stream (a captured graph must find the one the eager calls made): calls of the SAME shape must not run on two streams at
    once -- above 1024 rows they would share r, p, q and the arrival tickets.  A caller who needs that passes a scratch of its own to
    ``hip_renderer.spd_solve``.
    Differentiable in ``b`` (:class:`deodr_amd.fronthalf.SpdSolveFunc`): the gradient is the same solve of the incoming gradient, which is the
    adjoint of the CONVERGED operator ``A^-1``, not of the truncated recurrence -- exact only as far as ``iterations`` converge."""
    if torch.is_tensor(b) and b.requires_grad and torch.is_grad_enabled():
        from . import fronthalf

        return fronthalf.SpdSolveFunc.apply(b, system, int(iterations), float(rel_tol))
    return solve_no_grad(system, b, int(iterations), float(rel_tol))
