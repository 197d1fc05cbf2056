"""Reference for the sparse symmetric positive definite solve (include/deodr_hip_solve.h, deodr_amd/smoothing.py): the recurrence restated in NumPy long
double with plain loops over the rows -- no code shared with the library --, the systems the CPU and the GPU tests share, and the case table.

The systems are generated here: ``I + lambda L`` of the graph Laplacian of a triangle strip (exactly n vertices for any n), with a few HUB vertices
whose extra edges give rows of 7, 8, 9 and 17 entries (the trips of the kernels' group of 8 lanes per row: one trip less one, one exactly, two, three);
of a closed sphere (deodr_amd.scenes.bumpy_sphere) and of a triangulated grid, both through ``deodr_amd.smoothing.laplacian_system``; and three tiny
dense ones.  The sizes come from the kernels' constants (N_SMALL, ROWS, FH_BLOCK, BLOCKS below: DEODR_HIP_SOLVE_N_SMALL, SOLVE_ROWS, FH_BLOCK and
SOLVE_BLOCKS of deodr_amd/csrc; tests/test_smoothing_abi.py compares them with the source).

THE TOLERANCE OF THE GPU TESTS.  Float64 and long-double conjugate gradients drift apart exponentially with the number of steps (the recurrence
amplifies a rounding error by the growth of its Krylov basis), so the PARITY of the recurrence is tested only at m in {1, 2, 8, 16} with lambda <= 16:
tests/test_smoothing_reference.py::test_measure_the_tolerance runs the float64 torch recurrence against this restatement over every parity case and
prints, per number of steps, the largest error of x relative to ``max |x|`` of the case and of the residual relative to its value.  MEASURED holds
those figures (the largest of them, at 16 steps, is the one figure a single tolerance would be; the shorter runs are held to their own, smaller
ones); the kernels do the same arithmetic in float64 but add in another order, hence FACTOR = 8 on top.  The regular meshes used here (a sphere, a
strip) have many equal eigenvalues, which rounding splits: their drift at 16 steps is far larger than that of an irregular mesh.  Long runs are tested through the TRUE
residual ``|b - A x| / |b|`` recomputed in long double from the returned x (CONVERGENCE below)."""

import functools

import numpy as np

LD = np.longdouble
# test_measure_the_tolerance, per number of steps: the drift grows with it, and one figure for all would hold the short runs to the long runs' error
# (measured 2.040e-16, 1.728e-15, 1.525e-13 -- "hubs n=1025 lam=4 D=4 m=8 zero column" -- and 5.554e-9 -- "hubs n=1025 lam=4 D=3 m=16" --, rounded up by
# a few per cent; measured with torch on one thread, and the same figures came out on all of this machine's threads)
MEASURED = {1: 2.1e-16, 2: 1.8e-15, 8: 1.6e-13, 16: 5.7e-9}
FACTOR = 8
TOLERANCE = {m: FACTOR * e for m, e in MEASURED.items()}
RESIDUAL_FLOOR = 1e-20  # a squared relative residual below this is rounding noise (converged): its relative error says nothing
CONVERGENCE = 1e-8  # |b - A x|_2 / |b|_2 of the lambda = 4, m = 64 case

def _n_small():
    """the size at which the rule function changes the instance, from the header the library is built with (``deodr_hip_spd_solve_launches`` itself is
    asked in tests/test_smoothing_abi.py and tests/test_smoothing_gpu.py: the library may not be built when this table is)"""
    from deodr_amd import _abi

    return _abi.SOLVE_HEADER.defines["DEODR_HIP_SOLVE_N_SMALL"]


N_SMALL = _n_small()
FH_BLOCK, BLOCKS, LANES = 256, 512, 8  # FH_BLOCK, SOLVE_BLOCKS, SOLVE_LANES of deodr_amd/csrc (compared with the source by tests/test_smoothing_abi.py)
ROWS = FH_BLOCK // LANES


# ---- the recurrence, in long double --------------------------------------------------------------------------------------------------------


def matvec(offsets, cols, vals, p):
    """A p row by row; p [n, D] long double"""
    q = np.zeros_like(p)
    for row in range(len(offsets) - 1):
        s, e = offsets[row], offsets[row + 1]
        q[row] = vals[s:e] @ p[cols[s:e]]
    return q


def restate(offsets, cols, vals, b, iterations, rel_tol=0.0):
    """-> dict(x [n, D], residual [D], frozen_at [D]: the first step at which the column was not active, or ``iterations``), all in long double"""
    offsets, cols = np.asarray(offsets, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    vals, b = np.asarray(vals).astype(LD), np.asarray(b).astype(LD)
    n, D = b.shape
    x, r, p = np.zeros((n, D), dtype=LD), b.copy(), b.copy()
    rho = np.array([np.sum(r[:, d] * r[:, d]) for d in range(D)], dtype=LD)
    rho_b, tol2 = rho.copy(), LD(rel_tol) * LD(rel_tol)
    frozen_at = np.full(D, iterations)
    for it in range(iterations):
        q = matvec(offsets, cols, vals, p)
        for d in range(D):
            sigma = np.sum(p[:, d] * q[:, d])
            active = bool(rho[d] > tol2 * rho_b[d]) and bool(sigma > 0)
            if not active:
                frozen_at[d] = min(frozen_at[d], it)
            alpha = rho[d] / sigma if active else LD(0)
            x[:, d] += alpha * p[:, d]
            r[:, d] -= alpha * q[:, d]
            rho_new = np.sum(r[:, d] * r[:, d])
            beta = rho_new / rho[d] if active else LD(0)
            rho[d] = rho_new if active else rho[d]
            p[:, d] = r[:, d] + beta * p[:, d]
    residual = np.array([rho[d] / rho_b[d] if rho_b[d] > 0 else LD(0) for d in range(D)], dtype=LD)
    return dict(x=x, residual=residual, frozen_at=frozen_at)


def true_residual(offsets, cols, vals, b, x):
    """|b - A x|_2 / |b|_2 per column, in long double"""
    b, x = np.asarray(b).astype(LD), np.asarray(x).astype(LD)
    d = b - matvec(np.asarray(offsets, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(vals).astype(LD), x)
    return np.sqrt((d * d).sum(axis=0)) / np.sqrt((b * b).sum(axis=0))


# ---- systems -------------------------------------------------------------------------------------------------------------------------------


def csr_of_edges(n, edges, lam):
    """I + lam (deg - adjacency) of the undirected graph ``edges`` [E,2] on n vertices -> (offsets, cols, vals), columns sorted within a row"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    both = np.unique(np.concatenate((e, e[:, ::-1])), axis=0)  # every neighbour of every vertex, once
    degree = np.bincount(both[:, 0], minlength=n)
    rows = np.concatenate((both[:, 0], np.arange(n)))
    cols = np.concatenate((both[:, 1], np.arange(n)))
    vals = np.concatenate((np.full(len(both), -float(lam)), 1.0 + lam * degree))
    order = np.lexsort((cols, rows))
    offsets = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n))))
    return offsets, cols[order], vals[order]


def strip_faces(n):
    """a triangle strip on n >= 3 vertices: interior vertices have 4 neighbours (rows of 5 entries)"""
    i = np.arange(n - 2)
    return np.column_stack((i, i + 1, i + 2))


HUBS = ((5, 6), (15, 7), (25, 8), (35, 16))  # (vertex, neighbours it ends up with): rows of 7, 8, 9, 17 entries


def strip_system(n, lam, hubs=True):
    """the strip's ``I + lam L`` -- with ``hubs`` (n >= 128) the vertices HUBS are given far neighbours, up to the counts stated there"""
    f = strip_faces(n)
    edges = [f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]
    if hubs and n >= 128:
        for hub, count in HUBS:
            edges.append(np.array([(hub, 64 + 3 * t + hub % 3) for t in range(count - 4)]))
    return csr_of_edges(n, np.concatenate(edges), lam)


def grid_faces(nx, ny):
    """a triangulated nx x ny grid of vertices"""
    idx = np.arange(nx * ny).reshape(ny, nx)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    return np.concatenate((np.column_stack((a, b, c)), np.column_stack((b, d, c))))


def mesh_system(faces, nb_vertices, lam):
    """``deodr_amd.smoothing.laplacian_system`` of a mesh, on the CPU -> (offsets, cols, vals) as NumPy arrays (what the library builds: the tests of
    the recurrence take the matrix as given; tests/test_smoothing_reference.py compares it with csr_of_edges)"""
    from deodr_amd.smoothing import laplacian_system

    s = laplacian_system(np.asarray(faces).astype(np.int64), lam, nb_vertices, device="cpu")
    return s.offsets.numpy().view(np.uint32).astype(np.int64), s.cols.numpy().view(np.uint32).astype(np.int64), s.vals.numpy().copy()


def sphere(nu=16, n_rings=20):
    """the closed UV sphere of the repository's generator: nu * n_rings + 2 = 322 vertices, regular rows of 7 entries (6 next to a pole), the poles rows of nu + 1 = 17"""
    from deodr_amd import scenes

    vertices, faces = scenes.bumpy_sphere(nu, n_rings)
    return vertices, faces.astype(np.int64)


def tiny_system(n):
    """dense symmetric positive definite matrices of 1, 2, 3 rows"""
    m = {1: [[2.5]], 2: [[2.0, -0.5], [-0.5, 1.5]], 3: [[3.0, -1.0, 0.0], [-1.0, 3.0, -1.0], [0.0, -1.0, 2.0]]}[n]
    m = np.array(m)
    rows, cols = np.nonzero(m)
    return np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n)))), cols, m[rows, cols]


def right_hand_side(n, D, seed, zero_column=None):
    """random, zero-mean per column (what the fitters' projection leaves); ``zero_column``: that column all zeros"""
    b = np.random.RandomState(seed).randn(n, D)
    if n > 1:
        b -= b.mean(axis=0, keepdims=True)
    if zero_column is not None:
        b[:, zero_column] = 0
    return b


# ---- the case table: name -> (system builder, D, iterations, lambda or None, zero column or None) ----------------------------------------------

CASES = {}


def _case(name, build, D, iterations, zero_column=None, parity=True):
    CASES[name] = dict(name=name, build=build, D=D, iterations=iterations, zero_column=zero_column, parity=parity)


for _n in (1, 2, 3):
    _case(f"tiny n={_n} D=3 m=2", functools.partial(tiny_system, _n), 3, 2)
_case("tiny n=1 D=1 m=1", functools.partial(tiny_system, 1), 1, 1)
_case("tiny n=3 D=4 m=50 past n", functools.partial(tiny_system, 3), 4, 50, parity=False)  # frozen: no NaN, x at the solution
_case("strip n=40 with an isolated vertex D=3 m=8", lambda: csr_of_edges(40, np.concatenate([strip_faces(39)[:, [0, 1]], strip_faces(39)[:, [1, 2]], strip_faces(39)[:, [2, 0]]]), 4.0), 3, 8)
_case("sphere 322 lam=16 D=3 m=16", lambda: mesh_system(sphere()[1], 322, 16.0), 3, 16)
_case("sphere 322 lam=4 D=4 m=8 zero column", lambda: mesh_system(sphere()[1], 322, 4.0), 4, 8, zero_column=2)
_case("sphere 322 lam=4 D=3 m=64 convergence", lambda: mesh_system(sphere()[1], 322, 4.0), 3, 64, parity=False)
_case("grid 23x17 lam=1 D=1 m=16", lambda: mesh_system(grid_faces(23, 17), 23 * 17, 1.0), 1, 16)
_case("hubs n=200 lam=4 D=3 m=2", functools.partial(strip_system, 200, 4.0), 3, 2)
for _n, _D, _m in ((N_SMALL - 1, 3, 2), (N_SMALL, 3, 16), (N_SMALL + 1, 3, 16), (N_SMALL, 4, 8), (N_SMALL + 1, 4, 8), (N_SMALL + 1, 1, 1), (N_SMALL + 1, 4, 2),
                   (N_SMALL + ROWS - 1, 3, 2), (N_SMALL + ROWS, 3, 2), (N_SMALL + ROWS + 1, 3, 2),
                   (N_SMALL + FH_BLOCK - 1, 3, 1), (N_SMALL + FH_BLOCK, 3, 2), (N_SMALL + FH_BLOCK + 1, 3, 2)):  # fmt: skip
    _case(f"hubs n={_n} lam=4 D={_D} m={_m}", functools.partial(strip_system, _n, 4.0), _D, _m)
# a zero column through the multi-launch instance: its `active` flag, the held rho and the residual of rho_b = 0
_case(f"hubs n={N_SMALL + 1} lam=4 D=4 m=8 zero column", functools.partial(strip_system, N_SMALL + 1, 4.0), 4, 8, zero_column=1)
_case(f"hubs n={N_SMALL + 1} lam=4 D=3 m=2 zero column", functools.partial(strip_system, N_SMALL + 1, 4.0), 3, 2, zero_column=0)
# the grid of the row kernel strides (more than BLOCKS * ROWS rows) and grid_sum takes a second round (more than FH_BLOCK workgroups)
_case(f"hubs n={BLOCKS * ROWS + 1} lam=16 D=3 m=2 grid stride", functools.partial(strip_system, BLOCKS * ROWS + 1, 16.0), 3, 2)
# the grids of the thread-per-row kernels stride as well (more than BLOCKS * FH_BLOCK rows)
_case(f"hubs n={BLOCKS * FH_BLOCK + 1} lam=4 D=1 m=2 grid stride", functools.partial(strip_system, BLOCKS * FH_BLOCK + 1, 4.0), 1, 2)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (case: name, offsets, cols, vals, b, D, iterations, n; the long-double results of :func:`restate`), computed once"""
    c = CASES[name]
    offsets, cols, vals = (np.asarray(a) for a in c["build"]())
    n = len(offsets) - 1
    b = right_hand_side(n, c["D"], seed=len(name) + n, zero_column=c["zero_column"])
    case = dict(c, offsets=offsets, cols=cols, vals=vals, b=b, n=n)
    ref = restate(offsets, cols, vals, b, c["iterations"])
    ref["scale"] = np.abs(ref["x"]).max()
    return case, ref


def parity_cases():
    return [name for name, c in CASES.items() if c["parity"]]


def row_lengths(offsets):
    return np.diff(np.asarray(offsets))
