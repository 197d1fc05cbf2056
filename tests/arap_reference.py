"""The as-rigid-as-possible energy of include/deodr_hip_arap.h restated in NumPy, in any float type (long double: what the kernels and the torch
fallback are compared with; float64: the run whose distance to the long-double one the GPU tolerances derive from), the meshes and deformations of
the case tables the CPU and the GPU tests share, and the conditioning measure of a cell.

The operation (p = vertices [n,V,3], q = vertices_ref [V,3], w = the weights of the stored adjacency entries, e^p_ij = p_i - p_j, e^q_ij = q_i - q_j):

    S_i = sum_j w_ij e^p_ij (e^q_ij)^T                        entry (a, b): sum_j w_ij * (e^p_a * e^q_b), the entries of row i in order
    R_i = argmax over SO(3) of tr(R^T S_i)                    Horn's 4 x 4 matrix of S_i, SWEEPS sweeps of cyclic Jacobi over PAIRS, the eigenvector
                                                              of the largest eigenvalue (ties: the lowest index; the scalar part is index 0)
    d_ij = e^p_ij - R_i e^q_ij,   d'_ij = e^p_ij - R_j e^q_ij
    E   = 1/2 c sum_i sum_j w_ij |d_ij|^2
    g_i = c sum_j w_ij (d_ij + d'_ij)                         = c sum_j w_ij [2 e^p_ij - (R_i + R_j) e^q_ij]

Everything is vectorised over the cells; a row's sum runs over its entries in order (entry k of every row at step k), which is the order of the
kernels' thread per vertex.  The energy total is a plain sum here (the kernels: lanes, wavefronts, workgroups)."""

import functools

import numpy as np

SWEEPS = 5  # DEODR_HIP_ARAP_SWEEPS
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
THETA_BIG = 1e150  # above it theta^2 would overflow: t = 1 / (2 theta)
BLOCK, MAX_BLOCKS, FH_BLOCK = 256, 512, 256  # DEODR_HIP_ARAP_BLOCK, DEODR_HIP_ARAP_MAX_BLOCKS; the threads grid_sum adds the partials with
LD = np.longdouble

# The largest error of a float64 run of this restatement against the long-double run over the parity tables (tests/test_arap_reference.py measures
# it again and asserts it is within these figures): the gradient relative to g_scale, the energy relative to e_scale, the quaternion components
# absolute.  Measured: gradient 5.9e-16, energy 1.3e-16, quaternions 6.4e-15 (the smallest gamma of the tables is 7.0e-3).
F64_GRADIENT, F64_ENERGY, F64_QUATERNION = 6e-16, 1.5e-16, 7e-15
MARGIN = 8  # the project's margin between the measured float64 error and a GPU tolerance (the basis kernels)
TOL_GRADIENT, TOL_ENERGY, TOL_QUATERNION = MARGIN * F64_GRADIENT, MARGIN * F64_ENERGY, MARGIN * F64_QUATERNION
GAMMA_MIN = 1e-3


# ---- the operation ----------------------------------------------------------------------------------------------------------------------


def horn(S):
    """S [...,3,3] -> Horn's symmetric 4 x 4 matrix [...,4,4] whose top eigenvector (w, x, y, z) is the rotation that maximises tr(R^T S)"""
    N = np.zeros(S.shape[:-2] + (4, 4), dtype=S.dtype)
    xx, xy, xz, yx, yy, yz, zx, zy, zz = (S[..., a, b] for a in range(3) for b in range(3))
    N[..., 0, 0] = (xx + yy) + zz
    N[..., 0, 1] = zy - yz
    N[..., 0, 2] = xz - zx
    N[..., 0, 3] = yx - xy
    N[..., 1, 1] = (xx - yy) - zz
    N[..., 1, 2] = xy + yx
    N[..., 1, 3] = zx + xz
    N[..., 2, 2] = (yy - xx) - zz
    N[..., 2, 3] = yz + zy
    N[..., 3, 3] = (zz - xx) - yy
    for a in range(4):
        for b in range(a):
            N[..., a, b] = N[..., b, a]
    return N


def jacobi(N, sweeps=SWEEPS):
    """cyclic Jacobi on the symmetric N [...,4,4] -> (eigenvalues [...,4] (the diagonal), eigenvectors [...,4,4] in columns, off-diagonal norm / norm)"""
    A, E = N.copy(), np.zeros_like(N)
    one = N.dtype.type(1)
    for a in range(4):
        E[..., a, a] = one
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for _ in range(sweeps):
            for p, q in PAIRS:
                apq = A[..., p, q].copy()
                skip = apq == 0
                theta = (A[..., q, q] - A[..., p, p]) / (2 * np.where(skip, one, apq))
                big = ~(np.abs(theta) <= THETA_BIG)
                th = np.where(big, one, theta)
                t = np.where(th >= 0, one, -one) / (np.abs(th) + np.sqrt(th * th + one))
                t = np.where(big, one / (2 * theta), t)
                t = np.where(skip, 0 * one, t)
                c = one / np.sqrt(t * t + one)
                s = t * c
                A[..., p, p] = A[..., p, p] - t * apq
                A[..., q, q] = A[..., q, q] + t * apq
                A[..., p, q] = A[..., q, p] = 0
                for r in range(4):
                    if r != p and r != q:
                        arp, arq = A[..., r, p].copy(), A[..., r, q].copy()
                        A[..., r, p] = A[..., p, r] = c * arp - s * arq
                        A[..., r, q] = A[..., q, r] = s * arp + c * arq
                    erp, erq = E[..., r, p].copy(), E[..., r, q].copy()
                    E[..., r, p] = c * erp - s * erq
                    E[..., r, q] = s * erp + c * erq
    lam = np.stack([A[..., a, a] for a in range(4)], axis=-1)
    off = np.sqrt(sum(A[..., a, b] ** 2 for a in range(4) for b in range(4) if a != b))
    norm = np.sqrt((N * N).sum(axis=(-1, -2)))
    return lam, E, off / np.where(norm > 0, norm, one)


def top_quaternion(lam, E):
    """-> (x, y, z, w) [...,4] with w >= 0: the column of E of the largest eigenvalue, ties to the lowest index"""
    best, col = lam[..., 0], E[..., :, 0]
    for k in range(1, 4):
        better = lam[..., k] > best
        best = np.where(better, lam[..., k], best)
        col = np.where(better[..., None], E[..., :, k], col)
    col = np.where((col[..., 0] < 0)[..., None], -col, col)
    return np.stack((col[..., 1], col[..., 2], col[..., 3], col[..., 0]), axis=-1)


def rotation_matrix(quat):
    """(x, y, z, w) [...,4] -> R [...,3,3]"""
    x, y, z, w = (quat[..., a] for a in range(4))
    R = np.empty(quat.shape[:-1] + (3, 3), dtype=quat.dtype)
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return R


def _entries(offsets, cols, weights, dtype):
    """the entries of every row, step by step: yields (live [V], j [V], w [V]) for k = 0, 1, ... (dead entries: j = the row itself, w = 0)"""
    offsets = np.asarray(offsets).astype(np.int64)
    deg, V = np.diff(offsets), len(offsets) - 1
    for k in range(int(deg.max()) if V and len(cols) else 0):
        live = k < deg
        at = np.where(live, offsets[:-1] + k, 0)
        yield live, np.where(live, np.asarray(cols).astype(np.int64)[at], np.arange(V)), np.where(live, np.asarray(weights, dtype=dtype)[at], dtype(0))


def cell_matrices(offsets, cols, weights, q, p, dtype=LD):
    """S [n,V,3,3]"""
    q, p = np.asarray(q, dtype=dtype), np.asarray(p, dtype=dtype)
    S = np.zeros(p.shape[:2] + (3, 3), dtype=dtype)
    for _, j, w in _entries(offsets, cols, weights, dtype):
        ep, eq = p - p[:, j], q - q[j]
        S = S + w[None, :, None, None] * (ep[..., :, None] * eq[None, :, None, :])
    return S


def arap(offsets, cols, weights, q, p, cregu, dtype=LD, sweeps=SWEEPS, rotations=None):
    """-> (energy [n], gradient [n,V,3], quaternions [n,V,4] (x, y, z, w)) in ``dtype``.  ``rotations`` [n,V,3,3]: use these in place of the ones
    Horn + Jacobi give (the Kabsch / SVD comparison)"""
    dtype = np.dtype(dtype).type
    q, p = np.asarray(q, dtype=dtype), np.asarray(p, dtype=dtype)
    p = p[None] if p.ndim == 2 else p
    quat = None
    if rotations is None:
        lam, E, _ = jacobi(horn(cell_matrices(offsets, cols, weights, q, p, dtype)), sweeps)
        quat = top_quaternion(lam, E)
        R = rotation_matrix(quat)
    else:
        R = np.asarray(rotations, dtype=dtype)
    rot = lambda R, e: np.stack([(R[..., a, 0] * e[..., 0] + R[..., a, 1] * e[..., 1]) + R[..., a, 2] * e[..., 2] for a in range(3)], axis=-1)
    cell, g = np.zeros(p.shape[:2], dtype=dtype), np.zeros_like(p)
    for _, j, w in _entries(offsets, cols, weights, dtype):
        ep, eq = p - p[:, j], np.broadcast_to(q - q[j], p.shape)
        d, dj = ep - rot(R, eq), ep - rot(R[:, j], eq)
        cell = cell + w * ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        g = g + w[None, :, None] * (d + dj)
    c = dtype(cregu)
    return (c / 2) * cell.sum(axis=1), c * g, quat


def kabsch(S):
    """the rotations of the cells by NumPy's SVD (float64): R = U diag(1, 1, det(U V^T)) V^T; identity where S = 0"""
    S = np.asarray(S, dtype=np.float64)
    U, _, Vt = np.linalg.svd(S)
    D = np.ones(S.shape[:-2] + (3,))
    D[..., 2] = np.sign(np.linalg.det(U @ Vt))
    R = (U * D[..., None, :]) @ Vt
    zero = ~np.any(S.reshape(S.shape[:-2] + (9,)) != 0, axis=-1)
    R[zero] = np.eye(3)
    return R


def gamma(S):
    """the conditioning of every cell: (sigma_2 + sign(det S) sigma_3) / sigma_1; inf where S = 0 exactly.  The rotation's error grows like
    1 / gamma, at 0 the rotation is not unique"""
    S = np.asarray(S, dtype=np.float64)
    s = np.linalg.svd(S, compute_uv=False)
    zero = s[..., 0] == 0
    g = (s[..., 1] + np.sign(np.linalg.det(S)) * s[..., 2]) / np.where(zero, 1.0, s[..., 0])
    return np.where(zero, np.inf, g)


def scales(offsets, cols, weights, q, p, cregu):
    """(e_scale [n], g_scale [n]): the magnitudes of the terms that cancel -- 1/2 c sum w (|e^p| + |e^q|)^2 and c max_i sum_j w (|e^p| + |e^q|)"""
    q, p = np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64)
    p = p[None] if p.ndim == 2 else p
    row, tot = np.zeros(p.shape[:2]), np.zeros(p.shape[:2])
    for _, j, w in _entries(offsets, cols, weights, np.float64):
        m = np.linalg.norm(p - p[:, j], axis=-1) + np.linalg.norm(q - q[j], axis=-1)[None]
        row, tot = row + w * m, tot + w * m * m
    return 0.5 * cregu * tot.sum(axis=1), cregu * row.max(axis=1)


def quaternion_distance(a, b):
    """per component distance of unit quaternions up to the sign rule (w >= 0 leaves the sign open where w = 0) -> the largest"""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.minimum(np.abs(a - b).max(axis=-1), np.abs(a + b).max(axis=-1)).max()) if a.size else 0.0


# ---- meshes -----------------------------------------------------------------------------------------------------------------------------


def adjacency(faces, V, weights=None):
    """the vertex adjacency of a face list in compressed rows: (offsets [V+1] uint32, cols [nnz] uint32, weights [nnz] float64 -- uniform 1, or
    ``weights(i, j)`` symmetric), the columns of a row ascending, no diagonal"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    pairs = np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]], f[:, [1, 0]], f[:, [2, 1]], f[:, [0, 2]])) if len(f) else np.zeros((0, 2), dtype=np.int64)
    pairs = np.unique(pairs, axis=0)
    offsets = np.concatenate(([0], np.cumsum(np.bincount(pairs[:, 0], minlength=V)))).astype(np.uint32)
    w = np.ones(len(pairs)) if weights is None else np.array([weights(min(i, j), max(i, j)) for i, j in pairs], dtype=np.float64)
    return offsets, pairs[:, 1].astype(np.uint32), w


def _icosphere(level):
    t = (1 + 5**0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]  # fmt: skip
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * np.array([1.0, 0.8, 1.3]), np.array(f)  # (an ellipsoid: no ring keeps an exact symmetry)


def strip(V):
    """an open triangle strip of V >= 3 vertices in the plane z = 0, slightly sheared: valences 2, 3 and 4"""
    i = np.arange(V)
    q = np.stack((0.5 * i + 0.07 * (i % 2), 0.9 * (i % 2) + 0.01 * np.sin(0.7 * i), np.zeros(V)), axis=1)
    return q, np.stack((i[:-2], i[1:-1], i[2:]), axis=1)


def fan(valence):
    """a closed fan: a hub of the given valence and its rim (valence 3), the rim an uneven, slightly conical polygon"""
    k = np.arange(valence)
    a = 2 * np.pi * (k + 0.2 * np.sin(1.3 * k)) / valence
    r = 1 + 0.15 * np.cos(2.1 * k)
    q = np.concatenate(([[0.03, -0.02, 0.25]], np.stack((r * np.cos(a), r * np.sin(a), 0.05 * np.sin(1.7 * k)), axis=1)))
    return q, np.stack((np.zeros(valence, dtype=np.int64), 1 + k, 1 + (k + 1) % valence), axis=1)


FAN_VALENCES = (7, 8, 9, 16, 17, 40)
MESHES = ("vertex", "triangle", "tetrahedron", "icosphere42", "icosphere162", "strip23") + tuple(f"fan{v}" for v in FAN_VALENCES)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """-> (q [V,3], faces [T,3], (offsets, cols, weights)); `name` one of MESHES or "strip<V>" """
    if name == "vertex":
        q, f = np.array([[0.3, -0.2, 0.5]]), np.zeros((0, 3), dtype=np.int64)
    elif name == "triangle":
        q, f = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.3, 0.8, 0.2]]), np.array([[0, 1, 2]])
    elif name == "tetrahedron":  # (irregular: a regular one has sigma_2 = sigma_3 in every ring, and its mirror image no unique rotation)
        q, f = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.1], [0.2, 0.9, 0.0], [0.3, 0.2, 1.4]]), np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    elif name.startswith("icosphere"):
        q, f = _icosphere({"42": 1, "162": 2}[name[9:]])
    elif name.startswith("strip"):
        q, f = strip(int(name[5:]))
    elif name.startswith("fan"):
        q, f = fan(int(name[3:]))
    else:
        raise KeyError(name)
    q.setflags(write=False)
    return q, f, adjacency(f, len(q))


def edge_length(name):
    q, _, (offsets, cols, _) = mesh(name)
    rows = np.repeat(np.arange(len(q)), np.diff(offsets.astype(np.int64)))
    return float(np.linalg.norm(q[rows] - q[cols.astype(np.int64)], axis=1).mean()) if len(cols) else 1.0


# ---- deformations -----------------------------------------------------------------------------------------------------------------------


def axis_rotation(axis, degrees):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


RIGID_170 = axis_rotation((0.3, -0.5, 0.8), 170.0)
DEFORMATIONS = ("rest", "translation", "rigid170", "bend", "noise1", "noise30", "mirror", "coincident")
PARITY_DEFORMATIONS = DEFORMATIONS  # (rest and coincident: S is symmetric or 0; their exact contract is tested on its own as well)
POSE_GROUPS = (("rest",), ("translation", "rigid170"), ("bend", "noise1", "noise30"), ("mirror", "coincident", "rigid170"))  # n = 1, 2, 3, 3


def bend(q, radius=3.0):
    """the plane z = 0 rolled isometrically onto a cylinder about the y axis: a rotation by x / radius that varies smoothly along x"""
    a = q[:, 0] / radius
    return np.stack(((radius - q[:, 2]) * np.sin(a), q[:, 1], radius - (radius - q[:, 2]) * np.cos(a)), axis=1)


def deform(name, how, seed=0):
    q = mesh(name)[0]
    if how == "rest":
        return q.copy()
    if how == "translation":
        return q + np.array([0.25, -1.5, 3.0])
    if how == "rigid170":
        return q @ RIGID_170.T + np.array([0.1, 0.2, -0.3])
    if how == "bend":
        return bend(q)
    if how in ("noise1", "noise30"):
        rng = np.random.default_rng([seed, len(q), int(how[5:])])
        return q + 0.01 * int(how[5:]) * edge_length(name) * rng.uniform(-1, 1, q.shape)
    if how == "mirror":
        return q * np.array([-1.0, 1.0, 1.0])
    if how == "coincident":
        return np.broadcast_to(np.array([0.5, 0.25, -2.0]), q.shape).copy()
    raise KeyError(how)


CREGU = 3.0


@functools.lru_cache(maxsize=None)
def case(name, hows, seed=0):
    """the poses `hows` of mesh `name` -> a dict: the tables, q, p [n,V,3], cregu, the long-double energy / gradient / quaternions, the scales.
    Asserts the condition of the parity tables: every cell has gamma >= GAMMA_MIN or S = 0 exactly.  Computed once and shared: do not modify."""
    q, faces, (offsets, cols, weights) = mesh(name)
    p = np.stack([deform(name, how, seed) for how in hows])
    S = cell_matrices(offsets, cols, weights, q, p, np.float64)
    g = gamma(S)
    assert g.min() >= GAMMA_MIN, (name, hows, float(g.min()))
    energy, gradient, quat = arap(offsets, cols, weights, q, p, CREGU)
    e_scale, g_scale = scales(offsets, cols, weights, q, p, CREGU)
    out = dict(name=name, hows=hows, q=q, faces=faces, offsets=offsets, cols=cols, weights=weights, p=p, cregu=CREGU, energy=energy, gradient=gradient,
               quaternions=quat, e_scale=e_scale, g_scale=g_scale, gamma=g, S=S)  # fmt: skip
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def boundary_sizes(blocks, block, max_blocks):
    """the V at which the launch geometry changes, found from the exported rule ``blocks(V)`` alone: one below, at and one above a workgroup's worth
    of vertices; the first V whose partials need a second round of the last workgroup of grid_sum (more workgroups than FH_BLOCK threads); the
    first V beyond the grid cap (the threads stride)"""

    def first(pred, hi=1 << 30):  # the least V with pred(V), pred monotone
        lo = 1
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if pred(mid) else (mid + 1, hi)
        return lo

    two = first(lambda V: blocks(V) >= 2)  # = block + 1
    assert two == block + 1
    second_round = first(lambda V: blocks(V) > FH_BLOCK)
    capped = first(lambda V: blocks(V) >= max_blocks)  # the first V that reaches the cap; one full workgroup more and the threads stride
    beyond = capped + block
    assert blocks(beyond) == blocks(capped) == max_blocks and -(-beyond // block) == max_blocks + 1
    return [two - 2, two - 1, two, second_round, beyond]


def parity_cases():
    """(mesh, poses) of the parity tables: every mesh x every deformation, in groups of n = 1, 2, 3, 3 poses"""
    return [(name, hows) for name in MESHES for hows in POSE_GROUPS]


def errors(c, energy, gradient, quaternions=None):
    """the errors of a result against the long-double one of case `c`, in the units of the tolerances: (energy / e_scale, gradient / g_scale,
    quaternion components).  Where a scale is 0 (one vertex) the error must be 0 and counts as such."""
    safe = lambda s: np.where(s > 0, s, 1.0)
    e = np.abs(np.asarray(energy, dtype=LD) - c["energy"]) / safe(c["e_scale"])
    g = np.abs(np.asarray(gradient, dtype=LD) - c["gradient"]).max(axis=(1, 2)) / safe(c["g_scale"])
    return float(e.max()), float(g.max()), (quaternion_distance(quaternions, c["quaternions"]) if quaternions is not None else 0.0)
