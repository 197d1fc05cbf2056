"""NumPy restatement of the point-to-surface distance of include/deodr_hip_surface.h, for the tests.

The closest face, the barycentric coordinates and d2 come from float64 with exactly the header's operation sequence -- NumPy rounds each operation
and the library is built without contraction, so the kernels' ``nearest_face`` must be EQUAL to these and ``barycentric`` bit-equal, not close, and
the set of truncated pairs with them.  Ties between faces are the rule on a closed mesh (a closest point on a shared vertex or edge): ``argmin``
takes the first occurrence, the lowest face.  The mesh -> points side is tests/chamfer_reference.py's.  The sums of the terms and of the gradient
are in ``np.longdouble``; ``evaluate(..., dtype=np.float64)`` is the same code in float64 with the sums taken one after the other, the gradient of
a vertex over its corners in table order and per corner in increasing k.  tests/test_surface_reference.py measures its distance to the long-double
values over ``parity_cases()``, and the values it printed, rounded up, are ``TOL_TERMS`` and ``TOL_GRADIENT`` below.  The GPU tests allow 8 x
that (``GPU_TOL_*``), the project's factor.

The error measures.  Terms and loss: relative to ``|mix_0| term_0 + |mix_1| term_1``.  Gradient: the largest component error of a vertex relative to
``g_scale_i = 2 (|mix_0| sum w_k bary_c |q_k - p_k| + |mix_1| u_i |v_i - p_k*|)`` (Euclidean norms, the pairs within ``max_distance`` whose closest
face has vertex i as corner c); where ``g_scale_i`` is 0 the gradient must be 0 exactly."""

import numpy as np

import chamfer_reference as cr

LD = np.longdouble
BLOCK, TILE, MAX_BLOCKS, FH_BLOCK = cr.BLOCK, cr.TILE, cr.MAX_BLOCKS, cr.FH_BLOCK
CHUNK = 1 << 17  # (point, face) pairs at once
segments, change_points, relative = cr.segments, cr.change_points, cr.relative

# Measured by tests/test_surface_reference.py::test_float64_error_is_measured_and_inside_the_tolerances over parity_cases() (it prints them):
# terms 2.11e-15 (5 000 weighted distances added one after the other), gradient 1.44e-15 (the octahedron: a vertex adds the two rounded products
# of some 3 000 points one after the other).  Rounded up:
TOL_TERMS, TOL_GRADIENT = 3e-15, 2e-15
GPU_TOL_TERMS, GPU_TOL_GRADIENT = 8 * TOL_TERMS, 8 * TOL_GRADIENT


def scratch_bytes(V, F, P, n):
    sp, sg, sv = segments(P, F) * P, segments(F, P) * F, segments(V, P) * V
    return 64 + 8 * (n * (16 * F + sp + 6 * P + 9 * sg + sv + 2 * MAX_BLOCKS) + (n * (sp + sv + P + 2) + 1) // 2)


def corner_table(faces, V):
    """(offsets [V + 1], corners [3 F]): for vertex i the entries 3 f + c with faces[f][c] == i, in increasing order -- by a plain loop"""
    rows = [[] for _ in range(V)]
    for f, face in enumerate(np.asarray(faces)):
        for c, i in enumerate(face):
            rows[int(i)].append(3 * f + c)
    offsets = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    return offsets, np.array([e for r in rows for e in r], dtype=np.int32)


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def closest(p, a, b, c, want_region=False):
    """float64 arrays broadcastable to [..., 3] -> (v, w, e [..., 3], d2) by the header's sequence; ``want_region``: also the region taken, 0 .. 6 =
    A, B, AB, C, AC, BC, interior"""
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e_ab, e_ac, e_b, e_c = d1 - d3, d2 - d6, d4 - d3, d5 - d6
        e_bc, den = e_b + e_c, (va + vb) + vc
        conditions = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0) & (e_ab > 0), (d6 >= 0) & (d5 <= d6),
                      (vb <= 0) & (d2 >= 0) & (d6 <= 0) & (e_ac > 0), (va <= 0) & (e_b >= 0) & (e_c >= 0) & (e_bc > 0)]  # fmt: skip
        region = np.full(np.broadcast(d1, d1).shape, 6)
        for r in range(5, -1, -1):  # (the first that holds wins: assigned last)
            region = np.where(conditions[r], r, region)
        ok = den != 0
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        v_num = np.select([region == 1, region == 2, (region == 6) & ok], [one, d1, vb], zero)
        v_den = np.select([region == 2, (region == 6) & ok], [e_ab, den], one)
        w_num = np.select([region == 3, region == 4, region == 5, (region == 6) & ok], [one, d2, e_b, vc], zero)
        w_den = np.select([region == 4, region == 5, (region == 6) & ok], [e_ac, e_bc, den], one)
        w = w_num / w_den
        v = np.where(region == 5, 1.0 - w, v_num / v_den)
        e = ((a + v[..., None] * ab) + w[..., None] * ac) - p
        dist2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    return (v, w, e, dist2, region) if want_region else (v, w, e, dist2)


def nearest_face(p, a, b, c):
    """float64 p [P,3], a, b, c [F,3] -> (d2 [P], face [P], v, w [P], e [P,3]): the lowest face of the minimum (np.argmin: the first occurrence)"""
    P, F = len(p), len(a)
    best, arg, bv, bw, be = np.empty(P), np.empty(P, dtype=np.int64), np.empty(P), np.empty(P), np.empty((P, 3))
    step = max(1, CHUNK // F)
    for at in range(0, P, step):
        v, w, e, d2 = closest(p[at : at + step, None, :], a[None], b[None], c[None])
        f = d2.argmin(axis=1)
        rows = np.arange(len(f))
        arg[at : at + step], best[at : at + step], bv[at : at + step], bw[at : at + step], be[at : at + step] = f, d2[rows, f], v[rows, f], w[rows, f], e[rows, f]
    return best, arg, bv, bw, be


def _chain(indices, values, size, dtype):
    """out[indices[j]] += values[j] one after the other in the order given (np.add.at), in ``dtype``"""
    out = np.zeros((size,) + values.shape[1:], dtype=dtype)
    np.add.at(out, indices, values.astype(dtype))
    return out


def evaluate(vertices, faces, points, params, point_weights=None, vertex_weights=None, directions=3, dtype=LD):
    """-> dict(terms [n,2], loss [n], vertices_b [n,V,3], g_scale [n,V] in ``dtype``; nearest_face [n,P], barycentric [n,P,3] float64, nearest_point
    [n,V] (None for a direction that is off); near_p [n,P], near_v [n,V] bool: the pairs within max_distance)"""
    v, p = np.ascontiguousarray(vertices, dtype=np.float64), np.ascontiguousarray(points, dtype=np.float64)
    faces = np.asarray(faces, dtype=np.int64)
    n, V, P = v.shape[0], v.shape[1], p.shape[1]
    mix0, mix1, tau = (np.float64(x) for x in params)
    tau2 = tau * tau
    w = np.ones((n, P)) if point_weights is None else np.asarray(point_weights, dtype=np.float64)
    u = np.ones(V) if vertex_weights is None else np.asarray(vertex_weights, dtype=np.float64)
    out = dict(terms=np.zeros((n, 2), dtype=dtype), loss=np.zeros(n, dtype=dtype), vertices_b=np.zeros((n, V, 3), dtype=dtype), g_scale=np.zeros((n, V), dtype=dtype),
               nearest_face=np.zeros((n, P), dtype=np.int64) if directions & 1 else None, barycentric=np.zeros((n, P, 3)) if directions & 1 else None,
               nearest_point=np.zeros((n, V), dtype=np.int64) if directions & 2 else None, near_p=np.zeros((n, P), dtype=bool), near_v=np.zeros((n, V), dtype=bool))  # fmt: skip
    two = dtype(2)
    for b in range(n):
        if directions & 1:
            d2, f, bv, bw, e = nearest_face(p[b], v[b][faces[:, 0]], v[b][faces[:, 1]], v[b][faces[:, 2]])
            bary = np.stack(((1.0 - bv) - bw, bv, bw), axis=-1)
            near = d2 <= tau2
            out["nearest_face"][b], out["barycentric"][b], out["near_p"][b] = f, bary, near
            out["terms"][b, 0] = cr._sum(w[b].astype(dtype) * np.where(near, d2, tau2).astype(dtype), dtype)
            # float64: ((2 w) * bary_c) * e as the kernels round it; long double: the same products of the float64 bary and e, unrounded
            scale = (2.0 * w[b])[:, None] * bary if dtype != LD else (two * w[b].astype(dtype))[:, None] * bary.astype(dtype)
            pull = scale[:, :, None].astype(dtype) * e[:, None, :].astype(dtype)  # [P, corner, xyz]
            k = np.flatnonzero(near)
            entry, vertex = (3 * f[k, None] + np.arange(3)[None]).reshape(-1), faces[f[k]].reshape(-1)  # per (k, c): the table entry 3 f + c and its vertex
            order = np.lexsort((np.repeat(k, 3), entry, vertex))  # a vertex's corners in table order, per corner increasing k
            flat = pull[k].reshape(-1, 3)[order]
            out["vertices_b"][b] += dtype(mix0) * _chain(vertex[order], flat, V, dtype)
            out["g_scale"][b] += dtype(abs(mix0)) * _chain(vertex[order], np.sqrt((flat * flat).sum(axis=1)), V, dtype)
        if directions & 2:
            d2, k = cr.nearest(v[b], p[b])
            near = d2 <= tau2
            out["nearest_point"][b], out["near_v"][b] = k, near
            out["terms"][b, 1] = cr._sum(u.astype(dtype) * np.where(near, d2, tau2).astype(dtype), dtype)
            pull = (two * (u * near).astype(dtype))[:, None] * (v[b].astype(dtype) - p[b].astype(dtype)[k])
            out["vertices_b"][b] += dtype(mix1) * pull
            out["g_scale"][b] += dtype(abs(mix1)) * np.sqrt((pull * pull).sum(axis=1))
        out["loss"][b] = (dtype(mix0) * out["terms"][b, 0] if directions & 1 else 0) + (dtype(mix1) * out["terms"][b, 1] if directions & 2 else 0)
    return out


def errors(c, terms, loss, vertices_b, nearest_face=None, barycentric=None, nearest_point=None):
    """a result against the case's long-double values -> (terms and loss relative to |mix_0| term_0 + |mix_1| term_1, gradient relative to g_scale);
    the indices that are given must be EQUAL, the barycentric coordinates bit-equal"""
    ref = c["ref"]
    for name, got in (("nearest_face", nearest_face), ("nearest_point", nearest_point)):
        if got is not None:
            assert ref[name] is not None and np.array_equal(np.asarray(got).astype(np.int64) & 0xFFFFFFFF, ref[name]), (c["name"], name)
    if barycentric is not None:
        got = np.ascontiguousarray(barycentric, dtype=np.float64)
        assert np.array_equal(got.view(np.int64), np.ascontiguousarray(ref["barycentric"]).view(np.int64)), (c["name"], "barycentric")
    mix0, mix1 = abs(LD(c["params"][0])), abs(LD(c["params"][1]))
    t = np.asarray(terms).astype(LD)
    e_terms = max(relative(t[:, 0] - ref["terms"][:, 0], ref["terms"][:, 0]), relative(t[:, 1] - ref["terms"][:, 1], ref["terms"][:, 1]),
                  relative(np.asarray(loss).astype(LD) - ref["loss"], mix0 * ref["terms"][:, 0] + mix1 * ref["terms"][:, 1]))  # fmt: skip
    e_grad = relative(np.abs(np.asarray(vertices_b).astype(LD) - ref["vertices_b"]).max(axis=-1), ref["g_scale"])
    return e_terms, e_grad


# ---- meshes


def soup_faces(V, F, rs):
    """F triangles of three distinct vertices each (V >= 3), or whatever V allows"""
    if V < 3:
        return rs.randint(V, size=(F, 3))
    i0, o1 = rs.randint(V, size=F), 1 + rs.randint(V - 2, size=F)
    o2 = o1 + 1 + (rs.randint(V, size=F) % (V - 1 - o1))
    return np.stack((i0, (i0 + o1) % V, (i0 + o2) % V), axis=1)


OCTAHEDRON_V = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
OCTAHEDRON_F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])


def sphere(levels):
    """the octahedron subdivided ``levels`` times, on the unit sphere: 8 * 4^levels faces"""
    v, f = [tuple(x) for x in OCTAHEDRON_V], OCTAHEDRON_F.tolist()
    for _ in range(levels):
        index, mid, out = {x: i for i, x in enumerate(v)}, {}, []

        def middle(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = np.array(v[i]) + np.array(v[j])
                v.append(tuple(m / np.sqrt((m * m).sum())))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [[a, ab, ca], [ab, b, bc], [ca, bc, c], [ab, bc, ca]]
        f = out
    return np.array(v), np.array(f)


def outside_points(vertices, count, rs, special=True):
    """points outside the unit ball around a closed mesh on it: random directions, and (``special``) beyond vertices and beyond edge midpoints of
    the octahedron's axes, where several faces share the closest point exactly"""
    d = rs.randn(count, 3)
    p = d / np.sqrt((d * d).sum(axis=1))[:, None] * (1.5 + rs.rand(count, 1))
    if special and count >= 20:
        p[:6] = 2.0 * OCTAHEDRON_V
        p[6:12] = 3.0 * vertices[rs.randint(len(vertices), size=6)]
        p[12:16] = np.array([[1.5, 1.5, 0], [0, -1.5, 1.5], [-2.0, 0, 2.0], [0, 1.25, -1.25]])
    return p


def grid_mesh(nx, ny):
    """an integer-coordinate height field: every product and quotient the closest-point sequence forms on the points of exact_points() is exact"""
    xs, ys = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    v = np.stack((2.0 * xs, 2.0 * ys, ((xs * ys) % 3).astype(np.float64) * 2.0), axis=-1).reshape(-1, 3)
    idx = lambda i, j: i * ny + j
    f = [[idx(i, j), idx(i + 1, j), idx(i, j + 1)] for i in range(nx - 1) for j in range(ny - 1)] + \
        [[idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)] for i in range(nx - 1) for j in range(ny - 1)]  # fmt: skip
    return v, np.array(f)


def exact_points(v, f):
    """points bit-equal to vertices, to edge midpoints and to a + ab / 4 + ac / 2 inside faces (exact on integer coordinates)"""
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return np.concatenate((v, 0.5 * (a + b), 0.5 * (b + c), 0.5 * (a + c), a + 0.25 * (b - a) + 0.5 * (c - a)))


def case(F=None, P=None, n=1, seed=0, V=37, weights="random", kind="soup", max_distance=np.inf, mix=(0.7, 1.3), directions=3, name=None):
    """a problem and its long-double values.  ``kind``:
    "soup"        V vertices uniform in the unit cube, F random triangles, P points uniform in a slightly larger cube (all seven regions occur);
    "octahedron"  the octahedron (F = 8) with P outside points: many exact ties, and every point chooses among 8 faces;
    "sphere"      the octahedron subdivided 3 times (F = 512: two LDS tiles, and with few points two segments) with P outside points;
    "exact"       an integer-coordinate grid mesh, two exactly collinear triangles in front, with the points of exact_points(): e == 0, bit for bit;
    "degenerate"  a soup whose first faces have zero area -- (i, i, j), (i, i, i), three collinear vertices -- and face 0 = (i, i, j) an edge of
                  face 3, so that the zero-area face has the lowest index of an exact tie; P points, a third of them beyond that edge;
    "fan"         100 triangles around vertex 0 (more corners than a wavefront) and two vertices no face uses.
    ``weights``: "random", None (NULL) or "zeros" (a third of each at 0).  ``max_distance``: a value, "mid" (just above the median distance: about
    half the pairs truncated) or "below" (half the smallest)."""
    rs = np.random.RandomState(seed + 1000 * (F or 0) + 7 * (P or 0) + n)
    if kind == "soup":
        v, faces = rs.rand(n, V, 3), soup_faces(V, F, rs)
    elif kind == "octahedron":
        v, faces = np.repeat(OCTAHEDRON_V[None], n, axis=0), OCTAHEDRON_F
    elif kind == "sphere":
        sv, faces = sphere(3)
        v = np.repeat(sv[None], n, axis=0)
    elif kind == "exact":
        gv, faces = grid_mesh(6, 5)
        # two faces of three distinct, exactly collinear vertices in front (rows of the grid at height 0, in two corner orders): they have the
        # lowest indices of the exact ties along those rows
        faces = np.concatenate(([[0 * 5 + 0, 1 * 5 + 0, 2 * 5 + 0], [3 * 5 + 1, 3 * 5 + 3, 3 * 5 + 2]], faces))
        assert not np.cross(gv[faces[:2, 1]] - gv[faces[:2, 0]], gv[faces[:2, 2]] - gv[faces[:2, 0]]).any()
        v = np.repeat(gv[None], n, axis=0)
    elif kind == "degenerate":
        v, faces = rs.rand(n, V, 3), soup_faces(V, F, rs)
        v[:, 2] = 0.25 * v[:, 0] + 0.75 * v[:, 1]  # (vertex 2 on the segment 0 -- 1, up to rounding)
        faces[:6] = [[0, 0, 1], [5, 5, 5], [0, 2, 1], [0, 1, 7], [4, 9, 9], [8, 3, 8]]
    elif kind == "fan":
        ring = 100
        angles = 2 * np.pi * np.arange(ring) / ring
        fv = np.concatenate(([[0, 0, 0.5]], np.stack((np.cos(angles), np.sin(angles), 0.1 * np.cos(3 * angles)), axis=1), [[3.0, 3, 3], [-3.0, 3, 3]]))
        v, faces = np.repeat(fv[None], n, axis=0) + 0.01 * rs.rand(n, ring + 3, 3), np.array([[0, 1 + i, 1 + (i + 1) % ring] for i in range(ring)])
    else:
        raise AssertionError(kind)
    V, F = v.shape[1], len(faces)
    if kind in ("octahedron", "sphere"):
        p = np.stack([outside_points(v[b], P, rs) for b in range(n)])
    elif kind == "exact":
        p = np.repeat(exact_points(v[0], faces)[None], n, axis=0)
    else:
        p = 1.4 * rs.rand(n, P, 3) - 0.2
        if kind == "degenerate":  # beyond the edge 0 -- 1, on the side away from vertex 7: the closest point is on the edge, faces 0, 2 and 3 tie
            for b in range(n):
                a0, a1, away = v[b, 0], v[b, 1], 0.5 * (v[b, 0] + v[b, 1]) - v[b, 7]
                t = rs.rand(len(p[b, ::3]), 1)
                p[b, ::3] = a0 + t * (a1 - a0) + (0.2 + rs.rand(len(t), 1)) * away
    P = p.shape[1]
    pw = uw = None
    if weights is not None:
        pw, uw = 0.5 + rs.rand(n, P), 0.5 + rs.rand(V)
        if weights == "zeros":
            pw[:, ::3], uw[1::3] = 0.0, 0.0
    if isinstance(max_distance, str):
        d2 = []
        for b in range(n):
            if directions & 1:
                d2.append(nearest_face(p[b], v[b][faces[:, 0]], v[b][faces[:, 1]], v[b][faces[:, 2]])[0])
            if directions & 2:
                d2.append(cr.nearest(v[b], p[b])[0])
        d2 = np.concatenate(d2)
        max_distance = {"mid": 1.000001 * np.sqrt(np.median(d2)), "below": 0.5 * np.sqrt(d2.min())}[max_distance]
        assert max_distance > 0
    params = np.array([mix[0], mix[1], max_distance], dtype=np.float64)
    c = dict(name=name or f"{kind} V={V} F={F} P={P} n={n} weights={weights} max_distance={max_distance:.3g} directions={directions}", vertices=v,
             faces=faces.astype(np.int32), points=p, point_weights=pw, vertex_weights=uw, params=params, directions=directions)  # fmt: skip
    c["ref"] = evaluate(v, faces, p, params, pw, uw, directions)
    return c


SIZES = (1, 2, 63, 64, 65, 255, 256, 257)


def parity_cases():
    """the table the float64 error is measured over (and tests/test_surface_gpu.py runs): (arguments of case)"""
    rows = []
    for i, F in enumerate(SIZES):  # F and P through the sizes: every pairing of a size with its neighbours in the list, n = 1, 2, 3 in turn
        for j, P in enumerate(SIZES):
            if abs(i - j) <= 1 or (i + j) % 4 == 0:
                rows.append(dict(F=F, P=P, n=1 + (i + j) % 3, seed=i + j))
    rows += [dict(F=300, P=700, n=3, seed=5), dict(F=300, P=5000, seed=1), dict(F=1031, P=777, n=2, seed=2),
             dict(kind="octahedron", P=5000), dict(kind="octahedron", P=300, n=2, weights=None), dict(kind="sphere", P=65), dict(kind="sphere", P=1300, n=2),
             dict(kind="exact", n=2), dict(kind="exact", directions=1), dict(kind="degenerate", F=40, P=600), dict(kind="degenerate", F=300, P=257, n=2, V=20),
             dict(kind="fan", P=900), dict(kind="fan", P=300, n=2, max_distance="mid"), dict(kind="fan", P=400, directions=1),
             dict(F=257, P=600, weights=None), dict(F=257, P=600, weights="zeros", n=2), dict(F=400, P=900, max_distance="mid", n=2),
             dict(F=400, P=900, max_distance="below"), dict(F=130, P=2100, directions=1, max_distance="mid"), dict(F=130, P=2100, directions=1),
             dict(F=200, P=130, V=2100, directions=2), dict(F=3, P=400, V=3), dict(F=2, P=100, V=2)]  # fmt: skip
    return rows
