"""NumPy restatement of the closest-point (Chamfer) energy of include/deodr_hip_chamfer.h, for the tests.

The indices and d2 come from float64 with exactly the header's expression, ``((dx*dx + dy*dy) + dz*dz)`` -- NumPy rounds each operation and the
library is built without contraction, so the kernels' indices must be EQUAL to these, not close, and the set of truncated pairs with them.  The
sums of the terms and of the gradient are in ``np.longdouble``.  ``evaluate(..., dtype=np.float64)`` is the same code in float64 with the sums
taken one after the other (the order with the largest error); tests/test_chamfer_reference.py measures its distance to the long-double values over
the case tables, and the values it printed, rounded up, are ``TOL_TERMS`` and ``TOL_GRADIENT`` below.  The GPU tests allow 8 x that
(``GPU_TOL_*``), as the other kernel families do.

The error measures.  Terms and loss: relative to ``|mix_0| term_0 + |mix_1| term_1`` (sums of non-negative values).  Gradient: the largest
component error of a vertex relative to ``g_scale_i = 2 (|mix_0| sum_{k -> i} w_k |v_i - p_k| + |mix_1| u_i |v_i - p_k*|)`` (Euclidean norms, pairs
within ``max_distance``); where ``g_scale_i`` is 0 the gradient must be 0 exactly."""

import numpy as np

LD = np.longdouble
BLOCK = TILE = FH_BLOCK = 256  # DEODR_HIP_CHAMFER_BLOCK, _TILE and FH_BLOCK of dr_fronthalf.h (tests/test_chamfer_abi.py pins them)
MAX_BLOCKS, TARGET_BLOCKS, MAX_SEGMENTS = 512, 1024, 64
CHUNK = 1 << 22  # distances at once

# Measured by tests/test_chamfer_reference.py::test_float64_error_is_measured_and_inside_the_tolerances over parity_cases() (it prints them):
# terms 5.10e-15 (5 000 weighted distances added one after the other), gradient 3.13e-16.  Rounded up:
TOL_TERMS, TOL_GRADIENT = 6e-15, 4e-16
GPU_TOL_TERMS, GPU_TOL_GRADIENT = 8 * TOL_TERMS, 8 * TOL_GRADIENT


def segments(queries, references):
    """the split rule of the header, restated"""
    if queries <= 0 or references <= 0:
        return 0
    qblocks, tiles = -(-queries // BLOCK), -(-references // TILE)
    return min(tiles, MAX_SEGMENTS, -(-TARGET_BLOCKS // qblocks))


def scratch_bytes(V, P, n):
    sp, sv = segments(P, V) * P, segments(V, P) * V
    return 64 + 8 * (n * (sp + 4 * sv + 2 * MAX_BLOCKS) + (n * (sp + sv + P + 2) + 1) // 2)


def change_points(rule, queries, upto):
    """the numbers of references R <= upto at which rule(queries, R) differs from rule(queries, R - 1)"""
    values = [rule(queries, r) for r in range(1, upto + 1)]
    return [r + 1 for r in range(1, upto) if values[r] != values[r - 1]]


def nearest(q, r):
    """float64 [Q,3], [R,3] -> (d2 [Q], index [Q]): the lowest index of the minimum (np.argmin: the first occurrence)"""
    best, arg = np.empty(len(q)), np.empty(len(q), dtype=np.int64)
    step = max(1, CHUNK // len(r))
    for at in range(0, len(q), step):
        d = q[at : at + step, None, :] - r[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        arg[at : at + step] = d2.argmin(axis=1)
        best[at : at + step] = d2[np.arange(d2.shape[0]), arg[at : at + step]]
    return best, arg


def _sum(values, dtype):
    """long double: NumPy's sum; float64: one after the other, the order with the largest error"""
    values = np.asarray(values, dtype=dtype)
    return values.sum() if dtype == LD else (np.cumsum(values)[-1] if values.size else dtype(0))


def evaluate(vertices, points, params, point_weights=None, vertex_weights=None, directions=3, dtype=LD):
    """-> dict(terms [n,2], loss [n], vertices_b [n,V,3], g_scale [n,V] in ``dtype``; nearest_vertex [n,P], nearest_point [n,V] int64 (None for a
    direction that is off); near_p [n,P], near_v [n,V] bool: the pairs within max_distance)"""
    v, p = np.ascontiguousarray(vertices, dtype=np.float64), np.ascontiguousarray(points, dtype=np.float64)
    n, V, P = v.shape[0], v.shape[1], p.shape[1]
    mix0, mix1, tau = (np.float64(x) for x in params)
    tau2 = tau * tau  # (float64, as the kernels form it)
    w = np.ones((n, P)) if point_weights is None else np.asarray(point_weights, dtype=np.float64)
    u = np.ones(V) if vertex_weights is None else np.asarray(vertex_weights, dtype=np.float64)
    out = dict(terms=np.zeros((n, 2), dtype=dtype), loss=np.zeros(n, dtype=dtype), vertices_b=np.zeros((n, V, 3), dtype=dtype), g_scale=np.zeros((n, V), dtype=dtype),
               nearest_vertex=np.zeros((n, P), dtype=np.int64) if directions & 1 else None, nearest_point=np.zeros((n, V), dtype=np.int64) if directions & 2 else None,
               near_p=np.zeros((n, P), dtype=bool), near_v=np.zeros((n, V), dtype=bool))  # fmt: skip
    two = dtype(2)
    for b in range(n):
        vb, pb = v[b].astype(dtype), p[b].astype(dtype)
        if directions & 1:
            d2, j = nearest(p[b], v[b])
            near = d2 <= tau2
            out["nearest_vertex"][b], out["near_p"][b] = j, near
            out["terms"][b, 0] = _sum(w[b].astype(dtype) * np.where(near, d2, tau2).astype(dtype), dtype)
            pull = (two * (w[b] * near).astype(dtype))[:, None] * (vb[j] - pb)  # increasing k: np.add.at adds in the order of the array
            g = np.zeros((V, 3), dtype=dtype)
            np.add.at(g, j, pull)
            out["vertices_b"][b] += dtype(mix0) * g
            np.add.at(out["g_scale"][b], j, dtype(abs(mix0)) * np.sqrt((pull * pull).sum(axis=1)))
        if directions & 2:
            d2, k = nearest(v[b], p[b])
            near = d2 <= tau2
            out["nearest_point"][b], out["near_v"][b] = k, near
            out["terms"][b, 1] = _sum(u.astype(dtype) * np.where(near, d2, tau2).astype(dtype), dtype)
            pull = (two * (u * near).astype(dtype))[:, None] * (vb - pb[k])
            out["vertices_b"][b] += dtype(mix1) * pull
            out["g_scale"][b] += dtype(abs(mix1)) * np.sqrt((pull * pull).sum(axis=1))
        out["loss"][b] = (dtype(mix0) * out["terms"][b, 0] if directions & 1 else 0) + (dtype(mix1) * out["terms"][b, 1] if directions & 2 else 0)
    return out


def relative(err, scale):
    """max of err / scale; where the scale is 0 the error must be 0 exactly (-> inf otherwise)"""
    err, scale = np.abs(np.asarray(err, dtype=LD)), np.asarray(scale, dtype=LD)
    if not err.size:
        return 0.0
    ratio = np.where(scale > 0, err / np.where(scale > 0, scale, 1), np.where(err > 0, np.inf, 0))
    return float(ratio.max())


def errors(c, terms, loss, vertices_b, nearest_vertex=None, nearest_point=None):
    """a result against the case's long-double values -> (terms and loss relative to |mix_0| term_0 + |mix_1| term_1, gradient relative to g_scale);
    the indices that are given must be EQUAL"""
    ref = c["ref"]
    for name, got in (("nearest_vertex", nearest_vertex), ("nearest_point", nearest_point)):
        if got is not None:
            assert ref[name] is not None and np.array_equal(np.asarray(got).astype(np.int64) & 0xFFFFFFFF, ref[name]), (c["name"], name)
    mix0, mix1 = abs(LD(c["params"][0])), abs(LD(c["params"][1]))
    t = np.asarray(terms).astype(LD)
    e_terms = max(relative(t[:, 0] - ref["terms"][:, 0], ref["terms"][:, 0]), relative(t[:, 1] - ref["terms"][:, 1], ref["terms"][:, 1]),
                  relative(np.asarray(loss).astype(LD) - ref["loss"], mix0 * ref["terms"][:, 0] + mix1 * ref["terms"][:, 1]))  # fmt: skip
    e_grad = relative(np.abs(np.asarray(vertices_b).astype(LD) - ref["vertices_b"]).max(axis=-1), ref["g_scale"])
    return e_terms, e_grad


def case(V, P, n=1, seed=0, weights="random", kind="uniform", max_distance=np.inf, mix=(0.7, 1.3), directions=3, name=None):
    """a problem and its long-double values.  ``kind``: "uniform" (both sets uniform in the unit cube), "clustered" (every point within 1e-3 of one
    of min(V, 300) vertices chosen at random, so a few vertices own them all), "duplicates" (every second vertex a copy of the one TILE / 2 - 1 places
    before it where there is one, every third point likewise: ties across lanes, tiles and segments, where the lowest index must win), "coincident"
    (the points are copies of vertices, bit for bit: d2 == 0).  ``weights``: "random", None (NULL) or "zeros" (a third of each at 0).
    ``max_distance``: a value, "mid" (just above the median nearest distance: about half the pairs truncated) or "below" (half the smallest)."""
    rs = np.random.RandomState(seed + 1000 * V + 7 * P + n)
    v, p = rs.rand(n, V, 3), rs.rand(n, P, 3)
    if kind == "clustered":
        owners = rs.choice(V, size=min(V, 300), replace=False)
        p = v[:, owners[rs.randint(len(owners), size=P)], :] + 1e-3 * (rs.rand(n, P, 3) - 0.5)
    elif kind == "duplicates":
        back = TILE // 2 - 1
        for a, every in ((v, 2), (p, 3)):
            idx = np.arange(back, a.shape[1], every)
            a[:, idx] = a[:, idx - back]
            a[:, -1] = a[:, 0]  # (and one across everything in between)
    elif kind == "coincident":
        p = v[:, rs.randint(V, size=P), :].copy()
    else:
        assert kind == "uniform", kind
    pw = uw = None
    if weights is not None:
        pw, uw = 0.5 + rs.rand(n, P), 0.5 + rs.rand(V)
        if weights == "zeros":
            pw[:, ::3], uw[1::3] = 0.0, 0.0
    if isinstance(max_distance, str):
        d2 = np.concatenate([np.concatenate((nearest(p[b], v[b])[0], nearest(v[b], p[b])[0])) for b in range(n)])
        max_distance = {"mid": 1.000001 * np.sqrt(np.median(d2)), "below": 0.5 * np.sqrt(d2.min())}[max_distance]
        assert max_distance > 0
    params = np.array([mix[0], mix[1], max_distance], dtype=np.float64)
    c = dict(name=name or f"{kind} V={V} P={P} n={n} weights={weights} max_distance={max_distance:.3g} directions={directions}", vertices=v, points=p,
             point_weights=pw, vertex_weights=uw, params=params, directions=directions)  # fmt: skip
    c["ref"] = evaluate(v, p, params, pw, uw, directions)
    return c


def parity_cases():
    """the table the float64 error is measured over (and tests/test_chamfer_gpu.py runs): (arguments of case)"""
    rows = []
    for V, P in ((1, 1), (2, 65), (63, 64), (64, 2), (65, 63), (255, 257), (256, 256), (257, 255), (300, 5000), (1031, 777)):
        for n in (1, 2, 3):
            rows.append(dict(V=V, P=P, n=n, seed=n))
    rows += [dict(V=300, P=5000, kind="clustered"), dict(V=520, P=700, kind="duplicates", n=2), dict(V=97, P=400, kind="coincident"),
             dict(V=257, P=600, weights=None), dict(V=257, P=600, weights="zeros", n=2), dict(V=400, P=900, max_distance="mid", n=2),
             dict(V=400, P=900, max_distance="below"), dict(V=130, P=2100, directions=1, max_distance="mid"), dict(V=2100, P=130, directions=2)]  # fmt: skip
    return rows
