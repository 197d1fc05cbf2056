"""CPU checks of the restatement tests/surface_reference.py of the point-to-surface distance (include/deodr_hip_surface.h): against a dense random
sampling of the triangle (never above it), its gradient against central differences (the bound measured and held), all seven regions from one
triangle, a sweep of zero-area triangles with small integer coordinates (finite, barycentrics in [0, 1], equal to the minimum over the three
segments), ``deodr_amd.surface.surface_distance_torch`` against it (equal faces, bit-equal barycentrics), and the float64-against-long-double error
of the terms and the gradient MEASURED over the case table -- the printed values, rounded up, are ``TOL_TERMS`` / ``TOL_GRADIENT`` of the module,
which the GPU tests multiply by 8; no case is excluded.  Then the fact the operator exists for: on the hand, 4 000 samples of its own surface cost
nothing against the surface and a great deal against the vertices."""

import itertools
import os

import numpy as np
import torch

import surface_reference as sr
from conftest import GOLDEN


def test_never_above_a_dense_sampling_of_the_triangle():
    rs = np.random.RandomState(0)
    T, S = 300, 20000
    a, b, c = rs.randn(T, 3), rs.randn(T, 3), rs.randn(T, 3)
    p = 2 * rs.randn(T, 3)
    d2 = sr.closest(p, a, b, c)[3]
    s, t = rs.rand(S), rs.rand(S)
    s, t = np.where(s + t > 1, 1 - s, s), np.where(s + t > 1, 1 - t, t)
    worst_above, worst_gap = 0.0, 0.0
    for i in range(T):
        q = a[i] + s[:, None] * (b[i] - a[i]) + t[:, None] * (c[i] - a[i])
        sampled = ((q - p[i]) ** 2).sum(axis=1).min()
        worst_above, worst_gap = max(worst_above, (d2[i] - sampled) / sampled), max(worst_gap, (sampled - d2[i]) / sampled)
    print(f"closest point against {S} samples per triangle: above by {worst_above:.2e}, below by at most {worst_gap:.2e} (relative)")
    assert worst_above <= 1e-14  # never above any point of the triangle (rounding apart)
    assert worst_gap <= 0.2  # and the samples come close to it: the same point, not some lower bound


def test_all_seven_regions_from_one_triangle():
    a, b, c = np.array([0.0, 0, 0]), np.array([2.0, 0, 0]), np.array([0.0, 2, 0])
    p = np.array([[-1.0, -1, 1], [3.0, -0.5, 1], [1.0, -1, 1], [-0.5, 3, 1], [-1.0, 1, 1], [2.0, 2, 1], [0.5, 0.5, 1]])
    v, w, e, d2, region = sr.closest(p, a, b, c, want_region=True)
    assert region.tolist() == [0, 1, 2, 3, 4, 5, 6]
    q = a + v[:, None] * (b - a) + w[:, None] * (c - a)
    assert np.array_equal(q, [[0, 0, 0], [2, 0, 0], [1, 0, 0], [0, 2, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 0]])
    assert np.array_equal(d2, [3, 2.25, 2, 2.25, 2, 3, 1]) and np.array_equal(e, q - p)


def segment_d2(p, a, b):
    ab = b - a
    t = 0.0 if not ab.any() else min(1.0, max(0.0, float((p - a) @ ab) / float(ab @ ab)))
    return float(((a + t * ab - p) ** 2).sum())


def test_zero_area_triangles_with_small_integer_coordinates():
    """two equal corners, three equal corners, three distinct collinear corners, every corner order; points on a 4 x 4 x 3 integer grid around them"""
    corners = [np.array(x, dtype=np.float64) for x in ((0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (1, 1, 0), (2, 2, 0), (1, 2, 1), (2, 4, 2))]
    triangles = []
    for i, j, k in itertools.product(range(len(corners)), repeat=3):
        a, b, c = corners[i], corners[j], corners[k]
        if not np.cross(b - a, c - a).any():
            triangles.append((a, b, c))
    kinds = [len({tuple(x) for x in t}) for t in triangles]
    assert kinds.count(1) == 8 and kinds.count(2) > 100 and kinds.count(3) >= 30
    points = np.array(list(itertools.product((-1.0, 0.0, 1.0, 2.5), (-1.0, 0.0, 0.5, 2.0), (0.0, 1.0, -2.0))))
    count = 0
    for a, b, c in triangles:
        v, w, e, d2 = sr.closest(points, a, b, c)
        bary = np.stack(((1 - v) - w, v, w), axis=1)
        assert np.isfinite(v).all() and np.isfinite(w).all() and np.isfinite(d2).all()
        assert bary.min() >= 0 and bary.max() <= 1
        want = [min(segment_d2(p, a, b), segment_d2(p, b, c), segment_d2(p, a, c)) for p in points]
        assert np.allclose(d2, want, rtol=1e-13, atol=0), (a, b, c)
        count += len(points)
    print(f"{len(triangles)} zero-area triangles x {len(points)} points = {count} cases")


def test_gradient_against_central_differences():
    """the envelope-theorem gradient on random triangles across all seven regions (points -> mesh alone, one face: no tie to break)"""
    rs = np.random.RandomState(1)
    T = 700
    tri, p = rs.randn(T, 3, 3), 1.5 * rs.randn(T, 3)
    regions = sr.closest(p, tri[:, 0], tri[:, 1], tri[:, 2], want_region=True)[4]
    assert set(regions.tolist()) == set(range(7))
    loss = lambda t, i: float(sr.closest(p[i], t[0], t[1], t[2])[3])
    h, worst = 1e-6, 0.0
    for i in range(T):
        r = sr.evaluate(tri[i][None], [[0, 1, 2]], p[i][None, None], (1.0, 0.0, np.inf), directions=1)
        g = r["vertices_b"][0].astype(np.float64)
        for corner in range(3):
            for x in range(3):
                e = np.zeros((3, 3))
                e[corner, x] = h
                worst = max(worst, abs((loss(tri[i] + e, i) - loss(tri[i] - e, i)) / (2 * h) - g[corner, x]) / max(1.0, np.abs(g).max()))
    print(f"central differences over {T} triangles, all seven regions: {worst:.2e} relative to max(1, largest gradient entry)")
    assert worst <= 1e-7  # (measured: a few 1e-9, the truncation and rounding of the difference quotient at h = 1e-6)


def test_the_zero_area_face_with_the_lowest_index_wins_its_tie():
    c = sr.case(kind="degenerate", F=40, P=600)
    v, f, p = c["vertices"][0], c["faces"], c["points"][0]
    d2 = np.stack([sr.closest(p, v[f[j, 0]], v[f[j, 1]], v[f[j, 2]])[3] for j in range(len(f))], axis=1)
    mine = c["ref"]["nearest_face"][0] == 0
    assert mine.sum() >= 50 and np.array_equal(d2[mine, 0], d2[mine, 3])  # face 0 = (0, 0, 1) ties with face 3 = (0, 1, 7) bit for bit, and wins
    assert np.isfinite(c["ref"]["barycentric"]).all()
    o = sr.case(kind="octahedron", P=300)
    v, f, p = o["vertices"][0], o["faces"], o["points"][0]
    d2 = np.stack([sr.closest(p, v[f[j, 0]], v[f[j, 1]], v[f[j, 2]])[3] for j in range(8)], axis=1)
    ties = ((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) > 1).mean()
    print(f"octahedron: {100 * ties:.0f} % of the outside points have two or more faces with bit-identical d2")
    assert ties > 0.1 and np.array_equal(o["ref"]["nearest_face"][0], d2.argmin(axis=1))


def test_corner_tables_agree():
    from deodr_amd.surface import corner_table

    for kind in ("soup", "fan", "degenerate"):
        c = sr.case(kind=kind, F=50, P=5)
        V = c["vertices"].shape[1]
        offsets, corners = corner_table(c["faces"], V)
        ro, rc = sr.corner_table(c["faces"], V)
        assert np.array_equal(offsets, ro) and np.array_equal(corners, rc) and offsets.dtype == corners.dtype == np.int32
    fan = sr.case(kind="fan", P=5)
    offsets = sr.corner_table(fan["faces"], fan["vertices"].shape[1])[0]
    assert offsets[1] - offsets[0] == 100 > 64 and offsets[-1] == offsets[-2] == offsets[-3]  # a full ring; two vertices no face uses


def test_restatement_against_surface_distance_torch():
    """a small chunk, so that the chunked search is the one compared"""
    from deodr_amd.surface import surface_distance_torch

    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a))
    worst = [0.0, 0.0]
    for row in sr.parity_cases():
        c = sr.case(**row)
        out = surface_distance_torch(t(c["vertices"]), t(c["faces"]), t(c["points"]), t(c["params"]), t(c["point_weights"]), t(c["vertex_weights"]),
                                     c["directions"], chunk_bytes=1 << 20)  # fmt: skip
        terms, loss, g, nf, bary, npt = (None if o is None else o.numpy() for o in out)
        assert (nf is None) == (bary is None) == (not c["directions"] & 1) and (npt is None) == (not c["directions"] & 2)
        e = sr.errors(c, terms, loss, g, nf, bary, npt)
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert e[0] <= sr.GPU_TOL_TERMS and e[1] <= sr.GPU_TOL_GRADIENT, (c["name"], e)
    print(f"surface_distance_torch against long double: terms {worst[0]:.2e}, gradient {worst[1]:.2e}")


def test_float64_error_is_measured_and_inside_the_tolerances():
    worst = [0.0, 0.0]
    for row in sr.parity_cases():
        c = sr.case(**row)
        f = sr.evaluate(c["vertices"], c["faces"], c["points"], c["params"], c["point_weights"], c["vertex_weights"], c["directions"], dtype=np.float64)
        e = sr.errors(c, f["terms"], f["loss"], f["vertices_b"], f["nearest_face"], f["barycentric"], f["nearest_point"])
        worst = [max(a, b) for a, b in zip(worst, e)]
        zero = c["ref"]["g_scale"] == 0
        assert not f["vertices_b"][zero].any()  # a vertex of g_scale 0 gets exactly 0
    print(f"float64 against long double over {len(sr.parity_cases())} cases: terms {worst[0]:.2e}, gradient {worst[1]:.2e}")
    assert worst[0] <= sr.TOL_TERMS and worst[1] <= sr.TOL_GRADIENT
    assert worst[0] >= sr.TOL_TERMS / 4 and worst[1] >= sr.TOL_GRADIENT / 4  # (the tolerances are the measured values rounded up, not a guess)
    assert (sr.GPU_TOL_TERMS, sr.GPU_TOL_GRADIENT) == (8 * sr.TOL_TERMS, 8 * sr.TOL_GRADIENT)


def test_exact_points_cost_and_pull_exactly_nothing():
    c = sr.case(kind="exact", directions=1)
    assert not c["ref"]["terms"].any() and not c["ref"]["vertices_b"].any() and not c["ref"]["g_scale"].any()
    f = sr.evaluate(c["vertices"], c["faces"], c["points"], c["params"], c["point_weights"], c["vertex_weights"], 1, dtype=np.float64)
    assert not f["terms"].any() and not f["vertices_b"].any()


def test_on_the_hand_surface_samples_cost_nothing_against_the_surface():
    """the motivating fact: 4 000 seeded area-uniform samples of the hand's own surface at the true pose"""
    from deodr_amd import scenes
    from deodr_amd.chamfer import PointCloudTerm
    from deodr_amd.surface import PointSurfaceTerm, sample_surface

    vertices, faces = scenes.load_hand_mesh(os.path.join(GOLDEN, "hand_mesh.npz"))[:2]
    vertices, faces = np.asarray(vertices, dtype=np.float64), np.asarray(faces)
    cloud = sample_surface(vertices, faces, 4000, seed=0)[0]
    variance = vertices.var(axis=0).sum()
    v = torch.as_tensor(vertices)
    surface = PointSurfaceTerm(faces, len(vertices), cloud, directions="points_to_mesh", device="cpu").evaluate(v)[1][0, 0]
    vertex = PointCloudTerm(cloud, directions="points_to_mesh", device="cpu").evaluate(v)[1][0, 0]
    print(f"hand (variance {variance:.4f}), 4 000 surface samples, mean squared distance: to the surface {float(surface):.3e}, to the vertices {float(vertex):.4f}")
    assert float(surface) < 1e-24 * variance
    assert float(vertex) > 0.05 and float(vertex) > 0.05 * variance  # (0.0737, and 0.175 of the variance)
