"""CPU checks of the restatement tests/chamfer_reference.py of the closest-point energy (include/deodr_hip_chamfer.h): it is pinned on
``deodr_amd.chamfer.chamfer_torch`` (equal indices, values within the tolerances) and on central differences of the loss, the tie rules hold on
duplicated vertices and points, and the float64-against-long-double error of the terms and the gradient is MEASURED over the case table -- the
printed values, rounded up, are ``TOL_TERMS`` / ``TOL_GRADIENT`` of the module, which the GPU tests multiply by 8.  No case is excluded."""

import numpy as np
import torch

import chamfer_reference as cr


def torch_result(c, **keywords):
    from deodr_amd.chamfer import chamfer_torch

    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a))
    out = chamfer_torch(t(c["vertices"]), t(c["points"]), t(c["params"]), t(c["point_weights"]), t(c["vertex_weights"]), c["directions"], **keywords)
    return [None if o is None else o.numpy() for o in out]


def test_restatement_against_chamfer_torch():
    """a small chunk, so that the chunked search is the one compared"""
    worst = [0.0, 0.0]
    for row in cr.parity_cases():
        c = cr.case(**row)
        terms, loss, g, nv, npt = torch_result(c, chunk_bytes=1 << 16)
        assert (nv is None) == (not c["directions"] & 1) and (npt is None) == (not c["directions"] & 2)
        e = cr.errors(c, terms, loss, g, nv, npt)
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert e[0] <= cr.GPU_TOL_TERMS and e[1] <= cr.GPU_TOL_GRADIENT, (c["name"], e)
    print(f"chamfer_torch against long double: terms {worst[0]:.2e}, gradient {worst[1]:.2e}")


def test_gradient_against_central_differences():
    """V = 40, P = 90, a finite truncation: exact wherever the nearest neighbours are unique and no pair sits at max_distance"""
    c = cr.case(40, 90, max_distance="mid", seed=3)
    assert 0 < c["ref"]["near_p"].sum() < 90 and 0 < c["ref"]["near_v"].sum() < 40  # truncated pairs and others, both ways
    g = c["ref"]["vertices_b"][0].astype(np.float64)
    loss = lambda v: float(cr.evaluate(v[None], c["points"], c["params"], c["point_weights"], c["vertex_weights"])["loss"][0])
    h, worst = 1e-6, 0.0
    for i in range(40):
        for a in range(3):
            e = np.zeros((40, 3))
            e[i, a] = h
            worst = max(worst, abs((loss(c["vertices"][0] + e) - loss(c["vertices"][0] - e)) / (2 * h) - g[i, a]))
    print(f"central differences: {worst:.2e} of a largest gradient entry {np.abs(g).max():.2e}")
    assert worst <= 1e-7 * np.abs(g).max()


def test_the_lowest_index_wins_a_tie():
    v = np.array([[[0.0, 0, 0], [1.0, 0, 0], [0.0, 0, 0], [1.0, 0, 0]]])  # vertices 2, 3 copy 0, 1
    p = np.array([[[0.1, 0, 0], [0.9, 0, 0], [0.1, 0, 0], [0.5, 0, 0]]])  # point 2 copies 0; point 3 is halfway between vertices 0 and 1
    r = cr.evaluate(v, p, (1.0, 1.0, np.inf))
    assert r["nearest_vertex"].tolist() == [[0, 1, 0, 0]] and r["nearest_point"].tolist() == [[0, 1, 0, 1]]
    # the copies own nothing: the gradient of points -> mesh lands on the originals alone
    only = cr.evaluate(v, p, (1.0, 1.0, np.inf), directions=1)
    assert not only["vertices_b"][0, 2:].any() and only["vertices_b"][0, :2].any() and only["nearest_point"] is None
    c = cr.case(520, 700, kind="duplicates", n=2)
    v, p = c["vertices"], c["points"]
    back = cr.TILE // 2 - 1
    assert np.array_equal(v[:, back], v[:, 0]) and np.array_equal(p[:, back], p[:, 0]) and np.array_equal(v[:, -1], v[:, 0])
    for b in range(2):
        for name, own in (("nearest_vertex", v[b]), ("nearest_point", p[b])):
            idx = c["ref"][name][b]
            first = np.array([np.flatnonzero((own == own[i]).all(axis=1))[0] for i in idx])
            assert np.array_equal(first, idx), name  # never the copy
    c = cr.case(97, 400, kind="coincident")
    assert not c["ref"]["terms"][:, 0].any() and c["ref"]["g_scale"].max() > 0  # d2 == 0 for every point; the vertices still pull to points


def test_float64_error_is_measured_and_inside_the_tolerances():
    worst = [0.0, 0.0]
    for row in cr.parity_cases():
        c = cr.case(**row)
        f = cr.evaluate(c["vertices"], c["points"], c["params"], c["point_weights"], c["vertex_weights"], c["directions"], dtype=np.float64)
        e = cr.errors(c, f["terms"], f["loss"], f["vertices_b"], f["nearest_vertex"], f["nearest_point"])
        worst = [max(a, b) for a, b in zip(worst, e)]
    print(f"float64 against long double over {len(cr.parity_cases())} cases: terms {worst[0]:.2e}, gradient {worst[1]:.2e}")
    assert worst[0] <= cr.TOL_TERMS and worst[1] <= cr.TOL_GRADIENT
    assert worst[0] >= cr.TOL_TERMS / 4 and worst[1] >= cr.TOL_GRADIENT / 4  # (the tolerances are the measured values rounded up, not a guess)
    assert (cr.GPU_TOL_TERMS, cr.GPU_TOL_GRADIENT) == (8 * cr.TOL_TERMS, 8 * cr.TOL_GRADIENT)


def test_the_restated_split_rule():
    for Q in (1, 256, 257, 526, 10002, 40000, 262144, 262145):
        s = [cr.segments(Q, R) for R in range(1, 20000, 37)]
        assert all(1 <= a <= cr.MAX_SEGMENTS for a in s) and s == sorted(s)
    assert [cr.segments(526, 40000), cr.segments(40000, 526), cr.segments(10002, 40000), cr.segments(40000, 10002)] == [64, 3, 26, 7]
    assert cr.change_points(cr.segments, 65, 1000) == [257, 513, 769] and cr.segments(0, 5) == cr.segments(5, 0) == 0
