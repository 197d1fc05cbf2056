"""CPU checks of the restatement tests/chamfer_grid_reference.py of include/deodr_hip_chamfer_grid.h: the exactness property of the cell rule --
EVERY pair with the header's d2 <= tau2 lies within the rings the search visits, over random cases and over adversarial placements (multiples of
h and one ulp either side, negative coordinates, pairs exactly max_distance apart and one ulp either side across a cell face, coordinates where
x / h rounds coarsely and beyond the clamp) --, the ring-by-ring search with its early exit against the brute-force nearest neighbour (ties where
the lower index sits in a farther ring included), the hash against a scalar restatement, the stable order, and the float64 chain error of the
case table against long double, printed: the tolerances of the GPU tests are 8 x the rounded-up values."""

import itertools

import numpy as np

import chamfer_grid_reference as gr
import chamfer_reference as cr


def worst_ring(a, b, h):
    """the largest Chebyshev distance in cells of the pairs (a_i, b_j) given as boolean [A,B] mask -> int"""
    return np.abs(gr.cells(a, h)[:, None, :] - gr.cells(b, h)[None, :, :]).max(axis=2)


def test_every_pair_within_max_distance_lies_within_the_rings_random():
    rs = np.random.RandomState(0)
    for tau, cell in ((0.3, 0.15), (0.2, 1e-6), (0.2, 0.09), (0.2, 4.0), (0.05, 0.01), (1e-3, 1e-9), (3.0, 0.1)):
        for offset in (0.0, -0.5, 1e6, -1e9):
            a, b = rs.rand(400, 3) + offset, rs.rand(500, 3) + offset
            h = gr.cell_edge(cell, tau)
            within = gr.d2(a[:, None, :], b[None, :, :]) <= np.float64(tau) * np.float64(tau)
            rings = worst_ring(a, b, h)
            assert rings[within].max(initial=0) <= gr.last_ring(tau, h), (tau, cell, offset)
            assert gr.last_ring(tau, h) <= gr.RINGS + 1


def test_every_pair_within_max_distance_lies_within_the_rings_adversarial():
    worst = 0
    for tau, cell in ((0.25, 0.1), (0.25, 0.0625), (1.0, 0.25), (0.3, 0.1), (1e-3, 1e-3), (0.7, 0.1), (3.0, 1.0), (0.1, 7.0)):
        h = gr.cell_edge(cell, tau)
        xs = gr.placements(h, tau)
        tau2, last = np.float64(tau) * np.float64(tau), gr.last_ring(tau, h)
        cx = gr.cells(xs, h)
        # one axis: with the other two coordinates equal, d2 = fl(dx * dx) (+ 0 + 0)
        dx = xs[:, None] - xs[None, :]
        within = dx * dx <= tau2
        ring = np.abs(cx[:, None] - cx[None, :])
        assert ring[within].max() <= last, (tau, cell)
        worst = max(worst, int((ring[within] - (last - 1)).max()))
        # the same pairs with the other axes carrying a small distance: fewer pairs are within, never one more ring
        for dy in (0.0, h / 3, tau / 2):
            d2 = (dx * dx + np.float64(dy) * np.float64(dy)) + 0.0
            assert ring[d2 <= tau2].max(initial=0) <= last
    print(f"adversarial placements: the farthest pair within max_distance sits {worst} ring(s) beyond ceil(max_distance / h) (1 is allowed for)")
    assert worst <= 1


def test_cells_floor_negative_coordinates_and_clamp():
    h = 0.25
    assert gr.cells([-0.1, -0.25, -0.26, 0.0, 0.24, 0.25], h).tolist() == [-1, -1, -2, 0, 0, 1]
    assert gr.cells([1e300, -1e300, 2.0**29, -(2.0**29)], 1.0).tolist() == [gr.CELL_LIMIT, -gr.CELL_LIMIT, 2**29, -(2**29)]
    assert gr.cell_edge(1e-6, 0.2) == np.float64(0.2) / 4 and gr.cell_edge(0.3, 0.2) == 0.3
    assert gr.last_ring(0.2, gr.cell_edge(1e-6, 0.2)) == gr.RINGS + 1 and gr.last_ring(0.2, 4.0) == 2 and gr.last_ring(0.2, 0.2) == 2 and gr.last_ring(0.2, 0.19) == 3


def test_hash_against_a_scalar_restatement():
    def scalar(x, y, z):
        m = 0xFFFFFFFF
        k = ((x * 73856093) & m) ^ ((y * 19349663) & m) ^ ((z * 83492791) & m)
        k ^= k >> 16
        k = (k * 0x85EBCA6B) & m
        k ^= k >> 13
        k = (k * 0xC2B2AE35) & m
        return k ^ (k >> 16)

    rs = np.random.RandomState(1)
    c = np.concatenate((rs.randint(-(2**30), 2**30 + 1, size=(200, 3)), [[0, 0, 0], [-1, -1, -1], [2**30, -(2**30), 5], [1, 0, 0], [0, 1, 0]])).astype(np.int64)
    got = gr.hash_cells(c)
    assert got.dtype == np.uint32 and [int(g) for g in got] == [scalar(int(x), int(y), int(z)) for x, y, z in c]
    assert len(set(int(g) & 63 for g in gr.hash_cells(np.array(list(itertools.product(range(4), repeat=3)))))) > 32  # neighbours spread over the buckets


def test_ring_search_returns_the_brute_force_nearest_within_max_distance():
    rs = np.random.RandomState(2)
    visited = []
    for tau, cell, kind in ((0.3, 0.15, "uniform"), (0.2, 1e-6, "uniform"), (0.08, 0.02, "uniform"), (0.2, 4.0, "uniform"), (0.1, 0.03, "duplicates"), (0.05, 0.01, "lattice")):
        q, r = rs.rand(150, 3), rs.rand(260, 3)
        if kind == "duplicates":
            r[100:200] = r[:100]
            q[:50] = r[200:250]
        if kind == "lattice":  # equidistant references on cell faces: ties everywhere
            r = np.array(list(itertools.product(np.arange(7) * 0.01, repeat=3)))[::-1].copy()
            q = np.array(list(itertools.product(np.arange(6) * 0.01 + 0.005, repeat=3)))
        best, arg = cr.nearest(q, r)
        want = np.where(best <= np.float64(tau) * np.float64(tau), arg, -1)
        got, rings = gr.ring_search(q, r, tau, cell)
        assert np.array_equal(got, want), (tau, cell, kind)
        visited.append(int(rings.max()))
    assert min(visited) < max(visited)  # the early exit was taken somewhere and not everywhere


def test_a_tie_whose_lower_index_sits_in_a_farther_ring_is_won_by_the_lower_index():
    h = 1.0  # max_distance 2, cell_size 1: rings 0 .. 3
    q = np.array([[0.875, 0.5, 0.5]])
    r = np.array([[1.375, 0.5, 0.5], [0.375, 0.5, 0.5]])  # both exactly 0.5 away; index 1 in the query's own cell, index 0 one cell further
    assert gr.d2(q, r).tolist() == [0.25, 0.25] and gr.cells(r[:, 0], h).tolist() == [1, 0]
    got, rings = gr.ring_search(q, r, 2.0, h)
    assert got.tolist() == [0] and rings.tolist() == [1]  # not stopped after ring 0; stopped after ring 1: 0.25 < (1 - 2^-20)^2
    assert gr.exit_bound(h, 1) == (1 - 2.0**-20) ** 2 < 1.0 and gr.exit_bound(h, 3) < 9.0
    # a best of exactly (h s)^2 does not stop the search: both exactly 2 = max_distance away, two cells off; the lower index wins, in the last ring
    r = np.array([[0.875, 2.5, 0.5], [-1.125, 0.5, 0.5], [0.875, 0.5, 2.5]])[[2, 0, 1]]
    got, rings = gr.ring_search(q, r, 2.0, h)
    assert gr.d2(q, r).tolist() == [4.0] * 3 and got.tolist() == [0] and rings.tolist() == [3] == [gr.last_ring(2.0, h)]
    assert gr.ring_search(q, r, np.nextafter(2.0, 0.0), h)[0].tolist() == [-1]  # an ulp less: beyond max_distance, no correspondence


def test_stable_order_and_sizes():
    keys = np.array([[5, 1, 5, 0x105, 1, 0]], dtype=np.uint32)
    s, o = gr.stable_order(keys, 8)
    assert o.tolist() == [[5, 1, 4, 0, 2, 3]] and s.tolist() == [[0, 1, 1, 5, 5, 0x105]]  # (the high bits are ignored and kept)
    assert gr.stable_order(keys, 32)[1].tolist() == [[5, 1, 4, 0, 2, 3]] and gr.stable_order(keys, 1)[1].tolist() == [[5, 0, 1, 2, 3, 4]]
    assert [gr.table_bits(r) for r in (1, 32, 33, 64, 65, 2**23, 2**23 + 1, 2**24, 2**24 + 1, 0)] == [6, 6, 7, 7, 8, 24, 25, 25, 0, 0]
    assert [gr.assign_bits(v) for v in (1, 2, 3, 4, 255, 256, 2**24)] == [1, 2, 2, 3, 8, 9, 25]
    assert gr.sort_launches(5, 1, 8) == 3 and gr.sort_launches(5, 1, 9) == 6 and gr.sort_launches(5, 1, 32) == 12 and gr.sort_launches(0, 1, 8) == 0


def test_float64_error_is_measured_and_inside_the_tolerances():
    """the same sums in float64, one value after the other (the order with the largest error), against long double, over the table the GPU runs"""
    worst_terms = worst_gradient = 0.0
    for row in gr.grid_cases():
        c = gr.case(**row)
        f64 = cr.evaluate(c["vertices"], c["points"], c["params"], c["point_weights"], c["vertex_weights"], c["directions"], dtype=np.float64)
        e_terms, e_grad = gr.errors(c, f64["terms"], f64["loss"], f64["vertices_b"])
        worst_terms, worst_gradient = max(worst_terms, e_terms), max(worst_gradient, e_grad)
        ref = c["ref_grid"]
        for name, near in (("nearest_vertex", "near_p"), ("nearest_point", "near_v")):
            if ref[name] is not None:
                assert np.array_equal(ref[name] >= 0, ref[near]) and np.array_equal(ref[name][ref[near]], c["ref"][name][ref[near]])
    print(f"float64 chain against long double over grid_cases(): terms {worst_terms:.2e}, gradient {worst_gradient:.2e}")
    assert worst_terms <= gr.TOL_TERMS and worst_gradient <= gr.TOL_GRADIENT
    assert gr.TOL_TERMS <= cr.TOL_TERMS and gr.TOL_GRADIENT <= cr.TOL_GRADIENT  # (a chain over this table is no worse than over the older one)
