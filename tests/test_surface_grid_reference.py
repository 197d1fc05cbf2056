"""CPU checks of the restatement of the point-to-surface distance over a uniform grid of triangles (tests/surface_grid_reference.py): the shell
search -- its VISITED SET, not only its answer -- gives the brute-force closest face of tests/surface_reference.py wherever d2 <= tau2 and NONE
exactly elsewhere, over the whole case table and over adversarial placements (box corners on cell faces, negative coordinates, a face exactly
max_distance away, a box exactly h_f long, a quotient that rounds up to an integer, coordinates beyond the clamp); how many placements needed the
slack shell and the margin of the early exit is counted and printed; the float64 chain is measured against long double (DESIGN.md 4p quotes it)."""

import numpy as np

import chamfer_grid_reference as gr
import surface_grid_reference as sg
import surface_reference as sr


def corners(c, pose=0):
    v, f = c["vertices"][pose], c["faces"].astype(np.int64)
    return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]


def check_search(points, a, b, c, tau, cell, name):
    """the shell search against brute force over all faces -> (the search's result, the shells visited, brute-force d2, brute-force face)"""
    got, visited, evaluated = sg.shell_search(points, a, b, c, tau, cell)
    d2, face = sr.nearest_face(np.asarray(points, dtype=np.float64), a, b, c)[:2]
    tau2 = np.float64(tau) * np.float64(tau)
    assert np.array_equal(got < 0, d2 > tau2), name  # NONE exactly where the closest face is beyond max_distance
    assert np.array_equal(got[got >= 0], face[got >= 0]), name  # and the brute-force face, the lowest index of a tie, everywhere else
    assert (evaluated <= len(a)).all()  # a face is evaluated at most once per query
    return got, visited, d2, face


def test_the_shell_search_finds_the_brute_force_face_over_the_case_table():
    seen_mixed = 0
    for row in sg.grid_cases():
        c = sg.case(**row)
        tau = c["params"][2]
        if row.get("max_distance") == "mid" or isinstance(row.get("max_distance", 0.25), float) and row.get("max_distance", 0.25) < 1.0 and row.get("kind") not in ("exact",):
            seen_mixed += sg.mixed(c)
        if row.get("max_distance") == "mid":
            assert sg.mixed(c), c["name"]  # no such case passes by reporting NONE everywhere
        if not c["directions"] & 1:
            continue
        for pose in range(c["vertices"].shape[0]):
            got = check_search(c["points"][pose], *corners(c, pose), tau, c["cell_size"], c["name"])[0]
            assert np.array_equal(got, c["ref_grid"]["nearest_face"][pose]), c["name"]
    assert seen_mixed >= 10


def test_the_cell_edge_follows_the_longest_box_side_the_cell_size_or_max_distance():
    long_, tiny = sg.case(kind="long", F=300, P=50, max_distance=0.1, cell_size=0.03), sg.case(kind="tiny", F=300, P=50, max_distance=0.1, cell_size=0.03)
    assert sg.cell_edge(0.03, 0.1, *corners(long_)) == sg.longest_side(*corners(long_)) > 1.0
    assert sg.longest_side(*corners(tiny)) < 0.002 and sg.cell_edge(0.03, 0.1, *corners(tiny)) == 0.03
    assert sg.cell_edge(0.001, 0.1, *corners(tiny)) == np.float64(0.1) / 4
    # a face lies in the cells key .. key + 1 of its own key, per axis (up to the rounding the slack shell is for)
    for c in (long_, tiny, sg.case(kind="sphere", P=20, max_distance=0.5, cell_size=0.01)):
        a, b, cc = corners(c)
        h = sg.cell_edge(c["cell_size"], c["params"][2], a, b, cc)
        keys = sg.face_keys(a, b, cc, h)
        for corner in (a, b, cc):
            d = gr.cells(corner, h) - keys
            assert d.min() >= 0 and d.max() <= 1


def test_shells_partition_the_key_cells():
    offsets = np.array([[x, y, z] for x in range(-7, 7) for y in range(-7, 7) for z in range(-7, 7)])
    sh = sg.shells(offsets, np.zeros(3, dtype=np.int64))
    for s in range(6):
        assert (sh == s).sum() == (2 * s + 2) ** 3 - (2 * s) ** 3  # 8, 56, 152, ...
        inside = ((offsets >= -s - 1) & (offsets <= s)).all(axis=1)
        assert np.array_equal(sh <= s, inside)


def test_adversarial_placements_and_how_many_needed_the_slack():
    """faces whose box corner sits on a cell face, negative and far cells, boxes exactly h_f long, points exactly max_distance from them and an ulp
    either side.  Counted: the winners met only in the slack shell (beyond the real-number bound ceil(max_distance / h)), and the queries whose
    early exit needed its margin (an unvisited face below (h s)^2 that beats or ties the best)."""
    in_slack = needed_margin = total = at_tau = 0
    for tau, cell in ((0.25, 0.25), (0.25, 0.0625), (1.0, 0.25), (3.0, 1.0), (0.4, 0.1), (0.3, 0.1), (0.7, 0.7 / 3), (1.2, 0.3)):
        h = gr.cell_edge(cell, tau)
        for axis in range(3):
            v, f, p = sg.placement_problem(h, tau, axis)
            a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
            assert sg.cell_edge(cell, tau, a, b, c) == h == sg.longest_side(a, b, c)  # a box exactly h_f long
            got, visited, d2, face = check_search(p, a, b, c, tau, cell, (tau, cell, axis))
            tau2 = np.float64(tau) * np.float64(tau)
            assert (got >= 0).any() and (got < 0).any()
            at_tau += int((d2 == tau2).sum())
            keys = sg.face_keys(a, b, c, h)
            real_last = int(np.ceil(np.float64(tau) / h))
            for i in np.flatnonzero(got >= 0):
                in_slack += sg.shells(keys[got[i] : got[i] + 1], gr.cells(p[i], h))[0] > real_last
            loose = sg.shell_search(p, a, b, c, tau, cell, margin=False)[0]
            needed_margin += int((loose != got).sum())
            total += len(p)
    print(f"adversarial placements: {total} queries, {at_tau} exactly max_distance from their face, {in_slack} winners met only in the slack shell, "
          f"{needed_margin} answers change without the margin of the early exit")
    assert at_tau > 0


def test_a_quotient_that_rounds_up_to_an_integer_needs_the_slack_shell():
    """searched for, as DESIGN.md 4o did for points: a point x just below m h whose quotient x / h rounds UP to m (its cell is one too high), and
    a face whose near corner is exactly max_distance = 4 h below it and whose box is h long: the key of the face is 6 cells below the point's
    cell, in shell 5 = ceil(max_distance / h) + 1, the slack shell; without that shell the face within max_distance would be missed."""
    from fractions import Fraction

    found = met_in_slack = 0
    for h in (0.1, 0.3, 0.7 / 3, 1.0 / 3, 0.05, 0.011, 0.17):
        h, tau = np.float64(h), 4.0 * np.float64(h)
        for m in range(7, 400):
            x = np.nextafter(np.float64(m) * h, -np.inf)
            if not (np.floor(x / h) == m and Fraction(float(x)) / Fraction(float(h)) < m):
                continue
            near = np.float64(x - tau)
            lo = np.float64(near - h)
            if np.float64(near - lo) > h or x - near > tau:  # (the rounded side must not exceed h, the face must be within max_distance)
                continue
            v = np.array([[near, 0.0, 0.0], [lo, 0.0, 0.0], [0.5 * (near + lo), 0.0, 0.4 * h], [x + 9 * h, 0, 0], [x + 10 * h, 0, 0], [x + 9.5 * h, 0, 0.3 * h]])
            f = np.array([[0, 1, 2], [3, 4, 5]])
            a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
            if sg.cell_edge(h, tau, a, b, c) != h:
                continue
            p = np.array([[x, 0.0, 0.0]])
            got = check_search(p, a, b, c, tau, h, ("rounds up", float(h), m))[0]
            assert got[0] == 0
            found += 1
            met_in_slack += sg.shells(sg.face_keys(a, b, c, h)[:1], gr.cells(p[0], h))[0] == 5
    print(f"quotients that round up to an integer: {found} placements, {met_in_slack} of them met their face only in the slack shell")
    assert met_in_slack > 0


def test_far_cells_and_coordinates_beyond_the_clamp_stay_equal_to_brute_force():
    for axis in range(3):
        v, f, p = sg.placement_problem(0.25, 1.0, axis, far=True)
        a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        check_search(p, a, b, c, 1.0, 0.25, ("far", axis))


def test_ties_between_faces_keyed_in_different_cells_and_shells():
    """a closed sphere with the cell near the edge length: the faces around a vertex or an edge tie exactly and are keyed in different cells"""
    sv, faces = sr.sphere(2)
    rs = np.random.RandomState(4)
    p = np.concatenate((1.2 * sv, 1.1 * 0.5 * (sv[faces[:, 0]] + sv[faces[:, 1]]), sr.outside_points(sv, 200, rs) * 0.8))
    a, b, c = sv[faces[:, 0]], sv[faces[:, 1]], sv[faces[:, 2]]
    edge = sg.longest_side(a, b, c)
    dist = sr.closest(p[:, None, :], a[None], b[None], c[None])[3]
    tied = (dist == dist.min(axis=1, keepdims=True)).sum(axis=1)
    assert (tied >= 4).sum() >= len(sv) // 2  # beyond a vertex: every face around it
    for cell in (0.5 * edge, edge, 1.5 * edge):
        got, visited, d2, face = check_search(p, a, b, c, 0.9, cell, ("sphere ties", cell))
        h = sg.cell_edge(cell, 0.9, a, b, c)
        keys = sg.face_keys(a, b, c, h)
        spread = [len(np.unique(keys[np.flatnonzero(dist[i] == dist[i].min())], axis=0)) for i in np.flatnonzero(tied >= 4)]
        assert max(spread) >= 3  # one tie, several key cells


def test_near_degenerate_slivers_keep_their_closest_point_inside_their_box():
    """what both exactness statements rest on: the header's closest point lies in the face's box up to rounding, so its
    d2 is not below the distance to the box.  On faces whose third corner is a rounded point of the segment of the other two -- ``den`` of the
    order of an ulp, not zero -- with points from below an ulp of their line upwards: the interior region IS reached, its coordinates stay in
    [0, 1], no closest point leaves the box by more than 2^-23 h_f, and no d2 is below the squared distance to the box (less that slack)."""
    reached = 0
    for row in (r for r in sg.grid_cases() if r.get("kind") == "sliver"):
        c = sg.case(**row)
        for pose in range(c["vertices"].shape[0]):
            a, b, cc = corners(c, pose)
            assert (np.abs(np.cross(b - a, cc - a)).max(axis=1) > 0).all()  # near-degenerate, not degenerate
            p = c["points"][pose]
            h = sg.cell_edge(c["cell_size"], c["params"][2], a, b, cc)
            slack = 2.0**-23 * h
            v, w, e, d2, region = sr.closest(p[:, None, :], a[None], b[None], cc[None], want_region=True)
            inside = region == 6
            reached += int(inside.sum())
            assert ((v >= 0) & (v <= 1) & (w >= 0) & (w <= 1))[inside].all()
            lo, hi = np.minimum(np.minimum(a, b), cc), np.maximum(np.maximum(a, b), cc)
            q = p[:, None, :] + e
            assert np.maximum(np.maximum(lo[None] - q, q - hi[None]), 0).max() <= slack
            gap = np.sqrt((np.maximum(np.maximum(lo[None] - p[:, None, :], p[:, None, :] - hi[None]), 0) ** 2).sum(axis=-1))
            assert (np.sqrt(d2) >= (gap - 2 * slack) * (1 - 2.0**-50)).all()
    print(f"near-degenerate slivers: the interior region taken by {reached} (point, face) pairs")
    assert reached > 100


def test_sizes_follow_the_formula():
    assert sg.launches(526, 1048, 40000, 1, 3) == 31 and sg.scratch_bytes(526, 1048, 40000, 1) == 6756824
    assert sg.launches(5, 255, 7, 1, 1) + 3 == sg.launches(5, 256, 7, 1, 1)  # the assignment needs a ninth bit: one pass more
    assert sg.launches(5, 128, 7, 1, 1) + 3 == sg.launches(5, 129, 7, 1, 1)  # 2^9 buckets: one pass more
    assert sg.launches(0, 5, 5, 1, 3) == sg.launches(5, 5, 5, 1, 4) == sg.scratch_bytes(5, 0, 5, 1) == sg.scratch_bytes(5, 5, sg.MAX_ITEMS + 1, 1) == 0


def test_float64_error_is_measured_and_inside_the_tolerances():
    worst = [0.0, 0.0]
    for row in sg.grid_cases():
        c = sg.case(**row)
        f = sr.evaluate(c["vertices"], c["faces"], c["points"], c["params"], c["point_weights"], c["vertex_weights"], c["directions"], dtype=np.float64)
        mask = lambda x, near, none: None if x is None else np.where(near, x, none)
        e = sg.errors(c, f["terms"], f["loss"], f["vertices_b"], mask(f["nearest_face"], f["near_p"], -1), mask(f["barycentric"], f["near_p"][..., None], 0.0),
                      mask(f["nearest_point"], f["near_v"], -1))  # fmt: skip
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert not f["vertices_b"][c["ref"]["g_scale"] == 0].any()  # a vertex of g_scale 0 gets exactly 0
    print(f"float64 against long double over {len(sg.grid_cases())} cases: terms {worst[0]:.2e}, gradient {worst[1]:.2e}")
    assert worst[0] <= sg.TOL_TERMS and worst[1] <= sg.TOL_GRADIENT
    assert worst[0] >= sg.TOL_TERMS / 4 and worst[1] >= sg.TOL_GRADIENT / 4  # (the tolerances are the measured values rounded up, not a guess)
    assert (sg.GPU_TOL_TERMS, sg.GPU_TOL_GRADIENT) == (8 * sg.TOL_TERMS, 8 * sg.TOL_GRADIENT)
