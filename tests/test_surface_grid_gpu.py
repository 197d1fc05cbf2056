"""GPU checks of the point-to-surface distance over the uniform grid of triangles (include_staged/deodr_hip_surface_grid.h,
deodr_amd/csrc/dr_surface_grid.h).  Two oracles for every case: the long-double restatement (tests/surface_grid_reference.py: indices and the set
of truncated pairs EQUAL, barycentric bit-equal, terms, loss and gradient within 8 x the measured float64 error) and the brute-force operator
``hip_renderer.surface_distance`` on the same tensors (``nearest_face`` equal wherever not NONE, NONE exactly where its d2 is above tau2,
``barycentric`` bit-equal there, the terms its bits, the gradient within twice the tolerance).  Outputs between guards, the scratch exactly
``deodr_hip_surface_grid_scratch_bytes`` long between guards and filled with NaN, every index array written everywhere, two calls bit-identical.
The case table (F and P through 1, 2, 63 - 65, 255 - 257 in both roles, V = 3 and 37, n = 1 and 3, the directions, the weights, the kinds of
tests/surface_reference.py, a long face, tiny faces, the cell sizes, the truncations), the placements of the CPU file, ties across cells and
shells, 5 000 points on one face, a hub of 64 faces, a replayed graph with moved vertices and a shrinking max_distance, the autograd op, the
fitter eager and graphed, and one size the brute-force operator refuses, against that operator on the two halves of the cloud."""

import numpy as np
import pytest
import torch

import chamfer_grid_reference as gr
import chamfer_reference as cr
import surface_grid_reference as sg
import surface_reference as sr
from test_basis_gpu import Arena, host

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD_BYTES, GUARD_BYTE = 4096, 0xA5
PAD_WORDS, INDEX_GUARD = 1024, 0x5A5A5A5A
WORST = {"terms": 0.0, "gradient": 0.0}


class GuardedScratch:
    """exactly deodr_hip_surface_grid_scratch_bytes bytes filled with a NaN pattern, between two guards in the same allocation"""

    def __init__(self, V, F, P, n):
        from deodr_amd.hip_renderer import lib

        self.nbytes = int(lib().deodr_hip_surface_grid_scratch_bytes(V, F, P, n))
        assert self.nbytes == sg.scratch_bytes(V, F, P, n) and self.nbytes % 4 == 0
        self.buffer = torch.full((self.nbytes + 2 * GUARD_BYTES,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.front = self.buffer[GUARD_BYTES : GUARD_BYTES + self.nbytes]
        self.front.view(torch.int32).fill_(0x7FF80000)  # a NaN as a double (either word on top) and as a float
        assert self.front.data_ptr() % 8 == 0

    def check(self):
        assert bool((self.buffer[:GUARD_BYTES] == GUARD_BYTE).all()), "the memory in front of the scratch was written"
        assert bool((self.buffer[GUARD_BYTES + self.nbytes :] == GUARD_BYTE).all()), "the scratch was written beyond deodr_hip_surface_grid_scratch_bytes"


def tables(c):
    """(faces, corner_offsets, corners) int32 device tensors of a case, the table by the restatement's plain loop"""
    offsets, corners = sr.corner_table(c["faces"], c["vertices"].shape[1])
    return tuple(torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=DEV) for a in (c["faces"], offsets, corners))


def run(c, calls=2, nearest=True):
    """``calls`` calls of the grid operator on the case, outputs and scratch guarded, and one of the brute-force operator on the same tensors
    -> ([(terms, loss, vertices_b, nearest_face, barycentric, nearest_point)], the brute-force operator's six)"""
    from deodr_amd import hip_renderer as hr

    n, V, P, F = c["vertices"].shape[0], c["vertices"].shape[1], c["points"].shape[1], len(c["faces"])
    assert hr.surface_grid_launches(V, F, P, n, c["directions"]) == sg.launches(V, F, P, n, c["directions"]) > 0
    arena = Arena()
    carve = lambda a: None if a is None else arena.carve(a)
    v, p, pw, uw, params = carve(c["vertices"]), carve(c["points"]), carve(c["point_weights"]), carve(c["vertex_weights"]), carve(c["params"])
    faces, offsets, corners = tables(c)
    scratch = GuardedScratch(V, F, P, n)
    outs, guarded = [], []

    def indices(count):
        """[n, count] int32 between guards, pre-filled with a pattern no index has"""
        buffer = torch.full((n * count + 2 * PAD_WORDS,), INDEX_GUARD, dtype=torch.int32, device=DEV)
        guarded.append((buffer, n * count))
        return buffer[PAD_WORDS : PAD_WORDS + n * count].view(n, count)

    for _ in range(calls):
        terms, loss, g = arena.carve(shape=(n, 2)), arena.carve(shape=(n,)), arena.carve(shape=(n, V, 3))
        nf = indices(P) if nearest and c["directions"] & 1 else None
        bary = arena.carve(shape=(n, P, 3)) if nearest and c["directions"] & 1 else None
        npt = indices(V) if nearest and c["directions"] & 2 else None
        got = hr.surface_grid(v, faces, offsets, corners, p, params, c["cell_size"], pw, uw, c["directions"], terms=terms, loss=loss, vertices_b=g, nearest_face=nf,
                              barycentric=bary, nearest_point=npt, scratch=scratch.front)  # fmt: skip
        assert got[0] is terms and got[2] is g and got[3] is nf and got[4] is bary and got[5] is npt
        outs.append((terms, loss, g, nf, bary, npt))
    brute = hr.surface_distance(v, faces, offsets, corners, p, params, pw, uw, c["directions"], want_nearest=True)
    torch.cuda.synchronize()
    arena.check(), scratch.check()
    for buffer, numel in guarded:
        assert bool((buffer[:PAD_WORDS] == INDEX_GUARD).all()) and bool((buffer[PAD_WORDS + numel :] == INDEX_GUARD).all()), "written outside an index array"
        assert not bool((buffer[PAD_WORDS : PAD_WORDS + numel] == INDEX_GUARD).any()), "an index array was not written everywhere"
    return outs, brute


def brute_d2(c, face):
    """the header's d2 of every point to the face the brute-force operator chose [n,P]"""
    f = c["faces"].astype(np.int64)[face]  # [n,P,3]
    corner = lambda k: np.take_along_axis(c["vertices"], f[..., k, None].repeat(3, axis=-1), axis=1)
    return sr.closest(c["points"], corner(0), corner(1), corner(2))[3]


def against_brute(c, h, brute):
    """nearest_face equal to the brute-force operator's wherever not NONE, NONE exactly where its d2 is above tau2, barycentric its bits there (zeros
    elsewhere); the same for nearest_point; the terms and the loss are its bits (the same combine steps on the same values); its gradient within
    twice the tolerance (each is within one of the long-double value)"""
    tau2 = np.float64(c["params"][2]) * np.float64(c["params"][2])
    if h[3] is not None:
        got, theirs = sg.signed(h[3]), host(brute[3]).astype(np.int64) & 0xFFFFFFFF
        assert np.array_equal(got < 0, brute_d2(c, theirs) > tau2), c["name"]
        assert np.array_equal(got[got >= 0], theirs[got >= 0]), c["name"]
        bary = host(brute[4])
        assert np.array_equal(h[4][got >= 0].view(np.int64), bary[got >= 0].view(np.int64)) and not h[4][got < 0].any(), c["name"]
    if h[5] is not None:
        got, theirs = sg.signed(h[5]), host(brute[5]).astype(np.int64) & 0xFFFFFFFF
        d2 = gr.d2(c["vertices"], np.take_along_axis(c["points"], theirs[..., None], axis=1))
        assert np.array_equal(got < 0, d2 > tau2) and np.array_equal(got[got >= 0], theirs[got >= 0]), c["name"]
    assert np.array_equal(h[0], host(brute[0])) and np.array_equal(h[1], host(brute[1])), c["name"]
    scale = np.asarray(c["ref"]["g_scale"], dtype=np.float64)
    assert cr.relative(np.abs(h[2] - host(brute[2])).max(axis=-1), scale) <= 2 * sg.GPU_TOL_GRADIENT, c["name"]


def check_parity(c, nearest=True):
    (first, second), brute = run(c, nearest=nearest)
    for a, b in zip(first, second):
        assert (a is None and b is None) or torch.equal(a, b)  # bit-identical from run to run
    h = [None if t is None else host(t) for t in first]
    e_terms, e_grad = sg.errors(c, *h)  # (asserts the equality of the indices, NONE included, and of the bits of the barycentric coordinates)
    if nearest:
        for got, ref in ((h[3], c["ref_grid"]["nearest_face"]), (h[4], c["ref_grid"]["barycentric"]), (h[5], c["ref_grid"]["nearest_point"])):
            assert (got is None) == (ref is None)
        against_brute(c, h, brute)
    print(f"{c['name']}: terms {e_terms:.2e}, gradient / g_scale {e_grad:.2e}")
    WORST["terms"], WORST["gradient"] = max(WORST["terms"], e_terms), max(WORST["gradient"], e_grad)
    assert e_terms <= sg.GPU_TOL_TERMS and e_grad <= sg.GPU_TOL_GRADIENT, (c["name"], e_terms, e_grad)
    return h


@pytest.mark.parametrize("row", sg.grid_cases(), ids=lambda row: "-".join(f"{k}{v}" for k, v in row.items()))
def test_kernels_against_long_double_and_brute_force(row):
    c = sg.case(**row)
    h = check_parity(c)
    kind, ref = row.get("kind", "soup"), c["ref"]
    if kind == "exact":  # points bit-equal to vertices, edge midpoints and face points: they cost exactly 0 and pull exactly nothing
        assert not h[0][:, 0].any() and (h[3] == 0).any() and (h[3] == 1).any()  # (the collinear faces 0 and 1 win the ties along their rows)
        if c["directions"] == 1:
            assert not h[2].any()
    if kind == "degenerate":
        assert (h[3] == 0).any() and np.isfinite(h[4]).all()  # the zero-area face 0 wins its ties with faces 2 and 3 (those within max_distance)
    if kind == "fan" and c["directions"] == 1:
        assert h[2][:, 0].any() and not h[2][:, -2:].any()  # the hub of 100 corners is pulled; the two vertices no face uses get exactly 0
    if kind == "long":
        a, b, cc = (c["vertices"][0][c["faces"][:, k]] for k in range(3))
        assert sg.cell_edge(c["cell_size"], c["params"][2], a, b, cc) == sg.longest_side(a, b, cc) > 1.0  # E decided h_f
    if row.get("max_distance") == "below":
        assert not h[2].any() and not ref["near_p"].any() and not ref["near_v"].any()  # vertices_b == 0 exactly
        assert bool((sg.signed(h[3]) == -1).all()) and bool((sg.signed(h[5]) == -1).all()) and not h[4].any()  # and no correspondence at all
    if row.get("max_distance") == "mid":
        assert sg.mixed(c)
    if row.get("max_distance") == 3.0:
        assert (ref["near_p"].all() if c["directions"] & 1 else True) and (ref["near_v"].all() if c["directions"] & 2 else True)
    if row.get("directions", 3) != 3:
        off = 0 if row["directions"] == 2 else 1
        assert not h[0][:, off].any() and (h[3] is None if off == 0 else h[5] is None)
    if row.get("cell_size") == 0.001:  # h_f = max_distance / RINGS took over: the result is the one of the cell size it was raised to
        again = check_parity(sg.case(**dict(row, cell_size=float(np.float64(row["max_distance"]) / sg.RINGS))))
        assert all(np.array_equal(a, b) for a, b in zip(h, again))


def test_without_the_nearest_arrays():
    c = sg.case(F=300, P=700, n=3, seed=5, max_distance=0.15, cell_size=0.05)
    with_arrays, without = check_parity(c), check_parity(c, nearest=False)
    assert without[3] is None and without[4] is None and without[5] is None and all(np.array_equal(a, b) for a, b in zip(with_arrays[:3], without[:3]))


@pytest.mark.parametrize("tau, cell", ((0.25, 0.25), (1.0, 0.25), (0.4, 0.1), (0.7, 0.7 / 3)))
def test_placements_on_cell_faces_negative_exactly_max_distance_and_far_cells(tau, cell):
    """the problems of the CPU file's exactness test on one axis after the other: box corners on cell faces, boxes exactly h_f long, points exactly
    max_distance from a face and an ulp either side; then far cells and coordinates beyond the clamp"""
    h = gr.cell_edge(cell, tau)
    for axis in range(3):
        for far in (False, True):
            v, f, p = sg.placement_problem(h, tau, axis, far=far)
            c = sg.custom(v[None], f, p[None], tau, cell, f"placements tau={tau} cell_size={cell} axis={axis} far={far}")
            check_parity(c)
            assert c["ref"]["near_p"].any() and not c["ref"]["near_p"].all()


def test_ties_between_faces_keyed_in_different_cells_and_shells():
    """a closed sphere, the cell near the edge length: the faces around a vertex or an edge tie exactly and are keyed in different cells; the
    lowest index must win"""
    sv, faces = sr.sphere(2)
    rs = np.random.RandomState(4)
    p = np.concatenate((1.2 * sv, 1.1 * 0.5 * (sv[faces[:, 0]] + sv[faces[:, 1]]), sr.outside_points(sv, 200, rs) * 0.8))
    edge = sg.longest_side(sv[faces[:, 0]], sv[faces[:, 1]], sv[faces[:, 2]])
    for cell in (0.5 * edge, edge, 1.5 * edge):
        check_parity(sg.custom(sv[None], faces, p[None], 0.9, cell, f"sphere ties cell_size={cell:g}"))
    check_parity(sg.custom(sv[None], faces[::-1].copy(), p[None], 0.9, edge, "sphere ties, the faces in reverse order"))


def test_five_thousand_points_on_one_face_and_a_hub_of_64_faces():
    """the long run of the gather: a wavefront adds it strided, then in its tree; and a vertex with 64 corners in the vertices' combine step"""
    rs = np.random.RandomState(9)
    v = rs.rand(1, 30, 3) * 4.0
    faces = sr.soup_faces(30, 20, rs)
    a, b, c3 = (v[0][faces[7, k]] for k in range(3))
    st = rs.rand(5000, 2)
    st = np.where(st.sum(axis=1, keepdims=True) > 1, 1 - st, st)
    p = (a + st[:, :1] * (b - a) + st[:, 1:] * (c3 - a) + 1e-4 * (rs.rand(5000, 3) - 0.5))[None]
    c = sg.custom(v, faces, p, 0.5, 0.2, "5000 points on face 7", point_weights=0.5 + rs.rand(1, 5000), vertex_weights=0.5 + rs.rand(30), directions=1)
    assert (c["ref"]["nearest_face"] == 7).mean() > 0.9 and c["ref"]["near_p"].all()
    check_parity(c)
    ring = 64
    angles = 2 * np.pi * np.arange(ring) / ring
    hub = np.concatenate(([[0, 0, 0.5]], np.stack((np.cos(angles), np.sin(angles), 0.1 * np.cos(3 * angles)), axis=1)))[None]
    hub_faces = np.array([[0, 1 + i, 1 + (i + 1) % ring] for i in range(ring)])
    q = np.concatenate((0.6 * rs.randn(800, 3), 0.05 * rs.randn(200, 3) + [0, 0, 0.6]))[None]
    c = sg.custom(hub, hub_faces, q, 0.4, 0.1, "a hub of 64 faces")
    assert sg.mixed(c)
    assert check_parity(c)[2][0, 0].any()


def test_a_replayed_graph_follows_moved_vertices_and_a_shrinking_max_distance():
    from deodr_amd import hip_renderer as hr

    cell = 0.01  # below every max_distance / RINGS and every longest side here: h_f follows the vertices and params[2]
    c = sg.case(F=300, P=1000, n=3, seed=11, max_distance=0.3, cell_size=cell)
    others = [sg.case(F=300, P=1000, n=3, seed=11, max_distance=m, mix=mix, cell_size=cell) for m, mix in ((0.2, (1.0, 0.0)), (0.1, (0.2, 3.0)), (0.05, (1.5, 0.5)))]
    for k, other in enumerate(others):  # the same faces; the vertices moved and shrunk towards their centre, so E and h_f change with every replay
        scale = (0.5, 0.1, 0.02)[k]
        other["vertices"] = 0.5 + scale * (other["vertices"] - 0.5) + 0.01 * k
        other.update(sg.custom(other["vertices"], other["faces"], other["points"], other["params"][2], cell, other["name"], other["point_weights"], other["vertex_weights"],
                               mix=tuple(other["params"][:2])))  # fmt: skip
    edges = {float(sg.cell_edge(cell, o["params"][2], *(o["vertices"][0][o["faces"][:, k]] for k in range(3)))) for o in [c] + others}
    assert len(edges) == 4
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    v, p, pw, uw, params = t(c["vertices"]), t(c["points"]), t(c["point_weights"]), t(c["vertex_weights"]), t(c["params"])
    faces, offsets, corners = tables(c)
    V = c["vertices"].shape[1]
    scratch = hr.surface_grid_scratch(V, 300, 1000, 3, DEV)
    outs = hr.surface_grid(v, faces, offsets, corners, p, params, cell, pw, uw, 3, scratch=scratch, want_nearest=True)  # eager: allocates the outputs
    call = lambda: hr.surface_grid(v, faces, offsets, corners, p, params, cell, pw, uw, 3, *outs, scratch=scratch)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        call()
    for other in others:  # three replays; vertices, points and the weights overwritten in place and params changed between them
        for dst, name in ((v, "vertices"), (p, "points"), (pw, "point_weights"), (uw, "vertex_weights"), (params, "params")):
            dst.copy_(t(other[name]))
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o.clone() for o in outs]
        eager = hr.surface_grid(v, faces, offsets, corners, p, params, cell, pw, uw, 3, scratch=scratch, want_nearest=True)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(replayed, eager))
        e = sg.errors(other, *(host(o) for o in replayed))
        assert e[0] <= sg.GPU_TOL_TERMS and e[1] <= sg.GPU_TOL_GRADIENT, e


def test_op_under_autograd_against_surface_distance_s_gradient():
    from deodr_amd import hip_renderer as hr
    from deodr_amd.surface import PointSurfaceTerm

    c = sg.case(F=200, P=500, n=3, seed=21, max_distance="mid", cell_size=0.03)
    term = PointSurfaceTerm(c["faces"], c["vertices"].shape[1], c["points"], c["point_weights"], c["vertex_weights"], max_distance=c["params"][2],
                            mix=c["params"][:2], normalise=False, device=DEV, search="grid", cell_size=0.03)  # fmt: skip
    v = torch.tensor(c["vertices"], device=DEV, requires_grad=True)
    assert term.uses_kernel(v)
    loss, terms = term.evaluate(v)
    seed = torch.tensor([0.5, -2.0, 1.25], dtype=torch.float64, device=DEV)
    (g,) = torch.autograd.grad((loss * seed).sum(), v)
    vertices_b = term.evaluate_no_grad(v)[2]
    assert torch.equal(g, seed[:, None, None] * vertices_b) and not terms.requires_grad
    nf, bary, npt = term.correspondences(v)
    e = sg.errors(c, host(terms), host(loss.detach()), host(vertices_b), host(nf), host(bary), host(npt))
    assert e[0] <= sg.GPU_TOL_TERMS and e[1] <= sg.GPU_TOL_GRADIENT and nf.dtype == torch.int64 and int(nf.min()) == -1
    brute = hr.surface_distance(v.detach(), term.faces, term.corner_offsets, term.corners, term.points, term.params, term.point_weights, term.vertex_weights, 3)
    assert cr.relative(np.abs(host(vertices_b) - host(brute[2])).max(axis=-1), np.asarray(c["ref"]["g_scale"], dtype=np.float64)) <= 2 * sg.GPU_TOL_GRADIENT
    assert torch.equal(terms, brute[0]) and torch.equal(loss.detach(), brute[1])
    with pytest.raises(RuntimeError, match="does not require grad"):
        torch.autograd.grad(term.evaluate(v)[1].sum(), v)
    # what the kernels do not take goes through the torch ops, with the same correspondences
    cpu = term.correspondences(torch.tensor(c["vertices"]))
    assert cpu[0].device.type == "cpu" and np.array_equal(cpu[0].numpy(), host(nf)) and np.array_equal(cpu[1].numpy().view(np.int64), host(bary).view(np.int64))


def test_fit_eager_graphed_and_against_the_brute_force_fit():
    """an eager and a ``GraphedStep`` fit with ``surface_search="grid"`` give the same energies bit for bit.  Against the brute-force fit: the first
    energy has its bits (the terms are added by the same combine step over the same values); afterwards the two differ by the order in which a face
    adds the pulls of its points (each gradient within GPU_TOL_GRADIENT of the exact one), which ten damped steps carry into the energy: 1e-10 of
    it is five orders above that and five below anything a wrong correspondence would do -- the reasoned figure of
    tests/test_chamfer_grid_gpu.py, not a derived bound."""
    from deodr_amd.mesh_fitter import GraphedStep
    from test_chamfer_fit_host import hand
    from test_surface_fit_host import surface_fitter

    tau = 2 * hand()[0].std()
    eager = surface_fitter(DEV, surface_search="grid", max_distance=tau)
    assert eager.term.uses_kernel(eager.vertices) and eager.term.search == "grid"
    e_eager = [eager.step_device()[0].clone() for _ in range(10)]
    assert float(e_eager[-1]) < float(e_eager[0])
    f = surface_fitter(DEV, surface_search="grid", max_distance=tau)
    graphed = GraphedStep(f, warmup=3)  # 3 + 1 eager steps and 1 on the capture stream: iterations 0 .. 4
    assert f.iter == 5
    e_graph = [graphed.step_device()[0].clone() for _ in range(5)]  # iterations 5 .. 9
    print("eager:", [float(e) for e in e_eager], "graphed:", [float(e) for e in e_graph])
    assert all(torch.equal(a, b) for a, b in zip(e_graph, e_eager[5:]))
    assert torch.equal(f.vertices, eager.vertices)
    brute = surface_fitter(DEV, max_distance=tau)
    e_brute = [brute.step_device()[0].clone() for _ in range(10)]
    assert torch.equal(e_brute[0], e_eager[0])
    assert all(abs(float(a) - float(b)) <= 1e-10 * float(b) for a, b in zip(e_eager, e_brute))


def test_a_size_the_brute_force_operator_refuses_against_that_operator_on_the_halves_of_the_cloud():
    """the level-5 sphere (20 480 faces) against 2^18 points: 5.4e9 pairs.  The oracle is ``surface_distance`` on the two halves of the cloud, each
    under the cap: nearest_face and barycentric equal for all 262 144 points, term_0 within tolerance of the sum of the halves"""
    from deodr_amd import hip_renderer as hr
    from deodr_amd.surface import corner_table

    import arap_reference as ar

    sv, faces = ar._icosphere(5)  # the icosahedron subdivided five times
    sv = sv / np.sqrt((sv * sv).sum(axis=1))[:, None]  # (back on the unit sphere)
    F, P, V = len(faces), 2**18, len(sv)
    assert F == 20480 and F * P > hr.SURFACE_MAX_PAIRS >= F * (P // 2)
    rs = np.random.RandomState(5)
    d = rs.randn(P, 3)
    p = d / np.sqrt((d * d).sum(axis=1))[:, None] * (1.0 + 0.02 * rs.randn(P, 1))  # a noisy scan of the sphere, an edge is about 0.05 long
    p[::10] *= 1.5  # a tenth of outliers, beyond max_distance
    tau, cell = 0.15, 0.05
    w = 0.5 + rs.rand(1, P)
    offsets, corners = corner_table(faces, V)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    tv, tf, to, tc, tp, tw, params = t(sv[None]), t(faces.astype(np.int32)), t(offsets), t(corners), t(p[None]), t(w), t(np.array([0.7, 1.3, tau]))
    with pytest.raises(ValueError, match="outside the limits"):
        hr.surface_distance(tv, tf, to, tc, tp, params, tw, None, 1)
    terms, loss, g, nf, bary, _ = hr.surface_grid(tv, tf, to, tc, tp, params, cell, tw, None, 1, want_nearest=True)
    again = hr.surface_grid(tv, tf, to, tc, tp, params, cell, tw, None, 1, want_nearest=True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((terms, loss, g, nf, bary), again))
    halves = [hr.surface_distance(tv, tf, to, tc, tp[:, at : at + P // 2].contiguous(), params, tw[:, at : at + P // 2].contiguous(), None, 1, want_nearest=True)
              for at in (0, P // 2)]  # fmt: skip
    torch.cuda.synchronize()
    face = torch.cat([h[3] for h in halves], dim=1)
    their_bary = torch.cat([h[4] for h in halves], dim=1)
    none = nf == -1  # (int32 bit patterns: NONE is -1)
    assert 0.05 < float(none.double().mean()) < 0.2
    assert torch.equal(nf[~none], face[~none]) and torch.equal(bary[~none], their_bary[~none]) and not bool(bary[none].any())
    # NONE exactly where the brute-force d2 is above tau2: from the brute-force face and its barycentric coordinates, the header's closest point
    f = tf.long()[face[0].long()]
    a, b, c = tv[0][f[:, 0]], tv[0][f[:, 1]], tv[0][f[:, 2]]
    e = ((a + their_bary[0, :, 1:2] * (b - a)) + their_bary[0, :, 2:3] * (c - a)) - tp[0]
    d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    assert torch.equal(none[0], d2 > params[2] * params[2])
    total = sum(host(h[0])[0, 0].astype(cr.LD) for h in halves)
    error = cr.relative(host(terms)[0, 0] - total, total)
    print(f"F = {F}, P = {P}: {int((~none).sum())} correspondences equal, term_0 against the sum of the halves {error:.2e}")
    assert error <= sg.GPU_TOL_TERMS


def test_zz_report_the_largest_errors():
    """(runs last in the file: what DESIGN.md 4p quotes)"""
    print(f"largest errors of this run: terms {WORST['terms']:.2e} (allowed {sg.GPU_TOL_TERMS:.1e}), gradient {WORST['gradient']:.2e} (allowed {sg.GPU_TOL_GRADIENT:.1e})")
