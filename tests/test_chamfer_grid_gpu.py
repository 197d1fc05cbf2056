"""GPU checks of the closest-point energy over the uniform grid (include/deodr_hip_chamfer_grid.h, deodr_amd/csrc/dr_chamfer_grid.h).  Two
oracles for every case: the long-double restatement (tests/chamfer_grid_reference.py: indices and the set of truncated pairs EQUAL, terms, loss and
gradient within 8 x the measured float64 error) and the brute-force operator ``hip_renderer.chamfer`` on the same tensors (``nearest_*`` equal
wherever not NONE, NONE exactly where the brute-force d2 is above tau2).  Outputs between guards, the scratch exactly
``deodr_hip_chamfer_grid_scratch_bytes`` long between guards and filled with NaN, two calls bit-identical.  The case table (V and P through 1, 2,
63 - 65, 255 - 257 in both roles, 65 537, n = 1 and 3, the directions, the weights, the degenerate kinds, the truncations, the cell sizes), colliding
cells, the placements of the CPU file (cell faces, negative coordinates, exactly max_distance apart, beyond the clamp), ties across cells and
rings, padded clouds with 1 000 copies, 5 000 points on one vertex, a replayed graph with a shrinking max_distance, the autograd op, the fitter eager
and graphed, and one size the brute-force operator refuses, against a k-d tree."""

import itertools

import numpy as np
import pytest
import torch

import chamfer_grid_reference as gr
import chamfer_reference as cr
from test_basis_gpu import Arena, host

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD_BYTES, GUARD_BYTE = 4096, 0xA5
PAD_WORDS, INDEX_GUARD = 1024, 0x5A5A5A5A
WORST = {"terms": 0.0, "gradient": 0.0}


class GuardedScratch:
    """exactly deodr_hip_chamfer_grid_scratch_bytes bytes filled with a NaN pattern, between two guards in the same allocation"""

    def __init__(self, V, P, n):
        from deodr_amd.hip_renderer import lib

        self.nbytes = int(lib().deodr_hip_chamfer_grid_scratch_bytes(V, P, n))
        assert self.nbytes == gr.scratch_bytes(V, P, n) and self.nbytes % 4 == 0
        self.buffer = torch.full((self.nbytes + 2 * GUARD_BYTES,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.front = self.buffer[GUARD_BYTES : GUARD_BYTES + self.nbytes]
        self.front.view(torch.int32).fill_(0x7FF80000)  # a NaN as a double (either word on top) and as a float
        assert self.front.data_ptr() % 8 == 0

    def check(self):
        assert bool((self.buffer[:GUARD_BYTES] == GUARD_BYTE).all()), "the memory in front of the scratch was written"
        assert bool((self.buffer[GUARD_BYTES + self.nbytes :] == GUARD_BYTE).all()), "the scratch was written beyond deodr_hip_chamfer_grid_scratch_bytes"


def run(c, calls=2, nearest=True):
    """``calls`` calls of the grid operator on the case, outputs and scratch guarded, and one of the brute-force operator on the same tensors
    -> ([(terms, loss, vertices_b, nearest_vertex, nearest_point)], the brute-force operator's five)"""
    from deodr_amd import hip_renderer as hr

    n, V, P = c["vertices"].shape[0], c["vertices"].shape[1], c["points"].shape[1]
    assert hr.chamfer_grid_launches(V, P, n, c["directions"]) == gr.launches(V, P, n, c["directions"]) > 0
    arena = Arena()
    carve = lambda a: None if a is None else arena.carve(a)
    v, p, pw, uw, params = carve(c["vertices"]), carve(c["points"]), carve(c["point_weights"]), carve(c["vertex_weights"]), carve(c["params"])
    scratch = GuardedScratch(V, P, n)
    outs, guarded = [], []

    def indices(count):
        """[n, count] int32 between guards, pre-filled with a pattern no index has"""
        buffer = torch.full((n * count + 2 * PAD_WORDS,), INDEX_GUARD, dtype=torch.int32, device=DEV)
        guarded.append((buffer, n * count))
        return buffer[PAD_WORDS : PAD_WORDS + n * count].view(n, count)

    for _ in range(calls):
        terms, loss, g = arena.carve(shape=(n, 2)), arena.carve(shape=(n,)), arena.carve(shape=(n, V, 3))
        nv = indices(P) if nearest and c["directions"] & 1 else None
        npt = indices(V) if nearest and c["directions"] & 2 else None
        got = hr.chamfer_grid(v, p, params, c["cell_size"], pw, uw, c["directions"], terms=terms, loss=loss, vertices_b=g, nearest_vertex=nv, nearest_point=npt,
                              scratch=scratch.front)  # fmt: skip
        assert got[0] is terms and got[2] is g and got[3] is nv and got[4] is npt
        outs.append((terms, loss, g, nv, npt))
    brute = hr.chamfer(v, p, params, pw, uw, c["directions"], want_nearest=True)
    torch.cuda.synchronize()
    arena.check(), scratch.check()
    for buffer, numel in guarded:
        assert bool((buffer[:PAD_WORDS] == INDEX_GUARD).all()) and bool((buffer[PAD_WORDS + numel :] == INDEX_GUARD).all()), "written outside an index array"
        assert not bool((buffer[PAD_WORDS : PAD_WORDS + numel] == INDEX_GUARD).any()), "an index array was not written everywhere"
    return outs, brute


def against_brute(c, h, brute):
    """nearest_* equal to the brute-force operator's wherever not NONE, NONE exactly where its d2 is above tau2; the terms are its bits (the same
    combine step on the same values); its gradient within twice the tolerance (each is within one of the long-double value)"""
    tau2 = np.float64(c["params"][2]) * np.float64(c["params"][2])
    for got, theirs, queries, refs in ((h[3], brute[3], c["points"], c["vertices"]), (h[4], brute[4], c["vertices"], c["points"])):
        if got is None:
            continue
        got, theirs = gr.signed(got), host(theirs).astype(np.int64) & 0xFFFFFFFF
        d2 = gr.d2(queries, np.take_along_axis(refs, theirs[..., None], axis=1))
        assert np.array_equal(got < 0, d2 > tau2), c["name"]
        assert np.array_equal(got[got >= 0], theirs[got >= 0]), c["name"]
    assert np.array_equal(h[0], host(brute[0])) and np.array_equal(h[1], host(brute[1])), c["name"]
    scale = np.asarray(c["ref"]["g_scale"], dtype=np.float64)
    assert cr.relative(np.abs(h[2] - host(brute[2])).max(axis=-1), scale) <= 2 * gr.GPU_TOL_GRADIENT, c["name"]


def check_parity(c, nearest=True):
    (first, second), brute = run(c, nearest=nearest)
    for a, b in zip(first, second):
        assert (a is None and b is None) or torch.equal(a, b)  # bit-identical from run to run
    h = [None if t is None else host(t) for t in first]
    e_terms, e_grad = gr.errors(c, *h)  # (asserts the equality of the indices, NONE included; a gradient where g_scale is 0 must be 0 exactly)
    if nearest:
        for got, ref in ((h[3], c["ref_grid"]["nearest_vertex"]), (h[4], c["ref_grid"]["nearest_point"])):
            assert (got is None) == (ref is None)
        against_brute(c, h, brute)
    print(f"{c['name']}: terms {e_terms:.2e}, gradient / g_scale {e_grad:.2e}")
    WORST["terms"], WORST["gradient"] = max(WORST["terms"], e_terms), max(WORST["gradient"], e_grad)
    assert e_terms <= gr.GPU_TOL_TERMS and e_grad <= gr.GPU_TOL_GRADIENT, (c["name"], e_terms, e_grad)
    return h


def custom(vertices, points, max_distance, cell_size, name, point_weights=None, vertex_weights=None, mix=(0.7, 1.3), directions=3):
    """a case from arrays [n,V,3], [n,P,3]"""
    params = np.array([mix[0], mix[1], max_distance], dtype=np.float64)
    c = dict(name=name, vertices=np.ascontiguousarray(vertices, dtype=np.float64), points=np.ascontiguousarray(points, dtype=np.float64), point_weights=point_weights,
             vertex_weights=vertex_weights, params=params, directions=directions, cell_size=float(cell_size))  # fmt: skip
    c["ref"] = cr.evaluate(c["vertices"], c["points"], params, point_weights, vertex_weights, directions)
    c["ref_grid"] = gr.mask_beyond(c)
    return c


@pytest.mark.parametrize("row", gr.grid_cases(), ids=lambda row: "-".join(f"{k}{v}" for k, v in row.items()))
def test_kernels_against_long_double_and_brute_force(row):
    c = gr.case(**row)
    h = check_parity(c)
    ref = c["ref_grid"]
    if row.get("kind") == "coincident":
        assert not h[0][:, 0].any()  # d2 == 0 exactly for every point ...
        assert not check_parity(gr.case(**dict(row, directions=1)))[2].any()  # ... and their contribution to the gradient exactly 0
    if row.get("max_distance") == "below":
        assert not h[2].any() and not c["ref"]["near_p"].any() and not c["ref"]["near_v"].any()  # vertices_b == 0 exactly
        assert bool((gr.signed(h[3]) == -1).all()) and bool((gr.signed(h[4]) == -1).all())  # and no correspondence at all
    if row.get("max_distance") == "mid":
        near = c["ref"]["near_p"] if c["directions"] & 1 else c["ref"]["near_v"]
        assert 0.3 < near.mean() < 0.7
    if row.get("max_distance") == 3.0:
        assert ref["near_p"].all() and ref["near_v"].all()
    if row.get("directions", 3) != 3:
        off = 0 if row["directions"] == 2 else 1
        assert not h[0][:, off].any() and h[3 + off] is None
    if row.get("cell_size") == 1e-6:  # h = max_distance / RINGS took over: the result is the one of the cell size it was raised to
        again = check_parity(gr.case(**dict(row, cell_size=float(np.float64(row["max_distance"]) / gr.RINGS))))
        assert all(np.array_equal(a, b) for a, b in zip(h, again))


def test_without_the_nearest_arrays():
    c = gr.case(300, 700, n=3, seed=5, max_distance=0.15, cell_size=0.05)
    with_arrays, without = check_parity(c), check_parity(c, nearest=False)
    assert without[3] is None and without[4] is None and all(np.array_equal(a, b) for a, b in zip(with_arrays[:3], without[:3]))


def test_cells_that_share_a_bucket():
    """32 references spread over 32 far-apart cells share the 64 buckets of the smallest table: colliding cells only add candidates.  (A table
    has at least twice as many buckets as references, so "more occupied cells than buckets" cannot be reached literally; what it stands for --
    two cells in one bucket -- is asserted below.)"""
    from deodr_amd import hip_renderer as hr

    rs = np.random.RandomState(3)
    far = rs.permutation(np.array(list(itertools.product(range(4), repeat=3)), dtype=np.float64))[:32] * 10.0 + rs.rand(32, 3)
    assert hr.chamfer_grid_table_bits(32) == gr.table_bits(32) == gr.MIN_TABLE_BITS
    h = gr.cell_edge(0.5, 1.0)
    buckets = gr.hash_cells(gr.cells(far, h)) & 63
    assert len(np.unique(gr.cells(far, h), axis=0)) == 32 and len(np.unique(buckets)) < 32  # collisions there are
    near = far[rs.randint(32, size=3000)] + 1.5 * (rs.rand(3000, 3) - 0.5)
    check_parity(custom(far[None], near[None], 1.0, 0.5, "32 vertices in colliding cells, 3000 points around them"))
    check_parity(custom(near[None], far[None], 1.0, 0.5, "the same with the roles swapped"))


@pytest.mark.parametrize("tau, cell", ((0.25, 0.1), (0.25, 0.0625), (1.0, 0.25), (3.0, 1.0)))
def test_placements_on_cell_faces_negative_exactly_max_distance_and_beyond_the_clamp(tau, cell):
    """the coordinates of the CPU file's exactness test on one axis after the other.  The references are the multiples of h (and an ulp either side),
    the queries all placements: many queries have their nearest reference exactly max_distance away, or an ulp either side of it, across cell faces"""
    h = gr.cell_edge(cell, tau)
    xs = gr.placements(h, tau)
    xs = xs[np.abs(xs) < 1e30]  # (|x| ~ 2^60 h included; d2 stays finite)
    bases = gr.placement_bases(h)
    on_axis = lambda values, axis: np.stack([values if k == axis else np.full(len(values), -0.3 * cell) for k in range(3)], axis=-1)[None]
    for axis in range(3):
        c = custom(on_axis(bases, axis), on_axis(xs, axis)[:, ::-1], tau, cell, f"placements tau={tau} cell_size={cell} axis={axis}")
        check_parity(c)
        d2 = cr.nearest(c["points"][0], c["vertices"][0])[0]
        tau2 = np.float64(tau) * np.float64(tau)
        assert c["ref"]["near_p"].any() and not c["ref"]["near_p"].all() and (d2 == tau2).any() and (d2 == np.nextafter(tau2, np.inf)).any() | (d2 > tau2).any()
        check_parity(custom(on_axis(xs, axis), on_axis(bases, axis), tau, cell, f"placements, roles swapped, tau={tau} cell_size={cell} axis={axis}"))


def test_ties_across_cells_and_rings():
    """a lattice with the queries at the centres of its cubes: eight references at exactly the same distance, in different cells and rings; the lowest
    index must win.  And duplicates of every reference at a higher and at a lower index."""
    r = np.array(list(itertools.product(np.arange(7) * 0.25, repeat=3)))[::-1].copy()
    q = np.array(list(itertools.product(np.arange(6) * 0.25 + 0.125, repeat=3)))
    for cell in (0.25, 0.1, 0.5, 0.0625):
        c = custom(r[None], q[None], 0.75, cell, f"lattice cell_size={cell}")
        d = gr.d2(q[:, None, :], r[None, :, :])
        assert ((d == d.min(axis=1, keepdims=True)).sum(axis=1) == 8).all()
        check_parity(c)
    both = np.concatenate((r, r[::-1]))
    check_parity(custom(both[None], q[None], 0.75, 0.25, "lattice twice"))


def test_padded_clouds_with_a_thousand_copies_of_the_first_point():
    from deodr_amd.chamfer import PointCloudTerm

    rs = np.random.RandomState(7)
    clouds, v = [rs.rand(1300, 3), rs.rand(300, 3), rs.rand(257, 3)], rs.rand(3, 90, 3)
    for directions, mask in (("both", 3), ("points_to_mesh", 1), ("mesh_to_points", 2)):
        term = PointCloudTerm(clouds, directions=directions, mix=(0.7, 1.3), max_distance=0.2, search="grid", cell_size=0.05, device=DEV)
        brute = PointCloudTerm(clouds, directions=directions, mix=(0.7, 1.3), max_distance=0.2, device=DEV)
        assert tuple(term.points.shape) == (3, 1300, 3) and term.uses_kernel(torch.as_tensor(v, device=DEV))
        terms, loss, g, nv, npt = term.evaluate_no_grad(torch.as_tensor(v, device=DEV), want_nearest=True)
        assert torch.equal(terms, brute.evaluate_no_grad(torch.as_tensor(v, device=DEV))[0])
        for b, cloud in enumerate(clouds):  # each pose against its own cloud alone
            params = np.array([0.7, 1.3, 0.2])
            ref = cr.evaluate(v[b : b + 1], cloud[None], params, np.full((1, len(cloud)), 1.0 / len(cloud)), np.full(90, 1.0 / 90), mask)
            c = dict(name=f"padded {b}", params=params, ref=ref)
            c["ref_grid"] = gr.mask_beyond(c)
            e = gr.errors(c, host(terms[b : b + 1]), host(loss[b : b + 1]), host(g[b : b + 1]), None if nv is None else host(nv[b : b + 1, : len(cloud)]),
                          None if npt is None else host(npt[b : b + 1]))  # fmt: skip
            assert e[0] <= gr.GPU_TOL_TERMS and e[1] <= gr.GPU_TOL_GRADIENT, (directions, b, e)
            if nv is not None:
                assert bool((nv[b, len(cloud) :] == nv[b, 0]).all())  # a padded point: a copy of the first


def test_five_thousand_points_that_choose_one_vertex():
    """the long run of the gather: a wavefront adds it strided, then in its tree"""
    rs = np.random.RandomState(9)
    v = rs.rand(1, 50, 3) * 4.0
    p = v[:, 7:8, :] + 1e-4 * (rs.rand(1, 5000, 3) - 0.5)
    c = custom(v, p, 0.5, 0.2, "5000 points on vertex 7", point_weights=0.5 + rs.rand(1, 5000), vertex_weights=0.5 + rs.rand(50))
    assert (c["ref"]["nearest_vertex"] == 7).all() and c["ref"]["near_p"].all()
    h = check_parity(c)
    only = check_parity(custom(v, p, 0.5, 0.2, "5000 points on vertex 7, points -> mesh", c["point_weights"], c["vertex_weights"], directions=1))
    assert not np.delete(only[2], 7, axis=1).any() and only[2][0, 7].any() and h[2][0, 7].any()
    coincident = custom(v, np.repeat(v[:, 7:8, :], 5000, axis=1), 0.5, 0.2, "5000 copies of vertex 7", directions=1)
    assert not check_parity(coincident)[2].any()


def test_a_replayed_graph_sees_the_values_of_the_moment_and_a_shrinking_max_distance():
    from deodr_amd import hip_renderer as hr

    cell = 0.01  # below every max_distance / RINGS here: h follows params[2]
    c = gr.case(300, 1000, n=3, seed=11, max_distance=0.3, cell_size=cell)
    others = [gr.case(300, 1000, n=3, seed=s, max_distance=m, mix=mix, cell_size=cell) for s, m, mix in ((12, 0.2, (1.0, 0.0)), (13, 0.1, (0.2, 3.0)), (14, 0.05, (1.5, 0.5)))]
    assert len({float(gr.cell_edge(cell, o["params"][2])) for o in [c] + others}) == 4
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    v, p, pw, uw, params = t(c["vertices"]), t(c["points"]), t(c["point_weights"]), t(c["vertex_weights"]), t(c["params"])
    scratch = hr.chamfer_grid_scratch(300, 1000, 3, DEV)
    outs = hr.chamfer_grid(v, p, params, cell, pw, uw, 3, scratch=scratch, want_nearest=True)  # eager: allocates the outputs
    call = lambda: hr.chamfer_grid(v, p, params, cell, pw, uw, 3, *outs, scratch=scratch)
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
        eager = hr.chamfer_grid(v, p, params, cell, pw, uw, 3, scratch=scratch, want_nearest=True)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(replayed, eager))
        e = gr.errors(other, *(host(o) for o in replayed))
        assert e[0] <= gr.GPU_TOL_TERMS and e[1] <= gr.GPU_TOL_GRADIENT, e


def test_op_under_autograd_against_vertices_b():
    from deodr_amd.chamfer import PointCloudTerm

    c = gr.case(200, 500, n=3, seed=21, max_distance="mid", cell_size=0.03)
    term = PointCloudTerm(c["points"], c["point_weights"], c["vertex_weights"], max_distance=c["params"][2], mix=c["params"][:2], normalise=False, device=DEV,
                          search="grid", cell_size=0.03)  # fmt: skip
    v = torch.tensor(c["vertices"], device=DEV, requires_grad=True)
    loss, terms = term.evaluate(v)
    seed = torch.tensor([0.5, -2.0, 1.25], dtype=torch.float64, device=DEV)
    (g,) = torch.autograd.grad((loss * seed).sum(), v)
    vertices_b = term.evaluate_no_grad(v)[2]
    assert torch.equal(g, seed[:, None, None] * vertices_b) and not terms.requires_grad
    nv, npt = term.correspondences(v)
    e = gr.errors(c, host(terms), host(loss.detach()), host(vertices_b), host(nv), host(npt))
    assert e[0] <= gr.GPU_TOL_TERMS and e[1] <= gr.GPU_TOL_GRADIENT and nv.dtype == torch.int64 and int(nv.min()) == -1
    with pytest.raises(RuntimeError, match="does not require grad"):
        torch.autograd.grad(term.evaluate(v)[1].sum(), v)
    # what the kernels do not take goes through the torch ops, with the same correspondences
    cpu = term.correspondences(torch.tensor(c["vertices"], device=DEV).float().double().cpu())
    assert cpu[0].device.type == "cpu" and int(cpu[0].min()) == -1


def test_fit_eager_graphed_and_against_the_brute_force_fit():
    """an eager and a ``GraphedStep`` fit with ``search="grid"`` give the same energies bit for bit.  Against the brute-force fit: the first energy
    has its bits (the terms are added by the same combine step over the same values); afterwards the two differ by the order in which a vertex adds
    the pulls of its points (each gradient within GPU_TOL_GRADIENT of the exact one), which ten damped steps carry into the energy: 1e-10 of it is
    five orders above that and five below anything a wrong correspondence would do -- a reasoned figure, not a derived bound."""
    from deodr_amd.mesh_fitter import GraphedStep
    from test_chamfer_fit_host import cloud_fitter, hand

    tau = 2 * hand()[0].std()
    eager = cloud_fitter(DEV, search="grid", max_distance=tau)
    assert eager.term.uses_kernel(eager.vertices) and eager.term.search == "grid"
    e_eager = [eager.step_device()[0].clone() for _ in range(10)]
    assert float(e_eager[-1]) < float(e_eager[0])
    f = cloud_fitter(DEV, search="grid", max_distance=tau)
    graphed = GraphedStep(f, warmup=3)  # 3 + 1 eager steps and 1 on the capture stream: iterations 0 .. 4
    assert f.iter == 5
    e_graph = [graphed.step_device()[0].clone() for _ in range(5)]  # iterations 5 .. 9
    print("eager:", [float(e) for e in e_eager], "graphed:", [float(e) for e in e_graph])
    assert all(torch.equal(a, b) for a, b in zip(e_graph, e_eager[5:]))
    assert torch.equal(f.vertices, eager.vertices)
    brute = cloud_fitter(DEV, max_distance=tau)
    e_brute = [brute.step_device()[0].clone() for _ in range(10)]
    assert torch.equal(e_brute[0], e_eager[0])
    assert all(abs(float(a) - float(b)) <= 1e-10 * float(b) for a, b in zip(e_eager, e_brute))


def test_a_size_the_brute_force_operator_refuses_against_a_kd_tree():
    from scipy.spatial import cKDTree

    from deodr_amd import hip_renderer as hr

    V, P, tau, cell = 262144, 262145, 0.04, 0.016  # the mean spacing of 2^18 uniform points in the unit cube is 0.0156
    rs = np.random.RandomState(5)
    v, p, w, u = rs.rand(1, V, 3), rs.rand(1, P, 3), 0.5 + rs.rand(1, P), 0.5 + rs.rand(V)
    params = np.array([0.7, 1.3, tau])
    t = lambda a: torch.as_tensor(a, device=DEV)
    tv, tp = t(v), t(p)
    with pytest.raises(ValueError, match="outside the limits"):
        hr.chamfer(tv, tp, t(params), t(w), t(u), 3)
    terms, loss, g, nv, npt = hr.chamfer_grid(tv, tp, t(params), cell, t(w), t(u), 3, want_nearest=True)
    again = hr.chamfer_grid(tv, tp, t(params), cell, t(w), t(u), 3, want_nearest=True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((terms, loss, g, nv, npt), again))
    tau2 = np.float64(tau) * np.float64(tau)
    sums = []
    for got, queries, refs, weights in ((gr.signed(host(nv))[0], p[0], v[0], w[0]), (gr.signed(host(npt))[0], v[0], p[0], u)):
        _, tree = cKDTree(refs).query(queries, k=1, distance_upper_bound=tau * (1 + 1e-9))  # (len(refs): nothing within the bound)
        found = tree < len(refs)
        d_tree = np.where(found, gr.d2(queries, refs[np.minimum(tree, len(refs) - 1)]), np.inf)  # the header's d2 at the tree's index
        d_got = np.where(got >= 0, gr.d2(queries, refs[np.maximum(got, 0)]), np.inf)
        assert np.array_equal(got < 0, ~(d_tree <= tau2))  # NONE exactly where the nearest neighbour is beyond max_distance
        have = got >= 0
        same = got[have] == tree[have]
        tie = (d_got[have] == d_tree[have]) & (got[have] < tree[have])  # equal header-d2 at both indices, the lower index returned
        print(f"k-d tree: {int(have.sum())} correspondences, {int((~same).sum())} differ from the tree's index, all of them ties won by the lower index: {bool((same | tie).all())}")
        assert bool((same | tie).all()) and bool((d_got[have] <= tau2).all()) and have.mean() > 0.2
        sums.append((weights.astype(cr.LD) * np.minimum(d_got, tau2).astype(cr.LD)).sum())
    e = max(cr.relative(host(terms)[0, 0] - sums[0], sums[0]), cr.relative(host(terms)[0, 1] - sums[1], sums[1]),
            cr.relative(host(loss)[0] - (cr.LD(0.7) * sums[0] + cr.LD(1.3) * sums[1]), cr.LD(0.7) * sums[0] + cr.LD(1.3) * sums[1]))  # fmt: skip
    print(f"V = {V}, P = {P}: terms against the long-double sums over the tree's correspondences {e:.2e}")
    # grid_sum adds 2^18 values in a tree of depth < 32 (three per thread, a wavefront, four wavefronts, two partials per thread, the same again):
    # 32 roundings of 2^-53 are 3.6e-15, inside the table's tolerance
    assert e <= gr.GPU_TOL_TERMS


def test_zz_report_the_largest_errors():
    """(runs last in the file: what DESIGN.md 4o quotes)"""
    print(f"largest errors of this run: terms {WORST['terms']:.2e} (allowed {gr.GPU_TOL_TERMS:.1e}), gradient {WORST['gradient']:.2e} (allowed {gr.GPU_TOL_GRADIENT:.1e})")
