"""GPU checks of the point-to-surface kernels (include/deodr_hip_surface.h, deodr_amd/csrc/dr_surface.h) against the restatement of
tests/surface_reference.py: ``nearest_face``, ``nearest_point`` and the set of truncated pairs EQUAL everywhere, ``barycentric`` bit-equal, terms,
loss and gradient within 8 x the measured float64 error; outputs between guards, the scratch exactly ``deodr_hip_surface_distance_scratch_bytes``
long between guards and pre-filled with NaN; two calls bit-identical.  Sizes: the case table (F and P through 1, 2, 63, 64, 65, 255, 256, 257,
n = 1, 2, 3), every size at which the split rule changes its answer with its lower neighbour, as faces and as points, the first sizes where
grid_sum needs its second round; the three directions, NULL and zero weights, padded clouds, the truncation.  Geometry: the seven regions, an
octahedron and a sphere with outside points (exact ties across lanes, tiles and segments; 5 000 points that choose among 8 faces), points bit-equal
to vertices, edge points and face points, zero-area triangles (one of them the lowest index of a tie), vertices without a face, a vertex with
more corners than a wavefront.  Then a replayed graph, the autograd op and the fitter eager against graphed."""

import numpy as np
import pytest
import torch

import surface_reference as sr
from test_basis_gpu import Arena, host

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD_BYTES, GUARD_BYTE = 4096, 0xA5
PAD_WORDS, INDEX_GUARD = 1024, 0x5A5A5A5A
WORST = {"terms": 0.0, "gradient": 0.0}


class GuardedScratch:
    """exactly deodr_hip_surface_distance_scratch_bytes bytes filled with NaN, between two guards in the same allocation"""

    def __init__(self, V, F, P, n):
        from deodr_amd.hip_renderer import lib

        self.nbytes = int(lib().deodr_hip_surface_distance_scratch_bytes(V, F, P, n))
        assert self.nbytes == sr.scratch_bytes(V, F, P, n)
        self.buffer = torch.full((self.nbytes + 2 * GUARD_BYTES,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.front = self.buffer[GUARD_BYTES : GUARD_BYTES + self.nbytes]
        self.front.view(torch.float64).fill_(float("nan"))
        assert self.front.data_ptr() % 8 == 0

    def check(self):
        assert bool((self.buffer[:GUARD_BYTES] == GUARD_BYTE).all()), "the memory in front of the scratch was written"
        assert bool((self.buffer[GUARD_BYTES + self.nbytes :] == GUARD_BYTE).all()), "the scratch was written beyond deodr_hip_surface_distance_scratch_bytes"


def tables(c):
    """(faces, corner_offsets, corners) int32 device tensors of a case, the table by the restatement's plain loop"""
    offsets, corners = sr.corner_table(c["faces"], c["vertices"].shape[1])
    return tuple(torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=DEV) for a in (c["faces"], offsets, corners))


def run(c, calls=2, nearest=True):
    """``calls`` calls of the library on the case, outputs and scratch guarded -> [(terms, loss, vertices_b, nearest_face, barycentric, nearest_point)]"""
    from deodr_amd import hip_renderer as hr

    n, V, P, F = c["vertices"].shape[0], c["vertices"].shape[1], c["points"].shape[1], len(c["faces"])
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
        got = hr.surface_distance(v, faces, offsets, corners, p, params, pw, uw, c["directions"], terms=terms, loss=loss, vertices_b=g, nearest_face=nf,
                                  barycentric=bary, nearest_point=npt, scratch=scratch.front)  # fmt: skip
        assert got[0] is terms and got[2] is g and got[3] is nf and got[4] is bary and got[5] is npt
        outs.append((terms, loss, g, nf, bary, npt))
    torch.cuda.synchronize()
    arena.check(), scratch.check()
    for buffer, numel in guarded:
        assert bool((buffer[:PAD_WORDS] == INDEX_GUARD).all()) and bool((buffer[PAD_WORDS + numel :] == INDEX_GUARD).all()), "written outside an index array"
        assert not bool((buffer[PAD_WORDS : PAD_WORDS + numel] == INDEX_GUARD).any()), "an index array was not written everywhere"
    return outs


def check_parity(c, nearest=True):
    first, second = run(c, nearest=nearest)
    for a, b in zip(first, second):
        assert (a is None and b is None) or torch.equal(a, b)  # bit-identical from run to run
    h = [None if t is None else host(t) for t in first]
    e_terms, e_grad = sr.errors(c, *h)  # (asserts the equality of the indices and of the bits of the barycentric coordinates)
    if nearest:
        for got, ref in ((h[3], c["ref"]["nearest_face"]), (h[4], c["ref"]["barycentric"]), (h[5], c["ref"]["nearest_point"])):
            assert (got is None) == (ref is None)
    print(f"{c['name']}: terms {e_terms:.2e}, gradient / g_scale {e_grad:.2e}")
    WORST["terms"], WORST["gradient"] = max(WORST["terms"], e_terms), max(WORST["gradient"], e_grad)
    assert e_terms <= sr.GPU_TOL_TERMS and e_grad <= sr.GPU_TOL_GRADIENT, (c["name"], e_terms, e_grad)
    return h


@pytest.mark.parametrize("row", sr.parity_cases(), ids=lambda row: "-".join(f"{k}{v}" for k, v in row.items()))
def test_kernels_against_long_double(row):
    c = sr.case(**row)
    h = check_parity(c)
    kind = row.get("kind", "soup")
    if kind == "exact":  # points bit-equal to vertices, edge midpoints and face points: they cost exactly 0 and pull exactly nothing
        assert not h[0][:, 0].any() and (h[3] == 0).any() and (h[3] == 1).any()  # (the collinear faces 0 and 1 win the ties along their rows)
        if c["directions"] == 1:
            assert not h[2].any()
    if kind == "degenerate":
        assert (h[3] == 0).sum() >= 10 and np.isfinite(h[4]).all()  # the zero-area face 0 wins its ties with faces 2 and 3
    if kind == "octahedron":
        assert h[3].max() < 8 and len(np.unique(h[3])) == 8
    if kind == "fan" and c["directions"] == 1:
        assert h[2][:, 0].any() and not h[2][:, -2:].any()  # the hub of 100 corners is pulled; the two vertices no face uses get exactly 0
    if row.get("max_distance") == "below":
        w_sum, u_sum = c["point_weights"].sum(axis=1), c["vertex_weights"].sum()
        tau2 = c["params"][2] ** 2
        assert not h[2].any() and not c["ref"]["near_p"].any() and not c["ref"]["near_v"].any()  # vertices_b == 0 exactly
        assert np.abs(h[0][:, 0] - tau2 * w_sum).max() <= sr.GPU_TOL_TERMS * tau2 * w_sum.max() and abs(h[0][0, 1] - tau2 * u_sum) <= sr.GPU_TOL_TERMS * tau2 * u_sum
    if row.get("max_distance") == "mid" and kind == "soup":
        near = c["ref"]["near_p"] if c["directions"] & 1 else c["ref"]["near_v"]
        assert 0.3 < near.mean() < 0.7
        # the set of truncated pairs equals the reference's, one direction at a time: exactly the vertices that a pair within max_distance pulls
        # have a gradient (g_scale > 0: the weights are >= 0.5)
        for direction in (1, 2):
            if c["directions"] & direction:
                one = sr.case(**dict(row, directions=direction, max_distance=float(c["params"][2]))) if c["directions"] != direction else c
                assert one["params"][2] == c["params"][2]
                pulled = one["ref"]["g_scale"] > 0
                assert np.array_equal((check_parity(one)[2] != 0).any(axis=-1), pulled) and 0 < pulled.sum()
    if row.get("directions", 3) != 3:
        if row["directions"] == 2:
            assert not h[0][:, 0].any() and h[3] is None and h[4] is None
        else:
            assert not h[0][:, 1].any() and h[5] is None


def test_the_seven_regions_of_one_triangle():
    """one triangle, seven points, one per region; then 300 points around it"""
    v = np.array([[[0.0, 0, 0], [2.0, 0, 0], [0.0, 2, 0]]])
    p = np.array([[[-1.0, -1, 1], [3.0, -0.5, 1], [1.0, -1, 1], [-0.5, 3, 1], [-1.0, 1, 1], [2.0, 2, 1], [0.5, 0.5, 1]]])
    faces = np.array([[0, 1, 2]], dtype=np.int32)
    assert sr.closest(p[0], v[0, 0], v[0, 1], v[0, 2], want_region=True)[4].tolist() == [0, 1, 2, 3, 4, 5, 6]
    c = dict(name="seven regions", vertices=v, faces=faces, points=p, point_weights=None, vertex_weights=None, params=np.array([1.0, 1.0, np.inf]), directions=3)
    c["ref"] = sr.evaluate(v, faces, p, c["params"])
    h = check_parity(c)
    assert np.array_equal(h[4][0], [[1, 0, 0], [0, 1, 0], [0.5, 0.5, 0], [0, 0, 1], [0.5, 0, 0.5], [0, 0.5, 0.5], [0.5, 0.25, 0.25]])
    assert float(h[0][0, 0]) == 3 + 2.25 + 2 + 2.25 + 2 + 3 + 1
    check_parity(sr.case(F=1, P=300, V=3, seed=9))


def test_without_the_nearest_arrays():
    c = sr.case(F=300, P=700, n=2, seed=5)
    with_arrays, without = check_parity(c), check_parity(c, nearest=False)
    assert without[3] is None and without[4] is None and without[5] is None and all(np.array_equal(a, b) for a, b in zip(with_arrays[:3], without[:3]))


@pytest.mark.parametrize("part", range(9))
def test_where_the_split_rule_changes_its_answer(part):
    """every number of references up to the cap of the rule at which ``deodr_hip_chamfer_segments`` changes its answer (63 of them, seven per case
    of this test), one below and at it, as faces (65 points query them) and as points (65 faces gather from them, 37 vertices query them); the
    sizes come from the exported rule"""
    from deodr_amd import hip_renderer as hr

    upto = sr.TILE * hr.CHAMFER_MAX_SEGMENTS + 2
    changes = sr.change_points(hr.chamfer_segments, 65, upto)
    assert changes == sr.change_points(sr.segments, 65, upto) and len(changes) == hr.CHAMFER_MAX_SEGMENTS - 1 == 63
    for at in changes[7 * part : 7 * part + 7]:
        assert hr.chamfer_segments(65, at) == hr.chamfer_segments(65, at - 1) + 1
        for R in (at - 1, at):
            check_parity(sr.case(F=R, P=65, seed=R))
            check_parity(sr.case(F=65, P=R, seed=R, kind="soup"))


@pytest.mark.parametrize("many", ("points", "faces"))
def test_the_second_round_of_grid_sum(many):
    """the first size whose combine step has more workgroups than a workgroup has threads: P = 65 537 against F = 3, and F = 65 537 against P = 3"""
    from deodr_amd import hip_renderer as hr

    Q = sr.FH_BLOCK * sr.BLOCK + 1
    assert Q == 65537 and -(-Q // sr.BLOCK) == sr.FH_BLOCK + 1 <= hr.CHAMFER_MAX_BLOCKS
    check_parity(sr.case(F=3, P=Q, seed=2) if many == "points" else sr.case(F=Q, P=3, seed=1))


def test_padded_clouds_of_unequal_length():
    from deodr_amd.surface import PointSurfaceTerm

    rs = np.random.RandomState(7)
    clouds, v, faces = [rs.rand(300, 3), rs.rand(41, 3), rs.rand(257, 3)], rs.rand(3, 90, 3), sr.soup_faces(90, 170, rs)
    for directions, mask in (("both", 3), ("points_to_mesh", 1), ("mesh_to_points", 2)):
        term = PointSurfaceTerm(faces, 90, clouds, directions=directions, mix=(0.7, 1.3), device=DEV)
        assert tuple(term.points.shape) == (3, 300, 3) and term.uses_kernel(torch.as_tensor(v, device=DEV))
        terms, loss, g, nf, bary, npt = term.evaluate_no_grad(torch.as_tensor(v, device=DEV), want_nearest=True)
        for b, cloud in enumerate(clouds):  # each pose against its own cloud alone
            ref = sr.evaluate(v[b : b + 1], faces, cloud[None], (0.7, 1.3, np.inf), np.full((1, len(cloud)), 1.0 / len(cloud)), np.full(90, 1.0 / 90), mask)
            c = dict(name=f"padded {b}", params=np.array([0.7, 1.3, np.inf]), ref=ref)
            e = sr.errors(c, host(terms[b : b + 1]), host(loss[b : b + 1]), host(g[b : b + 1]), None if nf is None else host(nf[b : b + 1, : len(cloud)]),
                          None if bary is None else host(bary[b : b + 1, : len(cloud)]), None if npt is None else host(npt[b : b + 1]))  # fmt: skip
            assert e[0] <= sr.GPU_TOL_TERMS and e[1] <= sr.GPU_TOL_GRADIENT, (directions, b, e)
            if nf is not None:
                assert bool((nf[b, len(cloud) :] == nf[b, 0]).all())  # a padded point: a copy of the first


def test_a_replayed_graph_sees_the_values_of_the_moment():
    from deodr_amd import hip_renderer as hr

    c = sr.case(F=300, P=1000, n=2, seed=11, max_distance="mid")
    others = [sr.case(F=300, P=1000, n=2, seed=s, max_distance=m, mix=mix) for s, m, mix in ((12, np.inf, (1.0, 0.0)), (13, 0.05, (0.2, 3.0)), (14, "mid", (1.5, 0.5)))]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    v, p, pw, uw, params = t(c["vertices"]), t(c["points"]), t(c["point_weights"]), t(c["vertex_weights"]), t(c["params"])
    faces, offsets, corners = tables(c)
    V, F = c["vertices"].shape[1], len(c["faces"])
    scratch = hr.surface_scratch(V, F, 1000, 2, DEV)
    outs = hr.surface_distance(v, faces, offsets, corners, p, params, pw, uw, 3, scratch=scratch, want_nearest=True)  # eager: allocates the outputs
    call = lambda: hr.surface_distance(v, faces, offsets, corners, p, params, pw, uw, 3, *outs, scratch=scratch)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        call()
    for other in others:  # three replays; vertices, points, the weights and the tables overwritten in place and params changed between them
        of, oo, oc = tables(other)
        for dst, src in ((v, t(other["vertices"])), (p, t(other["points"])), (pw, t(other["point_weights"])), (uw, t(other["vertex_weights"])),
                         (params, t(other["params"])), (faces, of), (offsets, oo), (corners, oc)):  # fmt: skip
            dst.copy_(src)
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o.clone() for o in outs]
        eager = hr.surface_distance(v, faces, offsets, corners, p, params, pw, uw, 3, scratch=scratch, want_nearest=True)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(replayed, eager))
        e = sr.errors(other, *(host(o) for o in replayed))
        assert e[0] <= sr.GPU_TOL_TERMS and e[1] <= sr.GPU_TOL_GRADIENT, e


def test_op_under_autograd_against_vertices_b():
    from deodr_amd.surface import PointSurfaceTerm

    c = sr.case(F=200, P=500, n=2, seed=21, max_distance="mid")
    term = PointSurfaceTerm(c["faces"], c["vertices"].shape[1], c["points"], c["point_weights"], c["vertex_weights"], max_distance=c["params"][2],
                            mix=c["params"][:2], normalise=False, device=DEV)  # fmt: skip
    v = torch.tensor(c["vertices"], device=DEV, requires_grad=True)
    loss, terms = term.evaluate(v)
    seed = torch.tensor([0.5, -2.0], dtype=torch.float64, device=DEV)
    (g,) = torch.autograd.grad((loss * seed).sum(), v)
    vertices_b = term.evaluate_no_grad(v)[2]
    assert torch.equal(g, seed[:, None, None] * vertices_b) and not terms.requires_grad
    e = sr.errors(c, host(terms), host(loss.detach()), host(vertices_b))
    assert e[0] <= sr.GPU_TOL_TERMS and e[1] <= sr.GPU_TOL_GRADIENT
    nf, bary, npt = term.correspondences(v)
    sr.errors(c, host(terms), host(loss.detach()), host(vertices_b), host(nf), host(bary), host(npt))
    with pytest.raises(RuntimeError, match="does not require grad"):
        torch.autograd.grad(term.evaluate(v)[1].sum(), v)
    # what the kernels do not take goes through the torch ops
    l32, _ = term.evaluate(torch.tensor(c["vertices"], device=DEV).float())
    assert l32.dtype == torch.float32 and torch.allclose(l32.double(), loss.detach(), rtol=1e-3)


def test_fit_eager_against_graphed():
    """an eager and a ``GraphedStep`` fit of the hand against 4 000 surface samples give the same energies bit for bit over 10 iterations (no
    atomics on values anywhere in this iteration)"""
    from deodr_amd.mesh_fitter import GraphedStep
    from deodr_amd.surface import PointSurfaceTerm
    from test_surface_fit_host import surface_fitter

    eager = surface_fitter(DEV)
    assert isinstance(eager.term, PointSurfaceTerm) and eager.term.uses_kernel(eager.vertices)
    e_eager = [eager.step_device()[0].clone() for _ in range(10)]
    assert float(e_eager[-1]) < float(e_eager[0])
    f = surface_fitter(DEV)
    graphed = GraphedStep(f, warmup=3)  # 3 + 1 eager steps and 1 on the capture stream: iterations 0 .. 4
    assert f.iter == 5
    e_graph = [graphed.step_device()[0].clone() for _ in range(5)]  # iterations 5 .. 9
    print("eager:", [float(e) for e in e_eager], "graphed:", [float(e) for e in e_graph])
    assert all(torch.equal(a, b) for a, b in zip(e_graph, e_eager[5:]))
    assert torch.equal(f.vertices, eager.vertices)


def test_zz_report_the_largest_errors():
    """(runs last in the file: what DESIGN.md 4n quotes)"""
    print(f"largest errors of this run: terms {WORST['terms']:.2e} (allowed {sr.GPU_TOL_TERMS:.1e}), gradient {WORST['gradient']:.2e} (allowed {sr.GPU_TOL_GRADIENT:.1e})")
