"""GPU checks of the closest-point kernels (include/deodr_hip_chamfer.h, deodr_amd/csrc/dr_chamfer.h) against the restatement of
tests/chamfer_reference.py: the nearest indices EQUAL everywhere, terms, loss and gradient within 8 x the measured float64 error; outputs between
guards, the scratch exactly ``deodr_hip_chamfer_scratch_bytes`` long between guards and pre-filled with NaN; two calls bit-identical.  Sizes: the
case table (1, 2, 63, 64, 65, around a workgroup and an LDS tile, n = 1, 2, 3), every size at which the exported split rule changes its answer, the
first size where grid_sum needs its second round; the three directions, NULL and zero weights, padded clouds, ties across tiles and segments,
coincident points, the truncation, the clustered cloud, a replayed graph, the autograd op and the fitter eager, graphed and against the CPU."""

import numpy as np
import pytest
import torch

import chamfer_reference as cr
from test_basis_gpu import Arena, host

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD_BYTES, GUARD_BYTE = 4096, 0xA5
PAD_WORDS, INDEX_GUARD = 1024, 0x5A5A5A5A
WORST = {"terms": 0.0, "gradient": 0.0}


class GuardedScratch:
    """exactly deodr_hip_chamfer_scratch_bytes bytes filled with NaN, between two guards in the same allocation"""

    def __init__(self, V, P, n):
        from deodr_amd.hip_renderer import lib

        self.nbytes = int(lib().deodr_hip_chamfer_scratch_bytes(V, P, n))
        assert self.nbytes == cr.scratch_bytes(V, P, n)
        self.buffer = torch.full((self.nbytes + 2 * GUARD_BYTES,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.front = self.buffer[GUARD_BYTES : GUARD_BYTES + self.nbytes]
        self.front.view(torch.float64).fill_(float("nan"))
        assert self.front.data_ptr() % 8 == 0

    def check(self):
        assert bool((self.buffer[:GUARD_BYTES] == GUARD_BYTE).all()), "the memory in front of the scratch was written"
        assert bool((self.buffer[GUARD_BYTES + self.nbytes :] == GUARD_BYTE).all()), "the scratch was written beyond deodr_hip_chamfer_scratch_bytes"


def run(c, calls=2, nearest=True):
    """``calls`` calls of the library on the case, outputs and scratch guarded -> [(terms, loss, vertices_b, nearest_vertex, nearest_point)]"""
    from deodr_amd import hip_renderer as hr

    n, V, P = c["vertices"].shape[0], c["vertices"].shape[1], c["points"].shape[1]
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
        got = hr.chamfer(v, p, params, pw, uw, c["directions"], terms=terms, loss=loss, vertices_b=g, nearest_vertex=nv, nearest_point=npt, scratch=scratch.front)
        assert got[0] is terms and got[2] is g and got[3] is nv and got[4] is npt
        outs.append((terms, loss, g, nv, npt))
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
    e_terms, e_grad = cr.errors(c, *h)  # (asserts the equality of the indices)
    if nearest:
        for got, ref in ((h[3], c["ref"]["nearest_vertex"]), (h[4], c["ref"]["nearest_point"])):
            assert (got is None) == (ref is None)
    print(f"{c['name']}: terms {e_terms:.2e}, gradient / g_scale {e_grad:.2e}")
    WORST["terms"], WORST["gradient"] = max(WORST["terms"], e_terms), max(WORST["gradient"], e_grad)
    assert e_terms <= cr.GPU_TOL_TERMS and e_grad <= cr.GPU_TOL_GRADIENT, (c["name"], e_terms, e_grad)
    return h


@pytest.mark.parametrize("row", cr.parity_cases(), ids=lambda row: "-".join(f"{k}{v}" for k, v in row.items()))
def test_kernels_against_long_double(row):
    """V and P through 1, 2, 63, 64, 65, one below, at and one above a workgroup's queries and an LDS tile (both 256), n = 1, 2, 3; the three
    directions, NULL and zero weights, ties, coincident points, the truncation, the clustered cloud"""
    c = cr.case(**row)
    h = check_parity(c)
    if row.get("kind") == "coincident":
        assert not h[0][:, 0].any()  # d2 == 0 exactly for every point ...
        only = cr.case(**dict(row, directions=1))
        assert not check_parity(only)[2].any()  # ... and their contribution to the gradient exactly 0
    if row.get("max_distance") == "below":
        w_sum, u_sum = c["point_weights"].sum(axis=1), c["vertex_weights"].sum()
        tau2 = c["params"][2] ** 2
        assert not h[2].any() and not c["ref"]["near_p"].any() and not c["ref"]["near_v"].any()  # vertices_b == 0 exactly
        assert np.abs(h[0][:, 0] - tau2 * w_sum).max() <= cr.GPU_TOL_TERMS * tau2 * w_sum.max() and abs(h[0][0, 1] - tau2 * u_sum) <= cr.GPU_TOL_TERMS * tau2 * u_sum
    if row.get("max_distance") == "mid":
        near = c["ref"]["near_p"] if c["directions"] & 1 else c["ref"]["near_v"]
        assert 0.3 < near.mean() < 0.7
        # the set of truncated pairs equals the reference's, one direction at a time: exactly the vertices that a pair within max_distance pulls
        # have a gradient (the weights are >= 0.5 and no distance is 0 in a uniform case)
        for direction in (1, 2):
            if c["directions"] & direction:
                one = cr.case(**dict(row, directions=direction)) if c["directions"] != direction else c
                assert one["params"][2] == c["params"][2]
                pulled = np.zeros(h[2].shape[:2], dtype=bool)
                for b in range(pulled.shape[0]):
                    if direction == 1:
                        pulled[b, one["ref"]["nearest_vertex"][b][one["ref"]["near_p"][b]]] = True
                    else:
                        pulled[b] = one["ref"]["near_v"][b]
                assert np.array_equal((check_parity(one)[2] != 0).any(axis=-1), pulled) and 0 < pulled.sum() < pulled.size
    if row.get("directions", 3) != 3:
        off = 0 if row["directions"] == 2 else 1
        assert not h[0][:, off].any() and h[3 + off] is None


def test_without_the_nearest_arrays():
    c = cr.case(300, 700, n=2, seed=5)
    with_arrays, without = check_parity(c), check_parity(c, nearest=False)
    assert without[3] is None and without[4] is None and all(np.array_equal(a, b) for a, b in zip(with_arrays[:3], without[:3]))


@pytest.mark.parametrize("part", range(7))
def test_where_the_split_rule_changes_its_answer(part):
    """every number of references up to the cap of the rule at which ``deodr_hip_chamfer_segments`` changes its answer (63 of them, nine per case
    of this test), two below, one below and at it, as points (65 vertices query them, and gather from them) and as vertices (65 points query them);
    the sizes come from the exported rule"""
    from deodr_amd import hip_renderer as hr

    upto = cr.TILE * hr.CHAMFER_MAX_SEGMENTS + 2
    changes = cr.change_points(hr.chamfer_segments, 65, upto)
    assert changes == cr.change_points(cr.segments, 65, upto) and len(changes) == hr.CHAMFER_MAX_SEGMENTS - 1 == 63
    assert hr.chamfer_segments(65, changes[-1]) == hr.CHAMFER_MAX_SEGMENTS == hr.chamfer_segments(65, 10 * upto)
    for at in changes[9 * part : 9 * part + 9]:
        assert hr.chamfer_segments(65, at) == hr.chamfer_segments(65, at - 1) + 1
        for R in (at - 2, at - 1, at):
            check_parity(cr.case(65, R, seed=R))
            check_parity(cr.case(R, 65, seed=R, kind="clustered" if R % 2 else "uniform"))


@pytest.mark.parametrize("shift", (-1, 0, 1))
def test_where_the_split_rule_changes_with_the_queries(shift):
    """the first number of queries at which a search over two tiles is no longer cut: one below, at it, above"""
    from deodr_amd import hip_renderer as hr

    R = cr.TILE + 1
    Q = next(q for q in range(1, 2 * cr.BLOCK * cr.TARGET_BLOCKS, cr.BLOCK) if hr.chamfer_segments(q, R) == 1)
    assert hr.chamfer_segments(Q - 1, R) == 2 and Q == (cr.TARGET_BLOCKS - 1) * cr.BLOCK + 1
    # (the points are the many: the queries of the first search, which is the one the change is about, and the references of the gather)
    check_parity(cr.case(R, Q + shift, seed=shift, directions=1))


@pytest.mark.parametrize("many", ("vertices", "points"))
def test_the_second_round_of_grid_sum(many):
    """the first size whose combine step has more workgroups than a workgroup has threads"""
    from deodr_amd import hip_renderer as hr

    Q = cr.FH_BLOCK * cr.BLOCK + 1
    assert -(-Q // cr.BLOCK) == cr.FH_BLOCK + 1 <= hr.CHAMFER_MAX_BLOCKS
    check_parity(cr.case(Q, 70, seed=1) if many == "vertices" else cr.case(70, Q, seed=2))


def test_beyond_the_cap_of_the_combine_grid():
    Q = cr.MAX_BLOCKS * cr.BLOCK + 3  # (the threads of the combine step stride)
    check_parity(cr.case(Q, 40, seed=3, directions=2))
    check_parity(cr.case(40, Q, seed=4, directions=1))


def test_padded_clouds_of_unequal_length():
    from deodr_amd.chamfer import PointCloudTerm

    rs = np.random.RandomState(7)
    clouds, v = [rs.rand(300, 3), rs.rand(41, 3), rs.rand(257, 3)], rs.rand(3, 90, 3)
    for directions, mask in (("both", 3), ("points_to_mesh", 1), ("mesh_to_points", 2)):
        term = PointCloudTerm(clouds, directions=directions, mix=(0.7, 1.3), device=DEV)
        assert tuple(term.points.shape) == (3, 300, 3) and term.uses_kernel(torch.as_tensor(v, device=DEV))
        terms, loss, g, nv, npt = term.evaluate_no_grad(torch.as_tensor(v, device=DEV), want_nearest=True)
        for b, cloud in enumerate(clouds):  # each pose against its own cloud alone
            ref = cr.evaluate(v[b : b + 1], cloud[None], (0.7, 1.3, np.inf), np.full((1, len(cloud)), 1.0 / len(cloud)), np.full(90, 1.0 / 90), mask)
            c = dict(name=f"padded {b}", params=np.array([0.7, 1.3, np.inf]), ref=ref)
            e = cr.errors(c, host(terms[b : b + 1]), host(loss[b : b + 1]), host(g[b : b + 1]), None if nv is None else host(nv[b : b + 1, : len(cloud)]),
                          None if npt is None else host(npt[b : b + 1]))  # fmt: skip
            assert e[0] <= cr.GPU_TOL_TERMS and e[1] <= cr.GPU_TOL_GRADIENT, (directions, b, e)
            if nv is not None:
                assert bool((nv[b, len(cloud) :] == nv[b, 0]).all())  # a padded point: a copy of the first


def test_a_replayed_graph_sees_the_values_of_the_moment():
    from deodr_amd import hip_renderer as hr

    c = cr.case(300, 1000, n=2, seed=11, max_distance="mid")
    others = [cr.case(300, 1000, n=2, seed=s, max_distance=m, mix=mix) for s, m, mix in ((12, np.inf, (1.0, 0.0)), (13, 0.05, (0.2, 3.0)), (14, "mid", (1.5, 0.5)))]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    v, p, pw, uw, params = t(c["vertices"]), t(c["points"]), t(c["point_weights"]), t(c["vertex_weights"]), t(c["params"])
    scratch = hr.chamfer_scratch(300, 1000, 2, DEV)
    outs = hr.chamfer(v, p, params, pw, uw, 3, scratch=scratch, want_nearest=True)  # eager: allocates the outputs
    call = lambda: hr.chamfer(v, p, params, pw, uw, 3, *outs, scratch=scratch)
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
        eager = hr.chamfer(v, p, params, pw, uw, 3, scratch=scratch, want_nearest=True)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(replayed, eager))
        e = cr.errors(other, *(host(o) for o in replayed))
        assert e[0] <= cr.GPU_TOL_TERMS and e[1] <= cr.GPU_TOL_GRADIENT, e


def test_op_under_autograd_against_vertices_b():
    from deodr_amd.chamfer import PointCloudTerm

    c = cr.case(200, 500, n=2, seed=21, max_distance="mid")
    term = PointCloudTerm(c["points"], c["point_weights"], c["vertex_weights"], max_distance=c["params"][2], mix=c["params"][:2], normalise=False, device=DEV)
    v = torch.tensor(c["vertices"], device=DEV, requires_grad=True)
    loss, terms = term.evaluate(v)
    seed = torch.tensor([0.5, -2.0], dtype=torch.float64, device=DEV)
    (g,) = torch.autograd.grad((loss * seed).sum(), v)
    vertices_b = term.evaluate_no_grad(v)[2]
    assert torch.equal(g, seed[:, None, None] * vertices_b) and not terms.requires_grad
    e = cr.errors(c, host(terms), host(loss.detach()), host(vertices_b))
    assert e[0] <= cr.GPU_TOL_TERMS and e[1] <= cr.GPU_TOL_GRADIENT
    with pytest.raises(RuntimeError, match="does not require grad"):
        torch.autograd.grad(term.evaluate(v)[1].sum(), v)
    # what the kernels do not take goes through the torch ops
    l32, _ = term.evaluate(torch.tensor(c["vertices"], device=DEV).float())
    assert l32.dtype == torch.float32 and torch.allclose(l32.double(), loss.detach(), rtol=1e-4)


def test_fit_eager_graphed_and_against_the_cpu():
    """an eager and a ``GraphedStep`` fit of the hand give the same energies bit for bit (no atomics on values anywhere in this iteration); the first
    energy of the GPU fit against the CPU fallback's: both are float64 evaluations of the same sums, each within TOL_TERMS of the long-double value
    -- the kernels are held to 8 x that, so 9 x TOL_TERMS of the data term, plus the rigid energy, which is 0 at the first iteration"""
    from deodr_amd.mesh_fitter import GraphedStep
    from test_chamfer_fit_host import cloud_fitter

    eager = cloud_fitter(DEV)
    assert eager.term.uses_kernel(eager.vertices)
    e_eager = [eager.step_device()[0].clone() for _ in range(10)]
    assert float(e_eager[-1]) < float(e_eager[0])
    f = cloud_fitter(DEV)
    graphed = GraphedStep(f, warmup=3)  # 3 + 1 eager steps and 1 on the capture stream: iterations 0 .. 4
    assert f.iter == 5
    e_graph = [graphed.step_device()[0].clone() for _ in range(5)]  # iterations 5 .. 9
    print("eager:", [float(e) for e in e_eager], "graphed:", [float(e) for e in e_graph])
    assert all(torch.equal(a, b) for a, b in zip(e_graph, e_eager[5:]))
    assert torch.equal(f.vertices, eager.vertices)
    first_cpu = cloud_fitter("cpu").step()[0]
    assert abs(float(e_eager[0]) - first_cpu) <= 9 * cr.TOL_TERMS * first_cpu


def test_zz_report_the_largest_errors():
    """(runs last in the file: what DESIGN.md 4m quotes)"""
    print(f"largest errors of this run: terms {WORST['terms']:.2e} (allowed {cr.GPU_TOL_TERMS:.1e}), gradient {WORST['gradient']:.2e} (allowed {cr.GPU_TOL_GRADIENT:.1e})")


@pytest.mark.parametrize("operator", ["chamfer", "chamfer_grid", "surface_distance"])
def test_a_scratch_serves_the_next_call_whatever_directions_the_last_one_had(operator):
    """Which kernel clears the arrival tickets depends on ``directions`` (the first launch of the call does).  V = 65, P = 257 (F = 130), n = 2: two
    workgroups of points, two tiles of points; one scratch, every byte 0xFF at first (NaN as doubles, no ticket and no index as words), serves calls
    with directions 3, 2, 1, 3, and every result of each has the bits of the same call on a scratch filled afresh"""
    from deodr_amd import hip_renderer as hr

    V, P, F, n = 65, 257, 130, 2
    rs = np.random.RandomState(7)
    dev = lambda a: torch.as_tensor(a, device=DEV)
    v, p, pw, uw = dev(rs.rand(n, V, 3)), dev(rs.rand(n, P, 3)), dev(0.5 + rs.rand(n, P)), dev(0.5 + rs.rand(V))
    params = dev(np.array([0.7, 1.3, 0.25]))  # (a finite max_distance: some pairs are beyond it)
    if operator == "surface_distance":
        from deodr_amd.surface import corner_table

        faces = np.stack([rs.permutation(V)[:3] for _ in range(F)]).astype(np.int32)
        offsets, corners = corner_table(faces, V)
        fresh = lambda: hr.surface_scratch(V, F, P, n, DEV).fill_(0xFF)
        call = lambda d, scratch: hr.surface_distance(v, dev(faces), dev(offsets), dev(corners), p, params, pw, uw, d, scratch=scratch, want_nearest=True)
    elif operator == "chamfer_grid":
        fresh = lambda: hr.chamfer_grid_scratch(V, P, n, DEV).fill_(0xFF)
        call = lambda d, scratch: hr.chamfer_grid(v, p, params, 0.1, pw, uw, d, scratch=scratch, want_nearest=True)
    else:
        fresh = lambda: hr.chamfer_scratch(V, P, n, DEV).fill_(0xFF)
        call = lambda d, scratch: hr.chamfer(v, p, params, pw, uw, d, scratch=scratch, want_nearest=True)
    shared = fresh()
    for step, directions in enumerate((3, 2, 1, 3)):
        got, want = call(directions, shared), call(directions, fresh())
        assert len(got) == len(want) == (6 if operator == "surface_distance" else 5)
        for a, b in zip(got, want):
            assert (a is None) == (b is None), (step, directions)
            assert a is None or torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), (step, directions)
        # (the nearest_* arrays of the directions that are on were among them)
        assert all((t is None) == (not directions & 1) for t in got[3:-1]) and (got[-1] is None) == (not directions & 2)
