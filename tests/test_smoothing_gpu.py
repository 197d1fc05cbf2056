"""GPU tests of the sparse symmetric positive definite solve: ``deodr_hip_spd_solve`` against the long-double restatement of
tests/smoothing_reference.py over its case table -- systems of 1, 2 and 3 rows, a row with only its diagonal, rows of 7 / 8 / 9 / 17 entries, the sizes
either side of N_SMALL (both kernel instances on nearly the same system), of the rows a workgroup takes and of a capped grid, D = 1, 3, 4 and
m = 1, 2, 8, 16 --, the long run through its true residual, a run past n steps, the autograd op, a captured call replayed after ``b`` and ``vals``
were overwritten, and the ``smoothing=`` keyword of the fitters, eager and replayed as a HIP graph.

The tolerance is derived in tests/smoothing_reference.py: TOLERANCE[m] = 8 x (the largest float64 error of the torch recurrence at m steps),
relative to ``max |x|`` of the case for x and to its own value for the residual.

Every call of the case table: x and residual are carved out of larger NaN-filled buffers and the scratch has exactly
deodr_hip_spd_solve_scratch_bytes bytes, filled with a pattern (the header: it need not be zeroed), followed by a guard; all checked after the
call.  A second call gives the same bits."""

import numpy as np
import pytest
import torch

import smoothing_reference as sr
from test_basis_gpu import Arena, host

pytestmark = pytest.mark.gpu

LD = sr.LD
DEV = "cuda"
GUARD_BYTES, GUARD_BYTE, FILL_BYTE = 4096, 0xA5, 0x7F


class GuardedScratch:
    """exactly deodr_hip_spd_solve_scratch_bytes bytes filled with a pattern, between two guards in the same allocation"""

    def __init__(self, n, D):
        from deodr_amd.hip_renderer import lib

        self.nbytes = int(lib().deodr_hip_spd_solve_scratch_bytes(n, D))
        assert self.nbytes == 64 + 8 * (24 + 4 * sr.BLOCKS + 4 * n * D)
        self.buffer = torch.full((self.nbytes + 2 * GUARD_BYTES,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.front = self.buffer[GUARD_BYTES : GUARD_BYTES + self.nbytes]
        self.front.fill_(FILL_BYTE)
        assert self.front.data_ptr() % 8 == 0

    def check(self, counters_used):
        assert bool((self.buffer[: GUARD_BYTES] == GUARD_BYTE).all()), "the memory in front of the scratch was written"
        assert bool((self.buffer[GUARD_BYTES + self.nbytes :] == GUARD_BYTE).all()), "the scratch was written beyond deodr_hip_spd_solve_scratch_bytes"
        if counters_used:
            assert bool((self.front[:64] == 0).all()), "the counter words of the scratch were not left at zero"


def u32(a):
    return torch.as_tensor(np.ascontiguousarray(a).astype(np.uint32).view(np.int32), device=DEV)


def solve_case(case, iterations=None, rel_tol=0.0, calls=2):
    """``calls`` calls of the library on the case, outputs and scratch guarded -> [(x, residual)]"""
    from deodr_amd import hip_renderer as hr

    n, D = case["b"].shape
    arena = Arena()
    offsets, cols, vals, b = u32(case["offsets"]), u32(case["cols"]), arena.carve(case["vals"]), arena.carve(case["b"])
    scratch = GuardedScratch(n, D)
    outs = []
    for _ in range(calls):
        x, residual = arena.carve(shape=(n, D)), arena.carve(shape=(D,))
        got = hr.spd_solve(offsets, cols, vals, b, case["iterations"] if iterations is None else iterations, rel_tol, x=x, residual=residual, scratch=scratch.front)
        assert got[0] is x and got[1] is residual
        outs.append((x, residual))
    torch.cuda.synchronize()
    arena.check(), scratch.check(counters_used=n > sr.N_SMALL)
    return outs


@pytest.mark.parametrize("name", sr.parity_cases())
def test_kernels_against_long_double(name):
    from deodr_amd import hip_renderer as hr

    case, ref = sr.reference(name)
    n, D, m = case["n"], case["D"], case["iterations"]
    assert hr.spd_launches(n, len(case["cols"]), D, m) == (1 if n <= sr.N_SMALL else 2 + 2 * m)
    (x, residual), (x2, residual2) = solve_case(case)
    assert torch.equal(x, x2) and torch.equal(residual, residual2)  # a second call gives the same bits
    err_x = float(np.abs(host(x).astype(LD) - ref["x"]).max() / ref["scale"])
    live = ref["residual"] > sr.RESIDUAL_FLOOR
    err_r = float((np.abs(host(residual).astype(LD) - ref["residual"])[live] / ref["residual"][live]).max()) if live.any() else 0.0
    print(f"{name}: largest error of x relative to max |x| {err_x:.2e}, of the residual relative to its value {err_r:.2e}  (tolerance {sr.TOLERANCE[m]:.2e})")
    assert err_x <= sr.TOLERANCE[m] and err_r <= sr.TOLERANCE[m]
    assert bool(torch.isfinite(x).all()) and bool((residual >= 0).all())
    assert float(np.abs(host(residual).astype(LD) - ref["residual"])[~live].max() if (~live).any() else 0.0) <= sr.RESIDUAL_FLOOR
    if case["zero_column"] is not None:
        assert float(x[:, case["zero_column"]].abs().max()) == 0 and float(residual[case["zero_column"]]) == 0
    descent = (case["b"] * host(x)).sum(axis=0)
    assert np.all(descent[np.abs(case["b"]).sum(axis=0) > 0] > 0)  # g^T x > 0: a descent direction at every truncation


def test_both_instances_agree_on_the_same_system():
    """N_SMALL rows run as one launch, N_SMALL + 1 as 2 + 2 m: the same system with one more vertex that has no neighbour and a right-hand side
    of 0 -- in exact arithmetic the same recurrence, every sum gaining a zero.  Each is within the tolerance of the restatement, so the two agree
    within twice that."""
    from deodr_amd import hip_renderer as hr

    small, ref = sr.reference(f"hubs n={sr.N_SMALL} lam=4 D=4 m=8")
    large = dict(small, offsets=np.append(small["offsets"], len(small["cols"]) + 1), cols=np.append(small["cols"], sr.N_SMALL),
                 vals=np.append(small["vals"], 1.0), b=np.vstack((small["b"], np.zeros((1, 4)))))  # fmt: skip
    assert hr.spd_launches(sr.N_SMALL, len(small["cols"]), 4, 8) == 1 and hr.spd_launches(sr.N_SMALL + 1, len(large["cols"]), 4, 8) == 18
    (x_small, r_small), = solve_case(small, calls=1)
    (x_large, r_large), = solve_case(large, calls=1)
    scale = float(ref["scale"])
    errors = [float(np.abs(host(x)[: sr.N_SMALL].astype(LD) - ref["x"]).max()) / scale for x in (x_small, x_large)]
    difference = float((x_large[: sr.N_SMALL] - x_small).abs().max()) / scale
    print(f"one launch / 2 + 2 m launches against long double {errors[0]:.2e} / {errors[1]:.2e}, against one another {difference:.2e} (relative to max |x|)")
    assert max(errors) <= sr.TOLERANCE[8] and difference <= 2 * sr.TOLERANCE[8] and float(x_large[sr.N_SMALL].abs().max()) == 0
    assert torch.allclose(r_small, r_large, rtol=sr.TOLERANCE[8], atol=0)


def test_the_long_run_converges():
    """lambda = 4, m = 64 on the sphere: |b - A x| / |b| recomputed in long double from the returned x"""
    case, _ = sr.reference("sphere 322 lam=4 D=3 m=64 convergence")
    (x, residual), (x2, _) = solve_case(case)
    true = sr.true_residual(case["offsets"], case["cols"], case["vals"], case["b"], host(x))
    print(f"|b - A x| / |b| per column: {[f'{float(v):.2e}' for v in true]}; the recurrence's squared relative residual {host(residual).tolist()}")
    assert np.all(true <= sr.CONVERGENCE) and torch.equal(x, x2)
    import scipy.sparse as sp
    import scipy.sparse.linalg

    exact = scipy.sparse.linalg.spsolve(sp.csr_matrix((case["vals"], case["cols"], case["offsets"]), shape=(case["n"],) * 2).tocsc(), case["b"])
    assert np.all(np.sqrt(((host(x) - exact) ** 2).sum(axis=0)) <= sr.CONVERGENCE * np.sqrt((case["b"] ** 2).sum(axis=0)))


def test_the_long_run_converges_above_n_small():
    """the same through the other instance: the strip of N_SMALL + 1 rows at lambda = 1, m = 64"""
    offsets, cols, vals = sr.strip_system(sr.N_SMALL + 1, 1.0)
    case = dict(offsets=offsets, cols=cols, vals=vals, b=sr.right_hand_side(sr.N_SMALL + 1, 3, seed=11), iterations=64)
    own = sr.true_residual(offsets, cols, vals, case["b"], sr.restate(offsets, cols, vals, case["b"], 64)["x"])
    (x, residual), = solve_case(case, calls=1)
    true = sr.true_residual(offsets, cols, vals, case["b"], host(x))
    print(f"|b - A x| / |b| per column: {[f'{float(v):.2e}' for v in true]}, the restatement's own {[f'{float(v):.2e}' for v in own]}")
    assert np.all(own <= sr.CONVERGENCE / 10) and np.all(true <= sr.CONVERGENCE)


def test_a_run_past_n_steps_is_frozen_without_a_nan():
    case, ref = sr.reference("tiny n=3 D=4 m=50 past n")
    (x, residual), (x2, _) = solve_case(case)
    exact = np.linalg.solve(np.array([[3.0, -1, 0], [-1, 3, -1], [0, -1, 2]]), case["b"])
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(residual).all()) and torch.equal(x, x2)
    assert np.abs(host(x) - exact).max() <= 1e-14 * np.abs(exact).max() and float(residual.max()) < 1e-28
    (longer, _), = solve_case(case, iterations=500, calls=1)  # x stays where it froze
    assert np.abs(host(longer) - host(x)).max() <= 1e-15 * np.abs(exact).max()


@pytest.mark.parametrize("name, tolerances", [("sphere 322 lam=4 D=4 m=8 zero column", (1e-1, 1e-2)),
                                               (f"hubs n={sr.N_SMALL + 1} lam=4 D=4 m=8 zero column", (1e-1, 3e-2))], ids=["one launch", "2 + 2 m launches"])  # fmt: skip
def test_rel_tol_freezes_a_column_at_the_step_the_restatement_does(name, tolerances):
    """through both instances (above N_SMALL the `active` flag in the scratch, the held rho and beta = 0 of a frozen column, while the other columns go
    on): the tolerances freeze within 14 steps, where float64 and long double still agree to 1e-9, and the columns at different steps"""
    case, _ = sr.reference(name)
    zero = case["zero_column"]
    for rel_tol in tolerances:
        frozen = sr.restate(case["offsets"], case["cols"], case["vals"], case["b"], 40, rel_tol)["frozen_at"]
        assert frozen[zero] == 0 and all(0 < frozen[d] < 15 for d in range(4) if d != zero), frozen
        (x, residual), = solve_case(case, iterations=40, rel_tol=rel_tol, calls=1)
        assert float(x[:, zero].abs().max()) == 0 and float(residual[zero]) == 0 and bool(torch.isfinite(x).all())
        for d in (d for d in range(4) if d != zero):  # the column equals the run truncated at its own step
            (truncated, _), = solve_case(case, iterations=int(frozen[d]), calls=1)
            assert torch.equal(x[:, d], truncated[:, d]), (rel_tol, d)
            assert float(residual[d]) <= rel_tol**2


def test_op_kernel_against_the_torch_recurrence_and_its_gradient():
    from deodr_amd import smoothing

    for name in ("sphere 322 lam=4 D=4 m=8 zero column", f"hubs n={sr.N_SMALL + 1} lam=4 D=4 m=8"):
        case, ref = sr.reference(name)
        system = smoothing.SpdSystem(case["offsets"], case["cols"], case["vals"], device=DEV)
        b = torch.as_tensor(case["b"], device=DEV).requires_grad_(True)
        assert smoothing.uses_kernel(system, b) and not smoothing.uses_kernel(system, b.float()) and not smoothing.uses_kernel(system, b.cpu())
        x, residual = smoothing.spd_solve(system, b, iterations=8)
        x_torch, residual_torch = smoothing.spd_solve_torch(system, b, 8)
        for got in (x, x_torch):
            assert float(np.abs(host(got).astype(LD) - ref["x"]).max() / ref["scale"]) <= sr.TOLERANCE[8]
        w = torch.as_tensor(np.random.RandomState(4).randn(*case["b"].shape), device=DEV)
        (g,) = torch.autograd.grad((w * x).sum(), b)
        expected = sr.restate(case["offsets"], case["cols"], case["vals"], host(w), 8)["x"]
        assert float(np.abs(host(g).astype(LD) - expected).max() / np.abs(expected).max()) <= sr.TOLERANCE[8]
        assert not residual.requires_grad and torch.allclose(residual, residual_torch, rtol=1e-9)
        x32, _ = smoothing.spd_solve(system, b.detach().float(), iterations=8)  # what the kernels do not take goes through the torch recurrence
        assert x32.dtype == torch.float32 and float((x32.double() - x.detach()).abs().max()) <= 1e-4 * float(x.detach().abs().max())


@pytest.mark.parametrize("n", [526, sr.N_SMALL + 1], ids=["one launch", "2 + 2 m launches"])
def test_a_replayed_graph_sees_b_and_vals_of_the_moment(n):
    from deodr_amd import hip_renderer as hr

    m = 8
    offsets, cols, vals = sr.strip_system(n, 4.0)
    other_vals = sr.strip_system(n, 1.5)[2]
    b0, b1 = sr.right_hand_side(n, 3, seed=1), sr.right_hand_side(n, 3, seed=2)
    t = lambda a: torch.as_tensor(a, device=DEV)
    o, c, v, b = u32(offsets), u32(cols), t(vals), t(b0)
    scratch = hr.spd_scratch(n, 3, DEV)
    x, residual = hr.spd_solve(o, c, v, b, m, scratch=scratch)  # eager: allocates the outputs
    eager = (x.clone(), residual.clone())
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hr.spd_solve(o, c, v, b, m, x=x, residual=residual, scratch=scratch)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        hr.spd_solve(o, c, v, b, m, x=x, residual=residual, scratch=scratch)
    x.zero_(), residual.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(x, eager[0]) and torch.equal(residual, eager[1])
    b.copy_(t(b1)), v.copy_(t(other_vals))  # in place: the graph holds the addresses
    graph.replay()
    torch.cuda.synchronize()
    again = sr.restate(offsets, cols, other_vals, b1, m)
    assert float(np.abs(host(x).astype(LD) - again["x"]).max() / np.abs(again["x"]).max()) <= sr.TOLERANCE[8]
    assert not torch.equal(x, eager[0])


def depth_fitter(**keywords):
    from test_basis_gpu import depth_fitter as make

    return make(**keywords)


def test_smoothed_depth_fit_eager_and_graphed():
    """eager steps of ``MeshDepthFitter(smoothing=16)`` on the hand equal the steps under ``GraphedStep`` (the rasterizer's gradient accumulators are
    double atomics whose order is not fixed: 1e-6 of the first energy, as the other graphed fits are held to); the values of another lambda
    copied into ``smoothing_system.vals`` reach the replayed step"""
    from deodr_amd import smoothing
    from deodr_amd.mesh_fitter import GraphedStep

    lam = 16.0
    eager = depth_fitter(smoothing=lam)
    assert eager._direct_iteration(1, False) is None and eager.smoothing_system.n == 526 and eager.smoothing_iterations == smoothing.DEFAULT_ITERATIONS
    assert smoothing.uses_kernel(eager.smoothing_system, eager.vertices)
    e_eager = [float(eager.step_device()[0]) for _ in range(10)]
    print("eager:", e_eager, "residual of the last solve:", eager.smoothing_residual.tolist())
    assert e_eager[-1] < e_eager[0] and eager.smoothing_residual.shape == (3,) and 0 < float(eager.smoothing_residual.max()) < 0.1
    plain = depth_fitter()
    e_plain = [float(plain.step_device()[0]) for _ in range(10)]
    assert plain.smoothing_system is None and e_plain[0] == pytest.approx(e_eager[0], rel=1e-6) and e_plain[1] != pytest.approx(e_eager[1], rel=1e-6)
    f = depth_fitter(smoothing=lam)
    graphed = GraphedStep(f, warmup=3)  # 3 + 1 eager steps and 1 on the capture stream: iterations 0 .. 4
    assert f.iter == 5 and ("attr", "smoothing_residual") in graphed.state
    e_graph = [float(graphed.step_device()[0]) for _ in range(5)]  # iterations 5 .. 9
    print("graphed:", e_graph)
    assert np.abs(np.array(e_graph) - np.array(e_eager[5:])).max() <= 1e-6 * e_eager[0]
    assert torch.allclose(f.vertices, eager.vertices, rtol=0, atol=1e-9)
    other = smoothing.laplacian_system(f.control_mesh.topology, 1.0, device="cpu").vals
    for fitter in (eager, f):
        fitter.smoothing_system.vals.copy_(other)  # in place: the graph holds the address
    e_after, g_after = float(eager.step_device()[0]), float(graphed.step_device()[0])
    e_next, g_next = float(eager.step_device()[0]), float(graphed.step_device()[0])
    assert abs(g_after - e_after) <= 1e-6 * e_eager[0] and abs(g_next - e_next) <= 1e-6 * e_eager[0]
    assert torch.allclose(f.vertices, eager.vertices, rtol=0, atol=1e-9)


def test_smoothed_multiview_fit_eager_and_graphed():
    from deodr_amd.mesh_fitter import GraphedStep, MeshRGBFitterWithPoseMultiFrame
    from test_pyramid_fit_host import hand_fitter

    make = lambda: hand_fitter(2, DEV, torch.float64, shift_pixels=(3, -2), smoothing=16.0, smoothing_iterations=8)
    eager = make()
    assert isinstance(eager, MeshRGBFitterWithPoseMultiFrame) and eager._direct_iteration(3, True) is None and eager.smoothing_iterations == 8
    e_eager = [float(eager.step_device()[0]) for _ in range(8)]
    f = make()
    graphed = GraphedStep(f, warmup=3)
    assert f.iter == 5
    e_graph = [float(graphed.step_device()[0]) for _ in range(3)]  # iterations 5 .. 7
    print("eager:", e_eager, "graphed:", e_graph)
    assert e_eager[-1] < e_eager[0] and np.abs(np.array(e_graph) - np.array(e_eager[5:])).max() <= 1e-6 * e_eager[0]
    assert torch.allclose(f.vertices, eager.vertices, rtol=0, atol=1e-9)
    # the kernels' steps are the torch recurrence's steps: the same eight steps with the kernels switched off
    from deodr_amd import smoothing

    uses_kernel, smoothing.uses_kernel = smoothing.uses_kernel, lambda system, b: False
    try:
        again = make()
        e_again = [float(again.step_device()[0]) for _ in range(8)]
    finally:
        smoothing.uses_kernel = uses_kernel
    assert np.abs(np.array(e_again) - np.array(e_eager)).max() <= 1e-6 * e_eager[0] and torch.allclose(again.vertices, eager.vertices, rtol=0, atol=1e-7)
