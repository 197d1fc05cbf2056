"""CPU checks of deodr_amd/smoothing.py: the torch recurrence (``spd_solve_torch``) against the long-double restatement of tests/smoothing_reference.py
over the parity cases -- and the measurement the GPU tolerance derives from --, convergence through the true residual, the properties the header
states (zero mean kept, a descent direction at every truncation, a zero column, a run past n steps, ``rel_tol``), the systems and their host checks,
and the autograd op."""

import numpy as np
import pytest
import torch

import smoothing_reference as sr

LD = sr.LD


def system_of(case):
    from deodr_amd.smoothing import SpdSystem

    return SpdSystem(case["offsets"], case["cols"], case["vals"], device="cpu")


def measured_errors(name):
    """the float64 torch recurrence against the restatement -> (case, ref, x, residual, errors relative to max |x| and to the residual's value)"""
    from deodr_amd.smoothing import spd_solve_torch

    case, ref = sr.reference(name)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # (how torch splits its sums over its threads moves the figure: one thread, so that it is the same everywhere)
    try:
        x, residual = spd_solve_torch(system_of(case), torch.as_tensor(case["b"]), case["iterations"])
    finally:
        torch.set_num_threads(threads)
    x, residual = x.numpy(), residual.numpy()
    errors = dict(x=float(np.abs(x.astype(LD) - ref["x"]).max() / ref["scale"]))
    live = ref["residual"] > sr.RESIDUAL_FLOOR
    if live.any():
        errors["residual"] = float((np.abs(residual.astype(LD) - ref["residual"])[live] / ref["residual"][live]).max())
    return case, ref, x, residual, errors


@pytest.mark.parametrize("name", sr.parity_cases())
def test_torch_recurrence_against_long_double(name):
    case, ref, x, residual, errors = measured_errors(name)
    measured = sr.MEASURED[case["iterations"]]
    print(f"{name}: " + "  ".join(f"{k} {e:.2e}" for k, e in errors.items()) + f"  (MEASURED {measured:.2e})")
    assert all(e <= measured for e in errors.values()), errors
    assert x.shape == case["b"].shape and residual.shape == (case["D"],) and np.all(np.isfinite(x))
    if case["zero_column"] is not None:  # a zero column of b: a zero column of x, residual 0, and never a NaN
        assert np.all(x[:, case["zero_column"]] == 0) and residual[case["zero_column"]] == 0
        assert np.all(ref["x"][:, case["zero_column"]] == 0) and ref["frozen_at"][case["zero_column"]] == 0


def test_measure_the_tolerance():
    """the figure MEASURED of tests/smoothing_reference.py, from which the GPU tests take TOLERANCE = 8 MEASURED"""
    worst = {m: (0.0, None) for m in sr.MEASURED}
    for name in sr.parity_cases():
        m = sr.CASES[name]["iterations"]
        for k, e in measured_errors(name)[4].items():
            if e > worst[m][0]:
                worst[m] = (e, (name, k))
    for m, (e, where) in worst.items():
        print(f"m = {m}: largest float64 error relative to the scale {e:.3e} at {where}; MEASURED = {sr.MEASURED[m]:.3e}, TOLERANCE = {sr.TOLERANCE[m]:.3e}")
    for m, (e, _) in worst.items():
        assert e <= sr.TOLERANCE[m] / 8 and sr.MEASURED[m] <= 1.1 * e  # the figures in the file are the measured ones, rounded up by a few per cent
        assert sr.TOLERANCE[m] == 8 * sr.MEASURED[m]


def test_float64_and_long_double_drift_apart_with_the_step_count():
    """why parity stops at 16 steps: the error of the float64 recurrence against the long-double one on the sphere at lambda = 16 (printed)"""
    from deodr_amd.smoothing import spd_solve_torch

    case, _ = sr.reference("sphere 322 lam=16 D=3 m=16")
    system, b = system_of(case), torch.as_tensor(case["b"])
    errors = {}
    for m in (16, 32, 64):
        ref = sr.restate(case["offsets"], case["cols"], case["vals"], case["b"], m)
        errors[m] = float(np.abs(spd_solve_torch(system, b, m)[0].numpy().astype(LD) - ref["x"]).max() / np.abs(ref["x"]).max())
    print("float64 against long double, relative to max |x|: " + ", ".join(f"m = {m}: {e:.1e}" for m, e in errors.items()))
    assert errors[16] <= sr.MEASURED[16]


def test_convergence_through_the_true_residual():
    """lambda = 4, m = 64 on the sphere: |b - A x| / |b| recomputed in long double from the returned x; and, because the smallest eigenvalue of
    I + lambda L is 1, |x - x*| <= |b - A x|: the distance to SciPy's direct solve is held to that same bound"""
    import scipy.sparse as sp
    import scipy.sparse.linalg

    from deodr_amd.smoothing import spd_solve_torch

    case, ref = sr.reference("sphere 322 lam=4 D=3 m=64 convergence")
    system = system_of(case)
    x, residual = spd_solve_torch(system, torch.as_tensor(case["b"]), 64)
    true = sr.true_residual(case["offsets"], case["cols"], case["vals"], case["b"], x.numpy())
    own = sr.true_residual(case["offsets"], case["cols"], case["vals"], case["b"], ref["x"])
    print(f"|b - A x| / |b| per column: torch {[f'{float(v):.2e}' for v in true]}, the restatement's own {[f'{float(v):.2e}' for v in own]}; "
          f"the recurrence's squared relative residual {[f'{float(v):.2e}' for v in residual]}")  # fmt: skip
    assert np.all(true <= sr.CONVERGENCE) and np.all(own <= sr.CONVERGENCE / 10)  # a margin of more than 10 on this mesh
    A = sp.csr_matrix((case["vals"], case["cols"], case["offsets"]), shape=(case["n"],) * 2)
    exact = scipy.sparse.linalg.spsolve(A.tocsc(), case["b"])
    b_norm = np.sqrt((case["b"] ** 2).sum(axis=0))
    distance = np.sqrt(((x.numpy() - exact) ** 2).sum(axis=0))
    assert np.all(distance <= sr.CONVERGENCE * b_norm)
    assert abs(np.linalg.eigvalsh(A.toarray())[0] - 1) < 1e-9  # the rows sum to 1: the constant vector is the eigenvector of eigenvalue 1


def test_zero_mean_in_zero_mean_out_and_a_descent_direction_at_every_truncation():
    from deodr_amd.smoothing import spd_solve_torch

    case, _ = sr.reference("sphere 322 lam=16 D=3 m=16")
    system, b = system_of(case), torch.as_tensor(case["b"])
    assert float(b.mean(dim=0).abs().max()) < 1e-15
    for m in (1, 2, 8, 16, 64):
        x, _ = spd_solve_torch(system, b, m)
        assert float(x.mean(dim=0).abs().max()) <= 1e-15 * float(x.abs().max()) * 16
        assert bool(((b * x).sum(dim=0) > 0).all())
        assert torch.allclose((b * x).sum(dim=0), (x * system.matvec(x)).sum(dim=0), rtol=1e-9)  # g^T x_m = x_m^T A x_m


def test_a_run_past_n_steps_is_frozen_without_a_nan():
    from deodr_amd.smoothing import spd_solve_torch

    case, ref = sr.reference("tiny n=3 D=4 m=50 past n")
    system, b = system_of(case), torch.as_tensor(case["b"])
    x, residual = spd_solve_torch(system, b, 50)
    exact = np.linalg.solve(system.to_scipy().toarray(), case["b"])
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(residual).all())
    assert np.abs(x.numpy() - exact).max() <= 1e-14 * np.abs(exact).max() and np.abs(ref["x"].astype(np.float64) - exact).max() <= 1e-14 * np.abs(exact).max()
    assert torch.allclose(x, spd_solve_torch(system, b, 500)[0], rtol=0, atol=1e-15 * float(x.abs().max()))  # x stays where it froze
    assert float(residual.max()) < 1e-28


def test_rel_tol_freezes_a_column_at_the_step_the_restatement_does():
    from deodr_amd.smoothing import spd_solve_torch

    case, _ = sr.reference("sphere 322 lam=4 D=4 m=8 zero column")
    system, b = system_of(case), torch.as_tensor(case["b"])
    for rel_tol in (1e-1, 3e-2, 1e-2):  # (frozen within 14 steps, where float64 and long double still agree to 1e-10: later the step itself may differ)
        ref = sr.restate(case["offsets"], case["cols"], case["vals"], case["b"], 40, rel_tol)
        frozen = ref["frozen_at"]
        assert frozen[2] == 0 and all(0 < frozen[d] < 40 for d in (0, 1, 3)), frozen
        x, residual = spd_solve_torch(system, b, 40, rel_tol)
        for d in (0, 1, 3):  # the column equals the run truncated at its own step, and its residual is below the tolerance
            truncated = spd_solve_torch(system, b, int(frozen[d]))[0]
            assert torch.equal(x[:, d], truncated[:, d]), (rel_tol, d)
            assert float(residual[d]) <= rel_tol**2 and float(ref["residual"][d]) <= rel_tol**2
            assert float(spd_solve_torch(system, b, int(frozen[d]) - 1)[1][d]) > rel_tol**2  # not a step earlier


def test_laplacian_system_is_the_graph_laplacian_of_the_topology():
    from deodr_amd import smoothing
    from deodr_amd.scene3d import MeshTopology

    vertices, faces = sr.sphere()
    lam = 3.5
    topo = MeshTopology(faces, len(vertices), device="cpu")
    system = smoothing.laplacian_system(topo, lam)
    assert system.n == 322 and system.vals.device.type == "cpu" and system.vals.dtype == torch.float64 and system.offsets.dtype == torch.int32
    A = system.to_scipy().toarray()
    # L^T L is what the topology keeps (the rigid energy): the same L
    L = (A - np.eye(322)) / lam
    m = np.zeros((322, 322))
    np.add.at(m, (topo._m_rows.numpy(), topo._m_cols.numpy()), topo._m_vals.numpy())
    assert np.abs(L.T @ L - m).max() < 1e-12
    assert np.abs(A.sum(axis=1) - 1).max() < 1e-13 and np.abs(A - A.T).max() == 0
    assert sorted(set(sr.row_lengths(system.offsets.numpy()))) == [6, 7, 17]  # the rings next to the poles, regular vertices, the two poles
    offsets, cols, vals = sr.mesh_system(faces, 322, lam)
    by_edges = sr.csr_of_edges(322, np.concatenate((faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]])), lam)
    assert np.array_equal(offsets, by_edges[0]) and np.array_equal(cols, by_edges[1]) and np.allclose(vals, by_edges[2], rtol=0, atol=1e-15)
    same = smoothing.laplacian_system(faces, lam, 322, device="cpu")
    assert torch.equal(same.vals, system.vals) and torch.equal(same.cols, system.cols)
    zero = smoothing.laplacian_system(faces, 0.0, 322, device="cpu")  # lambda = 0: the identity, in the same pattern
    assert torch.equal(zero.cols, system.cols) and float(zero.vals.sum()) == 322
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lam must be a finite real number >= 0"):
            smoothing.laplacian_system(faces, bad, 322, device="cpu")
    assert sorted(set(sr.row_lengths(sr.strip_system(200, 1.0)[0]))) == [3, 4, 5, 6, 7, 8, 9, 17]  # the rows the lane groups are tested on


def test_spd_system_checks_its_tables_on_the_host():
    from deodr_amd.smoothing import SpdSystem

    offsets, cols, vals = sr.tiny_system(3)
    SpdSystem(offsets, cols, vals, device="cpu")
    with pytest.raises(ValueError, match="not a non-decreasing sequence from 0 to nnz"):
        SpdSystem([0, 2, 1, 7], cols, vals, device="cpu")
    with pytest.raises(ValueError, match="not a non-decreasing sequence from 0 to nnz"):
        SpdSystem([0, 2, 5, 6], cols, vals, device="cpu")
    with pytest.raises(ValueError, match="a column index is out of range"):
        SpdSystem(offsets, np.where(cols == 2, 3, cols), vals, device="cpu")
    lopsided = vals.copy()
    lopsided[1] = -0.75  # (0, 1) without (1, 0)
    with pytest.raises(ValueError, match="not symmetric"):
        SpdSystem(offsets, cols, lopsided, device="cpu")
    with pytest.raises(ValueError, match="the diagonal must be positive"):
        SpdSystem(offsets, cols, np.where(vals == 2.0, -2.0, vals), device="cpu")
    with pytest.raises(ValueError, match="vals must be finite"):
        SpdSystem(offsets, cols, np.where(vals == 2.0, np.nan, vals), device="cpu")
    with pytest.raises(ValueError, match="must be one-dimensional"):
        SpdSystem(offsets, cols, vals[:-1], device="cpu")


def test_autograd_op_is_the_same_solve_of_the_incoming_gradient():
    from deodr_amd import smoothing

    case, _ = sr.reference("sphere 322 lam=4 D=3 m=64 convergence")
    system = system_of(case)
    b = torch.as_tensor(case["b"]).requires_grad_(True)
    x, residual = smoothing.spd_solve(system, b, iterations=64)
    assert x.requires_grad and not residual.requires_grad
    w = torch.as_tensor(np.random.RandomState(3).randn(*case["b"].shape))
    (g,) = torch.autograd.grad((w * x).sum(), b)
    assert torch.equal(g, smoothing.spd_solve_torch(system, w, 64)[0])
    # converged: the gradient of w^T A^-1 b in b is A^-1 w
    exact = np.linalg.solve(system.to_scipy().toarray(), w.numpy())
    assert np.abs(g.numpy() - exact).max() <= 1e-8 * np.abs(exact).max()
    assert not smoothing.spd_solve(system, b.detach(), iterations=4)[0].requires_grad
    assert smoothing.DEFAULT_ITERATIONS >= 1 and torch.equal(smoothing.spd_solve(system, b.detach())[0], smoothing.spd_solve_torch(system, b.detach(), smoothing.DEFAULT_ITERATIONS)[0])
    with pytest.raises(ValueError, match=r"b must have shape \[322, D\]"):
        smoothing.spd_solve(system, torch.zeros(5, 3, dtype=torch.float64))
