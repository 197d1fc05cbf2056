"""CPU checks of the as-rigid-as-possible energy: the NumPy restatement (tests/arap_reference.py: Horn's matrix + cyclic Jacobi, in long double) against
Kabsch / SVD rotations and against central finite differences of the SVD energy; the torch fallback (``deodr_amd.arap``) against the restatement,
through ``evaluate`` and autograd; the two exact cases of the contract; what the feature exists for -- a rigid motion costs nothing while the
Laplacian energy charges it in full, a bent strip costs less --; and the measurement the GPU tolerances derive from: a float64 run of the restatement
against the long-double run over the parity tables."""

import numpy as np
import pytest
import torch

import arap_reference as ar

SMALL = [("tetrahedron", ("noise30",)), ("icosphere42", ("noise30", "bend")), ("fan9", ("noise30", "mirror")), ("strip23", ("bend", "noise1"))]


def device_energy(name, weights="uniform", cregu=ar.CREGU):
    from deodr_amd.arap import ArapEnergyDevice

    q, faces, _ = ar.mesh(name)
    return ArapEnergyDevice(faces, q, cregu, weights, device="cpu")


def test_horn_and_jacobi_give_the_rotations_of_kabsch():
    worst = 0.0
    for name, hows in ar.parity_cases():
        c = ar.case(name, hows)
        R = ar.rotation_matrix(c["quaternions"]).astype(np.float64)
        assert np.abs(np.linalg.det(R) - 1).max() < 1e-14 and np.abs(R @ R.swapaxes(-1, -2) - np.eye(3)).max() < 1e-14  # proper rotations, also for mirrors
        gamma = np.where(np.isfinite(c["gamma"]), c["gamma"], 1.0)
        worst = max(worst, float((np.abs(R - ar.kabsch(c["S"])).max(axis=(-1, -2)) * gamma).max()))
    print(f"|R - R_svd| gamma <= {worst:.2e}")
    assert worst <= 1e-13  # (float64 SVD: a few rounding errors of S over gamma; measured 4.4e-15)


@pytest.mark.parametrize("name,hows", SMALL)
def test_energy_and_gradient_against_the_svd_energy(name, hows):
    """the energy with Kabsch rotations, and its central finite differences: the gradient is that of the energy (the envelope theorem)"""
    c = ar.case(name, hows)
    tables = (c["offsets"], c["cols"], c["weights"], c["q"])
    svd_energy = lambda p: ar.arap(*tables, p, c["cregu"], rotations=ar.kabsch(ar.cell_matrices(*tables, p, np.float64)))[0]
    assert np.abs(svd_energy(c["p"]) - c["energy"]).max() <= 1e-12 * c["e_scale"].max()
    h = 1e-5 * ar.edge_length(name)  # truncation ~ h^2 E''' ~ 1e-10 relative, rounding ~ 1e-19 / 1e-5: both far below the bound
    for pose in range(len(hows)):
        for v in range(0, len(c["q"]), max(1, len(c["q"]) // 7)):
            for axis in range(3):
                plus, minus = c["p"].astype(ar.LD), c["p"].astype(ar.LD)
                plus[pose, v, axis] += h
                minus[pose, v, axis] -= h
                fd = (svd_energy(plus)[pose] - svd_energy(minus)[pose]) / (2 * ar.LD(h))
                assert abs(fd - c["gradient"][pose, v, axis]) <= 1e-7 * c["g_scale"][pose], (pose, v, axis)


def test_torch_fallback_against_the_restatement_through_evaluate_and_autograd():
    worst = [0.0, 0.0, 0.0]
    for name, hows in ar.parity_cases():
        c = ar.case(name, hows)
        dev = device_energy(name)
        assert np.array_equal(dev.offsets.numpy().view(np.uint32), c["offsets"]) and np.array_equal(dev.cols.numpy().view(np.uint32), c["cols"])
        v = torch.tensor(c["p"], requires_grad=True)
        energy, gradient = dev.evaluate(v)
        assert energy.shape == (len(hows),) and energy.requires_grad and not gradient.requires_grad
        (energy * torch.arange(1, len(hows) + 1)).sum().backward()
        assert torch.equal(v.grad, gradient * torch.arange(1, len(hows) + 1)[:, None, None])
        worst = [max(a, b) for a, b in zip(worst, ar.errors(c, energy.detach().numpy(), gradient.numpy(), dev.rotations(v.detach()).numpy()))]
        single_e, single_g = dev.evaluate(v.detach()[0])  # [V,3] -> a scalar and [V,3]
        assert single_e.shape == () and torch.equal(single_g, gradient[0]) and dev.rotations(v.detach()[0]).shape == (len(c["q"]), 4)
    print("torch fallback: energy / e_scale %.2e, gradient / g_scale %.2e, quaternions %.2e" % tuple(worst))
    # the SVD's rotations carry a few rounding errors of S over gamma (>= 7e-3 in the tables): 1e-13; the energy is second order in them
    assert worst[0] <= 1e-14 and worst[1] <= 1e-13 and worst[2] <= 1e-12
    f32 = device_energy("icosphere42").evaluate(torch.tensor(ar.case("icosphere42", ("noise30",))["p"], dtype=torch.float32))
    assert f32[0].dtype == torch.float32 and bool(torch.isfinite(f32[1]).all())


def test_weights_uniform_cotangent_and_given():
    from deodr_amd.arap import cotangent_weights

    q, faces, (offsets, cols, _) = ar.mesh("icosphere42")
    rows = np.repeat(np.arange(len(q)), np.diff(offsets.astype(np.int64)))
    cot = device_energy("icosphere42", "cotangent")
    m = cotangent_weights(faces, q)
    assert abs(m - m.T).max() < 1e-15 and m.data.min() >= 0 and np.array_equal(cot.weights.numpy(), np.asarray(m[rows, cols.astype(np.int64)]).ravel())
    # a right isosceles triangle: the hypotenuse is opposite 90 degrees (cot = 0), the legs opposite 45 degrees (cot = 1); an obtuse angle clamps
    tri = cotangent_weights([[0, 1, 2]], [[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]).toarray()
    assert np.allclose(tri, [[0, 0.5, 0.5], [0.5, 0, 0], [0.5, 0, 0]], atol=1e-15)
    obtuse = cotangent_weights([[0, 1, 2]], [[0.0, 0, 0], [1, 0, 0], [-1, 0.1, 0]]).toarray()
    assert obtuse[1, 2] == 0 and obtuse.min() == 0 and obtuse[0, 1] > 0
    given = np.random.default_rng(5).uniform(0, 2, len(cols))
    given = 0.5 * (given + given[np.lexsort((rows, cols.astype(np.int64)))])  # symmetric: entry (i, j) averaged with entry (j, i)
    dev = device_energy("icosphere42", given)
    c = ar.case("icosphere42", ("noise30",))
    energy, gradient, quats = ar.arap(offsets, cols, given, q, c["p"], ar.CREGU)
    e, g = dev.evaluate(torch.tensor(c["p"]))
    assert abs(float(e[0]) - float(energy[0])) <= 1e-13 * c["e_scale"][0] * 2 and np.abs(g.numpy() - gradient).max() <= 1e-13 * c["g_scale"][0] * 2


def test_the_two_exact_cases():
    identity = np.array([0.0, 0, 0, 1])
    for name in ar.MESHES:
        dev = device_energy(name)
        for dtype in (ar.LD, np.float64):
            c = ar.case(name, ("rest", "coincident"))
            energy, gradient, quats = ar.arap(c["offsets"], c["cols"], c["weights"], c["q"], c["p"], c["cregu"], dtype)
            assert np.all(quats == identity) and energy[0] == 0 and np.all(gradient[0] == 0), name  # bit-equal to the rest: zeros exactly
            assert np.all(c["S"][1] == 0)  # coincident points: S = 0, R = identity; the energy is that of the rest edges
            assert len(c["cols"]) == 0 or energy[1] > 0
        e, g = dev.evaluate(torch.tensor(c["p"]))
        assert float(e[0]) == 0.0 and not bool(g[0].any()) and torch.equal(dev.rotations(torch.tensor(c["p"])), torch.tensor(identity).expand(2, len(c["q"]), 4))
        assert abs(float(e[1]) - float(c["energy"][1])) <= 1e-14 * float(c["e_scale"][1])
    # weights that are all zero: S = 0 everywhere
    q, faces, (offsets, cols, w) = ar.mesh("fan9")
    _, _, quats = ar.arap(offsets, cols, 0 * w, q, ar.deform("fan9", "noise30"), 1.0)
    assert np.all(quats == identity)


def laplacian_energy(name, p, cregu):
    from deodr_amd.scene3d import LaplacianRigidEnergyDevice, MeshTopology

    q, faces, _ = ar.mesh(name)
    return float(LaplacianRigidEnergyDevice(MeshTopology(faces, len(q), device="cpu"), q.copy(), cregu).evaluate(torch.tensor(p))[0])


@pytest.mark.parametrize("name", ["tetrahedron", "icosphere42", "icosphere162", "fan17", "strip23"])
def test_a_rigid_motion_costs_nothing_and_the_laplacian_energy_charges_it(name):
    c = ar.case(name, ("translation", "rigid170"))
    energy, gradient, _ = ar.arap(c["offsets"], c["cols"], c["weights"], c["q"], c["p"], c["cregu"], np.float64)
    assert np.all(energy <= ar.TOL_ENERGY * c["e_scale"]) and np.all(np.abs(gradient).max(axis=(1, 2)) <= ar.TOL_GRADIENT * c["g_scale"])
    lap = laplacian_energy(name, c["p"][1], c["cregu"])
    print(f"{name}: rigid 170 degrees: ARAP {float(energy[1]):.3e}, Laplacian {lap:.3e}, e_scale {float(c['e_scale'][1]):.3e}")
    # |L (R - I) q|^2: the Laplacian of the rest shape rotated by nearly a half turn -- of the order of e_scale wherever the rest shape is curved
    # at the scale of its edges (the closed meshes and the fan's hub); the strip is flat, only its two ends are charged
    assert lap >= (1e-2 if name != "strip23" else 1e-4) * c["e_scale"][1]


def test_a_bent_strip_costs_less_than_under_the_laplacian_energy():
    """Measured: E_arap / E_laplacian = 6.2e-2 on the strip of 23 vertices rolled onto a cylinder of radius 3; asserted: below 1"""
    c = ar.case("strip23", ("bend",))
    lap = laplacian_energy("strip23", c["p"][0], c["cregu"])
    ratio = float(c["energy"][0]) / lap
    print(f"bent strip: ARAP {float(c['energy'][0]):.4e}, Laplacian {lap:.4e}, ratio {ratio:.3e}")
    assert 0 < ratio < 1


def test_float64_error_of_the_restatement_is_what_the_gpu_tolerances_derive_from():
    worst = [0.0, 0.0, 0.0]
    for name, hows in ar.parity_cases():
        c = ar.case(name, hows)
        e, g, quats = ar.arap(c["offsets"], c["cols"], c["weights"], c["q"], c["p"], c["cregu"], np.float64)
        worst = [max(a, b) for a, b in zip(worst, ar.errors(c, e, g, quats))]
    print("float64 against long double: energy / e_scale %.2e, gradient / g_scale %.2e, quaternions %.2e" % tuple(worst))
    assert worst[0] <= ar.F64_ENERGY and worst[1] <= ar.F64_GRADIENT and worst[2] <= ar.F64_QUATERNION
    assert worst[0] >= ar.F64_ENERGY / 2 and worst[1] >= ar.F64_GRADIENT / 2 and worst[2] >= ar.F64_QUATERNION / 2  # the constants are the measurement
    assert (ar.TOL_ENERGY, ar.TOL_GRADIENT, ar.TOL_QUATERNION) == (8 * ar.F64_ENERGY, 8 * ar.F64_GRADIENT, 8 * ar.F64_QUATERNION)


def test_sweep_table():
    """the table DEODR_HIP_ARAP_SWEEPS is chosen from (tools/arap_times.py --table prints it): 5 is the first count below double's rounding"""
    S = np.concatenate([ar.case(name, hows)["S"].reshape(-1, 3, 3) for name, hows in ar.parity_cases()]).astype(ar.LD)
    off = {sweeps: float(ar.jacobi(ar.horn(S), sweeps)[2].max()) for sweeps in (4, 5, 6)}
    print(off)
    assert off[4] > 1e-16 > off[5] > off[6] and ar.SWEEPS == 5
