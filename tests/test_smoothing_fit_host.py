"""CPU checks of the ``smoothing=`` / ``smoothing_iterations=`` keywords of the pose fitters on the checker-backed rasterizer of tests/cpu_raster.py:
0 changes nothing, the first smoothed step is the plain first step with its vertex gradient replaced by ``spd_solve_torch`` of it, the depth fit and
the one-view and multi-view colour fits lower their energy with the keyword -- also with ``subdivisions=1`` and with ``skin=`` --, the refusals,
and values copied into ``smoothing_system.vals`` show in the next step.  64 x 64 frames, as in the other ``*_fit_host`` files."""

import numpy as np
import pytest
import torch

import skinning_reference as skr
from test_pyramid_fit_host import PARAMETERS, hand_fitter
from test_skinning_fit_host import SIZE, render_target, rig_fitter


def depth_fitter(**keywords):
    """the depth fit of the centred hand at 64 x 64 against its own depth image with the vertices grown by 5 %"""
    f, _, focal = rig_fitter(skin="omit", **keywords)
    f.set_image(np.ones((SIZE, SIZE)), focal=focal)
    f.vertices = f.vertices_init * 1.05
    f._leaves()
    with torch.no_grad():
        target = f.energy()[3].detach().cpu().numpy().copy()
    f.reset()
    f.set_image(target, focal=focal)
    return f


def skinned_fitter(**keywords):
    f, _, focal = rig_fitter(**keywords)
    render_target(f, focal, skr.hand_target_quaternions())
    return f


def captured_update(f):
    """one step of ``f`` -> (energy, the entries its momentum update received: name -> (gradient, second gradient))"""
    seen = {}
    update_all = f.momentum.update_all
    f.momentum.update_all = lambda entries: seen.update({e[0]: (e[2].clone(), None if e[3] is None else e[3].clone()) for e in entries}) or update_all(entries)
    energy = f.step()[0]
    f.momentum.update_all = update_all
    return energy, seen


MAKERS = {
    "depth": depth_fitter,
    "colour": lambda **kw: hand_fitter(1, "cpu", shift_pixels=(2, 1), **kw),
    "multi-view": lambda **kw: hand_fitter(2, "cpu", shift_pixels=(2, 1), **kw),
}


def test_zero_and_no_keyword_are_the_same_fit(oracle_api):
    import cpu_raster

    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        for name, make in MAKERS.items():
            plain, zero = make(), make(smoothing=0.0, smoothing_iterations=7)
            assert zero.smoothing_system is None and plain.smoothing_system is None and zero.smoothing == 0.0 and zero.smoothing_residual is None
            assert [plain.step()[0] for _ in range(4)] == [zero.step()[0] for _ in range(4)], name
            compared = [k for k in PARAMETERS if torch.is_tensor(getattr(plain, k, None))]
            assert len(compared) >= 3 and all(torch.equal(getattr(plain, k), getattr(zero, k)) for k in compared)
            assert set(plain.momentum.speed) == set(zero.momentum.speed)


@pytest.mark.parametrize("name", list(MAKERS))
def test_first_step_is_the_plain_one_with_the_solve_of_its_vertex_gradient(oracle_api, name):
    import cpu_raster
    from deodr_amd import smoothing

    lam, m = 16.0, 12
    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        plain, f = MAKERS[name](), MAKERS[name](smoothing=lam, smoothing_iterations=m)
        assert f.smoothing_system.n == f.vertices.shape[0] and f.smoothing_iterations == m and f.smoothing == lam
        e_plain, got_plain = captured_update(plain)
        e, got = captured_update(f)
    assert e == e_plain  # the energy of the first step is taken before the update
    g, g_rigid = got_plain["vertices"]
    u, none = got["vertices"]
    assert none is None and g_rigid is not None
    expected, residual = smoothing.spd_solve_torch(f.smoothing_system, g + g_rigid, m)
    assert torch.allclose(u, expected, rtol=0, atol=1e-13 * float(expected.abs().max())) and float(u.abs().max()) > 0
    assert torch.allclose(f.smoothing_residual, residual, rtol=1e-9, atol=0) and f.smoothing_residual.shape == (3,)
    assert float((u * (g + g_rigid)).sum()) > 0  # a descent direction
    assert float(u.mean(dim=0).abs().max()) <= 1e-12 * float(u.abs().max())  # the data gradient is zero-mean, the rigid gradient is, and so is u
    for other in set(got) - {"vertices"}:  # poses, light, colour: untouched
        assert torch.equal(got[other][0], got_plain[other][0]), other
    # the rule acts on u: speed = (1 - damping) (1 - inertia) clamp(-factor u)
    step_max = 1.0 if name == "depth" else 0.5
    speed = (1 - f.damping) * (1 - f.inertia) * (-f.step_factor_vertices * u).clamp(-step_max, step_max)
    assert torch.allclose(f.momentum.speed["vertices"], speed, rtol=1e-12, atol=0)


def test_fits_lower_their_energy_with_the_keyword(oracle_api):
    """also through a subdivided cage (the cage's Laplacian, the cage gradient) and with a skin (the rest vertices' gradient).  The energies are
    printed for DESIGN.md 4k: the plain fit at its shipped step factor and the smoothed fit at the factors tried."""
    import cpu_raster

    makers = dict(MAKERS, **{"colour, subdivisions=1": lambda **kw: hand_fitter(1, "cpu", shift_pixels=(2, 1), subdivisions=1, **kw),
                             "depth, skin": skinned_fitter})  # fmt: skip
    N = 25
    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        for name, make in makers.items():
            row = {}
            for label, keywords, factor in (("plain", {}, 1), ("smoothing=16", dict(smoothing=16.0), 1), ("smoothing=16, factor x 10", dict(smoothing=16.0), 10)):
                f = make(**keywords)
                f.step_factor_vertices = f.step_factor_vertices * factor
                if keywords:
                    assert f._direct_iteration(3, True) is None
                    assert f.smoothing_system.n == f.control_mesh.nb_vertices == f.vertices.shape[0]
                energies = [f.step()[0] for _ in range(N)]
                row[label] = (energies[0], energies[-1])
                if keywords and factor == 1:
                    assert energies[-1] < energies[0], (name, energies)
                    assert bool(torch.isfinite(f.vertices).all()) and 0 <= float(f.smoothing_residual.max()) < 1
            print(f"{name}: energy after {N} iterations " + "; ".join(f"{k}: {a:.4f} -> {b:.4f}" for k, (a, b) in row.items()))


def test_refusals():
    import os

    from conftest import GOLDEN
    from deodr_amd import scenes
    from deodr_amd.mesh_fitter import MeshDepthFitter, MeshRGBFitterWithPose, MeshRGBFitterWithPoseMultiFrame

    d = np.load(os.path.join(GOLDEN, "rgb_hand_fit.npz"))
    vertices, faces = d["vertices_centered"], scenes.load_hand_mesh(os.path.join(GOLDEN, "hand_mesh.npz"))[1]
    colour = (d["default_color"], d["default_light_directional"], float(d["default_light_ambient"]))
    makers = [lambda **kw: MeshDepthFitter(vertices, faces, np.zeros(3), d["translation_init"], device="cpu", **kw),
              lambda **kw: MeshRGBFitterWithPose(vertices, faces, np.zeros(3), d["translation_init"], *colour, device="cpu", **kw),
              lambda **kw: MeshRGBFitterWithPoseMultiFrame(vertices, faces, np.zeros((2, 3)), np.tile(d["translation_init"], (2, 1)), *colour, device="cpu", **kw)]  # fmt: skip
    basis = np.random.RandomState(0).randn(2, *vertices.shape)
    for make in makers:
        for bad in (-0.5, float("nan"), float("inf"), "4", None, True):
            with pytest.raises(ValueError, match="smoothing must be a finite real number >= 0"):
                make(smoothing=bad)
        for bad in (0, -3, 2.5, "8", True):
            with pytest.raises(ValueError, match="smoothing_iterations must be an integer >= 1"):
                make(smoothing=4.0, smoothing_iterations=bad)
        with pytest.raises(ValueError, match="smoothing with shape_basis is not supported: the parameter is the coefficient vector"):
            make(smoothing=4.0, shape_basis=basis)
        assert make(smoothing=0.0, shape_basis=basis).smoothing_system is None  # 0 is off
        f = make(smoothing=np.float32(2.5), smoothing_iterations=np.int64(5))
        assert f.smoothing == 2.5 and f.smoothing_iterations == 5 and f.smoothing_system.vals.dtype == torch.float64


def test_values_copied_into_the_system_show_in_the_next_step(oracle_api):
    """the solve of the step after the copy is ``spd_solve_torch`` of the gradient that step handed over under the NEW values -- not under the old
    ones, not under a mix"""
    import cpu_raster
    from deodr_amd import smoothing

    handed = []
    spd_solve = smoothing.spd_solve

    def recording(system, b, *args, **kwargs):
        handed.append((system, b.clone()))
        return spd_solve(system, b, *args, **kwargs)

    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        f = depth_fitter(smoothing=16.0)
        vals = f.smoothing_system.vals
        old = vals.clone()
        f.step()
        new = smoothing.laplacian_system(f.control_mesh.topology, 1.0).vals
        f.smoothing_system.vals.copy_(new)
        assert f.smoothing_system.vals is vals and not torch.equal(old, new)
        smoothing.spd_solve = recording
        try:
            _, got = captured_update(f)
        finally:
            smoothing.spd_solve = spd_solve
    (system, g), = handed
    assert system is f.smoothing_system and float(g.abs().max()) > 0
    u = got["vertices"][0]
    lam1, lam16 = (smoothing.laplacian_system(f.control_mesh.topology, lam) for lam in (1.0, 16.0))
    assert torch.equal(lam1.cols, system.cols) and torch.equal(lam1.vals, system.vals) and torch.equal(lam16.vals, old)
    expected, stale = (smoothing.spd_solve_torch(s, g, f.smoothing_iterations)[0] for s in (lam1, lam16))
    assert torch.allclose(u, expected, rtol=0, atol=1e-13 * float(expected.abs().max()))
    assert float((u - stale).abs().max()) > 0.1 * float(expected.abs().max())  # far from what the old values give
    print(f"|u| at lambda = 1 over |u| at lambda = 16: {float(u.norm() / stale.norm()):.3f}")
