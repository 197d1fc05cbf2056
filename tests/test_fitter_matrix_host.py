"""The keyword combinations of the three pose fitters on CPU tensors, with the checker in the rasterizer's place (tests/fitter_matrix_cases.py has the
table, the driver and the restatement): what makes that path the reference the GPU suite (tests/test_fitter_matrix_gpu.py) compares the kernels with.

* every case runs three steps, hands ``momentum.update_all`` every group its keywords imply with a finite non-zero gradient, every prior it switches on
  with a non-zero second gradient, and the three energies differ;
* the posed vertices the fitter hands to the scene equal the restatement of ``S (skin(mean + c . B, q) - mean of the rest vertices)`` and the pose in
  long double, and the data gradients of ``update_all`` equal the restated adjoint of the adjoint a tensor hook reads off those posed vertices -- both
  within ``COMPOSITION_BOUND`` = skinning_reference.TOLERANCE + MEASURED_CHAIN (5.76e-14) of every element's scale, the sum of the absolute values of
  its terms.  Measured on this code, over all cases and steps: posed 5.0e-16, vertices 7.0e-16, coefficients 5.2e-17, quaternion 4.3e-16,
  translation 2.1e-16, joint quaternions 3.2e-16 of the scale (the output of ``pytest -s``).  The scale of a coefficient gradient is dominated by
  the rigid gradient's (cregu = 1000 times the Laplacian's row sums): that check sees a missing rigid term or a wrong contraction, the vertex and
  joint checks of the cases without a basis see the data terms at full resolution;
* a skin at identity and a basis at zero change nothing next to the same fitter without the keyword;
* the refused combinations raise their messages."""

import numpy as np
import pytest

import fitter_matrix_cases as fm
import fititer_reference as fr
from fitter_matrix_cases import CASES, COMPOSITION_BOUND, LD

needs_reference = pytest.mark.skipif(not fr.longdouble_is_extended(), reason="np.longdouble is not wider than float64 here: no reference")


_recordings = {}


def recording(name, oracle_api):
    """(the CPU fitter, its three recorded steps): made once per case, read by every test, left unchanged"""
    if name not in _recordings:
        _recordings[name] = fm.reference_recording(CASES[name], oracle_api)
    return _recordings[name]


@pytest.mark.parametrize("name", list(CASES))
def test_every_group_has_a_gradient_and_every_prior_a_second_one(name, oracle_api):
    case = CASES[name]
    f, rows = recording(name, oracle_api)
    assert f.iter == fm.STEPS and f.camera.height == f.camera.width == fm.SIZE and f.camera.n_views == case.views <= 3
    for row in rows:
        assert set(row["entries"]) == set(case.groups), (set(row["entries"]), set(case.groups))
        for group, (gradient, second) in row["entries"].items():
            assert np.all(np.isfinite(gradient)) and np.abs(gradient).max() > 0, group
            assert (second is not None) == case.groups[group], group
            if second is not None:
                assert second.shape == gradient.shape and np.all(np.isfinite(second)) and np.abs(second).max() > 0, group
        assert np.isfinite(row["energy"]) and row["energy"] > 0 and row["posed"].shape == (case.views, f.mesh.nb_vertices, 3)
        assert np.abs(row["posed_b"]).max() > 0 and row["image"].std() > 0
    energies = [row["energy"] for row in rows]
    assert len(set(energies)) == fm.STEPS, energies
    for a, b in zip(rows, rows[1:]):  # every parameter moved, every speed exists
        assert set(b["speed"]) == set(case.groups)
        for group in case.groups:
            attribute = fm.ATTRIBUTE_OF.get(group, group)
            assert np.abs(a["params"][attribute] - b["params"][attribute]).max() > 0, group


def composition_errors(name, outputs, oracle_api):
    """-> {output: largest error relative to the scale} over the three steps of the case"""
    f, rows = recording(name, oracle_api)
    worst = {}
    for row in rows:
        ref = fm.restate(f, row["params"], row["posed_b"], LD)
        for k in outputs(ref):
            got = row["posed"] if k == "posed" else row["entries"][k][0]
            worst[k] = max(worst.get(k, 0.0), fm.relative_to_scale(got, ref[k]))
    return worst


@needs_reference
@pytest.mark.parametrize("name", list(CASES))
def test_the_posed_vertices_are_the_restated_composition(name, oracle_api):
    worst = composition_errors(name, lambda ref: ["posed"], oracle_api)
    print(f"{name}: posed vertices {worst['posed']:.2e} of the scale (bound {COMPOSITION_BOUND:.2e})")
    assert worst["posed"] <= COMPOSITION_BOUND


@needs_reference
@pytest.mark.parametrize("name", list(CASES))
def test_the_data_gradients_are_the_restated_adjoint(name, oracle_api):
    """the gradients of ``update_all`` -- vertices or coefficients (the latter with the rigid gradient, as the basis adjoint is fed), view quaternions,
    translations, joint quaternions -- against the pull-back of dE_data / dposed through the restated adjoint: the pose adjoint summed over the views,
    S^T, the skin's adjoint, the projection on zero-mean displacements, the contraction with the basis"""
    case = CASES[name]
    worst = composition_errors(name, lambda ref: [k for k in ref if k != "posed"], oracle_api)
    print(f"{name}: " + "  ".join(f"{k} {e:.2e}" for k, e in worst.items()) + f" of the scale (bound {COMPOSITION_BOUND:.2e})")
    assert set(worst) == {k for k in case.groups if k in ("vertices", "coefficients", "quaternion", "translation", "joint_quaternions")}
    for k, e in worst.items():
        assert e <= COMPOSITION_BOUND, (k, e)


@needs_reference
def test_the_measured_figure_of_the_restatement_is_the_recorded_one(oracle_api):
    """float64 against long double, over the first step of every case: what MEASURED_CHAIN records (fitter_matrix_cases.py prints the table)"""
    worst = 0.0
    for name in CASES:
        f, rows = recording(name, oracle_api)
        f64, ld = (fm.restate(f, rows[0]["params"], rows[0]["posed_b"], dtype) for dtype in (np.float64, LD))
        worst = max([worst] + [fm.relative_to_scale(f64[k][0], ld[k]) for k in ld])
    print(f"largest float64 error of the restatement relative to the scale: {worst:.3e} (recorded: {fm.MEASURED_CHAIN:.1e})")
    assert 0 < worst <= fm.MEASURED_CHAIN


@pytest.mark.parametrize("name", ["multi-skin-sh3-albedo", "multi-basis3+skin-directional"])
def test_every_shared_gradient_goes_through_the_reduction(name, oracle_api):
    """One process cannot see a gradient that is left out of the list ``_reduce_shared`` sums over the ranks: the sum of one is itself.  Here the hook
    stands in for the all-reduce of two ranks that hold the same views -- it doubles what it is handed.  Every gradient of a parameter the views share
    (vertices, joint quaternions, lights, colour) must then arrive in ``update_all`` doubled, bit for bit (a factor of two is exact), the poses of the
    views unchanged, and the energy larger by the data term."""
    case = CASES[name]
    _f, rows = recording(name, oracle_api)
    with fm.reference_raster(oracle_api):
        f = fm.build(case, "cpu")
        f._reduce_shared = lambda grads: [2 * g for g in grads]
        doubled = fm.step_recorded(f)
    once = rows[0]
    assert all(np.array_equal(doubled["params"][k], once["params"][k]) for k in once["params"])  # the same start
    for group in case.groups:
        g2, g1 = doubled["entries"][group][0], once["entries"][group][0]
        if group in ("quaternion", "translation"):
            assert np.array_equal(g2, g1), group
        elif group == "coefficients":  # B . (2 g_data + g_rigid): not a multiple of the other
            assert np.abs(g2 - g1).max() > 0
        else:
            assert np.array_equal(g2, 2 * g1), group
    assert doubled["energy"] > once["energy"]


# ---- neutral values change nothing ------------------------------------------------------------------------------------------------------------

NEUTRAL = [fm.Case(f, s, light) for s in ("skin", "basis3") for f, light in (("depth", None), ("rgb", "directional"), ("multi", "sh3-albedo"))]


RASTER_CONDITION = 3 * fm.SIZE**2  # (test_neutral_values_change_nothing derives it)


def largest(a):
    return float(np.abs(a).max())


@pytest.mark.parametrize("case", NEUTRAL, ids=[c.name for c in NEUTRAL])
def test_neutral_values_change_nothing(case, oracle_api):
    """a skin at identity joint quaternions / a basis at c = 0 next to the same fitter without the keyword, one step at the reference shape: the same
    image and data energy, the same pose gradients; with the skin the same vertex gradient, with the basis ``g_coefficients = B . g_vertices``.  The
    plain fitters are pinned to the reference's golden curves elsewhere (tests/test_scene3d.py).

    Bounds.  What enters the rasterizer -- the posed vertices -- is held to COMPOSITION_BOUND of the largest entry: the skin at identity rounds
    (``sum_k w_k ((v - c_j) + t_j)`` is v within an ulp of |c_j|), and the plain fitter centres its vertices once more than the one with a basis.  What
    leaves the rasterizer cannot be held to it: an ulp in a posed vertex comes back as 1e-13 .. 1e-12 of a gradient.  Those outputs are held to the bound
    times RASTER_CONDITION = 3 SIZE^2 -- a CEILING, not a derivation.  The sketch behind it: a relative change e of a posed vertex moves its image
    coordinates ``focal x / z + centre`` by at most e (focal + SIZE) <= 3 SIZE e pixels (focal <= 2 SIZE); a pixel's colour changes by O(1) per pixel of
    movement of an edge (sigma = 1), and a gradient entry sums such pixels along edges that cross at most SIZE of them.  5.76e-14 * 12288 = 7.1e-10
    of the largest entry, about 600 times the worst figure measured (gradients 2e-15 .. 1.2e-12, printed by ``pytest -s``).  It is not tied to that
    measurement, because the figure comes from the code under test; what the ceiling separates is rounding from a term left out or a factor, which
    is of the order of the entry itself -- nine orders of magnitude above it."""
    with fm.reference_raster(oracle_api):
        plain, keyword = fm.build(case, "cpu", neutral="plain"), fm.build(case, "cpu", neutral="keyword")
        a, b = fm.step_recorded(plain), fm.step_recorded(keyword)
    posed_moved = largest(a["posed"] - b["posed"]) / largest(a["posed"])
    bound = COMPOSITION_BOUND * RASTER_CONDITION
    print(f"{case.name}: posed vertices differ by {posed_moved:.2e} of the largest (bound {COMPOSITION_BOUND:.2e}); images by "
          f"{largest(a['image'] - b['image']):.2e}, energies by {abs(a['energy'] - b['energy']) / a['energy']:.2e} (bound {bound:.2e})")  # fmt: skip
    assert posed_moved <= COMPOSITION_BOUND
    assert largest(a["image"] - b["image"]) <= bound * largest(a["image"]) and abs(a["energy"] - b["energy"]) <= bound * a["energy"]
    for group in ("quaternion", "translation") + (("vertices",) if case.shape == "skin" else ()):
        err = largest(a["entries"][group][0] - b["entries"][group][0]) / largest(a["entries"][group][0])
        print(f"  {group}: {err:.2e}")
        assert err <= bound, group
    if case.shape == "skin":
        assert largest(b["entries"]["joint_quaternions"][0]) > 0 and b["entries"]["joint_quaternions"][1] is None  # (joint_regu = 0: no prior)
    else:
        B = keyword.shape_basis.components.numpy().reshape(3, -1).astype(LD)
        g = (a["entries"]["vertices"][0] + a["entries"]["vertices"][1]).reshape(-1).astype(LD)
        expected, scale = B @ g, np.abs(B) @ np.abs(g)
        err = float((np.abs(b["entries"]["coefficients"][0] - expected) / scale).max())
        print(f"  coefficients against B . g_vertices: {err:.2e} of sum |term|")
        assert largest(expected) > 0 and err <= bound


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("fitter,shape,extra,message", fm.REFUSED, ids=[f"{f}-{s}{'-albedo' if e else ''}" for f, s, e, _m in fm.REFUSED])
def test_refused_combinations(fitter, shape, extra, message):
    with pytest.raises(ValueError, match=message):
        if fitter == "depth":
            from test_skinning_fit_host import rig_fitter

            rig_fitter(device="cpu", measured_from="far", **fm.shape_keywords(shape, "cpu", with_rig=False))
        else:
            from test_lighting_gpu import make_fitter

            make_fitter(3 if fitter == "multi" else 1, True, device="cpu", **fm.shape_keywords(shape, "cpu"), **extra)
