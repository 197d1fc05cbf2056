"""CPU checks of the multi-scale L2 data term: the NumPy restatement of tests/pyramid_reference.py against central differences in long double, the
torch formulas of deodr_amd/pyramid.py (value and autograd gradient) against the restatement, the properties the definition promises, and the
measurement the tolerance of the GPU tests is derived from."""

import numpy as np
import pytest
import torch

import pyramid_reference as pr

LD = pr.LD


def every_case():
    return [(name, variant, dtype) for name in sorted(pr.CASES) for variant in pr.VARIANTS for dtype in pr.DTYPES]


def test_restatement_against_central_differences_in_long_double():
    """d loss / d image, element by element: the loss is quadratic in the image, so a central difference is exact up to rounding, and long double
    leaves 1e-19 / h of it"""
    h = LD(1e-4)
    for name, variant in (("1x7x9x3_L4", "plain"), ("1x7x9x3_L4", "holes"), ("3x17x23x4_L5", "holes"), ("1x16x16x4_L1", "holes"), ("1x40x72x5_L4", "holes")):
        case = pr.make_case(name, variant, np.float64)
        ref = pr.restate(case["image"], case["obs"], case["weights"], case["levels"], case["lam"])
        assert np.all(np.isfinite(ref["image_b"].astype(np.float64)))
        rs = np.random.RandomState(0)
        image = case["image"].astype(LD)
        picks = {tuple(rs.randint(s) for s in image.shape) for _ in range(25)}
        if case["weights"] is not None:
            picks |= {(0, 0, 8, 0) if image.shape[2] > 8 else (0, 8, 0, 0)}  # inside the all-zero tile
        for at in picks:
            up, down = image.copy(), image.copy()
            up[at] += h
            down[at] -= h
            numeric = (pr.loss_only(up, case["obs"], case["weights"], case["levels"], case["lam"]) -
                       pr.loss_only(down, case["obs"], case["weights"], case["levels"], case["lam"])) / (2 * h)  # fmt: skip
            assert abs(numeric - ref["image_b"][at]) <= 1e-12 * max(1.0, float(ref["image_b_scale"][at])), (name, variant, at, numeric, ref["image_b"][at])
        if case["weights"] is not None:
            assert np.all(ref["image_b"][case["weights"] == 0] == 0)  # exactly


@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_torch_formulas_against_the_restatement(name):
    from deodr_amd.pyramid import pyramid_l2, pyramid_l2_torch, pyramid_terms, pyramid_terms_torch

    for variant in pr.VARIANTS:
        for dtype in pr.DTYPES:
            case = pr.make_case(name, variant, dtype)
            ref = pr.restate(case["image"], case["obs"], case["weights"], case["levels"], case["lam"])
            image, obs = torch.as_tensor(case["image"]).requires_grad_(True), torch.as_tensor(case["obs"])
            weights, lam = None if case["weights"] is None else torch.as_tensor(case["weights"]), torch.as_tensor(case["lam"])
            loss = pyramid_l2_torch(image, obs, weights, case["levels"], lam)
            assert loss.dtype == torch.float64 and loss.dim() == 0
            (image_b,) = torch.autograd.grad(loss, image)
            assert image_b.dtype == image.dtype and bool(torch.isfinite(image_b).all())
            terms = pyramid_terms_torch(image, obs, weights, case["levels"]).detach()
            got = dict(terms=terms.numpy(), loss=loss.detach().numpy(), image_b=image_b.numpy())
            # the torch formulas are another float64 evaluation: within the tolerance the kernels are held to (the gradient of a float32 image is
            # rounded to float32 by autograd at every level it passes, which the kernels do once: checked in float64 only)
            for k in ("terms", "loss") + (("image_b",) if dtype == np.float64 else ()):
                err, scale = np.abs(got[k].astype(LD) - ref[k]), ref[k + "_scale"]
                assert np.all(err <= pr.TOLERANCE * scale), (case["name"], k, float((err / np.maximum(scale, LD(1e-300))).max()))
            if dtype == np.float32:
                assert np.all(np.abs(got["image_b"].astype(LD) - ref["image_b"]) <= 1e-5 * np.maximum(ref["image_b_scale"], LD(1e-300)))
            if weights is not None:
                assert bool((image_b[weights == 0] == 0).all())
            # the public entry points take the torch formulas on CPU tensors
            assert torch.equal(pyramid_l2(image, obs, weights, case["levels"], lam), loss)
            assert torch.equal(pyramid_terms(image, obs, weights, case["levels"]), terms)


def test_properties_of_the_definition():
    for name, variant, dtype in every_case():
        case = pr.make_case(name, variant, dtype)
        ref = pr.restate(case["image"], case["obs"], case["weights"], case["levels"], case["lam"])
        image, obs = case["image"].astype(LD), case["obs"].astype(LD)
        w = np.ones(image.shape[:3], dtype=LD) if case["weights"] is None else case["weights"].astype(LD)
        weighted_l2 = (w[..., None] * (image - obs) ** 2).sum()  # today's data term
        assert abs(ref["terms"][0] - weighted_l2) <= 1e-17 * float(ref["terms_scale"][0]) + 0, case["name"]
        assert np.all(ref["terms"][1:] <= ref["terms"][:-1] * (1 + LD(1e-17))), case["name"]  # Cauchy-Schwarz, level by level
    # a constant residual gives every level the same value, holes or not: term_l = r^2 C sum(w)
    case = pr.make_case("3x17x23x4_L5", "holes", np.float64)
    obs = case["obs"]
    ref = pr.restate(obs + 0.375, obs, case["weights"], 5, case["lam"])
    expected = LD(0.375) ** 2 * 4 * case["weights"].astype(LD).sum()
    assert np.all(np.abs(ref["terms"] - expected) <= 1e-15 * expected)
    # once a level is 1 x 1 it stays 1 x 1
    case = pr.make_case("2x64x64x3_L8", "plain", np.float64)
    ref = pr.restate(case["image"], case["obs"], None, 8, case["lam"])
    assert ref["terms"][6] == ref["terms"][7] == ref["terms"][8] and ref["terms"][5] > ref["terms"][6]


def test_refusals_of_the_python_layer():
    from deodr_amd.pyramid import pyramid_l2

    image = torch.zeros(1, 4, 4, 3, dtype=torch.float64)
    for levels in (0, 9, -1, 2.5):
        with pytest.raises(ValueError, match="levels must be an integer in 1 .. 8"):
            pyramid_l2(image, image, None, levels)
    with pytest.raises(ValueError, match="level_weights must have 4 entries"):
        pyramid_l2(image, image, None, 3, [1.0, 1.0])
    with pytest.raises(ValueError, match=r"expected image and obs \[n,H,W,C\] and weights \[n,H,W\]"):
        pyramid_l2(image, image, torch.zeros(4, 4), 3)
    with pytest.raises(ValueError, match=r"expected image and obs \[n,H,W,C\]"):
        pyramid_l2(image, image[0], None, 3)


def test_measure_the_tolerance():
    """the float64 restatement against the long-double one over every case, variant and dtype: the figure MEASURED of tests/pyramid_reference.py"""
    worst, where = 0.0, None
    for name, variant, dtype in every_case():
        case = pr.make_case(name, variant, dtype)
        args = (case["image"], case["obs"], case["weights"], case["levels"], case["lam"])
        errors = pr.errors_relative_to_scale(pr.restate(*args, dtype=np.float64), pr.restate(*args))
        for k, e in errors.items():
            if e > worst:
                worst, where = e, (case["name"], k)
    print(f"largest float64 error relative to the scale: {worst:.3e} at {where}; MEASURED = {pr.MEASURED:.3e}, TOLERANCE = {pr.TOLERANCE:.3e}")
    assert worst <= pr.MEASURED and pr.MEASURED <= 2 * worst  # the figure in the file is the measured one, rounded up
    assert pr.TOLERANCE == 16 * pr.MEASURED
