"""CPU checks of the structural (SSIM) data term: the torch formulas of deodr_amd/ssim.py (value and autograd gradient) against the long-double
restatement of tests/ssim_reference.py and its closed-form adjoint, the properties the definition promises, and the measurement the tolerance of
the GPU tests is derived from."""

import numpy as np
import pytest
import torch

import ssim_reference as sr

LD = sr.LD


def torch_outputs(case, want_gradient=True):
    """the torch formulas on the tensors of ``case`` -> dict(terms, loss, image_b | None) as arrays"""
    from deodr_amd.ssim import ssim_l2_torch, ssim_terms_torch

    image, obs = torch.as_tensor(case["image"]).requires_grad_(want_gradient), torch.as_tensor(case["obs"])
    weights = None if case["weights"] is None else torch.as_tensor(case["weights"])
    loss = ssim_l2_torch(image, obs, weights, case["mix"], case["data_range"])
    assert loss.dtype == torch.float64 and loss.dim() == 0
    image_b = torch.autograd.grad(loss, image)[0].numpy() if want_gradient else None
    terms = ssim_terms_torch(image, obs, weights, case["data_range"]).detach().numpy()
    return dict(terms=terms, loss=loss.detach().numpy(), image_b=image_b)


def measured_errors(combo):
    """the float64 torch formulas against the long-double restatement, relative to the scales: the terms and the loss for every dtype, the gradient
    for float64 frames (autograd rounds the gradient of a float32 image to float32, which the kernels do once: held to its own bound below)"""
    case, ref = sr.reference(*combo)
    got = torch_outputs(case)
    keys = ("terms", "loss") + (("image_b",) if combo[2] == np.float64 else ())
    return case, ref, got, sr.errors_relative_to_scale(got, ref, keys)


def test_the_window_is_normalised_and_symmetric():
    from deodr_amd import ssim

    g = ssim.gaussian_window()
    assert len(g) == ssim.WINDOW == 11 and ssim.SIGMA == 1.5 and g == g[::-1] and abs(sum(g) - 1) <= 2.0**-52
    assert g[5] == max(g) and all(g[k] < g[k + 1] for k in range(5))
    # the same doubles as the restatement's, which computes its own
    taps = np.array(g).astype(LD)
    assert np.array_equal(sr.window_2d(), taps[:, None] * taps[None, :])


@pytest.mark.parametrize("combo", sr.every_case(), ids=sr.case_id)
def test_torch_formulas_and_autograd_against_the_restatement(combo):
    """value, and torch's autograd gradient against the closed-form adjoint of the issue (the restatement's image_b)"""
    from deodr_amd.ssim import ssim_l2, ssim_map_torch, ssim_terms

    case, ref, got, errors = measured_errors(combo)
    print(f"{case['name']}: " + "  ".join(f"{k} {e:.2e}" for k, e in errors.items()) + f"  (MEASURED {sr.MEASURED:.2e})")
    assert all(e <= sr.MEASURED for e in errors.values()), errors
    assert np.all(np.isfinite(got["image_b"]))
    if combo[2] == np.float32:
        assert np.all(np.abs(got["image_b"].astype(LD) - ref["image_b"]) <= 1e-5 * max(float(ref["image_b_scale"]), 1e-300))
    ssim = ssim_map_torch(torch.as_tensor(case["image"]), torch.as_tensor(case["obs"]), case["data_range"]).numpy()
    assert ssim.shape == case["image"].shape and np.abs(ssim.astype(LD) - ref["ssim"]).max() <= 1e-12
    if combo[0] in sr.SMALL[:4]:  # the public entry points take the torch formulas on CPU tensors
        image, obs = torch.as_tensor(case["image"]), torch.as_tensor(case["obs"])
        weights = None if case["weights"] is None else torch.as_tensor(case["weights"])
        assert float(ssim_l2(image, obs, weights, case["mix"], case["data_range"])) == float(got["loss"])
        assert np.array_equal(ssim_terms(image, obs, weights, case["data_range"]).numpy(), got["terms"])


def textured(n=1, H=40, W=23, C=3, seed=0):
    """a smooth pattern plus noise in [0.1, 0.9]: local means, contrasts and correlations that vary over the frame"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W]
    base = 0.5 + 0.25 * np.sin(0.7 * xx + 0.3 * yy)[None, :, :, None] * np.cos(0.2 * yy)[None, :, :, None]
    return np.clip(base + 0.15 * (rs.rand(n, H, W, C) - 0.5), 0.1, 0.9)


def test_identical_frames_have_no_structural_term_and_no_gradient():
    x = textured()
    ref = sr.restate(x, x, None, (0.0, 1.0), 1.0)
    assert abs(ref["terms"][1]) <= 1e-15 * x.size and ref["terms"][0] == 0 and np.abs(ref["ssim"] - 1).max() <= 1e-15
    assert np.abs(ref["image_b"]).max() <= 1e-12  # SSIM has its maximum there
    got = torch_outputs(dict(image=x, obs=x, weights=None, mix=(0.0, 1.0), data_range=1.0))
    assert abs(float(got["terms"][1])) <= 1e-12 * x.size and np.abs(got["image_b"]).max() <= 1e-9


def test_ssim_is_at_most_one_and_symmetric():
    for combo in (("2x2 tiles ragged 1x29x53x5", "plain", np.float64), ("1x5x7x4", "plain", np.float64), ("1x11x11x5", "holes255", np.float64)):
        case, ref = sr.reference(*combo)
        assert ref["ssim"].max() <= 1 + 1e-15
        swapped = sr.restate(case["obs"], case["image"], case["weights"], case["mix"], case["data_range"])
        assert np.abs(swapped["ssim"] - ref["ssim"]).max() <= 1e-17 and abs(swapped["terms"][1] - ref["terms"][1]) <= 1e-15 * abs(ref["terms"][1])
    x, y = textured(seed=1), textured(seed=2)
    from deodr_amd.ssim import ssim_map_torch

    s_xy, s_yx = ssim_map_torch(torch.as_tensor(x), torch.as_tensor(y)), ssim_map_torch(torch.as_tensor(y), torch.as_tensor(x))
    assert float(s_xy.max()) <= 1 + 1e-12 and float((s_xy - s_yx).abs().max()) <= 1e-12


def test_a_change_of_exposure_moves_the_pixel_term_more_than_the_structural_one():
    """the reason the term exists: obs -> a obs + b (mean and contrast changed) against the same obs, each term relative to what it is against an
    unrelated textured frame"""
    y, other = textured(seed=3), textured(seed=4)
    exposed = 0.7 * y + 0.12
    same, unrelated = sr.restate(exposed, y, None, (0.5, 0.5), 1.0), sr.restate(other, y, None, (0.5, 0.5), 1.0)
    moved = same["terms"] / unrelated["terms"]
    print(f"exposure changed: term_0 {float(same['terms'][0]):.3f}, term_1 {float(same['terms'][1]):.3f}; unrelated frame: "
          f"{float(unrelated['terms'][0]):.3f}, {float(unrelated['terms'][1]):.3f}; ratios {float(moved[0]):.3f}, {float(moved[1]):.3f}")  # fmt: skip
    assert moved[0] > moved[1] and same["terms"][1] > 0


def test_zero_weights_drop_their_pixels_from_both_terms():
    case, ref = sr.reference("2x2 tiles ragged 1x29x53x5", "holes", np.float64)
    x, y, w = case["image"].astype(LD), case["obs"].astype(LD), case["weights"].astype(LD)
    kept = w > 0
    assert 0.1 < 1 - kept.mean() < 0.3
    full = sr.restate(case["image"], case["obs"], None, case["mix"], 1.0)
    assert abs(ref["terms"][0] - (w[kept][:, None] * (x - y)[kept] ** 2).sum()) <= 1e-16 * ref["terms"][0]
    assert abs(ref["terms"][1] - (w[kept][:, None] * (1 - full["ssim"])[kept]).sum()) <= 1e-16 * ref["terms"][1]  # the map itself does not see the weights
    assert np.abs(ref["ssim_b"][~kept]).max() > 0  # ... so a pixel of weight 0 still has a gradient: its neighbours' windows hold it
    _, zero = sr.reference("2x2 tiles ragged 1x29x53x5", "zero", np.float64)
    assert np.all(zero["terms"] == 0) and np.all(zero["image_b"] == 0)


def test_mix_scales_linearly():
    from deodr_amd.ssim import ssim_l2_torch

    case, ref = sr.reference("1x11x11x5", "plain", np.float64)
    image, obs = torch.as_tensor(case["image"]), torch.as_tensor(case["obs"])
    t0, t1 = (float(v) for v in ref["terms"])
    for alpha, beta in ((1.0, 0.0), (0.0, 1.0), (0.8, 0.2), (2.0, 3.0)):
        assert float(ssim_l2_torch(image, obs, None, (alpha, beta))) == pytest.approx(alpha * t0 + beta * t1, rel=1e-13)
    assert float(ssim_l2_torch(image, obs, None, None)) == pytest.approx(t1, rel=1e-13)  # None: the structural term alone
    only_pixels = sr.restate(case["image"], case["obs"], None, (1.0, 0.0), 1.0)
    assert np.array_equal(only_pixels["image_b"], 2 * (case["image"].astype(LD) - case["obs"].astype(LD)))


def test_refusals_of_the_python_layer():
    from deodr_amd.ssim import ssim_l2, ssim_terms

    image = torch.zeros(1, 4, 4, 3, dtype=torch.float64)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="data_range must be finite and > 0"):
            ssim_l2(image, image, None, None, bad)
        with pytest.raises(ValueError, match="data_range must be finite and > 0"):
            ssim_terms(image, image, None, bad)
    with pytest.raises(ValueError, match="mix must have 2 entries"):
        ssim_l2(image, image, None, [1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match=r"expected image and obs \[n,H,W,C\] and weights \[n,H,W\]"):
        ssim_l2(image, image, torch.zeros(4, 4))
    with pytest.raises(ValueError, match=r"expected image and obs \[n,H,W,C\]"):
        ssim_l2(image, image[0])


def test_measure_the_tolerance():
    """the float64 torch formulas against the long-double restatement over every case, variant and dtype: the figure MEASURED of
    tests/ssim_reference.py, from which the GPU tests take TOLERANCE = 8 MEASURED"""
    worst, where = 0.0, None
    for combo in sr.every_case():
        case, _ref, _got, errors = measured_errors(combo)
        for k, e in errors.items():
            if e > worst:
                worst, where = e, (case["name"], k)
    print(f"largest float64 error relative to the scale: {worst:.3e} at {where}; MEASURED = {sr.MEASURED:.3e}, TOLERANCE = {sr.TOLERANCE:.3e}")
    assert worst <= sr.TOLERANCE / 8 and sr.MEASURED <= 2 * worst  # the figure in the file is the measured one, rounded up
    assert sr.TOLERANCE == 8 * sr.MEASURED
