"""What the tests of the structural (SSIM) data term share: the term of include/deodr_hip_ssim.h restated in NumPy long double -- value and the
closed-form adjoint, as direct two-dimensional window sums over a zero-padded frame, sharing no code with deodr_amd/ssim.py --, the case table the
CPU and the GPU tests run, and the tolerance of the GPU tests.

THE CASE TABLE was built for the kernels' tile of TILE = (16 rows, 32 columns) pixels, their halo of 5 and their cap of GRID_CAP = 1024 workgroups
(SSIM_TH, SSIM_TW, SSIM_BLOCKS of deodr_amd/csrc/dr_ssim.h; tests/test_ssim_abi.py compares them with the source): a change of the tile shape moves
the cases named "tile ...", "2x2 tiles" and "grid cap".

THE TOLERANCE OF THE GPU TESTS.  tests/test_ssim_reference.py::test_measure_the_tolerance runs the float64 torch formulas of deodr_amd/ssim.py against
this restatement over every case, variant and dtype below and prints the largest error relative to the SCALE of each quantity: ``max |image_b|`` of
the case for the gradient, the term's own value for each of the two terms, ``|alpha| term_0 + |beta| term_1`` for the loss.  MEASURED is that figure
(it already contains the division by b1 b2 and the cancellations in the variances; the cases keep their frames in [0, R]).  The kernels compute the
same formulas in float64 but add in another order and with fused multiply-adds, hence FACTOR = 8 on top of it.  A float32 ``image_b`` is rounded once
more when it is stored: 2^-23 |reference| is added for it (float32 inputs are exact in double, so the terms keep the double tolerance)."""

import functools
import math

import numpy as np

LD = np.longdouble
MEASURED = 1.3e-15  # test_measure_the_tolerance: "largest float64 error relative to the scale: 1.225e-15" (image_b of "2x2 tiles ragged 1x29x53x5 holes float64")
FACTOR = 8
TOLERANCE = FACTOR * MEASURED
F32_ROUNDING = 2.0**-23

TILE = (16, 32)  # rows, columns
GRID_CAP = 1024

# (n, H, W, C): what it exercises
CASES = {
    "1x1x1x1": ((1, 1, 1, 1), "the window is larger than the frame: all padding"),
    "1x1x12x3": ((1, 1, 12, 3), "one row, wider than the window"),
    "1x5x7x4": ((1, 5, 7, 4), "smaller than the window both ways"),
    "1x11x11x5": ((1, 11, 11, 5), "the window exactly; run-time C beyond 4"),
    "tile 3x16x32x1": ((3, 16, 32, 1), "one tile exactly, several views"),
    "tile-1 down 1x15x32x3": ((1, 15, 32, 3), "one row short of a tile"),
    "tile+1 down 1x17x32x4": ((1, 17, 32, 4), "one row of a second tile"),
    "tile-1 across 1x16x31x4": ((1, 16, 31, 4), "one column short of a tile"),
    "tile+1 across 1x16x33x3": ((1, 16, 33, 3), "one column of a second tile"),
    "2x2 tiles 3x32x64x3": ((3, 32, 64, 3), "two tiles by two: the halo crosses both seams; several views and channels in the planar maps"),
    "2x2 tiles ragged 1x29x53x5": ((1, 29, 53, 5), "two tiles by two, the last ones partial"),
    # 2 x 513 = 1026 tiles (the second row of tiles is one pixel high, the last column one pixel wide) on 1024 workgroups: the first two workgroups walk
    # a second tile, and the 1024 partials are four rounds of the 256 threads that add them.  n = 1 and C = 1 keep the frame at 278 545 pixels.
    "grid cap 1x17x16385x1": ((1, 17, 16385, 1), "more tiles than the capped grid: a workgroup walks two tiles"),
}
SMALL = [name for name in CASES if not name.startswith("grid cap")]
# weights, mix = (alpha, beta), data_range (the frames are scaled by it)
VARIANTS = {
    "plain": ("none", (0.8, 0.2), 1.0),
    "holes": ("random", (0.0, 1.0), 1.0),
    "holes255": ("random", (0.8, 0.2), 255.0),
    "pixel-only": ("random", (1.0, 0.0), 1.0),
    "zero": ("zero", (0.8, 0.2), 1.0),
}
DTYPES = (np.float32, np.float64)


def every_case():
    """every (case, variant, dtype) the CPU and the GPU tests run: the small frames in every combination, the large one in two"""
    combos = [(name, variant, dtype) for name in SMALL for variant in VARIANTS for dtype in DTYPES]
    return combos + [("grid cap 1x17x16385x1", "holes", np.float32), ("grid cap 1x17x16385x1", "plain", np.float64)]


def case_id(combo):
    return f"{combo[0]} {combo[1]} {np.dtype(combo[2]).name}".replace(" ", "_")


def make_case(name, variant, dtype):
    """-> dict(image, obs [n,H,W,C] in [0, R] and weights [n,H,W] | None as arrays of ``dtype`` (the stored values), mix (alpha, beta), data_range)"""
    (n, H, W, C), _ = CASES[name]
    kind, mix, R = VARIANTS[variant]
    rs = np.random.RandomState(sorted(CASES).index(name) * 16 + sorted(VARIANTS).index(variant) * 2 + DTYPES.index(dtype))
    image, obs = (rs.rand(n, H, W, C) * R).astype(dtype), (rs.rand(n, H, W, C) * R).astype(dtype)
    if kind == "none":
        weights = None
    elif kind == "zero":
        weights = np.zeros((n, H, W), dtype=dtype)
    else:
        w = rs.rand(n, H, W) + 0.25
        w[rs.rand(n, H, W) < 0.2] = 0  # about 20 % zeros
        weights = w.astype(dtype)
    return dict(name=f"{name} {variant} {np.dtype(dtype).name}", image=image, obs=obs, weights=weights, mix=mix, data_range=R)


def window_2d():
    """the 11 x 11 window in long double: the outer product of the taps g_k = exp(-k^2 / (2 1.5^2)) / sum, which are DOUBLES (the definition)"""
    e = [math.exp(-(k * k) / (2 * 1.5 * 1.5)) for k in range(-5, 6)]
    total = sum(e)
    g = np.array([v / total for v in e], dtype=np.float64).astype(LD)
    return g[:, None] * g[None, :]


def windowed(t):
    """[n,H,W,C] long double -> G*t: 121 shifted copies of the zero-padded frame, each times its tap, added row by row of the window"""
    n, H, W, C = t.shape
    G = window_2d()
    padded = np.zeros((n, H + 10, W + 10, C), dtype=LD)
    padded[:, 5 : 5 + H, 5 : 5 + W] = t
    out = np.zeros_like(t)
    for i in range(11):
        for j in range(11):
            out += G[i, j] * padded[:, i : i + H, j : j + W]
    return out


def restate(image, obs, weights, mix, data_range):
    """-> dict(ssim [n,H,W,C], terms [2], loss, image_b [n,H,W,C]) in long double, and the scales "terms_scale" [2], "loss_scale", "image_b_scale"
    (one number: the largest |image_b|)"""
    x, y = image.astype(LD), obs.astype(LD)
    w = (np.ones(x.shape[:3], dtype=LD) if weights is None else weights.astype(LD))[..., None]
    alpha, beta, R = LD(mix[0]), LD(mix[1]), LD(data_range)
    C1, C2 = (LD(0.01) * R) ** 2, (LD(0.03) * R) ** 2
    mx, my = windowed(x), windowed(y)
    sxx, syy, sxy = windowed(x * x) - mx * mx, windowed(y * y) - my * my, windowed(x * y) - mx * my
    a1, a2, b1, b2 = 2 * mx * my + C1, 2 * sxy + C2, mx * mx + my * my + C1, sxx + syy + C2
    ssim = a1 * a2 / (b1 * b2)
    terms = np.array([(w * (x - y) ** 2).sum(), (w * (1 - ssim)).sum()], dtype=LD)
    S_xy, S_xx = 2 * a1 / (b1 * b2), -ssim / b2
    S_m = 2 * my * a2 / (b1 * b2) - 2 * mx * ssim / b1 - 2 * mx * S_xx - my * S_xy
    A, B, Cm = -w * S_m, -w * S_xx, -w * S_xy
    ssim_b = windowed(A) + 2 * x * windowed(B) + y * windowed(Cm)  # d term_1 / d image
    image_b = 2 * alpha * w * (x - y) + beta * ssim_b
    return dict(ssim=ssim, terms=terms, loss=alpha * terms[0] + beta * terms[1], image_b=image_b, ssim_b=ssim_b, terms_scale=np.abs(terms),
                loss_scale=abs(alpha) * abs(terms[0]) + abs(beta) * abs(terms[1]), image_b_scale=np.abs(image_b).max())  # fmt: skip


@functools.lru_cache(maxsize=None)
def reference(name, variant, dtype):
    """-> (case, its long-double restatement), computed once and shared by the tests: do not change either"""
    case = make_case(name, variant, dtype)
    return case, restate(case["image"], case["obs"], case["weights"], case["mix"], case["data_range"])


def errors_relative_to_scale(got, ref, keys=("terms", "loss", "image_b")):
    """-> {output: largest |got - ref| / scale over its elements} (an element of scale 0 must be exactly the reference's)"""
    worst = {}
    for k in keys:
        err = np.abs(np.asarray(got[k]).astype(LD) - ref[k])
        scale = np.broadcast_to(np.asarray(ref[k + "_scale"]), err.shape)
        assert np.all(err[scale == 0] == 0), k
        worst[k] = float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0
    return worst
