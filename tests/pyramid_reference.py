"""What the tests of the multi-scale L2 data term share: the term of include/deodr_hip_pyramid.h restated in NumPy -- value and hand-written adjoint, in
float64 or in long double --, the case table the CPU and the GPU tests run, and the tolerance of the GPU tests.

Every output of the restatement comes with its SCALE: the same formula evaluated with the absolute value of every term (|image| + |obs| for the
residual, sums of magnitudes for the sums over cells and levels), computed in long double.  An output's error is measured against that.

THE TOLERANCE OF THE GPU TESTS.  tests/test_pyramid_reference.py::test_measure_the_tolerance runs the float64 restatement against the long-double one
over every case and variant below and prints the largest ``|float64 - long double| / scale`` over every element of every output: MEASURED is that
figure.  The kernels compute the same formulas in float64 but add in another order (butterflies over the lanes of a tile, partial sums per workgroup,
a fixed-order tree over them), hence FACTOR = 16 on top of it.  A float32 ``image_b`` is rounded once more when it is stored: 2^-24 |reference| is
added for it (float32 inputs are exact in double)."""

import numpy as np

LD = np.longdouble
MEASURED = 2.2e-16  # test_measure_the_tolerance: "largest float64 error relative to the scale: 2.157e-16" (image_b of "1x16x16x4_L1 holes float64")
FACTOR = 16
TOLERANCE = FACTOR * MEASURED
F32_ROUNDING = 2.0**-24

# (n, H, W, C, levels): what it exercises
CASES = {
    "1x1x1x1_L3": ((1, 1, 1, 1, 3), "every level is the same cell"),
    "1x7x9x3_L4": ((1, 7, 9, 3, 4), "one partial tile each way"),
    "1x8x8x1_L3": ((1, 8, 8, 1, 3), "exactly one tile; top level = the wave"),
    "1x9x8x4_L4": ((1, 9, 8, 4, 4), "one row of a second tile"),
    "1x8x9x4_L4": ((1, 8, 9, 4, 4), "one column of a second tile"),
    "1x16x16x4_L1": ((1, 16, 16, 4, 1), "fewer levels than a tile holds: one pass, value and adjoint"),
    "1x16x16x4_L3": ((1, 16, 16, 4, 3), "the last level of the one-pass path"),
    "1x16x16x4_L4": ((1, 16, 16, 4, 4), "level 4 is 1 x 1: the first level of the tile-grid kernel"),
    "3x17x23x4_L5": ((3, 17, 23, 4, 5), "odd at several levels, several views"),
    "2x64x64x3_L6": ((2, 64, 64, 3, 6), "the top level is 1 x 1"),
    "2x64x64x3_L8": ((2, 64, 64, 3, 8), "levels beyond 1 x 1"),
    "1x65x63x2_L7": ((1, 65, 63, 2, 7), "run-time C"),
    "1x40x72x5_L4": ((1, 40, 72, 5, 4), "run-time C"),
    # where the launch geometry changes: a workgroup of the tile kernel takes 4 tiles and there are at most 1024 of them -- 65 x 65 = 4225 tiles are
    # more than 4096, so some workgroups stride to a second tile, and 1024 partials are four rounds of the 256 threads that add them; a region of the
    # tile-grid kernel is 32 x 32 tiles = 256 x 256 pixels: 520 pixels are three regions each way, the last one tile wide, and 3 x 3 cells at level 8
    "1x520x520x1_L8": ((1, 520, 520, 1, 8), "grid cap of the tile kernel, later rounds of its fixed-order sum, 3 x 3 regions of the tile-grid kernel"),
    "2x264x40x3_L6": ((2, 264, 40, 3, 6), "two regions down, one across, two views: the region index of a workgroup"),
}
VARIANTS = ("plain", "holes")  # weights None and level weights of 1; random weights with zero cells and random level weights with a zero entry
DTYPES = (np.float32, np.float64)


def make_case(name, variant, dtype):
    """-> dict(image, obs [n,H,W,C] and weights [n,H,W] | None as arrays of ``dtype`` (the stored values), lam [levels+1] float64, levels)"""
    (n, H, W, C, levels), _ = CASES[name]
    rs = np.random.RandomState(sorted(CASES).index(name) * 4 + VARIANTS.index(variant) * 2 + DTYPES.index(dtype))
    image, obs = rs.rand(n, H, W, C).astype(dtype), rs.rand(n, H, W, C).astype(dtype)
    if variant == "plain":
        return dict(name=f"{name} {variant} {np.dtype(dtype).name}", image=image, obs=obs, weights=None, lam=np.ones(levels + 1), levels=levels)
    w = rs.rand(n, H, W) + 0.25
    w[rs.rand(n, H, W) < 0.1] = 0  # scattered zeros
    if W > 8:  # one all-zero aligned 8 x 8 tile
        w[:, :8, 8:16] = 0
    elif H > 8:
        w[:, 8:16, :8] = 0
    if H > 32:  # one all-zero aligned 32 x 32 block: zero cells up to level 5
        w[:, 32:64, :32] = 0
    elif W > 32:
        w[:, :32, 32:64] = 0
    lam = rs.rand(levels + 1) * 2
    lam[rs.randint(levels + 1)] = 0
    return dict(name=f"{name} {variant} {np.dtype(dtype).name}", image=image, obs=obs, weights=w.astype(dtype), lam=lam, levels=levels)


def children_sum(x):
    """[n,H,W,...] -> [n,ceil(H/2),ceil(W/2),...]: every cell the sum of the up to four children that exist"""
    n, H, W = x.shape[:3]
    padded = np.zeros((n, H + H % 2, W + W % 2) + x.shape[3:], dtype=x.dtype)
    padded[:, :H, :W] = x
    return padded.reshape((n, padded.shape[1] // 2, 2, padded.shape[2] // 2, 2) + x.shape[3:]).sum(axis=(2, 4))


def to_children(x, H, W):
    """the value of every cell's parent: [n,ceil(H/2),ceil(W/2),...] -> [n,H,W,...]"""
    return np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)[:, :H, :W]


def restate(image, obs, weights, levels, lam, dtype=LD):
    """-> dict(terms [levels+1], loss, image_b [n,H,W,C]) and, under the same names + "_scale", the scale of each, all in ``dtype``"""
    image, obs, lam = image.astype(dtype), obs.astype(dtype), np.asarray(lam).astype(dtype)
    w = np.ones(image.shape[:3], dtype=dtype) if weights is None else weights.astype(dtype)
    q, m = w[..., None] * (image - obs), w[..., None] * (np.abs(image) + np.abs(obs))  # value and magnitude
    qs, ms, iws, terms, scales = [], [], [], [], []
    for level in range(levels + 1):
        if level:
            q, m, w = children_sum(q), children_sum(m), children_sum(w)
        iw = np.where(w > 0, 1 / np.where(w > 0, w, 1), 0).astype(dtype)
        qs.append(q), ms.append(m), iws.append(iw)
        terms.append((q * q * iw[..., None]).sum()), scales.append((m * m * iw[..., None]).sum())
    terms, scales = np.array(terms, dtype=dtype), np.array(scales, dtype=dtype)
    g = g_scale = None
    for level in range(levels, -1, -1):  # g_L = 2 lambda_L q_L iw_L; g_l = 2 lambda_l q_l iw_l + g_{l+1} of the parent
        H, W = qs[level].shape[1:3]
        mine, mine_scale = 2 * lam[level] * qs[level] * iws[level][..., None], 2 * lam[level] * ms[level] * iws[level][..., None]
        g = mine if g is None else mine + to_children(g, H, W)
        g_scale = mine_scale if g_scale is None else mine_scale + to_children(g_scale, H, W)
    w0 = (np.ones(image.shape[:3], dtype=dtype) if weights is None else weights.astype(dtype))[..., None]
    return dict(terms=terms, terms_scale=scales, loss=(lam * terms).sum(), loss_scale=(lam * scales).sum(), image_b=w0 * g, image_b_scale=w0 * g_scale)


def loss_only(image, obs, weights, levels, lam, dtype=LD):
    return restate(image, obs, weights, levels, lam, dtype)["loss"]


def errors_relative_to_scale(got, ref):
    """-> {output: largest |got - ref| / scale over its elements} (an element of scale 0 must be exactly the reference's)"""
    worst = {}
    for k in ("terms", "loss", "image_b"):
        err, scale = np.abs(np.asarray(got[k]).astype(LD) - ref[k]), np.asarray(ref[k + "_scale"])
        assert np.all(err[scale == 0] == 0), k
        worst[k] = float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0
    return worst
