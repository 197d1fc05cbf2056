"""The two texture kernels (include/deodr_hip_texture.h, deodr_amd/csrc/dr_texfit.h) where their paths change: a long-double restatement of both
(``cpu_raster_texture.np_smoothness`` / ``np_step`` stay the second opinion in float64), a restatement of WHICH 16-byte pieces of a texture the
smoothness kernel takes through its vector path, the grids both launches get (``capped_blocks`` of dr_host.h, the caps parsed from dr_texfit.h), and
the case table tests/test_texture_kernel_cases.py (CPU: every case is in its regime) and tests/test_texture_kernels_gpu.py share.

A texture [Ht, Wt, C] is walked as one flat array of N = Ht R elements, R = Wt C, in pieces of VEC = 16 / itemsize elements; piece i (elements
e0 = i VEC ...) goes the vector way when ``e0 >= R and e0 + VEC + R <= N``, element by element otherwise, and the N % VEC elements behind the last
piece always go one by one.  What the conditions leave no room for, asserted by the CPU test rather than assumed:
* 3 x 2 x 1 in float32 has ONE piece and it starts in the first row: no vector piece.  5 x 2 x 1 is the smallest texture of rows shorter than a
  vector that has one; with R = 2 such a piece holds two whole rows, with R = 3 a whole row and parts of its neighbours (j wraps inside it either way).
* the last whole piece is a vector piece only if R <= N % VEC: with a tail of 1 never (R >= 2), so never in float64."""

import functools
import os
import re

import numpy as np

LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "deodr_amd", "csrc")


# ---- the restatements, in long double (or ``dtype``) -------------------------------------------------------------------------------------------


def smoothness(t, weight, dtype=LD):
    """-> (E, dE/dt) of E = 0.5 weight (sum of the squared differences of x- and y-neighbours), free boundary: every element's own sum over the
    neighbours that exist, ``weight (t - neighbour)`` each"""
    t = np.asarray(t).astype(dtype)
    w = dtype(weight)
    dx, dy = t[:, 1:] - t[:, :-1], t[1:] - t[:-1]
    energy = dtype(0.5) * w * ((dx * dx).sum() + (dy * dy).sum())
    g = np.zeros_like(t)
    g[:, 1:] += dx
    g[:, :-1] -= dx
    g[1:] += dy
    g[:-1] -= dy
    return energy, w * g


def step(t, s, g, factor, step_max=None, inertia=0.0, damping=0.0, clamp=None, dtype=LD):
    """-> (new texture, new speed): s = (1 - damping)(inertia s + (1 - inertia) clip(-factor g, +-step_max)), t += s; with ``clamp`` t is clipped and s
    is 0 where it clipped"""
    t, s, g = (np.asarray(a).astype(dtype) for a in (t, s, g))
    move = -dtype(factor) * g
    if step_max is not None and step_max > 0:
        move = np.minimum(np.maximum(move, -dtype(step_max)), dtype(step_max))
    s = (1 - dtype(damping)) * (dtype(inertia) * s + (1 - dtype(inertia)) * move)
    t = t + s
    if clamp is not None:
        lo, hi = dtype(clamp[0]), dtype(clamp[1])
        s = np.where((t < lo) | (t > hi), dtype(0), s)
        t = np.minimum(np.maximum(t, lo), hi)
    return t, s


# ---- which way a piece goes, and the grids -----------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def kernel_constants():
    found = {}
    for name in ("dr_texfit.h", "dr_fronthalf.h"):
        with open(os.path.join(CSRC, name)) as f:
            found.update({k: int(v) for k, v in re.findall(r"constexpr\s+int\s+(\w+)\s*=\s*(\d+)\s*;", f.read())})
    missing = [k for k in ("TEX_SMOOTH_BLOCKS", "TEX_STEP_BLOCKS", "FH_BLOCK") if k not in found]
    assert not missing, f"constants not found in the kernel headers: {missing}"
    return found


def capped_blocks(count, per_block, cap):
    """dr_host.h: the quotient rounded UP, at least 1, at most ``cap``"""
    want = count // per_block + (count % per_block != 0)
    return 1 if want < 1 else (want if want < cap else cap)


def geometry(kernel, shape, itemsize, k=None):
    """the launch of ``texture_smoothness_kernel`` ("smooth") or ``texture_step_kernel`` ("step") -> dict: VEC, N, R, pieces, tail, grid, the trips
    of the busiest thread over the pieces, and ``cap`` = blocks x FH_BLOCK, the pieces one trip of a full grid takes"""
    k = k or kernel_constants()
    Ht, Wt, C = shape
    vec, N = 16 // itemsize, Ht * Wt * C
    blocks = k["TEX_SMOOTH_BLOCKS" if kernel == "smooth" else "TEX_STEP_BLOCKS"]
    pieces = N // vec
    grid = capped_blocks(pieces, k["FH_BLOCK"], blocks)
    return {"VEC": vec, "N": N, "R": Wt * C, "pieces": pieces, "tail": N - pieces * vec, "grid": grid, "trips": -(-pieces // (grid * k["FH_BLOCK"])),
            "cap": blocks * k["FH_BLOCK"]}  # fmt: skip


def vector_pieces(shape, itemsize):
    """the pieces i the smoothness kernel takes through its vector path (dr_texfit.h: ``e0 >= R && e0 + VEC + R <= N``), as an array"""
    Ht, Wt, C = shape
    vec, R, N = 16 // itemsize, Wt * C, Ht * Wt * C
    e0 = np.arange(N // vec, dtype=np.int64) * vec
    return np.flatnonzero((e0 >= R) & (e0 + vec + R <= N))


def rows_inside(piece, shape, itemsize):
    """-> (whole rows of the texture that lie inside the piece, row ends strictly inside it: where j wraps)"""
    Ht, Wt, C = shape
    vec, R = 16 // itemsize, Wt * C
    e0 = int(piece) * vec
    whole = sum(1 for y in range(Ht) if e0 <= y * R and (y + 1) * R <= e0 + vec)
    wraps = sum(1 for e in range(e0 + 1, e0 + vec) if e % R == 0)
    return whole, wraps


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------

# rows shorter than a float32 vector (R = 2, 3); in float64 R = VEC or R = VEC + 1
SHORT_ROWS = [(3, 2, 1), (5, 2, 1), (6, 2, 1), (7, 3, 1), (9, 3, 1)]
ONE_INTERIOR_ROW = [(3, 8, 1), (3, 5, 3)]
# (shape, itemsize) -> (N % VEC, the last whole piece is a vector piece)
TAILS = {
    ((3, 7, 1), 4): (1, False), ((5, 5, 2), 4): (2, False), ((3, 7, 3), 4): (3, False), ((7, 2, 1), 4): (2, True), ((9, 3, 1), 4): (3, True),
    ((3, 7, 1), 8): (1, False), ((5, 3, 1), 8): (1, False),
}  # fmt: skip
CHANNELS = [(4, Wt, C) for C in (2, 5, 64) for Wt in (2, 7)]
MISALIGNED = [(6, 2, 1), (9, 3, 1), (5, 7, 3), (4, 7, 5)]  # run 1, 2, 3 elements behind a 16-byte boundary in float32, 1 in float64
# (kernel, itemsize) -> shapes whose piece counts are exactly blocks x FH_BLOCK, one more, and more than twice that: 1, 2 and 3 trips
CAPS = {
    ("smooth", 4): [(512, 256, 4), (3, 43691, 4), (1025, 256, 4)],
    ("smooth", 8): [(512, 128, 4), (3, 43691, 2), (1025, 128, 4)],
    ("step", 4): [(1024, 512, 4), (3, 174763, 4), (1025, 1024, 4)],
    ("step", 8): [(1024, 256, 4), (3, 174763, 2), (1025, 512, 4)],
}
SMALL = SHORT_ROWS + ONE_INTERIOR_ROW + sorted({shape for shape, _ in TAILS}) + CHANNELS
SMALL = sorted(set(SMALL), key=SMALL.index)

# the step's parameters: step_max None, 0 and positive; inertia 0 and 1; damping 1 (every speed exactly 0); clamp with lo == hi
STEP_PARAMETERS = [
    dict(), dict(step_max=0.0, inertia=0.5), dict(step_max=0.2, inertia=0.9, damping=0.05, clamp=(0.0, 1.0)), dict(inertia=1.0, damping=0.25),
    dict(inertia=0.0, step_max=0.1, clamp=(0.25, 0.75)), dict(damping=1.0, inertia=0.7), dict(damping=1.0, clamp=(0.0, 1.0)), dict(inertia=0.3, clamp=(0.5, 0.5)),
    dict(step_max=0.05, inertia=0.2, damping=0.1),
]  # fmt: skip
FACTOR, WEIGHT = 0.3, 0.37


def arrays(shape, float32, seed=0):
    """-> texture, speed, gradient g0 of a case as float64 arrays that hold float32 values where ``float32``; two texels meet the walls of a [0, 1]
    clamp whatever the size: at rest on 0 and on 1, pushed outwards"""
    rs = np.random.RandomState(seed + 131 * shape[0] + 7 * shape[1] + shape[2])
    t, g, s = rs.rand(*shape), rs.randn(*shape), 0.05 * rs.randn(*shape)
    t.reshape(-1)[:2], s.reshape(-1)[:2], g.reshape(-1)[:2] = (0.0, 1.0), (0.0, 0.0), (5.0, -5.0)
    if float32:
        t, s, g = (a.astype(np.float32).astype(np.float64) for a in (t, s, g))
    return t, s, g
