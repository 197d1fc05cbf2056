"""NumPy restatement of include/deodr_hip_chamfer_grid.h, for the tests: the stable sort by key, the cell rule of the grid (h, floor, clamp, hash,
the last ring, the early-exit bound), a ring-by-ring simulation of the search, and the energy -- that of tests/chamfer_reference.py, with the
correspondences beyond ``max_distance`` masked (-1, which is DEODR_HIP_CHAMFER_GRID_NONE as a signed 32-bit word).

The tolerances.  The kernels add the terms in the order of the brute-force operator and the gradient of a vertex's points strided over 64 lanes and
then in a tree; tests/chamfer_reference.py measured its tolerances on a chain, one value after the other, the order with the largest error, so
another fixed order stays inside them for cases within that table's sizes (5 000 values added).  tests/test_chamfer_grid_reference.py measures the
same chain error over THIS file's table (``grid_cases``, up to 65 537 values added, most of them the constant of a truncated pair) against long
double and prints it: terms 3.64e-15, gradient 2.60e-16 -- inside the older table's values, as expected.  Rounded up, and 8 x that for the GPU, as
the other kernel families do."""

import numpy as np

import chamfer_reference as cr

LD = np.longdouble
DIGIT_BITS, SORT_BLOCK, SORT_ITEMS, SORT_MAX_ITEMS = 8, 256, 2048, 2**24  # DEODR_HIP_SORT_* (tests/test_chamfer_grid_abi.py pins them)
NONE, RINGS, TABLE_LOAD, CELL_LIMIT, MAX_ITEMS, MIN_TABLE_BITS, MAX_TABLE_BITS, GATHER_VERTICES = 0xFFFFFFFF, 4, 2, 2**30, 2**24, 6, 25, 4  # DEODR_HIP_CHAMFER_GRID_*
EXIT_MARGIN = 1.0 - 2.0**-20

TOL_TERMS, TOL_GRADIENT = 4e-15, 3e-16  # measured over grid_cases(), see above
GPU_TOL_TERMS, GPU_TOL_GRADIENT = 8 * TOL_TERMS, 8 * TOL_GRADIENT


# ---- the sort


def stable_order(keys, bits):
    """[n,N] uint32 -> (sorted_keys, order): per row the stable permutation by the low ``bits`` bits, and keys[order] (all 32 bits)"""
    keys = np.asarray(keys, dtype=np.uint32)
    mask = np.uint32(0xFFFFFFFF if bits >= 32 else (1 << bits) - 1)
    order = np.argsort(keys & mask, axis=1, kind="stable")
    return np.take_along_axis(keys, order, axis=1), order.astype(np.uint32)


def sort_passes(bits):
    return -(-bits // DIGIT_BITS)


def sort_ok(N, n, bits):
    return 1 <= N <= SORT_MAX_ITEMS and 1 <= n <= 65535 and 1 <= bits <= 32


def sort_launches(N, n, bits):
    return 3 * sort_passes(bits) if sort_ok(N, n, bits) else 0


def sort_scratch_bytes(N, n, bits):
    return 4 * n * (4 * N + (1 << DIGIT_BITS) * -(-N // SORT_ITEMS)) if sort_ok(N, n, bits) else 0


# ---- the sizes of the operator


def table_bits(references):
    if not 1 <= references <= MAX_ITEMS:
        return 0
    b = MIN_TABLE_BITS
    while b < MAX_TABLE_BITS and (1 << b) < TABLE_LOAD * references:
        b += 1
    return b


def assign_bits(V):
    return max(1, int(V).bit_length())  # ceil(log2(V + 1))


def dims_ok(V, P, n):
    return 1 <= V <= MAX_ITEMS and 1 <= P <= MAX_ITEMS and 1 <= n <= 65535


def launches(V, P, n, directions):
    if not dims_ok(V, P, n) or not 1 <= directions <= 3:
        return 0
    count = 1
    if directions & 1:
        count += 2 + 3 * sort_passes(table_bits(V)) + 3 + 3 * sort_passes(assign_bits(V))
    if directions & 2:
        count += 2 + 3 * sort_passes(table_bits(P)) + 1
    return count


def scratch_bytes(V, P, n):
    if not dims_ok(V, P, n):
        return 0
    Tv, Tp = 1 << table_bits(V), 1 << table_bits(P)
    return 64 + 8 * n * (8 * V + 5 * P + 2 * cr.MAX_BLOCKS) + 4 * n * (7 * P + 4 * V + 2 * Tv + 2 * Tp + 2) + sort_scratch_bytes(max(V, P), n, 32)


# ---- the cell rule


def cell_edge(cell_size, max_distance):
    """h = max(cell_size, max_distance / RINGS), float64"""
    return max(np.float64(cell_size), np.float64(max_distance) / np.float64(RINGS))


def cells(x, h):
    """float64 [...] -> int64: floor(x / h) clamped to +- CELL_LIMIT (x / h rounds once)"""
    with np.errstate(over="ignore"):
        return np.clip(np.floor(np.asarray(x, dtype=np.float64) / np.float64(h)), -CELL_LIMIT, CELL_LIMIT).astype(np.int64)


def hash_cells(c):
    """int64 [...,3] cells -> uint32: the hash of the kernels (32-bit wrap-around arithmetic)"""
    c = np.asarray(c).astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    k = ((c[..., 0] * np.uint64(73856093)) & m) ^ ((c[..., 1] * np.uint64(19349663)) & m) ^ ((c[..., 2] * np.uint64(83492791)) & m)
    k ^= k >> np.uint64(16)
    k = (k * np.uint64(0x85EBCA6B)) & m
    k ^= k >> np.uint64(13)
    k = (k * np.uint64(0xC2B2AE35)) & m
    k ^= k >> np.uint64(16)
    return k.astype(np.uint32)


def last_ring(max_distance, h):
    """the last ring the search visits: ceil(max_distance / h) + 1, at most RINGS + 1"""
    return int(min(np.ceil(np.float64(max_distance) / np.float64(h)) + 1.0, RINGS + 1))


def exit_bound(h, s):
    """after ring s >= 1 the search stops when its best d2 is < this"""
    clear = np.float64(h) * (np.float64(s) * np.float64(EXIT_MARGIN))
    return clear * clear


def d2(a, b):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def ring_search(queries, refs, max_distance, cell_size):
    """the search of the kernels, ring by ring with the early exit, in NumPy: float64 [Q,3], [R,3] -> (index [Q] int64, -1 beyond max_distance;
    the number of rings visited [Q]).  Cells that share a bucket only add candidates, which a lexicographic minimum ignores: not simulated."""
    tau = np.float64(max_distance)
    tau2, h = tau * tau, cell_edge(cell_size, max_distance)
    last = last_ring(max_distance, h)
    rc = cells(refs, h)
    out, rings = np.full(len(queries), -1, dtype=np.int64), np.zeros(len(queries), dtype=np.int64)
    for i, q in enumerate(np.asarray(queries, dtype=np.float64)):
        ring = np.abs(rc - cells(q, h)[None]).max(axis=1)  # Chebyshev distance in cells
        dist = d2(q[None], refs)
        best, arg = np.inf, -1
        for s in range(last + 1):
            for j in np.nonzero(ring == s)[0][::-1]:  # (any visiting order: here the highest index first)
                if dist[j] < best or (dist[j] == best and j < arg):
                    best, arg = dist[j], j
            rings[i] = s
            if s >= 1 and best < exit_bound(h, s):
                break
        out[i] = arg if best <= tau2 else -1
    return out, rings


# ---- the energy


def mask_beyond(c):
    """the case's reference with the correspondences beyond max_distance set to -1 (a copy; the other values are the same)"""
    ref = dict(c["ref"])
    if ref["nearest_vertex"] is not None:
        ref["nearest_vertex"] = np.where(ref["near_p"], ref["nearest_vertex"], -1)
    if ref["nearest_point"] is not None:
        ref["nearest_point"] = np.where(ref["near_v"], ref["nearest_point"], -1)
    return ref


def case(V, P, cell_size=0.1, max_distance=0.25, **keywords):
    """``chamfer_reference.case`` (a finite max_distance) with ``cell_size`` and ``ref_grid``: the reference with the masked correspondences"""
    c = cr.case(V, P, max_distance=max_distance, **keywords)
    c["cell_size"] = float(cell_size)
    c["name"] += f" cell_size={cell_size:g}"
    c["ref_grid"] = mask_beyond(c)
    return c


def signed(indices):
    """uint32 bit patterns (as the int32 tensors of the wrappers hold them) -> int64 with NONE as -1"""
    a = np.asarray(indices).astype(np.int64) & 0xFFFFFFFF
    return np.where(a == NONE, -1, a)


def errors(c, terms, loss, vertices_b, nearest_vertex=None, nearest_point=None):
    """``chamfer_reference.errors`` against the masked reference: the indices EQUAL, NONE exactly where the pair is beyond max_distance"""
    ref = c["ref_grid"]
    for name, got in (("nearest_vertex", nearest_vertex), ("nearest_point", nearest_point)):
        if got is not None:
            assert ref[name] is not None and np.array_equal(signed(got), ref[name]), (c["name"], name)
    return cr.errors(c, terms, loss, vertices_b)


def grid_cases():
    """the table the float64 error is measured over and tests/test_chamfer_grid_gpu.py runs: (arguments of case).  V and P through 1, 2, 63 - 65,
    255 - 257 in both roles, n = 1 and 3, the three directions, the weights, the degenerate kinds, the truncations, the cell sizes (far below the
    spacing: h = max_distance / RINGS takes over; about the spacing; above the extent: one cell), 65 537 for the second round of grid_sum"""
    rows = []
    for V, P in ((1, 1), (2, 65), (63, 64), (64, 2), (65, 63), (255, 257), (256, 256), (257, 255), (1, 257), (257, 1)):
        for n in (1, 3):
            rows.append(dict(V=V, P=P, n=n, seed=n, max_distance=0.3, cell_size=0.15))
    rows += [dict(V=300, P=5000, kind="clustered", max_distance=0.05, cell_size=0.01), dict(V=520, P=700, kind="duplicates", n=3, max_distance=0.2, cell_size=0.07),
             dict(V=97, P=400, kind="coincident", max_distance=0.1, cell_size=0.05), dict(V=257, P=600, weights=None, max_distance=0.2, cell_size=0.1),
             dict(V=257, P=600, weights="zeros", n=3, max_distance=0.2, cell_size=0.1), dict(V=400, P=900, max_distance="mid", n=3, cell_size=0.02),
             dict(V=400, P=900, max_distance="below", cell_size=0.02), dict(V=130, P=2100, directions=1, max_distance="mid", cell_size=0.05),
             dict(V=2100, P=130, directions=2, max_distance="mid", cell_size=0.05),
             dict(V=700, P=900, max_distance=0.2, cell_size=1e-6), dict(V=700, P=900, max_distance=0.2, cell_size=0.09), dict(V=700, P=900, max_distance=0.2, cell_size=4.0),
             dict(V=700, P=900, max_distance=3.0, cell_size=0.1, n=3),  # (every pair within max_distance: nothing is NONE)
             dict(V=65537, P=70, max_distance=0.1, cell_size=0.03, seed=1), dict(V=70, P=65537, max_distance=0.1, cell_size=0.03, seed=2)]  # fmt: skip
    return rows


PLACEMENT_CELLS = (0, 1, -1, 3, -3, 7, -8, 1000, -1000, 2**20 + 1, -(2**20) - 1, 2**31 - 3, -(2**31) + 3)
TINY = np.float64(2.0**-1000)


def beside(x):
    """[one ulp below, x, one ulp above]; around 0: +- 2^-1000 (an ulp of 0 is subnormal, where a relative error means nothing)"""
    x = np.float64(x)
    return [-TINY, x, TINY] if x == 0 else [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]


def placement_bases(h):
    """the multiples of h of ``placements`` and an ulp either side, with the clamp and far beyond it: what the GPU test takes as references"""
    cells_ = PLACEMENT_CELLS + (CELL_LIMIT, -CELL_LIMIT, 2**40, 2**60)
    return np.unique(np.concatenate([beside(np.float64(m) * np.float64(h)) for m in cells_]))


def placements(h, tau):
    """adversarial coordinates for the exactness property (one axis; the tests put them on every axis): exact multiples of h and one ulp either
    side, negative ones, pairs exactly tau apart and one ulp either side across a cell face, far out where x / h rounds coarsely, beyond the clamp"""
    h, tau = np.float64(h), np.float64(tau)
    xs = []
    for m in PLACEMENT_CELLS:
        for x in beside(np.float64(m) * h):
            xs += [x] + beside(x + tau) + beside(x - tau) + beside(x + tau / 2)
    for far in (np.float64(CELL_LIMIT) * h, np.float64(2**40) * h, np.float64(2**60) * h):
        for x in beside(far) + beside(-far):
            xs += [x] + beside(x + tau) + beside(x - tau)
    return np.unique(np.array(xs, dtype=np.float64))
