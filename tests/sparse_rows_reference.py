"""Reference for the sparse-row product (include/deodr_hip_subdiv.h, deodr_amd/csrc/dr_subdiv.h): ``y[b, r, :] (= | +=) sum_k vals[k] x[b, cols[k], :]``
over the entries k of row r, restated in NumPy long double -- no code shared with the library --, the matrices the CPU and the GPU tests share, the
instance rule restated, and the case table.

THE BOUND is derived, not measured.  Lane s of the LANES adjacent lanes of a row adds the entries s, s + LANES, ... in order: at most
T = ceil(L / LANES) products and as many additions (L: the length of THAT row); the butterfly over the lanes adds log2 LANES more; a product is one
rounding, or none where the compiler contracts it into the addition.  With the addition of the value y held (``accumulate``) and one rounding to
spare, every element lies within

    (T + log2 LANES + 2) 2^-53 m,      m = sum_k |vals[k] x[b, cols[k], :]| (+ |y0| with accumulate)

of the exact value, plus 2^-24 |value| for the one rounding of a stored float32 (float32 inputs are float32 values, converted exactly).  The
restatement's own error, about L 2^-64 m, is negligible beside it.  A term that goes missing, a lane that is not added or a row stored to the wrong place
is of the order of m / L: twelve orders of magnitude above the bound -- and the rows built from near-cancelling pairs (below) make m itself
10^5 times the value, so that an error which is small beside the VALUE still shows.

The matrices are generated here (:func:`matrix`).  Columns within a row are "sorted", "shuffled" (distinct, in random order) or "repeated" (every
column of a row twice, in random order): the header asks for neither order nor distinctness.  In every fourth row (``r % 4 == 1``) the entries come in
pairs on ONE column with values v and -v (1 + 2^-17 randn): sum |term| is far above |sum term|."""

import functools
import os
import re

import numpy as np

from fititer_reference import longdouble_is_extended  # noqa: F401  (the consumers' skip condition)

LD = np.longdouble
U = 2.0**-53
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "deodr_amd", "csrc")
INCLUDE = os.path.join(HERE, "..", "include")
GOLDEN = os.path.join(HERE, "golden")


# ---- the constants of the sources, the instance rule and the launch geometry ---------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def kernel_constants():
    """``constexpr int | unsigned NAME = value`` (also several in one statement) of dr_subdiv.h and dr_fronthalf.h, DEODR_HIP_MAX_COLORS of deodr_hip.h"""
    found = {}
    for name in ("dr_subdiv.h", "dr_fronthalf.h"):
        with open(os.path.join(CSRC, name)) as f:
            for statement in re.findall(r"constexpr\s+(?:int|unsigned)\s+([^;()]*);", f.read()):
                found.update({k: int(v) for k, v in re.findall(r"(\w+)\s*=\s*(\d+)\s*(?:,|$)", statement.strip())})
    with open(os.path.join(INCLUDE, "deodr_hip.h")) as f:
        found.update({k: int(v) for k, v in re.findall(r"#define\s+(DEODR_HIP_MAX_COLORS)\s+(\d+)", f.read())})
    missing = [k for k in ("SUBDIV_LANES_SHORT", "SUBDIV_LANES_LONG", "SUBDIV_LONG_ROW", "FH_BLOCK", "DEODR_HIP_MAX_COLORS") if k not in found]
    assert not missing, f"constants not found in the sources: {missing}"
    return found


def subdiv_lanes(n_rows, nnz, k=None):
    """``subdiv_lanes`` of dr_subdiv.h: the integer quotient nnz / n_rows against SUBDIV_LONG_ROW"""
    k = k or kernel_constants()
    return k["SUBDIV_LANES_LONG"] if int(nnz) // int(n_rows) >= k["SUBDIV_LONG_ROW"] else k["SUBDIV_LANES_SHORT"]


def ceil_div(a, b):
    return -(-int(a) // int(b))


def geometry(lengths, k=None):
    """the launch of ``deodr_hip_subdiv_apply`` for rows of these lengths -> dict: lanes, rows a wavefront and a workgroup take, workgroups (grid.x),
    wavefronts that hold a live row, the live rows of the last such wavefront, the trips of the longest row's lanes, the empty rows"""
    k = k or kernel_constants()
    lengths = np.asarray(lengths, dtype=np.int64)
    n_rows, nnz = len(lengths), int(lengths.sum())
    lanes = subdiv_lanes(n_rows, nnz, k)
    per_wave, per_group = 64 // lanes, k["FH_BLOCK"] // lanes
    return {"lanes": lanes, "rows_per_wavefront": per_wave, "rows_per_workgroup": per_group, "workgroups": ceil_div(n_rows * lanes, k["FH_BLOCK"]),
            "wavefronts": ceil_div(n_rows, per_wave), "rows_in_last_wavefront": (n_rows - 1) % per_wave + 1, "trips": ceil_div(lengths.max(), lanes),
            "empty": tuple(int(r) for r in np.flatnonzero(lengths == 0))}  # fmt: skip


# ---- the matrices ------------------------------------------------------------------------------------------------------------------------------


def cancelling(row, length):
    """the rows :func:`matrix` builds from near-cancelling pairs"""
    return row % 4 == 1 and length >= 2


def matrix(row_lengths, n_cols, seed, columns="sorted"):
    """-> offsets [rows + 1] uint32, cols [nnz] uint32, vals [nnz] float64 of a matrix whose row r has ``row_lengths[r]`` entries (see the module docstring)"""
    assert columns in ("sorted", "shuffled", "repeated")
    rs = np.random.RandomState(seed)
    cols, vals = [], []
    for row, L in enumerate(int(v) for v in row_lengths):
        pairs = cancelling(row, L)
        distinct = L // 2 + L % 2 if (pairs or columns == "repeated") else L  # the columns drawn; each is then used twice (the last one once if L is odd)
        c = rs.choice(n_cols, distinct, replace=False) if distinct <= n_cols else rs.randint(0, n_cols, distinct)
        v = rs.randn(L)
        if pairs or columns == "repeated":
            c = np.repeat(c, 2)[:L]
        if pairs:
            v[1::2] = -v[0 : L - L % 2 : 2] * (1 + 2.0**-17 * rs.randn(L // 2))
        order = np.argsort(c, kind="stable") if columns == "sorted" else rs.permutation(L)
        cols.append(c[order]), vals.append(v[order])
    offsets = np.concatenate(([0], np.cumsum(np.asarray(row_lengths, dtype=np.int64))))
    cols = np.concatenate(cols).astype(np.uint32) if cols else np.zeros(0, dtype=np.uint32)
    return offsets.astype(np.uint32), cols, np.concatenate(vals).astype(np.float64)


def with_a_zero_entry(offsets, cols, vals):
    """the same matrix with one more entry of value 0.0 at the end of the last row: the same product in exact arithmetic"""
    offsets = offsets.copy()
    offsets[-1] += 1
    return offsets, np.concatenate((cols, cols[:1])), np.concatenate((vals, [0.0]))


def scipy_matrix(offsets, cols, vals, n_cols):
    import scipy.sparse as sp

    return sp.csr_matrix((vals, cols.astype(np.int64), offsets.astype(np.int64)), shape=(len(offsets) - 1, n_cols))  # (not canonical: repeats stay apart)


# ---- the product, in long double ---------------------------------------------------------------------------------------------------------------


def restate(offsets, cols, vals, x, y0=None):
    """``sum_k vals[k] x[b, cols[k], :]`` (+ y0) -> (value, m = sum of |term| (+ |y0|)), both [batch, rows, D] long double.  Rows of one length are
    walked together; within a row the terms are added in the order of the table."""
    offsets, cols = np.asarray(offsets).astype(np.int64), np.asarray(cols).astype(np.int64)
    vals, x = np.asarray(vals).astype(LD), np.asarray(x).astype(LD)
    batch, _n_cols, D = x.shape
    lengths = np.diff(offsets)
    value, m = np.zeros((batch, len(lengths), D), dtype=LD), np.zeros((batch, len(lengths), D), dtype=LD)
    for L in np.unique(lengths[lengths > 0]):
        rows = np.flatnonzero(lengths == L)
        for j in range(int(L)):
            k = offsets[rows] + j
            term = vals[k][None, :, None] * x[:, cols[k], :]
            value[:, rows] += term
            m[:, rows] += np.abs(term)
    if y0 is not None:
        y0 = np.asarray(y0).astype(LD)
        value, m = value + y0, m + np.abs(y0)
    return value, m


def bound(lengths, lanes, m, value, float32):
    """the element-wise bound of the module docstring, [batch, rows, D] float64"""
    lengths = np.asarray(lengths, dtype=np.int64)
    roundings = -(-lengths // lanes) + int(np.log2(lanes)) + 2
    out = roundings[None, :, None].astype(np.float64) * U * np.asarray(m, dtype=np.float64)
    return out + (2.0**-24 * np.abs(np.asarray(value, dtype=np.float64)) if float32 else 0.0)


# ---- the case table ------------------------------------------------------------------------------------------------------------------------------

SHORT_CYCLE = (1, 7, 8, 9, 15, 16, 17, 0)  # either side of one and two trips of 8 lanes, and an empty row
LONG_CYCLE = (63, 64, 65, 127, 128, 129, 1, 0, 1000)  # either side of one and two trips of 64 lanes, one entry, none, sixteen trips
D_SWEEP = (1, 2, 3, 4, 5, 7, 8, 9, 64)  # the compile-time instance (3), whole pieces of 4, a ragged last piece, DEODR_HIP_MAX_COLORS
D_ELSEWHERE = (3, 5)
BATCHES = (1, 3)
MAX_BATCH = 65535  # the limit of grid.y


def cycle(values, n):
    return tuple(values[i % len(values)] for i in range(n))


def _case(name, lengths, n_cols, lanes, workgroups, wavefronts, trips, empty=(), columns="sorted", D=D_ELSEWHERE, batches=BATCHES, **more):
    """one generated case: the instance, the geometry, the trips of the longest row and the empty rows it MUST have (tests/test_sparse_rows_reference.py
    derives them again from the parsed constants)"""
    return dict(name=name, lengths=tuple(lengths), n_cols=n_cols, lanes=lanes, workgroups=workgroups, wavefronts=wavefronts, trips=trips, empty=tuple(empty),
                columns=columns, D=D, batches=batches, **more)  # fmt: skip


def _empty_rows_lengths():
    lengths = [3 + (7 * r) % 10 for r in range(40)]  # 3 .. 12 entries
    for r in (0, 8, 39, *range(16, 24)):  # the first row, the first row of a wavefront, the last row, a whole wavefront
        lengths[r] = 0
    return lengths


def _one_long_row():
    lengths = [0] * 64
    lengths[5], lengths[37] = 1500, 9
    return lengths


def _cycle_empty(values, n):
    return tuple(i for i in range(n) if values[i % len(values)] == 0)


GENERATED = (
    # ---- 8 lanes per row: n_rows either side of one wavefront's 8 rows and one workgroup's 32
    [_case(f"short rows={n}", cycle(SHORT_CYCLE, n), 50, 8, -(-n // 32), -(-n // 8), 3 if n >= 7 else (2 if n >= 4 else 1), _cycle_empty(SHORT_CYCLE, n),
           D=D_SWEEP if n == 33 else D_ELSEWHERE) for n in (1, 7, 8, 9, 31, 32, 33, 65)]
    + [
        _case("short empty rows", _empty_rows_lengths(), 30, 8, 2, 5, 2, (0, 8, 16, 17, 18, 19, 20, 21, 22, 23, 39), whole_wavefront_empty=2),
        _case("short one long row", _one_long_row(), 2000, 8, 2, 8, 188, tuple(r for r in range(64) if r not in (5, 37))),
        _case("short one column", cycle(SHORT_CYCLE, 9), 1, 8, 1, 2, 3, (7,)),
        _case("short 100000 columns", cycle(SHORT_CYCLE, 9), 100000, 8, 1, 2, 3, (7,)),
        _case("short shuffled", cycle(SHORT_CYCLE, 33), 50, 8, 2, 5, 3, _cycle_empty(SHORT_CYCLE, 33), columns="shuffled"),
        _case("short repeated", cycle(SHORT_CYCLE, 33), 50, 8, 2, 5, 3, _cycle_empty(SHORT_CYCLE, 33), columns="repeated"),
    ]
    # ---- a wavefront per row: n_rows either side of a workgroup's 4
    + [_case(f"long rows={n}", cycle(LONG_CYCLE, n), 1200, 64, -(-n // 4), n, 16 if n == 9 else (2 if n >= 3 else 1), _cycle_empty(LONG_CYCLE, n),
             D=D_SWEEP if n == 5 else D_ELSEWHERE) for n in (1, 3, 4, 5, 9)]
    + [
        _case("long empty rows", (0, 200, 0, 0, 64, 1, 0, 500, 128, 0, 65, 0), 600, 64, 3, 12, 8, (0, 2, 3, 6, 9, 11)),
        # ---- the rule, as twins: the same product from the two instances
        _case("twin 319", (31,) * 9 + (40,), 60, 8, 1, 2, 5),
        _case("twin 320", (31,) * 9 + (41,), 60, 64, 3, 10, 1, twin_of="twin 319"),
        # ---- grid.y at its limit
        _case("short batch 65535", (2, 1, 2), 2, 8, 1, 1, 1, D=(1,), batches=(MAX_BATCH,)),
        _case("long batch 65535", (40,), 4, 64, 1, 1, 1, D=(1,), batches=(MAX_BATCH,)),
    ]
)  # fmt: skip

# the hand at three levels (LoopSubdivision(faces, 526, 3)): (rows, shortest row, longest row) of S and of S^T, as tests/test_subdivision_gpu.py pins its own
HAND3 = {False: (33538, 5, 20), True: (526, 421, 1198)}
HAND_CASES = [
    dict(name="hand3", transposed=False, n_cols=526, lanes=8, workgroups=1049, wavefronts=4193, trips=3, empty=(), D=D_ELSEWHERE, batches=BATCHES),
    dict(name="hand3T", transposed=True, n_cols=33538, lanes=64, workgroups=132, wavefronts=526, trips=19, empty=(), D=D_ELSEWHERE, batches=BATCHES),
]
CASES = {c["name"]: c for c in GENERATED + HAND_CASES}
assert len(CASES) == len(GENERATED) + len(HAND_CASES)


@functools.lru_cache(maxsize=None)
def hand3():
    """the three-level subdivision of the hand (its tables are only read)"""
    from deodr_amd.subdivision import LoopSubdivision

    faces = np.load(os.path.join(GOLDEN, "hand_mesh.npz"))["faces"].astype(np.int64)
    return LoopSubdivision(faces, 526, 3)


@functools.lru_cache(maxsize=None)
def tables(name):
    """-> (offsets uint32, cols uint32, vals float64, n_cols) of a case; built once, never written"""
    case = CASES[name]
    if "transposed" in case:
        operator = hand3()._vertices
        m = operator.transposed if case["transposed"] else operator.matrix
        out = m.indptr.astype(np.uint32), m.indices.astype(np.uint32), m.data.astype(np.float64)
    elif "twin_of" in case:
        out = with_a_zero_entry(*tables(case["twin_of"])[:3])
    else:
        out = matrix(case["lengths"], case["n_cols"], seed=sum(case["name"].encode()), columns=case["columns"])
    for a in out:
        a.setflags(write=False)
    return (*out, case["n_cols"])


def inputs(name, batch, D, float32, seed=0):
    """-> x [batch, n_cols, D], y0 [batch, rows, D] as float64 arrays that hold float32 values where ``float32``"""
    offsets, _cols, _vals, n_cols = tables(name)
    rs = np.random.RandomState(seed + 1000 * D + batch % 1000)
    x, y0 = rs.randn(batch, n_cols, D), rs.randn(batch, len(offsets) - 1, D)
    if float32:
        x, y0 = x.astype(np.float32).astype(np.float64), y0.astype(np.float32).astype(np.float64)
    return x, y0
