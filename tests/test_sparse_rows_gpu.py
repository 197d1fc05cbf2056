"""GPU checks of the sparse-row product (``deodr_hip_subdiv_apply``, deodr_amd/csrc/dr_subdiv.h) over the case table of tests/sparse_rows_reference.py:
both instances where the launch geometry or a loop changes, against the long-double restatement, every element within its own derived bound
(the module's docstring).  ``x``, ``y`` and ``vals`` are carved out of NaN-filled buffers and the index tables sit between integer guard words; after a
call every surrounding is intact, ``y`` is written everywhere (an empty row: exactly 0, or exactly what it held with ``accumulate``), the inputs are
bit-unchanged, and a second call into a fresh ``y`` gives the same bits."""

import numpy as np
import pytest
import torch

import sparse_rows_reference as sr
from test_basis_gpu import Arena, host

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not sr.longdouble_is_extended(), reason="np.longdouble is not wider than float64 here: no reference")]

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
GUARD_WORDS, GUARD = 1024, 0x5A5A5A5A


def guarded(table):
    """a uint32 table as an int32 device tensor (the bit patterns) between guard words -> (buffer, tensor)"""
    words = np.ascontiguousarray(table).astype(np.uint32).view(np.int32)
    buffer = torch.full((len(words) + 2 * GUARD_WORDS,), GUARD, dtype=torch.int32, device=DEV)
    t = buffer[GUARD_WORDS : GUARD_WORDS + len(words)]
    t.copy_(torch.as_tensor(words))
    return buffer, t


def intact(buffer, table):
    words = torch.as_tensor(np.ascontiguousarray(table).astype(np.uint32).view(np.int32), device=DEV)
    inside = buffer[GUARD_WORDS : GUARD_WORDS + len(words)]
    return bool((buffer[:GUARD_WORDS] == GUARD).all()) and bool((buffer[GUARD_WORDS + len(words) :] == GUARD).all()) and torch.equal(inside, words)


class Device:
    """the tables of a case on the device, between their guards"""

    def __init__(self, name):
        self.name, self.case = name, sr.CASES[name]
        self.offsets, self.cols, self.vals, self.n_cols = sr.tables(name)
        self.lengths = np.diff(self.offsets.astype(np.int64))
        self.arena = Arena()
        (self.offsets_buffer, self.d_offsets), (self.cols_buffer, self.d_cols) = guarded(self.offsets), guarded(self.cols)
        self.d_vals = self.arena.carve(self.vals.copy())  # (the shared table is read-only)

    def check(self):
        self.arena.check()
        assert intact(self.offsets_buffer, self.offsets) and intact(self.cols_buffer, self.cols), "an index table or its surroundings were written"
        assert np.array_equal(host(self.d_vals), self.vals), "vals were written"


def run_point(dev, dtype, batch, D, accumulate, product=None):
    """one call (and its repetition) with every check of the module's docstring -> (error / bound at worst, the result as float64, its bound)"""
    from deodr_amd import hip_renderer as hr

    float32 = dtype == F32
    x, y0 = sr.inputs(dev.name, batch, D, float32)
    value, m = product if product is not None else sr.restate(dev.offsets, dev.cols, dev.vals, x)
    if accumulate:
        value, m = value + y0.astype(sr.LD), m + np.abs(y0).astype(sr.LD)
    arena = Arena()
    d_x = arena.carve(x, dtype=dtype)
    runs = []
    for _ in range(2):
        y = arena.carve(y0, dtype=dtype) if accumulate else arena.carve(shape=y0.shape, dtype=dtype)  # (not accumulated into: NaN wherever it is not written)
        out = hr.sparse_rows_apply(dev.d_offsets, dev.d_cols, dev.d_vals, d_x, out=y, accumulate=accumulate)
        assert out is y
        runs.append(y)
    torch.cuda.synchronize()
    arena.check(), dev.check()
    assert np.array_equal(host(d_x).astype(np.float64), x), "x was written"
    assert torch.equal(runs[0], runs[1]), "two calls differ"
    got = host(runs[0]).astype(np.float64)
    assert np.isfinite(got).all()
    empty = dev.lengths == 0
    if empty.any():  # written, and exactly: 0, or what y held
        assert np.array_equal(got[:, empty], y0[:, empty] if accumulate else np.zeros_like(got[:, empty]))
    limit = sr.bound(dev.lengths, dev.case["lanes"], m, value, float32)
    err = np.abs(got - value).astype(np.float64)
    assert np.all(err <= limit), (dev.name, dtype, batch, D, accumulate, float((err / np.maximum(limit, 1e-300)).max()))
    return float((err[:, ~empty] / limit[:, ~empty]).max()), got, limit


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(sr.CASES))
def test_case_against_the_long_double_restatement(name, dtype):
    from deodr_amd import hip_renderer as hr

    dev = Device(name)
    case = dev.case
    assert hr.sparse_rows_lanes(len(dev.lengths), len(dev.cols)) == case["lanes"] == sr.subdiv_lanes(len(dev.lengths), len(dev.cols))
    worst = 0.0
    for batch in case["batches"]:
        for D in case["D"]:
            x, _y0 = sr.inputs(name, batch, D, dtype == F32)
            product = sr.restate(dev.offsets, dev.cols, dev.vals, x)  # (shared by the two calls below, never written)
            for accumulate in (False, True):
                worst = max(worst, run_point(dev, dtype, batch, D, accumulate, product)[0])
    print(f"{name} {dtype}: {case['lanes']} lanes, largest error / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_the_twins_either_side_of_the_rule_agree(dtype):
    """the same product from the 8-lane and the 64-lane instance: each within its bound of the reference (the case test), and within the sum of the two
    bounds of one another"""
    a, b = Device("twin 319"), Device("twin 320")
    assert (a.case["lanes"], b.case["lanes"]) == (8, 64)
    for D in (1, 3, 5):
        for accumulate in (False, True):
            _, got_a, limit_a = run_point(a, dtype, 3, D, accumulate)
            _, got_b, limit_b = run_point(b, dtype, 3, D, accumulate)
            apart = np.abs(got_a - got_b)
            print(f"twins {dtype} D={D} accumulate={accumulate}: apart by {float((apart / (limit_a + limit_b)).max()):.3f} of the two bounds")
            assert np.all(apart <= limit_a + limit_b)


@pytest.mark.parametrize("name", ["short rows=33", "long rows=5"])
def test_one_graph_replayed_over_overwritten_values(name):
    from deodr_amd import hip_renderer as hr

    dev = Device(name)
    batch, D = 3, 5
    x0, y0 = sr.inputs(name, batch, D, False)
    arena = Arena()
    d_x, y = arena.carve(x0), arena.carve(shape=y0.shape)
    args = (dev.d_offsets, dev.d_cols, dev.d_vals, d_x)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hr.sparse_rows_apply(*args, out=y)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        hr.sparse_rows_apply(*args, out=y)
    rs = np.random.RandomState(7)
    for _ in range(2):
        vals, x = rs.randn(*dev.vals.shape), rs.randn(*x0.shape)
        dev.d_vals.copy_(torch.as_tensor(vals)), d_x.copy_(torch.as_tensor(x))
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        arena.check()
        value, m = sr.restate(dev.offsets, dev.cols, vals, x)
        limit = sr.bound(dev.lengths, dev.case["lanes"], m, value, False)
        err = np.abs(host(y) - value).astype(np.float64)
        assert np.all(err <= limit) and float(np.abs(host(y)).max()) > 0


def test_the_op_on_the_three_level_tables():
    """``LoopSubdivision(..., 3).apply`` and its autograd transpose: the op path that takes the tables of the hand at three levels"""
    sub = sr.hand3()
    S, ST = (sr.tables(n) for n in ("hand3", "hand3T"))
    rs = np.random.RandomState(5)
    for dtype in (F64, F32):
        x = torch.as_tensor(rs.randn(2, 526, 3)).to(dtype).to(DEV).requires_grad_(True)
        w = torch.as_tensor(rs.randn(2, 33538, 3)).to(dtype).to(DEV)
        y = sub.apply(x)
        (g,) = torch.autograd.grad((y * w).sum(), x)
        assert y.shape == (2, 33538, 3) and g.shape == (2, 526, 3) and y.dtype == g.dtype == dtype
        for what, got, (offsets, cols, vals, _n), source, lanes in (("S x", y, S, x, 8), ("S^T w", g, ST, w, 64)):
            value, m = sr.restate(offsets, cols, vals, host(source).astype(np.float64))
            limit = sr.bound(np.diff(offsets.astype(np.int64)), lanes, m, value, dtype == F32)
            err = np.abs(host(got).astype(np.float64) - value).astype(np.float64)
            print(f"{what} {dtype}: largest error / bound = {float((err / limit).max()):.3f}")
            assert np.all(err <= limit), what
