"""CPU checks of tests/sparse_rows_reference.py: every case of its table is in the regime it claims (the instance by the restated rule, the wavefronts
and workgroups it straddles, its empty rows, the trips of its longest row -- all from constants parsed out of the sources), the long-double
restatement agrees with SciPy's product in float64 within the bound the GPU tests use, and the restated rule agrees with the pairs
tests/test_subdiv_abi.py pins for the library's."""

import numpy as np
import pytest

import sparse_rows_reference as sr

pytestmark = pytest.mark.skipif(not sr.longdouble_is_extended(), reason="np.longdouble is not wider than float64 here: no reference")

K = sr.kernel_constants()


def test_the_constants_are_the_ones_the_table_was_written_for():
    assert (K["SUBDIV_LANES_SHORT"], K["SUBDIV_LANES_LONG"], K["SUBDIV_LONG_ROW"], K["FH_BLOCK"], K["DEODR_HIP_MAX_COLORS"]) == (8, 64, 32, 256, 64)
    assert K["FH_BLOCK"] // K["SUBDIV_LANES_SHORT"] == 32 and K["FH_BLOCK"] // K["SUBDIV_LANES_LONG"] == 4  # the rows a workgroup takes
    assert max(sr.D_SWEEP) == K["DEODR_HIP_MAX_COLORS"] and sr.MAX_BATCH == 65535


def test_the_restated_rule_agrees_with_the_pinned_pairs():
    """the pairs of tests/test_subdiv_abi.py::test_instance_rule"""
    pinned = {(2098, 9958): 8, (526, 9958): 8, (8386, 67930): 8, (526, 67930): 64, (33538, 340306): 8, (526, 340306): 64, (10, 319): 8, (10, 320): 64}
    for (n_rows, nnz), lanes in pinned.items():
        assert sr.subdiv_lanes(n_rows, nnz) == lanes, (n_rows, nnz)


@pytest.mark.parametrize("name", list(sr.CASES))
def test_every_case_is_in_the_regime_it_claims(name):
    case = sr.CASES[name]
    offsets, cols, vals, n_cols = sr.tables(name)
    lengths = np.diff(offsets.astype(np.int64))
    assert offsets[0] == 0 and offsets[-1] == len(cols) == len(vals) >= 1 and lengths.min() >= 0 and cols.max() < n_cols
    if "transposed" in case:
        assert (len(lengths), lengths.min(), lengths.max()) == sr.HAND3[case["transposed"]] and len(cols) == 340306
    else:
        assert tuple(lengths) == case["lengths"]
    g = sr.geometry(lengths, K)
    claimed = {k: case[k] for k in ("lanes", "workgroups", "wavefronts", "trips", "empty")}
    assert {k: g[k] for k in claimed} == claimed, (g, claimed)
    average = len(cols) / len(lengths)
    assert (average >= K["SUBDIV_LONG_ROW"]) == (case["lanes"] == K["SUBDIV_LANES_LONG"])  # (no case sits where the integer quotient and the ratio part)
    for D in case["D"]:
        assert 1 <= D <= K["DEODR_HIP_MAX_COLORS"]
    assert all(1 <= b <= sr.MAX_BATCH for b in case["batches"])
    # no array of a case is beyond a few megabytes (the largest, 12 MB: 100 000 columns, batch 3, D = 5 in float64)
    assert max(b * max(len(lengths), n_cols) * max(case["D"]) * 8 for b in case["batches"]) <= 16 << 20
    if "whole_wavefront_empty" in case:
        w, per = case["whole_wavefront_empty"], g["rows_per_wavefront"]
        assert not lengths[w * per : (w + 1) * per].any() and lengths[(w - 1) * per : w * per].any() and lengths[(w + 1) * per : (w + 2) * per].any()
    # a generated matrix has what the generator promises
    if "lengths" in case and "twin_of" not in case:
        for row in range(len(lengths)):
            c = cols[offsets[row] : offsets[row + 1]].astype(np.int64)
            if case["columns"] == "sorted":
                assert np.all(np.diff(c) >= 0)
            if sr.cancelling(row, lengths[row]) and lengths[row] % 2 == 0:  # (whatever the order: an odd row has one entry without a partner)
                v = vals[offsets[row] : offsets[row + 1]]
                assert abs(v.sum()) < 1e-3 * np.abs(v).sum()
        if case["columns"] == "shuffled":
            assert any(np.any(np.diff(cols[offsets[r] : offsets[r + 1]].astype(np.int64)) < 0) for r in range(len(lengths)))
        if case["columns"] == "repeated":
            assert any(len(np.unique(cols[offsets[r] : offsets[r + 1]])) < lengths[r] for r in range(len(lengths)))


def test_the_regimes_the_table_is_built_for_are_all_there():
    names = {8: [n for n, c in sr.CASES.items() if c["lanes"] == 8], 64: [n for n, c in sr.CASES.items() if c["lanes"] == 64]}
    rows = lambda lanes, prefix: sorted(len(sr.CASES[n]["lengths"]) for n in names[lanes] if n.startswith(prefix))
    assert rows(8, "short rows=") == [1, 7, 8, 9, 31, 32, 33, 65] and rows(64, "long rows=") == [1, 3, 4, 5, 9]
    for lanes in (8, 64):  # the sweep over D on one case of each instance; a wavefront without a live row next to live ones; the limit of grid.y
        assert sum(sr.CASES[n]["D"] == sr.D_SWEEP for n in names[lanes]) == 1
        assert sum(sr.CASES[n]["batches"] == (sr.MAX_BATCH,) for n in names[lanes]) == 1
    one_long = sr.CASES["short one long row"]
    assert one_long["lengths"][5] == 1500 and one_long["lengths"][37] == 9 and sum(one_long["lengths"]) == 1509 and one_long["trips"] == 188
    assert sr.CASES["long empty rows"]["lengths"] == (0, 200, 0, 0, 64, 1, 0, 500, 128, 0, 65, 0)
    # the twins: one entry of value 0.0 apart, either side of the rule
    a, b = sr.tables("twin 319"), sr.tables("twin 320")
    assert len(a[1]) == 319 and len(b[1]) == 320 and b[2][-1] == 0.0 and np.array_equal(a[1], b[1][:-1]) and np.array_equal(a[2], b[2][:-1])
    assert np.array_equal(a[0][:-1], b[0][:-1]) and b[0][-1] == 320
    assert sr.subdiv_lanes(10, 319) == 8 and sr.subdiv_lanes(10, 320) == 64


@pytest.mark.parametrize("name", list(sr.CASES))
def test_the_restatement_agrees_with_scipy(name):
    """SciPy adds a row's L products one after the other in float64: L roundings of the sum and one of each product, within (L + 2) 2^-53 m -- the
    bound of the module with one lane per row"""
    case = sr.CASES[name]
    offsets, cols, vals, n_cols = sr.tables(name)
    lengths = np.diff(offsets.astype(np.int64))
    A = sr.scipy_matrix(offsets, cols, vals, n_cols)
    batch, D = min(case["batches"][-1], 3), case["D"][-1] if case["D"] != sr.D_SWEEP else 9
    for float32 in (False, True):
        x, y0 = sr.inputs(name, batch, D, float32)
        value, m = sr.restate(offsets, cols, vals, x)
        assert value.dtype == sr.LD and value.shape == (batch, len(lengths), D)
        assert np.all(value[:, lengths == 0] == 0) and np.all(m[:, lengths == 0] == 0)
        got = np.stack([A @ x[b] for b in range(batch)])
        limit = sr.bound(lengths, 1, m, value, False)
        err = np.abs(got - value).astype(np.float64)
        assert np.all(err <= limit), float((err / np.maximum(limit, 1e-300)).max())
        total, m_total = sr.restate(offsets, cols, vals, x, y0)
        assert np.array_equal(total, value + y0.astype(sr.LD)) and np.array_equal(m_total, m + np.abs(y0).astype(sr.LD))
    # the near-cancelling rows: m is far above the value
    rows = [r for r in range(len(lengths)) if sr.cancelling(r, lengths[r]) and lengths[r] % 2 == 0 and "transposed" not in case]
    if rows:
        assert np.median(np.abs(value[:, rows]) / m[:, rows]) < 1e-3
