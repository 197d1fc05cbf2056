"""No GPU.  (i) Every case of tests/binning_cases.py is in the regime it is named for, by the restatement of setup_bin_kernel's dealing there.
(ii) The binning rule itself -- deodr_amd/csrc/dr_binning.h, the one copy the kernel and the simulator compile, walked block by block as the kernel
walks a box -- never drops a tile a primitive draws into: the two properties of tests/test_sim.py on a frame of 13 x 10 tiles, where boxes span
several 3 x 3 blocks with every remainder of their sides, over triangles that reach 10^4 pixels beyond the frame, slivers, and integer vertices on
integer pixel centres -- among them an exactly horizontal edge on a pixel row, whose row the non-strict rule of the reference draws beyond the
triangle (shown here from the checker alone; the sample found the kernel dropping those tiles).  (iii) A broken rule is caught: with the
simulator's test-only switch that drops the kept column, or the kept rows, of the non-strict fill rule the triangle property fails, and passes
again with the switch off."""

import ctypes as C

import numpy as np
import pytest

import binning_cases as bc
import sim_util
import test_sim
from test_sim import one_triangle_scene

W, H, TILE = bc.W, bc.H, bc.TILE


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_case_is_in_its_regime(name):
    bc.assert_regime(name)


def test_constants_come_from_the_sources_and_the_simulator_is_built_for_them():
    lib = sim_util.lib()
    assert lib.sim_tile() == bc.K["TILE"] == sim_util.kernel_tile()
    s = one_triangle_scene([[3.2, 4.1], [30.7, 6.3], [12.4, 27.9]])
    with pytest.raises(ValueError):
        sim_util.bin_counts(s, tile=16)
    assert bc.ROUND == 64 * bc.K["BIN_ITEMS"] and bc.dense_T() * 8 > bc.K["SPARSE_MAX"] >= (bc.dense_T() - 1) * 8


def test_every_group_runs_every_channel_instance():
    """setup_bin_kernel<., 2>, <., 3> and <., 4> (NC = 0 takes one channel and more than four): each group has a case of each"""
    for group in bc.GROUPS:
        channels = {bc.built(n)[0][0].nb_colors for n, c in bc.CASES.items() if c.group == group}
        assert {2, 3, 4} <= channels, (group, channels)


def test_restated_dealing_adds_up():
    """the restatement against the simulator's census: the blocks it deals hold every tile the census counts, and at most nine each"""
    for name in ("box_7x5", "rounds_twice_sparse", "bands_long_sparse", "clip_100x77"):
        _views, _sigma, d = bc.built(name)
        for v in d.views:
            binned = (v.tri[:, 0] != 0) & (v.tri[:, 1] != 0)
            blocks = int(v.tri_extra.sum() + binned.sum())
            assert blocks == sum(w.total for w in v.tri_waves) + int(binned.sum())
            assert int(v.tc.sum()) <= 9 * blocks and int(v.tc.sum()) >= int(binned.sum())
            dealt = sum(w.total for b in v.edge_blocks for r in b.waves for w in r)
            assert dealt == int(v.edge_extra.sum()) and int(v.ec.sum()) <= 9 * dealt


# ----------------------------------------------------------------------------------------------------------- the rule


def triangle_sample(seed, n):
    """triangles of a 104 x 80 frame: a third each inside / across / around it, then vertices up to 10^4 pixels outside, slivers of area below
    10^-6, and integer vertices (run with integer_pixel_centers: pixel centres exactly on the edge lines) -> [(vertices, integer_pixel_centers)]"""
    rs = np.random.RandomState(seed)
    size = np.array([W, H])
    plain = [rs.rand(2) * size + (rs.rand(3, 2) - 0.5) * size * rs.choice([0.3, 1.0, 2.5]) for _ in range(n)]
    far = []
    for t in plain[: n // 5]:  # one or two vertices thrown far out, the others stay
        t = t.copy()
        for i in rs.choice(3, rs.randint(1, 3), replace=False):
            t[i] += (rs.rand(2) - 0.5) * 2e4
        far.append(t)
    slivers = []
    for t in plain[: n // 5]:  # the third vertex on the line of the other two, moved off it by less than 2e-6 / length
        u = t[1] - t[0]
        length = max(np.hypot(*u), 1e-3)
        slivers.append(np.array([t[0], t[1], t[0] + rs.rand() * u + np.array([-u[1], u[0]]) / length * rs.rand() * 1e-6 / length]))
    whole = [np.round(t) for t in plain[: n // 3]] + [np.array(v) for v in bc.HORIZONTAL.values()]  # (and an exactly horizontal edge on a pixel row)
    return [(t, False) for t in plain + far + slivers] + [(t, True) for t in whole]


def scene_of(ij, strict, ipc, edgeflags=(True, True, True)):
    s = one_triangle_scene(ij, W=W, H=H, strict=strict, edgeflags=edgeflags)
    s.integer_pixel_centers = bool(ipc)
    return s


def tiles(counts):
    return counts.reshape(-(-H // TILE), -(-W // TILE))


def triangle_property(strict, seed=5, n=600):
    """-> (triangles with a pixel, remainders (ntx % 3, nty % 3) of the boxes of several blocks seen)"""
    lib = sim_util.lib()
    drawn, remainders = 0, set()
    for ij, ipc in triangle_sample(seed, n):
        if abs(np.linalg.det(np.column_stack((ij, np.ones(3))))) == 0:
            continue  # three vertices exactly on a line
        s = scene_of(ij, strict, ipc)
        c, _keep = sim_util.sim_scene(s, sigma=1.0)
        mask = np.zeros((H, W), dtype=np.uint8)
        lib.sim_tri_coverage(C.byref(c), 0, mask.ctypes.data)
        tri_cnt, _ = sim_util.bin_counts(s, sigma=1.0, tile=TILE, exact=True)
        ys, xs = np.nonzero(mask)
        assert np.all(tiles(tri_cnt)[ys // TILE, xs // TILE] == 1), (np.asarray(ij).tolist(), ipc)
        drawn += int(len(ys) > 0)
        box = sim_util.prim_boxes(s, 1.0)[0][0]
        if box[1] and bc.bin_blocks(box[4], box[5]) > 1:
            remainders.add((int(box[4]) % 3, int(box[5]) % 3))
    return drawn, remainders


@pytest.mark.parametrize("strict", [True, False])
def test_binning_keeps_every_tile_a_triangle_draws_into_on_13_by_10_tiles(strict):
    drawn, remainders = triangle_property(strict)
    assert drawn > 400 and remainders == {(a, b) for a in range(3) for b in range(3)}, (drawn, sorted(remainders))


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("sigma", [0.5, 1.0, 3.0])
def test_binning_keeps_every_tile_an_edge_band_draws_into_on_13_by_10_tiles(strict, sigma):
    lib = sim_util.lib()
    pixels, remainders = 0, set()
    for ij, ipc in triangle_sample(11, 200):
        if abs(np.linalg.det(np.column_stack((ij, np.ones(3))))) == 0:
            continue
        for n in range(3):
            s = scene_of(ij, strict, ipc, edgeflags=tuple(i == n for i in range(3)))
            c, _keep = sim_util.sim_scene(s, sigma=sigma)
            mask = np.zeros((H, W), dtype=np.uint8)
            lib.sim_edge_coverage(C.byref(c), 0, n, mask.ctypes.data)
            _, edge_cnt = sim_util.bin_counts(s, sigma=sigma, tile=TILE, exact=True)
            ys, xs = np.nonzero(mask)
            pixels += len(ys)
            assert np.all(tiles(edge_cnt)[ys // TILE, xs // TILE] == 1), (np.asarray(ij).tolist(), ipc, n)
            box = sim_util.prim_boxes(s, sigma)[1][0, n]
            if box[1] and bc.bin_blocks(box[4], box[5]) > 1:
                remainders.add((int(box[4]) % 3, int(box[5]) % 3))
    assert pixels > 10000 and remainders == {(a, b) for a in range(3) for b in range(3)}, (pixels, sorted(remainders))


@pytest.fixture(params=[1, 2], ids=["kept_column_dropped", "kept_rows_dropped"])
def broken_rule(request):
    lib = sim_util.lib()
    lib.sim_set_fault(request.param)
    yield request.param
    lib.sim_set_fault(0)


def test_a_broken_rule_is_rejected(oracle_api, broken_rule):
    """The planted faults: what the property tests are worth.  The switch only exists in the simulator's walk (the kernel has no such switch)."""
    if broken_rule == 1:  # (the 40 x 32 sample of tests/test_sim.py has no horizontal edge on a pixel row: it sees the first fault only)
        with pytest.raises(AssertionError):
            test_sim.test_binning_keeps_every_tile_a_triangle_draws_into(oracle_api, False)
    with pytest.raises(AssertionError):
        triangle_property(False)
    # (the strict rule keeps neither a column nor rows: the switch changes nothing there)
    test_sim.test_binning_keeps_every_tile_a_triangle_draws_into(oracle_api, True)
    triangle_property(True, n=100)


def test_the_reference_draws_the_row_of_a_horizontal_edge_beyond_the_triangle(oracle_api):
    """what the kept rows are for, from the checker alone: under the non-strict rule two of the four triangles of binning_cases.HORIZONTAL have
    pixels outside their half-planes on the row of their horizontal edge, out to the triangle's x_max (the edge on the first row, the third
    vertex to the right) or x_min (on the last row, to the left); their mirror images and the strict rule draw the edge's own pixels at the most"""
    for name, ij in bc.HORIZONTAL.items():
        for strict in (False, True):
            _image, z = (oracle_api.ref() or oracle_api.port()).render(scene_of(np.array(ij), strict, True), 0.0)
            row = int(ij[0][1])
            xs = np.flatnonzero(np.isfinite(z[row]))
            lo, hi = int(min(p[0] for p in ij)), int(max(p[0] for p in ij))
            if strict or name in ("top_left", "bottom_right"):
                assert len(xs) == 0 or (xs.min() >= min(ij[0][0], ij[1][0]) and xs.max() <= max(ij[0][0], ij[1][0])), (name, xs)
            else:
                assert (xs.min(), xs.max()) == ((ij[0][0], hi) if name == "top_right" else (lo, ij[0][0])), (name, xs.min(), xs.max())


def test_the_rule_passes_again_with_the_switch_off(oracle_api):
    test_sim.test_binning_keeps_every_tile_a_triangle_draws_into(oracle_api, False)
    assert triangle_property(False, n=60)[0] > 0
