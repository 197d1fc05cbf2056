"""Every case of tests/texture_window_cases.py is in the regime it is named for -- shown with the CPU checker alone, so that a case that drifts
out of its regime fails here and not silently on the GPU -- and the predictor's small pieces are what the kernel computes."""

import numpy as np
import pytest

import texture_window_cases as twc
from texture_window_cases import CAP_EDGE, CAP_FREE, CASES, EDGE_CASES, K


def checker(api):
    return api.ref() or api.port()


def regime_of(api, s, cap, sigma, tx=0, ty=0):
    _image, z = checker(api).render(s, sigma)
    return twc.tile_regime(s, z, cap, tx, ty), z


def test_capacities_read_from_the_kernel_sources_are_usable():
    assert CAP_FREE > CAP_EDGE >= 32 * 12  # (at least RUNS * NMOM: what the run totals need afterwards)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_in_its_regime(oracle_api, name):
    c = CASES[name]
    s = twc.single_tile_scene(c)
    assert not np.asarray(s.edgeflags).any()
    for cap in (CAP_FREE, CAP_EDGE):
        got, z = regime_of(oracle_api, s, cap, 1.0)
        tex, _fu, _fv, _out, margin = twc.first_texels(s, z)
        assert tex.all() or name.startswith("mixed"), "the rectangle covers the tile"
        assert margin > 1e-3, "u and v stay away from the integers: rounding does not decide a first texel"
        assert twc.matches(got, c.expect[cap]), (name, cap, got)
    assert not twc.chunked_frame(s, 1, 1.0)  # one plain work list: the tile cannot pair, and without an edge it has the whole LDS


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_edge_case_is_in_its_regime(oracle_api, name):
    c = EDGE_CASES[name]
    s = twc.single_tile_scene(c, edge=True)
    assert np.asarray(s.edgeflags).sum() == 1 and bool(np.asarray(s.textured)[np.asarray(s.edgeflags).any(axis=1)].all())  # a flagged textured edge
    got, z = regime_of(oracle_api, s, CAP_EDGE, 1.0)
    tex, _fu, _fv, _out, margin = twc.first_texels(s, z)
    assert not tex[:, 7].any() and tex[:, :7].any(), "the last pixel column is background behind the flagged edge"
    image0 = checker(oracle_api).render(s, 0.0)[0]
    image1 = checker(oracle_api).render(s, 1.0)[0]
    assert np.abs(image1[:, 7] - image0[:, 7]).max() > 1e-3, "the edge is drawn: it blends the textured side over the background"
    assert margin > 1e-3
    assert twc.matches(got, c.expect[CAP_EDGE]), (name, got)


def test_border_cases_touch_and_cross_the_borders(oracle_api):
    s = twc.single_tile_scene(CASES["border_touch"])
    _tex, fu, fv, out, _m = twc.first_texels(s, checker(oracle_api).render(s, 1.0)[1])
    th, tw = s.texture.shape[:2]
    assert fu.min() == 0 and fv.min() == 0 and fu.max() + 1 == tw - 1 and fv.max() + 1 == th - 1 and not out.any()
    s = twc.single_tile_scene(CASES["border_beyond"])
    _tex, fu, fv, out, _m = twc.first_texels(s, checker(oracle_api).render(s, 1.0)[1])
    # out on the low and on the high side of both axes, and pixels inside
    assert out[:, 0, 0].all() and out[:, 7, 0].all() and out[0, :, 1].all() and out[7, :, 1].all() and not out[3, 3].any()
    s = twc.single_tile_scene(CASES["side_65535_far_end"])
    _tex, fu, _fv, out, _m = twc.first_texels(s, checker(oracle_api).render(s, 1.0)[1])
    assert fu.max() == 65535 - 2 and not out.any()
    for name in ("side_65537_u_fits", "side_65537_v_fits"):
        s = twc.single_tile_scene(CASES[name])
        _tex, fu, fv, out, _m = twc.first_texels(s, checker(oracle_api).render(s, 1.0)[1])
        assert max(fu.max(), fv.max()) == 65537 - 2 and not out.any()  # (a first texel that 16 bits do not hold)


def test_row_lengths_cover_every_shape_of_a_flush_pass():
    rows = sorted({c.expect[CAP_FREE]["rowlen"] for n, c in CASES.items() if n.startswith("row")})
    assert rows == [6, 9, 12, 20, 21, 31, 33, 63, 64, 65, 66]
    assert any(64 % r for r in rows if r < 32) and any(64 % r == 0 for r in rows)


def test_flush_lane_split_formula_is_the_integer_division():
    """window_flush finds a lane's row by a float32 reciprocal ("exact for these sizes").  This checks a numpy copy of that formula, not the
    kernel -- no change to window_flush can make it fail: under IEEE float32 arithmetic (what the library's build flags give: no fast-math
    option) the formula is the integer division for every row length below 64.  The kernel's own split is run by the row* cases on the GPU."""
    lane = np.arange(64)
    for rowlen in range(1, 64):
        per_pass, lr, li = twc.flush_lane_split(rowlen)
        assert per_pass == 64 // rowlen and np.array_equal(lr, lane // rowlen) and np.array_equal(li, lane % rowlen), rowlen


def pair_scene():
    """tile A exactly at the capacity of the whole LDS, tile B with mixed quadrants: the second call of the pair meets the table the first one used"""
    return twc.two_tile_scene(CASES[f"cap{CAP_FREE}_c3"].builder, CASES["mixed_c3"].builder, (96, 96))


def test_pair_scene_pairs_up_and_its_tiles_differ(oracle_api):
    s = pair_scene()
    z = checker(oracle_api).render(s, 1.0)[1]
    assert twc.chunked_frame(s, 1, 1.0) and twc.pairs_up(s, z, 1, 1.0, 0, 0)
    assert twc.tile_counts(s, z, 0, 0)[:2] == (2, 2) and twc.tile_counts(s, z, 1, 0)[:2] == (6, 6)  # <= 12 triangles in the two tiles
    assert not twc.pairs_up(s, z, K["TEX_TWO_KERNELS"], 1.0, 0, 0), "from TEX_TWO_KERNELS views on the scan kernel forms no textured pair"
    assert not twc.pairs_up(s, z, 1, 0.0, 0, 0), "sigma = 0: no fused edge tiles, no pairs in a textured scene"
    assert twc.matches(twc.tile_regime(s, z, CAP_FREE, 0, 0), CASES[f"cap{CAP_FREE}_c3"].expect[CAP_FREE])
    assert twc.matches(twc.tile_regime(s, z, CAP_FREE, 1, 0), CASES["mixed_c3"].expect[CAP_FREE])
    assert not np.isfinite(z[:, 16:]).any() and not np.isfinite(z[8:]).any()  # the other 510 tiles are empty
    # in a frame of two tiles the same scene cannot pair: tiny frames are one plain work list
    small = twc.build_scene(16, 8, CASES[f"cap{CAP_FREE}_c3"].builder.pieces(16, 8, 0, 0) + CASES["mixed_c3"].builder.pieces(16, 8, 1, 0), 96, 96)
    assert not twc.pairs_up(small, checker(oracle_api).render(small, 1.0)[1], 1, 1.0, 0, 0)
