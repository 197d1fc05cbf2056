"""CPU checks of tests/texture_kernel_cases.py: every case is in the regime it is there for (which pieces go the vector way, the tails, the grids at
and above their caps -- from constants parsed out of dr_texfit.h and ``capped_blocks`` as dr_host.h defines it), and the long-double restatements
agree with the float64 ones of tests/cpu_raster_texture.py."""

import numpy as np
import pytest

import cpu_raster_texture as crt
import texture_kernel_cases as tk
from fititer_reference import longdouble_is_extended

pytestmark = pytest.mark.skipif(not longdouble_is_extended(), reason="np.longdouble is not wider than float64 here: no reference")

K = tk.kernel_constants()


def test_the_constants_and_capped_blocks():
    assert (K["TEX_SMOOTH_BLOCKS"], K["TEX_STEP_BLOCKS"], K["FH_BLOCK"]) == (512, 2048, 256)
    assert [tk.capped_blocks(c, 256, 512) for c in (0, 1, 256, 257, 511 * 256, 511 * 256 + 1, 512 * 256, 512 * 256 + 1, 10**9)] == [1, 1, 1, 2, 511, 512, 512, 512, 512]


def test_rows_shorter_than_a_vector():
    for shape in tk.SHORT_ROWS:
        R = shape[1] * shape[2]
        assert R < 4 and R in (2, 3)
        fast = tk.vector_pieces(shape, 4)
        inside = [tk.rows_inside(p, shape, 4) for p in fast]
        if shape == (3, 2, 1):  # ONE piece, and it starts in the first row: the texture has an interior row and no vector piece
            assert tk.geometry("smooth", shape, 4)["pieces"] == 1 and len(fast) == 0
            continue
        assert len(fast) > 0 and all(wraps >= 1 for _, wraps in inside)  # j wraps inside every such piece
        if R == 2:
            assert all(whole == 2 for whole, _ in inside)  # one piece holds two whole rows
        else:
            assert any(whole == 1 for whole, _ in inside) and any(whole == 0 for whole, _ in inside)  # a whole row and parts of two, or parts of two rows
        # float64: R = VEC (Wt = 2) or VEC + 1
        fast64 = tk.vector_pieces(shape, 8)
        assert len(fast64) > 0 and R - 2 in (0, 1)
    assert len(tk.vector_pieces((5, 2, 1), 4)) == 1 and len(tk.vector_pieces((4, 2, 1), 4)) == 0  # 5 x 2 is the smallest with one
    assert [len(tk.vector_pieces(s, 4)) for s in tk.SHORT_ROWS] == [0, 1, 1, 3, 5]


def test_one_interior_row():
    for shape in tk.ONE_INTERIOR_ROW:
        assert shape[0] == 3
        for itemsize in (4, 8):
            vec, R = 16 // itemsize, shape[1] * shape[2]
            fast = tk.vector_pieces(shape, itemsize)
            assert len(fast) > 0 and all(R <= p * vec and (p + 1) * vec <= 2 * R for p in fast)  # vector pieces, all of them inside row 1
            slow_in_row_1 = [p for p in range(3 * R // vec) if p not in fast and p * vec < 2 * R and (p + 1) * vec > R]
            assert (len(slow_in_row_1) > 0) == (R % vec != 0)  # (the pieces that straddle a row of the border go one by one)


def test_tails():
    seen = set()
    for (shape, itemsize), (tail, last_is_vector) in tk.TAILS.items():
        g = tk.geometry("smooth", shape, itemsize)
        assert g["tail"] == tail == g["N"] % g["VEC"] and tail > 0
        fast = tk.vector_pieces(shape, itemsize)
        assert ((g["pieces"] - 1) in fast) == last_is_vector == (g["R"] <= tail and (g["pieces"] - 1) * g["VEC"] >= g["R"])
        seen.add((itemsize, tail, last_is_vector))
    # every tail with the last whole piece going one by one; going the vector way wherever R <= tail leaves room (R >= 2: not with a tail of 1)
    assert seen == {(4, 1, False), (4, 2, False), (4, 3, False), (4, 2, True), (4, 3, True), (8, 1, False)}


def test_channels_and_misalignment():
    assert sorted({s[2] for s in tk.CHANNELS}) == [2, 5, 64] and sorted({s[1] for s in tk.CHANNELS}) == [2, 7]
    for shape in tk.CHANNELS + tk.MISALIGNED:
        for itemsize in (4, 8):
            fast = tk.vector_pieces(shape, itemsize)
            assert 0 < len(fast) < tk.geometry("smooth", shape, itemsize)["pieces"]  # both ways are taken


def test_the_grids_at_and_above_their_caps():
    for (kernel, itemsize), shapes in tk.CAPS.items():
        trips = []
        for shape in shapes:
            g = tk.geometry(kernel, shape, itemsize, K)
            assert g["grid"] == K["TEX_SMOOTH_BLOCKS" if kernel == "smooth" else "TEX_STEP_BLOCKS"] and g["cap"] == g["grid"] * K["FH_BLOCK"]
            assert g["N"] <= 1 << 30 and g["tail"] == 0
            trips.append(g["trips"])
        at, above, twice = (tk.geometry(kernel, s, itemsize, K) for s in shapes)
        assert at["pieces"] == at["cap"] and above["pieces"] == at["cap"] + 1 and twice["pieces"] > 2 * at["cap"] and trips == [1, 2, 3]
    # below the cap the grid is what the pieces ask for
    for g in (tk.geometry(k, s, i, K) for k in ("smooth", "step") for s in tk.SMALL for i in (4, 8)):
        assert g["grid"] == max(1, -(-g["pieces"] // K["FH_BLOCK"])) < K["TEX_SMOOTH_BLOCKS"] and g["trips"] == 1


@pytest.mark.parametrize("shape", tk.SMALL + tk.MISALIGNED[2:] + [tk.CAPS[("smooth", 8)][1]], ids=str)
def test_the_restatements_agree_with_the_float64_ones(shape):
    """float64 restatements of the same formulas: the gradient within 16 x 2^-53 of the largest |t| term (degree <= 4, one product), the energy
    within N 2^-53 of itself, a step within 8 x 2^-53 of the largest magnitude"""
    u = 2.0**-53
    for float32 in (False, True):
        t, s, g = tk.arrays(shape, float32)
        energy, gradient = tk.smoothness(t, tk.WEIGHT)
        e_np, g_np = crt.np_smoothness(t, tk.WEIGHT)
        assert gradient.dtype == tk.LD and abs(float(energy) - e_np) <= t.size * u * e_np
        assert np.abs(gradient - g_np).max() <= 16 * u * tk.WEIGHT * 4 * np.abs(t).max()
        e64, g64 = tk.smoothness(t, tk.WEIGHT, dtype=np.float64)
        assert abs(e64 - e_np) <= t.size * u * e_np and np.abs(g64 - g_np).max() <= 16 * u * tk.WEIGHT * 4 * np.abs(t).max()
        for kwargs in tk.STEP_PARAMETERS:
            t_ld, s_ld = tk.step(t, s, g, tk.FACTOR, **kwargs)
            t_np, s_np = crt.np_step(t, s, g, tk.FACTOR, **kwargs)
            scale = max(np.abs(t).max(), np.abs(s).max(), tk.FACTOR * np.abs(g).max())
            assert np.abs(t_ld - t_np).max() <= 8 * u * scale and np.abs(s_ld - s_np).max() <= 8 * u * scale, kwargs
            assert np.array_equal(s_ld == 0, s_np == 0)
            if kwargs.get("damping") == 1.0:
                assert not s_ld.any() and np.array_equal(t_ld, t.astype(tk.LD))
            if kwargs.get("clamp") == (0.5, 0.5):
                assert np.all(t_ld == 0.5) and not s_ld.any()


def test_the_step_parameters_cover_what_the_table_is_for():
    p = tk.STEP_PARAMETERS
    assert {None, 0.0} < {k.get("step_max") for k in p} and any((k.get("step_max") or 0) > 0 for k in p)
    assert {0.0, 1.0} <= {k.get("inertia", 0.0) for k in p} and any(k.get("damping") == 1.0 for k in p)
    assert any(k.get("clamp") and k["clamp"][0] == k["clamp"][1] for k in p) and any(k.get("clamp") is None for k in p)
    # an infinite gradient under a positive step_max: clipped, finite
    t, s, g = tk.arrays((5, 7, 3), False)
    g.reshape(-1)[[3, 10]] = np.inf, -np.inf
    for kwargs in p:
        if (kwargs.get("step_max") or 0) > 0:
            t1, s1 = tk.step(t, s, g, tk.FACTOR, **kwargs)
            assert np.isfinite(t1).all() and np.isfinite(s1).all()
            move = (s1.reshape(-1)[[3, 10]] / (1 - kwargs.get("damping", 0.0)) - kwargs.get("inertia", 0.0) * s.reshape(-1)[[3, 10]]) / (1 - kwargs.get("inertia", 0.0))
            if kwargs.get("clamp") is None:
                assert np.allclose(np.asarray(move, dtype=np.float64), [-kwargs["step_max"], kwargs["step_max"]], rtol=1e-12)
