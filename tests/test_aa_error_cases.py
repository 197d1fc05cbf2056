"""Every case of tests/aa_error_cases.py is in the regime it is named for -- shown on the CPU from the device's binning (tests/sim_util.bin_counts), the
constants of the kernel sources and the restated host formulas, so that a case that drifts out of its regime fails here and not silently on the
GPU --, the repaired checker is finite on it, and where the regime is about an edge's transparency the checker's own diagnostic says so."""

import numpy as np
import pytest

import aa_error_cases as ac
from aa_error_cases import CASES, K, TB


def test_constants_read_from_the_kernel_sources():
    assert K["TILE"] == 8, "the cases are laid out for tiles of 8 x 8 pixels (one wavefront)"
    assert K["PRIO_EDGES"] < TB < K["K_EDGE"] < K["EMAX"] and K["EMAX"] % TB == 0 and K["FIRST_PRIMS"] <= TB and K["EDGE_WAVES"] >= 64


def test_restated_host_formulas():
    """the restatements at the sizes the cases use (values worked out by hand from dr_forward.h: a quarter of the tiles in whole units of
    8 WORK_CHUNK walkers, else a walker per tile; a quarter of those walkers on the head up to 2 048 walkers in all)"""
    assert [ac.fwd_tile_blocks(n, 1) for n in (30, 64, 144, 511, 512, 529, 1056, 2051, 2052, 4096)] == [30, 64, 144, 511, 512, 512, 512, 512, 1024, 1024]
    assert ac.fwd_tile_blocks(16384, 8, True) == 3072 and ac.fwd_tile_blocks(16384, 8, False) == 4096 and ac.fwd_tile_blocks(16384, 7, True) == 4096
    assert [ac.heavy_share_for(v, 512) for v in (1, 3, 4, 16, 17, 32, 33, 64)] == [4, 4, 4, 4, 8, 8, 16, 16]
    assert ac.heavy_share_for(8, 4096, True) == 4 and ac.heavy_share_for(16, 4096, True) == 16
    assert ac.walkers(512, 1) == (512, 128) and ac.walkers(512, 3) == (512, 128) and ac.walkers(511, 1) == (511, 0) and ac.walkers(64, 1) == (64, 0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_in_its_regime(oracle_api, name):
    ac.assert_regime(name)
    for image, z, err, g in ac.reference(oracle_api, name):
        assert np.isfinite(image).all() and np.isfinite(err).all() and np.isfinite(z).any()
        for k, v in g.items():
            assert np.isfinite(v).all(), (name, k)
        assert np.abs(g["ij_b"]).max() > 0 and np.abs(g["colors_b"]).max() + np.abs(g["shade_b"]).max() > 0


def test_what_the_cases_leave_out_the_permuted_rank():
    """Left out, and said so: with G = 512 walkers and a head of 128 the two parts of the list have strides 128 and 384, neither a whole number of
    units of 8 WORK_CHUNK = 512, so every walker of every case takes entry q, q + stride, ... in plain order.  The permuted rank of fwd_tiles
    needs G >= 2 048 (a head of 512): more than 6 144 tiles, a frame of 640 x 640 -- beyond the sizes this suite keeps its cases to."""
    for name in CASES:
        for c in ac.case(name)[2]:
            assert ac.rank_is_permuted(c.G, c.Gh) == (False, False), name
    assert ac.rank_is_permuted(*ac.walkers(6400, 1)) == (True, True) and ac.walkers(6400, 1) == (2048, 512)


def test_views_differ_and_share_a_topology():
    views, _sigma, cs = ac.case("views")
    assert len(views) == 3 and all(np.array_equal(v.faces, views[0].faces) and v.texture is views[0].texture for v in views)
    assert np.allclose(views[2].ij - views[0].ij, [0.74, 0.42]) and len({c.head for c in cs}) > 1  # (the moved views bin differently)


def smallest_T(api, name):
    """smallest |T| the restatement's adjoint divides by on the case (its diagnostic counter; the reference's build has none)"""
    views, sigma, _cs = ac.case(name)
    obs, err_b = ac.inputs(name)
    port = api.port(fixed=True)
    api.min_abs_T()  # reset
    image, z, err = port.render(views[0], sigma, True, obs[0])
    port.grads(views[0], sigma, image, z, None, True, obs[0], err, err_b[0])
    return api.min_abs_T()


def one_ulp_sensitivity(api, name):
    """largest change of the checker's ij_b, relative to its largest entry, when its input err_buffer moves by one ulp (every pixel, up or down)"""
    views, sigma, _cs = ac.case(name)
    obs, err_b = ac.inputs(name)
    image, z, err, g = ac.reference(api, name)[0]
    worst = 0.0
    for way in (np.inf, -np.inf):
        moved = ac.checker(api).grads(views[0], sigma, image, z, None, True, obs[0], np.nextafter(err, way), err_b[0])
        worst = max(worst, float(np.abs(moved["ij_b"] - g["ij_b"]).max() / np.abs(g["ij_b"]).max()))
    return worst


@pytest.mark.parametrize("name", ["replay", "replay_untextured"])
def test_replay_case_replays_and_the_checker_is_still_a_reference_there(oracle_api, name):
    """A pixel centre 2^-21 4 / sqrt(17) = 4.63e-07 pixels from the line of the nearest edge: bwd_err_tile takes its need_replay branch
    (!(T > 1e-6)) and rebuilds the error buffer from the 32 edges of the tile behind it (20 drawn over the pixel, 12 not), across two batch
    boundaries of tm[]; the checker un-blends with a division by that T.  Measured on the checker (never on the kernel): one ulp of its input
    err_buffer moves its ij_b by 1.7e-10 (textured form) / 1.9e-10 (untextured) of the largest entry -- asserted <= 1e-9, a tenth of the 1e-8 the
    kernel is compared at with float64 frames.  (At d = 2^-10, the twin: 8.4e-14.)  Not lower than 2^-22: below d = 2^-24 the checker's own
    noise passes that bound (divergence (5))."""
    T = smallest_T(oracle_api, name)
    assert 2.0**-22 <= T <= 1e-6, T
    assert abs(T - ac.REPLAY_T(ac.REPLAY_D)) < 1e-14, "the smallest T is the near edge's at the pixel centres on its line"
    views, _sigma, cs = ac.case(name)
    assert cs[0].ec[ac.tile_of(*ac.REPLAY_PIXEL, views[0])] == ac.REPLAY_FAR + ac.REPLAY_ASIDE + 1 > 2 * TB  # the replay crosses two batch boundaries
    assert ac.replay_reads_every_batch(views[0].replay_drawn)
    sens = one_ulp_sensitivity(oracle_api, name)
    print(f"{name}: min |T| = {T:.3e}, one-ulp sensitivity of the checker's ij_b = {sens:.2e}")
    assert sens <= 1e-9, sens


def test_unblend_twin_stays_on_the_unblend_branch(oracle_api):
    T = smallest_T(oracle_api, "unblend_twin")
    assert 1e-6 < T < 1e-2 and abs(T - ac.REPLAY_T(ac.UNBLEND_D)) < 1e-12, T
    assert one_ulp_sensitivity(oracle_api, "unblend_twin") <= 1e-11


def test_min_abs_T_leaves_the_defect_switch_alone(oracle_api):
    """a handle from port(fixed=True) computes the repaired adjoint before and after a min_abs_T() call, bit for bit (it used to go through
    port(), which set the process-wide switch of the library back to the defects)"""
    views, sigma, _cs = ac.case("chunked_head_twice_textured")
    obs, err_b = ac.inputs("chunked_head_twice_textured")
    s = views[0]
    port = oracle_api.port(fixed=True)
    image, z, err = port.render(s, sigma, True, obs[0])
    before = port.grads(s, sigma, image, z, None, True, obs[0], err, err_b[0])
    assert oracle_api.min_abs_T() > 0
    after = port.grads(s, sigma, image, z, None, True, obs[0], err, err_b[0])
    stock = oracle_api.port(fixed=False).grads(s, sigma, image, z, None, True, obs[0], err, err_b[0])
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert not np.array_equal(stock["ij_b"], before["ij_b"]) and not np.array_equal(stock["texture_b"], before["texture_b"])  # (the switch does matter here: D2, D1)
    oracle_api.min_abs_T()
    again = oracle_api.port(fixed=False).grads(s, sigma, image, z, None, True, obs[0], err, err_b[0])
    assert np.array_equal(again["ij_b"], stock["ij_b"])  # ... and it leaves the stock setting alone as well


def test_the_emulated_abi_refuses_a_null_image_like_the_library(oracle_api):
    """tests/fake_hip.py keeps the contract of include/deodr_hip.h: antialiase_error with image == NULL is refused with a message that names
    `image`, and the gradient arrays are untouched (the library's own refusal: tests/test_aa_error_gpu.py::test_null_image_is_refused_on_the_host)"""
    import ctypes as C

    import torch

    import fake_hip
    from deodr_amd import hip_renderer as hr
    from hip_util import device_scene

    views, sigma, _cs = ac.case("few_channels_2")
    obs, err_b = ac.inputs("few_channels_2")
    with fake_hip.emulate(oracle_api.ref() or oracle_api.port(), ac.checker(oracle_api)):
        ds = device_scene(views, torch.float64)
        r = hr.HipRasterizer.for_scene(ds)
        obs_t, eb_t = torch.as_tensor(obs), torch.as_tensor(err_b)
        image, _z, _err = r.render(ds, sigma, True, obs_t)
        grads = ds.zero_grads()
        for v in grads.values():
            if v is not None:
                v.fill_(0.625)
        args = (sigma, 1, hr._ptr(obs_t), None, hr._ptr(eb_t), hr._ptr(r.workspace), r.nbytes, 1, None)
        rc = hr.lib().deodr_hip_render_scene_b(C.byref(ds.c_struct(grads)), None, None, None, *args)
        assert rc != 0 and "image" in hr.lib().deodr_hip_last_error().decode()
        assert all(v is None or bool((v == 0.625).all()) for v in grads.values())
        assert hr.lib().deodr_hip_render_scene_b(C.byref(ds.c_struct(grads)), hr._ptr(image), None, None, *args) == 0
        assert not bool((grads["ij_b"] == 0.625).all())
