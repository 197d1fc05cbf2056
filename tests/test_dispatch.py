"""Which template instance of a kernel a call runs (deodr_amd/csrc/dr_dispatch.h, compiled for the CPU by tests/sim/dispatch_sim.cpp).

Every instance of a kernel computes the same result, so no parity test can see a call that falls into a slower instance; the instance is the
project's main performance lever (dr_forward.h: NC 0.160 -> 0.150 ms, COMMON 0.144 -> 0.141 ms, the two-kernel textured form 0.84 -> 0.80 ms).
The pins below were recorded from the hand-written launch ladders this header replaced (compiled for the host against stand-ins that record
their own template arguments) and agree with the kernel names in profiles/r06z2_kernel_stats.csv and profiles/fit_weights_kernel_trace.txt;
they are the contract, not a description of the code: a change that moves one of them is a performance change and needs a measurement.
"""

import ctypes
import itertools

import pytest

import sim_util

F32, F64 = 0, 1
# (tile_blocks, heavy_share): the split point of the two-kernel form falls between two groups of eight workgroups of a chunked work list (the
# walkers in whole units of 8 x 64, the head walkers a whole multiple of eight) / does not
SPLIT_OK = [(512, 8), (1024, 16), (4096, 8), (1536, 8)]
SPLIT_BAD = [(500, 4), (512, 3), (512, 128), (64, 1), (1024, 24)]
assert all(tb % 512 == 0 and tb % hs == 0 and (tb // hs) % 8 == 0 for tb, hs in SPLIT_OK)
assert not any(tb % 512 == 0 and tb % hs == 0 and (tb // hs) % 8 == 0 for tb, hs in SPLIT_BAD)


@pytest.fixture(scope="module")
def lib():
    return sim_util.dispatch_lib()


def forward(lib, f64=F32, fused=False, tex=False, fuse_edges=None, clamp=False, weights=False, aa_err=False, C=3, common=True, n_views=1,
            tile_blocks=512, heavy_share=8, capturing=False, sigma_positive=True):  # fmt: skip
    """-> list of instances (FUSED, TEX, CLAMP, NC, COMMON, TEXE, VAR): one, or the two of the two-kernel form."""
    if fuse_edges is None:  # as render_scene_fit sets it: untextured fit steps always, textured ones with sigma > 0
        fuse_edges = fused and (not tex or sigma_positive)
    args = (ctypes.c_int * 13)(f64, fused, tex, fuse_edges, clamp, weights, aa_err, C, common, n_views, tile_blocks, heavy_share, capturing)
    out = (ctypes.c_int * 7)()
    two = lib.dispatch_forward(args, out)
    first = tuple(out)
    return [first, first[:5] + (3,) + first[6:]] if two else [first]


def table(fn, width, *args):
    out = (ctypes.c_int * (width * 64))()
    n = fn(*args, out, 64)
    assert 0 < n <= 64
    rows = [tuple(out[width * i : width * i + width]) for i in range(n)]
    assert len(set(rows)) == n, "an instance is listed twice"
    return rows


# ---------------------------------------------------------------------------------------------------------------- pins

FIT = dict(fused=True)
FORWARD_PINS = {
    # the benchmark's headline step: float32, untextured, C = 4, 1024 x 1024, strict_edge
    "headline": (dict(FIT, C=4), [(1, 0, 0, 4, 1, 0, 0)]),
    "headline 8 views": (dict(FIT, C=4, n_views=8), [(1, 0, 0, 4, 1, 0, 0)]),
    "rgb fit step": (dict(FIT, C=3), [(1, 0, 0, 3, 1, 0, 0)]),
    "side not a multiple of 8": (dict(FIT, C=4, common=False), [(1, 0, 0, 4, 0, 0, 0)]),  # loses COMMON, keeps NC
    "float64 pixels": (dict(FIT, C=4, f64=F64), [(1, 0, 0, 0, 0, 0, 0)]),  # run-time C
    "two channels": (dict(FIT, C=2), [(1, 0, 0, 0, 0, 0, 0)]),
    "textured, sigma > 0, 1 view": (dict(FIT, tex=True, C=3), [(1, 1, 0, 3, 0, 1, 0)]),
    "textured, sigma > 0, 7 views": (dict(FIT, tex=True, C=3, n_views=7), [(1, 1, 0, 3, 0, 1, 0)]),
    "textured, sigma > 0, 8 views": (dict(FIT, tex=True, C=3, n_views=8), [(1, 1, 0, 3, 0, 2, 0), (1, 1, 0, 3, 0, 3, 0)]),
    "textured, sigma > 0, 8 views, capturing": (dict(FIT, tex=True, C=3, n_views=8, capturing=True), [(1, 1, 0, 3, 0, 1, 0)]),
    "textured, sigma > 0, 8 views, split point off": (dict(FIT, tex=True, C=3, n_views=8, heavy_share=3), [(1, 1, 0, 3, 0, 1, 0)]),
    "textured, sigma > 0, 9 views, 4 channels": (dict(FIT, tex=True, C=4, n_views=9, tile_blocks=1024, heavy_share=16), [(1, 1, 0, 0, 0, 2, 0), (1, 1, 0, 0, 0, 3, 0)]),
    "textured, sigma > 0, 8 views, float64": (dict(FIT, tex=True, C=3, n_views=8, f64=F64), [(1, 1, 0, 0, 0, 2, 0), (1, 1, 0, 0, 0, 3, 0)]),
    "textured, sigma = 0, 8 views": (dict(FIT, tex=True, C=3, n_views=8, sigma_positive=False), [(1, 1, 0, 3, 0, 0, 0)]),
    "clamped depth step": (dict(FIT, clamp=True, C=1), [(1, 0, 1, 1, 0, 0, 0)]),
    "clamped rgb step": (dict(FIT, clamp=True, C=3), [(1, 0, 1, 0, 0, 0, 0)]),
    "clamped textured step, 8 views": (dict(FIT, clamp=True, tex=True, C=3, n_views=8), [(1, 1, 1, 0, 0, 1, 0)]),
    "weighted step": (dict(FIT, weights=True, C=3), [(1, 0, 1, 0, 0, 0, 3)]),
    "weighted depth step": (dict(FIT, weights=True, clamp=True, C=1), [(1, 0, 1, 1, 0, 0, 3)]),
    "weighted textured step": (dict(FIT, weights=True, tex=True, C=3), [(1, 1, 1, 0, 0, 1, 3)]),
    "weighted textured step, 8 views": (dict(FIT, weights=True, tex=True, C=3, n_views=8), [(1, 1, 1, 0, 0, 1, 3)]),
    "weighted textured step, sigma = 0": (dict(FIT, weights=True, tex=True, C=3, sigma_positive=False), [(1, 1, 1, 0, 0, 0, 3)]),
    "antialiase_error forward": (dict(aa_err=True, C=3), [(0, 0, 0, 0, 0, 0, 1)]),
    "antialiase_error forward, textured": (dict(aa_err=True, tex=True, C=3), [(0, 1, 0, 0, 0, 0, 1)]),
    "15-channel forward-only frame": (dict(C=15), [(0, 0, 0, 0, 0, 0, 2)]),
    "forward only, C = 3": (dict(C=3), [(0, 0, 0, 3, 0, 0, 0)]),
    "forward only, C = 4": (dict(C=4), [(0, 0, 0, 4, 0, 0, 0)]),
    "forward only, C = 5": (dict(C=5), [(0, 0, 0, 0, 0, 0, 2)]),
    "forward only, C = 1": (dict(C=1), [(0, 0, 0, 0, 0, 0, 0)]),
    "forward only, textured": (dict(tex=True, C=3), [(0, 1, 0, 3, 0, 0, 0)]),
    "forward only, textured, float64": (dict(tex=True, C=3, f64=F64), [(0, 1, 0, 0, 0, 0, 0)]),
}


@pytest.mark.parametrize("name", list(FORWARD_PINS))
def test_forward_instance_of_the_calls_that_matter(lib, name):
    call, want = FORWARD_PINS[name]
    assert forward(lib, **call) == want


def test_per_primitive_and_adjoint_instances_of_the_calls_that_matter(lib):
    out = (ctypes.c_int * 4)()

    def setup(vtx_f64, nc):
        lib.dispatch_setup(vtx_f64, nc, out)
        return tuple(out[:2])

    def finalize(vtx_f64, nc, det=0, prim_tables=0):
        lib.dispatch_finalize(vtx_f64, nc, det, prim_tables, out)
        return tuple(out)

    def adjoint(f64, tex, nc):
        lib.dispatch_adjoint_raster(f64, tex, nc, out)
        return tuple(out[:2])

    # the headline step: float64 vertex arrays, C = 4, 8 views x 20 k triangles (KParams::prim_tables)
    assert setup(1, 4) == (1, 4)  # setup_bin_kernel<true, 4>
    assert finalize(1, 4, prim_tables=1) == (1, 4, 0, 1)  # finalize_kernel<true, 4, false, true>
    assert finalize(1, 4) == (1, 4, 0, 0)  # one view
    assert setup(1, 3) == (1, 3) and finalize(1, 3, prim_tables=1) == (1, 3, 0, 1)
    assert setup(0, 4) == (0, 4) and setup(0, 1) == (0, 0) and setup(1, 15) == (1, 0)
    assert finalize(0, 2, prim_tables=1) == (0, 0, 0, 1)
    assert finalize(1, 15, prim_tables=1) == (1, 0, 0, 0)  # (the table instances are for the staged channel counts)
    assert finalize(1, 4, det=1, prim_tables=1) == (1, 0, 1, 0) and finalize(0, 3, det=1) == (0, 0, 1, 0)
    # the two-call path's adjoint raster kernels <PixT, TEX, NC>
    assert adjoint(F32, 0, 4) == (0, 4) and adjoint(F32, 0, 3) == (0, 3) and adjoint(F32, 0, 1) == (0, 0)
    assert adjoint(F32, 1, 3) == (1, 3) and adjoint(F32, 1, 4) == (1, 0)
    assert adjoint(F64, 0, 4) == (0, 0) and adjoint(F64, 1, 3) == (1, 0)


# --------------------------------------------------------------------------------------------------------------- sweep


def test_table_sizes(lib):
    # the number of compiled instances is build time (and what tools/kernel_resources.sh lists): it does not change unnoticed
    assert len(table(lib.dispatch_forward_table, 7, F32)) == 29
    assert len(table(lib.dispatch_forward_table, 7, F64)) == 16
    assert len(table(lib.dispatch_adjoint_raster_table, 2, F32)) == 5
    assert len(table(lib.dispatch_adjoint_raster_table, 2, F64)) == 2
    assert len(table(lib.dispatch_setup_table, 4)) == 6
    assert len(table(lib.dispatch_finalize_table, 4)) == 14


@pytest.mark.parametrize("f64", [F32, F64])
def test_forward_sweep_selects_only_and_all_table_entries(lib, f64):
    have = set(table(lib.dispatch_forward_table, 7, f64))
    seen = set()
    two_kernel_inputs = 0
    for flags in itertools.product([False, True], repeat=8):
        fused, tex, fuse_edges, clamp, weights, aa_err, common, capturing = flags
        for nc, n_views, (tile_blocks, heavy_share) in itertools.product([1, 2, 3, 4, 5, 6, 15], [1, 2, 7, 8, 9], SPLIT_OK + SPLIT_BAD):
            got = forward(lib, f64, fused, tex, fuse_edges, clamp, weights, aa_err, nc, common, n_views, tile_blocks, heavy_share, capturing)
            assert set(got) <= have, (flags, nc, n_views, tile_blocks, heavy_share, got)
            seen.update(got)
            two = fused and tex and fuse_edges and not clamp and not weights and not capturing and n_views >= 8 and (tile_blocks, heavy_share) in SPLIT_OK
            assert (len(got) == 2) == two, (flags, nc, n_views, tile_blocks, heavy_share, got)
            assert [k[5] for k in got] == [2, 3] if two else got[0][5] == (1 if fused and tex and fuse_edges and nc <= 4 else 0)
            two_kernel_inputs += two
            if f64:
                assert all(k[3] == 0 and k[4] == 0 for k in got)
    assert two_kernel_inputs > 0
    assert seen == have, f"instances no call selects: {sorted(have - seen)}"


def test_other_sweeps_select_only_and_all_table_entries(lib):
    out = (ctypes.c_int * 4)()
    channels = [1, 2, 3, 4, 5, 6, 15]
    for f64 in (F32, F64):
        have, seen = set(table(lib.dispatch_adjoint_raster_table, 2, f64)), set()
        for tex, nc in itertools.product([0, 1], channels):
            lib.dispatch_adjoint_raster(f64, tex, nc, out)
            seen.add(tuple(out[:2]))
        assert seen == have
    have, seen = set(table(lib.dispatch_setup_table, 4)), set()
    for vtx_f64, nc in itertools.product([0, 1], channels):
        lib.dispatch_setup(vtx_f64, nc, out)
        seen.add(tuple(out))
    assert seen == have
    have, seen = set(table(lib.dispatch_finalize_table, 4)), set()
    for vtx_f64, nc, det, prim_tables in itertools.product([0, 1], channels, [0, 1], [0, 1]):
        lib.dispatch_finalize(vtx_f64, nc, det, prim_tables, out)
        seen.add(tuple(out))
    assert seen == have
