"""The head of the fused forward's work list (tile_scan_kernel, fwd_tiles) where its shape changes: fewer head entries than head walkers, exactly
as many, more than three rows of them, split copies inside several rows, a frame whose copies SPLIT_BUDGET mostly refuses, a mesh whose
edge-free tiles of FIRST_PRIMS + 1 .. HEAD_TRIS triangles must NOT be head entries, and a frame too small for the chunked walk.

Every case goes through compare_fit_step of tests/test_hip_parity.py (oracle/_ref, the two-call path of the same library) at its tolerances, with
float32 and float64 frames, at 1, 2 and 8 views (the same pose in every view: the views share one topology).  A case asserts the regime it
exists for with a host formula: tests/sim_util.bin_counts (the binning of the device, on the CPU) and the constants of the kernel headers.  The
head count the scan kernel wrote is read back from the workspace header where the case is about which tiles the head holds.

256 x 128 frames have 512 tiles: fwd_tile_blocks gives G = 512 walkers per view (with the divisor 4 and with 6), heavy_share_for a quarter of them
for the head -- 128, the smallest frame that takes the chunked walk."""

import os
import re

import numpy as np
import pytest
import torch

from deodr_amd import scenes
from sim_util import bin_counts
from test_finalize_paths_gpu import fit_step
from test_hip_parity import F32, F64, compare_fit_step

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deodr_amd", "csrc")


def constants():
    found = {}
    for name in ("dr_workspace.h", "dr_forward.h"):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        for stmt in re.findall(r"constexpr\s+int\s+([^;]+);", text):
            found.update({k: v for k, v in re.findall(r"(\w+)\s*=\s*(\w+)\s*(?:,|$)", stmt.strip())})
    value = lambda v: int(v) if v.isdigit() else value(found[v])  # (HEAD_TRIS = TB)
    need = ("TILE", "FIRST_PRIMS", "HEAD_TRIS", "TB", "EMAX", "SCAN_TILES", "SPLIT_BUDGET", "WORK_CHUNK")
    missing = [k for k in need if k not in found]
    assert not missing, f"constants not found in the kernel headers: {missing}"
    return {k: value(found[k]) for k in need}


K = constants()


def walkers(ntiles, n_views):
    """(walkers per view, head walkers per view; 0 head walkers: the list has one class) of a fit step of an untextured scene, launches of at most
    8 192 walkers -- fwd_tile_blocks, heavy_share_for (a quarter) and split_part_for (8 edges per part) of dr_forward.h"""
    unit = 8 * K["WORK_CHUNK"]
    g = -(-(ntiles // (6 if n_views >= 8 else 4)) // unit) * unit
    G = g if 0 < g <= ntiles else ntiles
    assert n_views * G <= 8192
    return G, (G // 4 if G % unit == 0 else 0)


def head_entries(tc, ec, split_part=8):
    """(head tiles, copies of split tiles) the scan kernel lists for a fit step of an untextured scene on a chunked grid"""
    head = (ec > 0) | (tc > K["HEAD_TRIS"])
    want = np.where(head & (ec > K["TB"]) & (ec <= K["EMAX"]), (ec.astype(np.int64) + split_part - 1) // split_part - 1, 0)
    copies = 0
    for b0 in range(0, len(tc), K["SCAN_TILES"]):  # granted in tile order while the requests of the block so far fit its budget
        w = want[b0 : b0 + K["SCAN_TILES"]]
        before = np.cumsum(w) - w
        copies += int(w[before + w <= K["SPLIT_BUDGET"]].sum())
    return int(head.sum()), copies


def device_head_count(views, sigma, pix):
    ds, r, *_ = fit_step(views, sigma, pix=pix)
    assert r.nbytes % ds.n_views == 0
    ws = r.workspace.view(torch.uint8).cpu().numpy()
    return [int(ws[v * (r.nbytes // ds.n_views) :][:64].view(np.uint32)[13]) for v in range(ds.n_views)]  # WsHeader::work_count[0]


_CACHE = {}


def scene(name):
    if name not in _CACHE:
        make, sigma = SCENES[name]
        s = make()
        _CACHE[name] = (s, sigma) + bin_counts(s, sigma, K["TILE"], exact=True)
    return _CACHE[name]


SCENES = {
    "soup40": (lambda: scenes.soup_scene(n_tri=40, width=256, height=128, seed=2), 1.0),
    "soup200": (lambda: scenes.soup_scene(n_tri=200, width=256, height=128, seed=2), 3.0),
    "soup1000": (lambda: scenes.soup_scene(n_tri=1000, width=256, height=128, seed=2), 3.0),
    "sphere256": (lambda: scenes.sphere_scene(size=256, nu=24, n_rings=24), 1.0),
    "soup5": (lambda: scenes.soup_scene(n_tri=5, width=256, height=128, seed=2), 1.0),
    "soup9": (lambda: scenes.soup_scene(n_tri=9, width=256, height=128, seed=18), 1.0),
    "soup64x64": (lambda: scenes.soup_scene(n_tri=40, width=64, height=64, seed=2), 1.0),
}

VIEWS = [1, 2, 8]
PIX = [F32, F64]


@pytest.mark.parametrize("pix", PIX)
@pytest.mark.parametrize("n_views", VIEWS)
def test_more_than_three_rows(oracle_api, n_views, pix):
    s, sigma, tc, ec = scene("soup40")
    G, Gh = walkers(len(tc), n_views)
    tiles, copies = head_entries(tc, ec)
    assert (G, Gh) == (512, 128) and tiles == 400 and copies == 0 and tiles > 3 * Gh  # regime
    compare_fit_step(oracle_api, [s] * n_views, sigma, pix)


@pytest.mark.parametrize("pix", PIX)
@pytest.mark.parametrize("n_views", VIEWS)
def test_split_copies_inside_several_rows(oracle_api, n_views, pix):
    s, sigma, tc, ec = scene("soup200")
    G, Gh = walkers(len(tc), n_views)
    tiles, copies = head_entries(tc, ec)
    # regime: every tile is a head entry, 49 of them have more than one batch of edges, and copies are granted in both blocks of the scan
    assert Gh == 128 and tiles == len(tc) == 512 and int((ec > K["TB"]).sum()) == 49 and int(ec.max()) <= K["EMAX"]
    assert K["SPLIT_BUDGET"] < copies <= 2 * K["SPLIT_BUDGET"]
    compare_fit_step(oracle_api, [s] * n_views, sigma, pix)


@pytest.mark.parametrize("pix", PIX)
@pytest.mark.parametrize("n_views", VIEWS)
def test_split_budget_refuses_most_copies(oracle_api, n_views, pix):
    s, sigma, tc, ec = scene("soup1000")
    G, Gh = walkers(len(tc), n_views)
    tiles, copies = head_entries(tc, ec)
    many = (ec > K["TB"]) & (ec <= K["EMAX"])
    asked = int(((ec[many].astype(np.int64) + 7) // 8 - 1).sum())
    assert Gh == 128 and tiles == 512 and int(many.sum()) == 511 and int(ec.max()) == 89  # regime
    assert 0 < copies <= 2 * K["SPLIT_BUDGET"] and asked > 10 * copies  # regime: the budget refuses most of what is asked for
    compare_fit_step(oracle_api, [s] * n_views, sigma, pix)


@pytest.mark.parametrize("pix", PIX)
@pytest.mark.parametrize("n_views", VIEWS)
def test_short_edge_free_tiles_are_not_head_entries(oracle_api, n_views, pix):
    s, sigma, tc, ec = scene("sphere256")
    G, Gh = walkers(len(tc), n_views)
    tiles, copies = head_entries(tc, ec)
    short = int(((ec == 0) & (tc > K["FIRST_PRIMS"]) & (tc <= K["HEAD_TRIS"])).sum())
    # regime: edge-free tiles of 9 .. 16 triangles exist (11 of them), and the head has a second row without them
    assert (G, Gh) == (512, 128) and short > 0 and tiles > Gh
    compare_fit_step(oracle_api, [s] * n_views, sigma, pix)
    assert device_head_count([s] * n_views, sigma, pix) == [tiles + copies] * n_views  # (with them it would be tiles + copies + short)


@pytest.mark.parametrize("pix", PIX)
@pytest.mark.parametrize("n_views", VIEWS)
@pytest.mark.parametrize("name, expect", [("soup5", 67), ("soup9", 128)])
def test_at_most_one_entry_per_head_walker(oracle_api, name, expect, n_views, pix):
    s, sigma, tc, ec = scene(name)
    G, Gh = walkers(len(tc), n_views)
    tiles, copies = head_entries(tc, ec)
    assert Gh == 128 and (tiles, copies) == (expect, 0) and expect <= Gh  # regime: fewer head entries than head walkers / exactly as many
    compare_fit_step(oracle_api, [s] * n_views, sigma, pix)
    assert device_head_count([s] * n_views, sigma, pix) == [tiles] * n_views


@pytest.mark.parametrize("pix", PIX)
def test_frame_too_small_for_the_chunked_walk(oracle_api, pix):
    s, sigma, tc, ec = scene("soup64x64")
    assert walkers(len(tc), 1) == (64, 0) and int((ec > 0).sum()) > 0  # regime: one walker per tile, one class
    compare_fit_step(oracle_api, s, sigma, pix)
    assert device_head_count([s], sigma, pix) == [0]
