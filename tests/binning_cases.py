"""Scenes for the binning of setup_bin_kernel (deodr_amd/csrc/dr_setup.h, the rule in dr_binning.h) and for the tile lists it writes where their
paths change, and a restatement of how the kernel deals a launch's binning work over its wavefronts.  No GPU: tests/test_binning_cases.py proves
every case to be in the regime it is named for, tests/test_binning_gpu.py asserts it again and runs them.

The restatement (`dealing`) reads its constants from the kernel sources, never copied.  Which tiles a primitive is binned into comes from the
simulator (tests/sim/tile_sim.cpp, which compiles the kernel's own rule); what is restated here is the geometry of the launch: a triangle every
`sparse` lanes of the triangle wavefronts, each lane's `extra` 3 x 3 blocks (all but the first, which the triangle's own thread bins), the
wavefront's total and the rounds of 64 BIN_ITEMS blocks bin_rest needs for it; the flagged slots of an edge block compacted and taken PRIM_BLOCK at
a time, every block of a band dealt.  The device keeps no record of which lane served which block: if the kernel's split changes, this has to follow.

A scene is a list of pieces (tests/texture_window_cases.py: every triangle has vertices, a constant depth and colours of its own; depths are
distinct, so no depth tie decides a pixel).  Frames are 104 x 80 pixels (13 x 10 tiles) unless a case says otherwise."""

import copy
import os
import re
from types import SimpleNamespace

import numpy as np

import sim_util
import texture_window_cases as twc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deodr_amd", "csrc")


def constants():
    """The numbers of the kernel sources the cases are placed at: every `constexpr int / long long NAME = number` of the four files, and the lanes
    per triangle of a small launch (the value the host gives KParams::setup_sparse)"""
    found = {}
    for name in ("dr_workspace.h", "dr_setup.h", "dr_forward.h", "dr_kernels.hip"):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        for stmt in re.findall(r"constexpr\s+(?:int|long long)\s+([^;()\[\]]+);", text):
            found.update({k: v for k, v in re.findall(r"(\w+)\s*=\s*(\w+)\s*(?:,|$)", stmt.strip())})
        m = re.search(r"p\.setup_sparse\s*=[^;?]*<=\s*SPARSE_MAX\s*\?\s*(\d+)\s*:\s*1\s*;", text)
        if m:
            found["SPARSE"] = m.group(1)
    value = lambda v: int(v) if v.isdigit() else value(found[v])
    need = ("PRIM_BLOCK", "EDGE_SLOTS", "BIN_ITEMS", "K_TRI", "K_EDGE", "TB", "EMAX", "SPARSE_MAX", "TILE", "SPARSE")
    missing = [k for k in need if k not in found]
    assert not missing, f"constants not found in the kernel sources: {missing}"
    return {k: value(found[k]) for k in need}


K = constants()
TILE, K_TRI, K_EDGE, TB, EMAX = K["TILE"], K["K_TRI"], K["K_EDGE"], K["TB"], K["EMAX"]
ROUND = 64 * K["BIN_ITEMS"]  # blocks one round of bin_rest deals over a wavefront
W, H = 104, 80
TX, TY = W // TILE, H // TILE
assert TILE == 8 and K["PRIM_BLOCK"] % 64 == 0 and 64 % K["SPARSE"] == 0, "the cases are laid out for 8 x 8 tiles and wavefronts of 64"


# ------------------------------------------------------------------------------------------------------ the dealing, restated


def bin_blocks(ntx, nty):
    """3 x 3 blocks of a box of ntx x nty tiles"""
    return ((ntx + 2) // 3) * ((nty + 2) // 3)


def rounds_of(total):
    """rounds of bin_rest's loop `for (base = 0; base < total; base += 64 * BIN_ITEMS)`"""
    return -(-total // ROUND)


def wave(lanes, extra):
    return SimpleNamespace(lanes=[int(v) for v in lanes], extra=[int(v) for v in extra], total=int(np.sum(extra)), rounds=rounds_of(int(np.sum(extra))))


def dealing(views, sigma):
    """What setup_bin_kernel makes of one launch -> namespace: T, n_views, dense (one triangle per lane, EDGE_SLOTS slots per thread of an edge block)
    or sparse, and per view (list `views`): tri, edge (the boxes of sim_util.prim_boxes), tri_waves (per triangle wavefront: the lanes that hold a
    triangle, each one's extra, the total, bin_rest's rounds), edge_blocks (per block: n_flagged, rounds of PRIM_BLOCK, and waves[round][wavefront]
    like tri_waves), tc, ec per tile, tri_pooled / edge_pooled (pairs in the spill pools), work (tiles with a primitive), edge_tiles"""
    T, n = len(np.asarray(views[0].faces)), len(views)
    sparse = K["SPARSE"] if T * n <= K["SPARSE_MAX"] else 1
    per_thread = 1 if sparse > 1 else K["EDGE_SLOTS"]
    out = SimpleNamespace(T=T, n_views=n, dense=sparse == 1, sparse=sparse, views=[])
    for s in views:
        tri, edge = sim_util.prim_boxes(s, sigma)
        t_extra = np.where((tri[:, 0] != 0) & (tri[:, 1] != 0), bin_blocks(tri[:, 4], tri[:, 5]) - 1, 0)
        e_extra = np.where((edge[..., 0] != 0) & (edge[..., 1] != 0), bin_blocks(edge[..., 4], edge[..., 5]), 0).reshape(-1)
        tri_waves = []
        for w0 in range(0, T * sparse, 64):
            lanes = [l for l in range(64) if (w0 + l) % sparse == 0 and (w0 + l) // sparse < T]
            tri_waves.append(wave(lanes, [t_extra[(w0 + l) // sparse] for l in lanes]))
        flagged = (np.asarray(s.edgeflags).reshape(-1) != 0) & (sigma > 0)
        span = K["PRIM_BLOCK"] * per_thread
        edge_blocks = []
        for b0 in range(0, 3 * T, span):
            slots = b0 + np.flatnonzero(flagged[b0 : b0 + span])
            rounds = []
            for r0 in range(0, len(slots), K["PRIM_BLOCK"]):
                chunk = slots[r0 : r0 + K["PRIM_BLOCK"]]
                rounds.append([wave(range(len(chunk[q : q + 64])), e_extra[chunk[q : q + 64]]) for q in range(0, len(chunk), 64)])
            edge_blocks.append(SimpleNamespace(n_flagged=len(slots), rounds=len(rounds), waves=rounds))
        tc, ec = sim_util.bin_counts(s, sigma, TILE, exact=True)
        tc, ec = tc.astype(np.int64), ec.astype(np.int64)
        out.views.append(SimpleNamespace(
            tri=tri, edge=edge, tri_extra=t_extra, edge_extra=e_extra, tri_waves=tri_waves, edge_blocks=edge_blocks, tc=tc, ec=ec,
            tri_pooled=int(np.maximum(0, tc - K_TRI).sum()), edge_pooled=int(np.maximum(0, ec - K_EDGE).sum()),
            work=int(((tc > 0) | (ec > 0)).sum()), edge_tiles=int((ec > 0).sum()),
        ))  # fmt: skip
    return out


def census(d):
    """what deodr_amd.hip_renderer.tile_census reads back after a forward of the launch: (tiles with a primitive, tiles with silhouette edges)"""
    return sum(v.work for v in d.views), sum(v.edge_tiles for v in d.views)


# ---------------------------------------------------------------------------------------------------------------- pieces

ALL_EDGES = ((0, 1), (1, 2), (2, 0))


def box_tri(tx0, ty0, ntx, nty, jitter=0.0, flag=(), uvmap=None):
    """a triangle whose box of tiles is (tx0, ty0, ntx, nty): vertices more than a pixel inside the box's corner tiles (`dealing` asserts the box)"""
    x0, y0, x1, y1 = tx0 * TILE, ty0 * TILE, (tx0 + ntx) * TILE - 1, (ty0 + nty) * TILE - 1
    j = jitter
    return twc.tri([(x0 + 1.3 + j, y0 + 1.2 + j), (x1 - 1.4 - j, y0 + 2.1 + j), (x0 + 2.2 + j, y1 - 1.3 - j)], uvmap, flag)


def boxes_by_extra(tx, ty):
    """{extra: (ntx, nty)}: for every number of blocks a box can have in a frame of tx x ty tiles, a box of extra + 1 blocks whose sides are no
    multiples of three tiles where the frame allows it"""
    out = {}
    for nby in range(1, -(-ty // 3) + 1):
        for nbx in range(1, -(-tx // 3) + 1):
            out.setdefault(nbx * nby - 1, (min(3 * nbx - 2, tx), min(3 * nby - 1 if nby > 1 else 1, ty)))
    return out


def tiny(i):
    """filler: a triangle between four pixel centres (no pixel of its own: off the screen for the kernel, or one rejected tile)"""
    x, y = 3 + 7 * (i % 14), 2 + 5 * ((i // 14) % 15)
    return twc.tri([(x + 0.2, y + 0.2), (x + 0.7, y + 0.3), (x + 0.3, y + 0.8)])


def small(i):
    """filler with pixels: a triangle of ~3 pixels inside one tile"""
    x, y = TILE * (i % TX) + 2, TILE * ((i // TX) % TY) + 2
    return twc.tri([(x - 0.3, y - 0.4), (x + 2.6, y + 0.3), (x + 0.4, y + 2.7)])


def culled(i):
    t = small(i)
    t.culled = True
    return t


def offscreen(i, flag=(), w=W, h=H):
    """drawn (front-facing) but wholly outside the frame, on the side i % 4"""
    cx, cy = [(-30.0, 40.0), (w + 30.0, 40.0), (50.0, -30.0), (50.0, h + 30.0)][i % 4]
    return twc.tri([(cx - 8.3, cy - 7.1), (cx + 9.2, cy - 3.4), (cx - 2.1, cy + 8.6)], flag=flag)


def filler(i):
    return (tiny, culled, offscreen, tiny)[i % 4](i)


def build(pieces, C=3, strict=True, width=W, height=H, seed=0):
    """twc.build_scene, then: the pieces marked `culled` turned to face away, the fill rule, no texture unless a piece is textured"""
    textured = any(p.uvmap is not None for p in pieces)
    s = twc.build_scene(width, height, pieces, 24, 24, C=C, seed=seed)
    ij = np.array(s.ij).reshape(-1, 3, 2)
    for t, p in enumerate(pieces):
        if getattr(p, "culled", False):
            ij[t] = ij[t][[0, 2, 1]]
    s.ij = ij.reshape(-1, 2)
    s.strict_edge = bool(strict)
    if not textured:
        s.texture = np.zeros((0, 0))
    return s


def dense_T(n_views=8):
    """triangles per view of the smallest launch of n_views views above SPARSE_MAX"""
    return K["SPARSE_MAX"] // n_views + 1


def padded(pieces, T):
    return list(pieces) + [filler(i) for i in range(len(pieces), T)]


def moved(s, v):
    """view v of one topology: `s` moved by 1/64 v pixels (the boxes stay: box_tri keeps a pixel's distance from its tiles' borders)"""
    c = copy.copy(s)
    c.ij = np.asarray(s.ij) + 0.015625 * v
    return c


# ----------------------------------------------------------------------------------------------------------------- cases
#
# name -> namespace(group, make: () -> list of views, sigma, check: (views, dealing) -> None, asserting the regime)

CASES = {}


def case(name, group, make, sigma, check):
    assert name not in CASES
    CASES[name] = SimpleNamespace(name=name, group=group, make=make, sigma=sigma, check=check)


def tri_box_is(d, view, k, box, extra):
    row = d.views[view].tri[k]
    assert (row[0], row[1]) == (1, 1) and tuple(row[2:]) == box and d.views[view].tri_extra[k] == extra, (view, k, row.tolist(), box, extra)


# 1. box sizes: one drawn triangle, every edge flagged; sparse one by one, and the eight as the views of one dense launch
BOXES = {"1x1": ((5, 4, 1, 1), 0), "3x3": ((4, 3, 3, 3), 0), "4x1": ((3, 5, 4, 1), 1), "1x4": ((6, 2, 1, 4), 1), "4x4": ((2, 1, 4, 4), 3),
         "6x6": ((5, 3, 6, 6), 3), "7x5": ((1, 2, 7, 5), 5), "13x10": ((0, 0, 13, 10), 19)}  # fmt: skip


def _check_box(name, dense):
    def check(views, d):
        assert d.dense == dense
        names = list(BOXES) if dense else [name]
        for v, n in enumerate(names):
            tri_box_is(d, v, 0, *BOXES[n])
            assert d.views[v].tri_waves[0].lanes[0] == 0 and d.views[v].tri_waves[0].extra[0] == BOXES[n][1]
            if not dense:  # the triangle alone: the wavefront's total is its extra, one round at the most; its bands are blocks of their own
                assert d.views[v].tri_waves[0].total == BOXES[n][1] and d.views[v].tri_waves[0].rounds == (1 if BOXES[n][1] else 0)
                assert d.views[v].edge_blocks[0].n_flagged == 3 and d.views[v].edge_blocks[0].rounds == 1
            else:  # extra == 0 lanes between the owners: the filler
                assert d.T == dense_T() and sum(1 for e in d.views[v].tri_waves[0].extra if e == 0) >= 60
    return check


for _name, (_box, _extra) in BOXES.items():
    for _C in (3,) if _name not in ("7x5", "4x4") else (3, 2 if _name == "7x5" else 4):
        case(f"box_{_name}" + (f"_c{_C}" if _C != 3 else ""), "boxes", (lambda b=_box, C=_C: [build([box_tri(*b, flag=ALL_EDGES)], C=C)]), 1.0,
             _check_box(_name, False))  # fmt: skip
case("box_all_dense", "boxes", lambda: [build(padded([box_tri(*b, flag=ALL_EDGES)], dense_T())) for b, _e in BOXES.values()], 1.0,
     _check_box(None, True))  # fmt: skip


# 2. rounds of bin_rest: the first triangle wavefront's extras total ROUND - 1, ROUND, ROUND + 1 and more than 2 ROUND
def rounds_pieces(total, lanes, tx=TX, ty=TY):
    """`lanes` pieces (one per lane of the first wavefront that can hold a triangle) whose extras sum to `total`: the widest at the first and
    the last lane, a culled, an off-screen and a tiny triangle right behind the first, the others greedily, then triangles of one tile"""
    boxes = boxes_by_extra(tx, ty)
    extras, left = [], total
    while left > 0:
        e = max(e for e in boxes if e <= left)
        extras.append(e)
        left -= e
    assert len(extras) + 3 <= lanes and len(extras) >= 2, (total, lanes, extras)
    extras.sort(reverse=True)
    first, last, mid = extras[0], extras[1], extras[2:]

    def wide(e, i):
        ntx, nty = boxes[e]
        return box_tri((i * 3) % (tx - ntx + 1), (i * 2) % (ty - nty + 1), ntx, nty, jitter=0.01 * i)

    pieces = [wide(first, 0), culled(1), offscreen(1, w=tx * TILE, h=ty * TILE), tiny(3)] + [wide(e, 4 + i) for i, e in enumerate(mid)]
    pieces += [small(i) for i in range(len(pieces), lanes - 1)] + [wide(last, lanes - 1)]
    return pieces


def _check_rounds(total, dense):
    def check(views, d):
        assert d.dense == dense
        for v in d.views:
            w = v.tri_waves[0]
            assert len(w.lanes) == (64 if dense else 64 // K["SPARSE"]) and w.lanes[-1] == (63 if dense else 64 - K["SPARSE"])
            assert w.total == total and w.rounds == (1 if total <= ROUND else -(-total // ROUND)), (w.total, w.rounds)
            assert w.extra[0] == max(w.extra) > 0 and w.extra[-1] > 0 and w.extra[1:4] == [0, 0, 0]
            assert (v.tri[1, 0], tuple(v.tri[2, :2]), v.tri[3, 0]) == (0, (1, 0), 1)  # culled; drawn and off the screen; tiny but drawn
            assert int(v.tc.max()) <= K_TRI  # (this group is about the dealing: no pool)
    return check


# (16 lanes of a sparse wavefront hold at most 13 boxes of the 20 blocks of the 104 x 80 frame next to the three without work: the sparse case of more
# than 2 ROUND blocks has a frame of 16 x 13 tiles)
BIG_TX, BIG_TY = 16, 13
assert 13 * (bin_blocks(TX, TY) - 1) <= 2 * ROUND < 13 * (bin_blocks(BIG_TX, BIG_TY) - 1)
ROUND_TOTALS = {"below": ROUND - 1, "exact": ROUND, "above": ROUND + 1, "twice": 2 * ROUND + 4}


def sparse_rounds(total, C=3):
    big = total > 2 * ROUND
    tx, ty = (BIG_TX, BIG_TY) if big else (TX, TY)
    return [build(rounds_pieces(total, 64 // K["SPARSE"], tx, ty), C=C, width=tx * TILE, height=ty * TILE)]


for _name, _total in ROUND_TOTALS.items():
    case(f"rounds_{_name}_sparse", "rounds", (lambda t=_total: sparse_rounds(t)), 1.0, _check_rounds(_total, False))
    case(f"rounds_{_name}_dense", "rounds",
         (lambda t=_total: [moved(build(padded(rounds_pieces(t, 64), dense_T())), v) for v in range(8)]), 1.0, _check_rounds(_total, True))  # fmt: skip
case("rounds_above_sparse_c2", "rounds", lambda: sparse_rounds(ROUND + 1, C=2), 1.0, _check_rounds(ROUND + 1, False))
case("rounds_twice_sparse_c4", "rounds", lambda: sparse_rounds(2 * ROUND + 4, C=4), 1.0, _check_rounds(2 * ROUND + 4, False))


# 3. the non-strict rule: a triangle that leaves the frame on the right, its kept column ntx - 1 in a block bin_rest deals; the strict twin
LEAVES_RIGHT = [(60.3, 20.2), (140.7, 35.1), (70.2, 60.4)]


def _check_kept_column(strict):
    def check(views, d):
        s, v = views[0], d.views[0]
        assert bool(s.strict_edge) == strict and v.tri[0, 0] == 1 and v.tri[0, 1] == 1
        tx0, ty0, ntx, nty = (int(q) for q in v.tri[0, 2:])
        assert ntx > 3 and tx0 + ntx == TX and (ntx - 1) // 3 > 0, "the kept column lies in a later block"
        lib = sim_util.lib()
        lib.sim_set_fault(1)
        try:
            tc_dropped, _ec = sim_util.bin_counts(s, 1.0, TILE, exact=True)
        finally:
            lib.sim_set_fault(0)
        lost = np.flatnonzero(tc_dropped.astype(np.int64) != v.tc)
        if strict:
            assert len(lost) == 0
        else:  # tiles the rejection alone would drop, all of them in the box's last column
            assert len(lost) > 0 and all(t % TX == TX - 1 for t in lost), lost
    return check


for _strict in (False, True):
    for _C in (3,) if _strict else (3, 2, 4):
        case(("strict_twin" if _strict else "kept_column") + (f"_c{_C}" if _C != 3 else ""), "non_strict",
             (lambda st=_strict, C=_C: [build([twc.tri(LEAVES_RIGHT, flag=ALL_EDGES), small(17), small(40)], C=C, strict=st)]), 1.0,
             _check_kept_column(_strict))  # fmt: skip


# 3b. the same rule and an exactly horizontal edge on a pixel row (integer vertices, integer pixel centres): the reference draws that row from the
# triangle's other edge out to x_max, or from x_min (floor_div / ceil_div with a = 0 and a zero numerator leave the bound unclipped), over tiles
# every half-plane test rejects -- where the edge is on the triangle's first row and the third vertex to the right, or on its last row and the
# third vertex to the left (tests/test_binning_cases.py shows it from the checker); the kernel keeps the rows of tiles for every horizontal edge.
# The four triangles: the edge on the first / the last row of the triangle, the third vertex to the right / left.
HORIZONTAL = {"top_right": [(20.0, 16.0), (33.0, 16.0), (90.0, 41.0)], "top_left": [(84.0, 18.0), (71.0, 18.0), (12.0, 45.0)],
              "bottom_right": [(15.0, 60.0), (31.0, 60.0), (88.0, 27.0)], "bottom_left": [(92.0, 63.0), (70.0, 63.0), (9.0, 30.0)]}  # fmt: skip


def _check_horizontal(strict):
    """(no edge is flagged: with integer vertices on integer pixel centres the reference's own adjoint of a silhouette edge can be NaN)"""
    def check(views, d):
        s, v = views[0], d.views[0]
        assert bool(s.strict_edge) == strict and s.integer_pixel_centers and (v.tri[:4, :2] == 1).all()
        lib = sim_util.lib()
        lib.sim_set_fault(2)
        try:
            tc_dropped, _ec = sim_util.bin_counts(s, 1.0, TILE, exact=True)
        finally:
            lib.sim_set_fault(0)
        lost = np.flatnonzero(tc_dropped.astype(np.int64) != v.tc)
        if strict:
            assert len(lost) == 0
        else:  # tiles the rejection alone would drop, in the first or last row of tiles of a box of several blocks
            rows = {(int(b[3]), int(b[3] + b[5] - 1)) for b in v.tri[:4]}
            assert len(lost) >= 4 and all(any(t // TX in r for r in rows) for t in lost) and (v.tri_extra[:4] > 0).all(), lost
    return check


for _strict in (False, True):
    for _C in (3,) if _strict else (3, 2, 4):
        case(("horizontal_strict_twin" if _strict else "horizontal_edge_row") + (f"_c{_C}" if _C != 3 else ""), "non_strict",
             (lambda st=_strict, C=_C: [build([twc.tri(v) for v in HORIZONTAL.values()] + [small(17)], C=C, strict=st)]), 1.0,
             _check_horizontal(_strict))  # fmt: skip


# 4. clipping: boxes clamped at each border and at two at once, a triangle wholly outside on each side; a frame of 100 x 77
def clip_pieces(w, h):
    across = [[(-20.4, 30.3), (14.6, 22.1), (9.2, 50.7)], [(w - 15.3, 25.2), (w + 30.6, 33.4), (w - 9.1, 58.8)],
              [(40.3, -25.2), (66.7, 11.4), (30.1, 13.2)], [(35.2, h - 14.3), (70.8, h - 9.6), (50.4, h + 28.1)],
              [(-12.3, -9.4), (21.6, 6.2), (5.3, 19.7)], [(w - 18.2, h - 6.3), (w + 9.4, h - 20.7), (w + 4.1, h + 12.6)]]  # fmt: skip
    return [twc.tri(v, flag=ALL_EDGES) for v in across] + [offscreen(i, ALL_EDGES, w, h) for i in range(4)] + [small(31)]


def _check_clip(w, h):
    def check(views, d):
        s, v = views[0], d.views[0]
        tx, ty = -(-w // TILE), -(-h // TILE)
        assert (s.width, s.height) == (w, h) and len(v.tc) == tx * ty
        b = v.tri[:, 2:].astype(int)
        assert (v.tri[:6, :2] == 1).all()
        assert b[0, 0] == 0 and b[1, 0] + b[1, 2] == tx and b[2, 1] == 0 and b[3, 1] + b[3, 3] == ty  # left, right, top, bottom
        assert tuple(b[4, :2]) == (0, 0) and (b[5, 0] + b[5, 2], b[5, 1] + b[5, 3]) == (tx, ty)  # two borders at once
        assert (v.tri[6:10, 0] == 1).all() and (v.tri[6:10, 1] == 0).all()  # drawn, wholly outside
        assert (v.edge[:6, :, 0] == 1).all() and (v.edge[:6, :, 1].sum(axis=1) >= 2).all(), "bands of the clamped triangles reach the frame"
        # (bands left and right of the frame have no columns; above and below it edge_stencil clamps their rows to the frame's first / last: a box
        # of one row of tiles, every tile of which the rejection drops)
        assert (v.edge[6:10, :, 0] == 1).all() and (v.edge[6:8, :, 1] == 0).all() and (v.edge[8:10, :, 5] == 1).all()
        assert int(v.tc[tx - 1 :: tx].sum()) > 0 and int(v.tc[(ty - 1) * tx :].sum()) > 0  # the partial last column and row hold work
    return check


for _w, _h in ((W, H), (100, 77)):
    for _C in (3,) if _w == W else (3, 2, 4):
        case(f"clip_{_w}x{_h}" + (f"_c{_C}" if _C != 3 else ""), "clipping", (lambda w=_w, h=_h, C=_C: [build(clip_pieces(w, h), C=C, width=w, height=h)]),
             1.0, _check_clip(_w, _h))  # fmt: skip


# 5. edge bands at sigma = 3: bands of several blocks; more than PRIM_BLOCK flagged slots in one edge block of a dense launch; the sparse twin
N_SHORT, N_LONG = 64, 32
LONG_EDGED = [[(6.3 + 2 * i, 5.2 + i), (96.4 - i, 12.7 + 2 * i), (14.8 + 2.5 * i, 73.1 - 2 * i)] for i in reversed(range(N_LONG))]  # the longest last


def band_pieces():
    """N_SHORT triangles of a few pixels, one per tile, then N_LONG triangles across the frame: every edge flagged, the long ones last, so that
    in a dense launch (one edge block of PRIM_BLOCK EDGE_SLOTS slots) their slots are those of the second round of PRIM_BLOCK"""
    short = [small(i) for i in range(N_SHORT)]
    for t in short:
        t.flag = ALL_EDGES
    return short + [twc.tri(v, flag=ALL_EDGES) for v in LONG_EDGED]


def _check_bands(dense):
    def check(views, d):
        assert d.dense == dense and 3 * (N_SHORT + N_LONG) > K["PRIM_BLOCK"] and 3 * N_SHORT <= K["PRIM_BLOCK"]
        for v in d.views:
            assert int(v.ec.max()) <= EMAX  # (every tile on the staged kernels' own path)
            long_blocks = v.edge_extra[3 * N_SHORT : 3 * (N_SHORT + N_LONG)]
            assert (long_blocks >= 2).all() and int(long_blocks.max()) >= 8, "bands of several blocks, four half-planes, blk from 0"
            if dense:
                b = v.edge_blocks[0]
                assert b.n_flagged == 3 * (N_SHORT + N_LONG) and b.rounds == 2
                second = b.waves[1]
                assert len(second) == 1 and second[0].total == int(long_blocks[K["PRIM_BLOCK"] - 3 * N_SHORT :].sum()) > ROUND and second[0].rounds >= 2
                assert all(e.n_flagged == 0 for e in v.edge_blocks[1:])
            else:  # one slot per thread: a block never holds more than PRIM_BLOCK flagged slots
                assert len(v.edge_blocks) == 2 and all(e.rounds == 1 and 0 < e.n_flagged <= K["PRIM_BLOCK"] for e in v.edge_blocks)
                assert max(w.rounds for e in v.edge_blocks for w in e.waves[0]) >= 2  # (a wavefront of long bands: several rounds of bin_rest)
    return check


case("bands_long_sparse", "bands", lambda: [build(band_pieces())], 3.0, _check_bands(False))
case("bands_long_sparse_c2", "bands", lambda: [build(band_pieces(), C=2)], 3.0, _check_bands(False))
case("bands_long_sparse_c4", "bands", lambda: [build(band_pieces(), C=4)], 3.0, _check_bands(False))
case("bands_second_round_dense", "bands", lambda: [moved(build(padded(band_pieces(), dense_T())), v) for v in range(8)], 3.0, _check_bands(True))


# 6. / 7. list capacity: a stack of triangles strictly inside one interior tile
def stack(n, tx, ty, n_edges=0, uvmap=None):
    """n triangles inside tile (tx, ty), vertices 2 - 4.9 pixels from its corner (the columns edge_stencil gives a band of sigma = 1 -- the edge's
    own and sigma + 1 on either side, rounded outwards -- stay in the tile), of which the first n_edges edge slots (triangle by triangle) are flagged"""
    x0, y0 = tx * TILE, ty * TILE
    out = []
    for i in range(n):
        a, b = 0.004 * i, 0.003 * (i % 7)
        flags = [ALL_EDGES[e] for e in range(3) if 3 * i + e < n_edges]
        out.append(twc.tri([(x0 + 2.1 + a, y0 + 2.2 + b), (x0 + 4.8 - b, y0 + 2.6 + a), (x0 + 2.7 + b, y0 + 4.9 - a)], uvmap, flags))
    return out


def _check_stack(tiles, pooled_tri, pooled_edge):
    """tiles: {(tx, ty): (triangles, edges)}"""
    def check(views, d):
        v = d.views[0]
        assert not d.dense
        want_t, want_e = np.zeros(TX * TY, np.int64), np.zeros(TX * TY, np.int64)
        for (tx, ty), (nt, ne) in tiles.items():
            assert 0 < tx < TX - 1 and 0 < ty < TY - 1
            want_t[ty * TX + tx], want_e[ty * TX + tx] = nt, ne
        assert np.array_equal(v.tc, want_t) and np.array_equal(v.ec, want_e), "every triangle and every band stays in its tile"
        assert (v.tri_pooled, v.edge_pooled) == (pooled_tri, pooled_edge)
    return check


TRI_STACKS = {"below": K_TRI - 1, "exact": K_TRI, "one_pooled": K_TRI + 1, "batch_pooled": K_TRI + TB, "batch_and_one_pooled": K_TRI + TB + 1,
              "second_chunk": K_TRI + 64 + 1}  # fmt: skip
for _name, _n in TRI_STACKS.items():
    case(f"tri_stack_{_name}", "tri_lists", (lambda n=_n: [build(stack(n, 5, 4))]), 1.0, _check_stack({(5, 4): (_n, 0)}, max(0, _n - K_TRI), 0))
# (two tiles whose triangles alternate in the scene: their pairs share the pool's chunks, in the order the atomics decide)
case("tri_stack_two_tiles", "tri_lists", lambda: [build([p for pair in zip(stack(K_TRI + TB + 1, 5, 4), stack(K_TRI + TB + 1, 9, 6)) for p in pair])], 1.0,
     _check_stack({(5, 4): (K_TRI + TB + 1, 0), (9, 6): (K_TRI + TB + 1, 0)}, 2 * (TB + 1), 0))  # fmt: skip
case("tri_stack_textured", "tri_lists", lambda: [build(stack(K_TRI + 64 + 1, 5, 4, uvmap=(3.25, 0.35, 2.25, 0.3)))], 1.0,
     _check_stack({(5, 4): (K_TRI + 64 + 1, 0)}, 64 + 1, 0))  # fmt: skip
case("tri_stack_one_pooled_c2", "tri_lists", lambda: [build(stack(K_TRI + 1, 5, 4), C=2)], 1.0, _check_stack({(5, 4): (K_TRI + 1, 0)}, 1, 0))
case("tri_stack_second_chunk_c4", "tri_lists", lambda: [build(stack(K_TRI + 64 + 1, 5, 4), C=4)], 1.0, _check_stack({(5, 4): (K_TRI + 64 + 1, 0)}, 65, 0))

EDGE_STACKS = {"below": K_EDGE - 1, "exact": K_EDGE, "one_pooled": K_EDGE + 1, "emax": EMAX, "beyond_emax": EMAX + 1}
for _name, _n in EDGE_STACKS.items():
    case(f"edge_stack_{_name}", "edge_lists", (lambda n=_n: [build(stack(-(-n // 3), 5, 4, n_edges=n))]), 1.0,
         _check_stack({(5, 4): (-(-_n // 3), _n)}, 0, max(0, _n - K_EDGE)))  # fmt: skip
case("edge_stack_one_pooled_c2", "edge_lists", lambda: [build(stack(22, 5, 4, n_edges=K_EDGE + 1), C=2)], 1.0, _check_stack({(5, 4): (22, K_EDGE + 1)}, 0, 1))
case("edge_stack_emax_c4", "edge_lists", lambda: [build(stack(43, 5, 4, n_edges=EMAX), C=4)], 1.0, _check_stack({(5, 4): (43, EMAX)}, 0, EMAX - K_EDGE))

GROUPS = sorted({c.group for c in CASES.values()})
_BUILT = {}


def built(name):
    """-> (views, sigma, dealing) of a case; built once per process"""
    if name not in _BUILT:
        c = CASES[name]
        views = c.make()
        _BUILT[name] = (views, c.sigma, dealing(views, c.sigma))
    return _BUILT[name]


def assert_regime(name):
    """the facts the case exists for; raises AssertionError if the scene has left its regime"""
    views, sigma, d = built(name)
    T = len(np.asarray(views[0].faces))
    assert all(len(np.asarray(v.faces)) == T for v in views) and d.dense == (T * len(views) > K["SPARSE_MAX"])
    depths = np.asarray(views[0].depths)[np.asarray(views[0].faces, dtype=np.int64)][:, 0]
    assert len(set(depths.tolist())) == T, "a depth per triangle, all distinct: no depth tie decides a pixel"
    CASES[name].check(views, d)
    return d


def observation(name, seed=11):
    """obs [n, H, W, C] of a case"""
    views, _sigma, _d = built(name)
    s = views[0]
    return np.random.RandomState(seed).rand(len(views), s.height, s.width, s.nb_colors)
