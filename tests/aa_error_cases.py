"""Scenes for the antialiase_error mode on the LDS-staged kernels (the VAR = 1 instances of raster_fwd_fast_kernel, the p.aa_err branch of
bwd_fast_tile, bwd_err_tile / raster_bwd_edge_err_kernel) where their paths change, and the predicates that say which path a scene takes.  No GPU:
tests/test_aa_error_cases.py proves every case to be in the regime it is named for, tests/test_aa_error_gpu.py asserts it again and runs them.

A regime is stated over tests/sim_util.bin_counts (the device's binning on the CPU, exact=True: triangles and silhouette edges per tile), the
constants of the kernel sources (parsed below, never copied) and the host formulas fwd_tile_blocks and heavy_share_for of dr_forward.h, restated here
for the two-call path of this mode (no fused edge tiles, no dealt fill).  The device keeps no record of which walker took which entry: if a rule in
the kernels changes, its restatement here has to follow.

The counts a case pins ("exactly 529 tiles") are those of the scene constructors of deodr_amd/scenes.py at the seeds used; where a count is
incidental it is bracketed.  If a constructor changes them, pick another seed and keep the regime."""

import copy
import os
import re
from types import SimpleNamespace

import numpy as np

import texture_window_cases as twc
from deodr_amd import scenes
from sim_util import bin_counts

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deodr_amd", "csrc")


def constants():
    """The numbers of the kernel sources the cases are placed at (as tests/test_head_by_cost_gpu.py::constants reads them): the headers' constexpr
    ints, and EDGE_WAVES of dr_kernels.hip"""
    found = {}
    for name in ("dr_workspace.h", "dr_forward.h", "dr_kernels.hip"):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        for stmt in re.findall(r"constexpr\s+int\s+([^;()\[\]]+);", text):
            found.update({k: v for k, v in re.findall(r"(\w+)\s*=\s*(\w+)\s*(?:,|$)", stmt.strip())})
    value = lambda v: int(v) if v.isdigit() else value(found[v])
    need = ("TILE", "TB", "EMAX", "K_EDGE", "K_TRI", "PRIO_EDGES", "FIRST_PRIMS", "WORK_CHUNK", "SCAN_TILES", "EDGE_WAVES")
    missing = [k for k in need if k not in found]
    assert not missing, f"constants not found in the kernel sources: {missing}"
    return {k: value(found[k]) for k in need}


K = constants()
TILE, TB, EMAX = K["TILE"], K["TB"], K["EMAX"]
assert EMAX % TB == 0 and K["K_EDGE"] < EMAX and K["PRIO_EDGES"] < TB


# -------------------------------------------------------------------------------------------------- host formulas, restated


def fwd_tile_blocks(ntiles, n_views, dealt_fill=False):
    """fwd_tile_blocks of dr_forward.h: walkers per view of the forward raster (and of the owner-tile launch of raster_bwd_fast_kernel, which
    launch_adjoint_raster recomputes with dealt_fill = false)"""
    unit = 8 * K["WORK_CHUNK"]
    div = 6 if (dealt_fill and n_views >= 8) else 4
    g = ((ntiles // div + unit - 1) // unit) * unit
    return g if 0 < g <= ntiles else ntiles


def heavy_share_for(n_views, tile_blocks, fuse_edges=False):
    """heavy_share_for of dr_forward.h: one walker in this many walks the head of the work list"""
    want = (n_views * tile_blocks + (4095 if fuse_edges else 2047)) // (4096 if fuse_edges else 2048)
    if fuse_edges and want <= 8:
        return 4
    share = 4
    while share < 16 and share < want:
        share *= 2
    return share


def walkers(ntiles, n_views):
    """(G walkers per view, Gh of them on the head of the work list; Gh = 0: one plain list, a walker per tile) of a forward of this mode"""
    G = fwd_tile_blocks(ntiles, n_views)
    chunked = G % (8 * K["WORK_CHUNK"]) == 0
    return G, (G // heavy_share_for(n_views, G) if chunked else 0)


# ------------------------------------------------------------------------------------------------------- regime predicates


def census(s, sigma, n_views=1):
    """What tile_scan_kernel makes of the scene in a forward of this mode (two calls: no fused edge tiles) -> namespace: tc, ec per tile, ntiles, G,
    Gh, chunked, head (entries of the head of the work list), other (of its rest), empty / edge_free / edge_tiles counts, the three edge lists
    (1 .. PRIO_EDGES, .. TB, more), pooled (K_EDGE < ec <= EMAX: through the edge pool), at_emax, beyond (ec > EMAX)"""
    tc, ec = bin_counts(s, sigma, TILE, exact=True)
    tc, ec = tc.astype(np.int64), ec.astype(np.int64)
    ntiles = len(tc)
    assert ntiles == -(-s.width // TILE) * -(-s.height // TILE)
    G, Gh = walkers(ntiles, n_views)
    work = (tc > 0) | (ec > 0)
    heavy = work & (Gh > 0) & ((tc > K["FIRST_PRIMS"]) | (ec > K["FIRST_PRIMS"]))
    return SimpleNamespace(
        tc=tc, ec=ec, ntiles=ntiles, G=G, Gh=Gh, chunked=Gh > 0, head=int(heavy.sum()), other=int((work & ~heavy).sum()), empty=int((~work).sum()),
        edge_free=int((work & (ec == 0)).sum()), edge_tiles=int((ec > 0).sum()),
        lists=(int(((ec > 0) & (ec <= K["PRIO_EDGES"])).sum()), int(((ec > K["PRIO_EDGES"]) & (ec <= TB)).sum()), int((ec > TB).sum())),
        pooled=int(((ec > K["K_EDGE"]) & (ec <= EMAX)).sum()), at_emax=int((ec == EMAX).sum()), beyond=int((ec > EMAX).sum()),
    )  # fmt: skip


def rank_is_permuted(G, Gh):
    """(head, rest): whether the walkers of that part of the list take the entry `rank(q)` that deals chunks of WORK_CHUNK entries to the XCDs --
    fwd_tiles and raster_bwd_fast_kernel: only where the part's stride (Gh, G - Gh) is a whole number of units of 8 WORK_CHUNK; else entry q"""
    unit = 8 * K["WORK_CHUNK"]
    return (Gh > 0 and Gh % unit == 0, Gh > 0 and (G - Gh) % unit == 0)


def later_entries_without_edges(c):
    """The fewest edge-free tiles that are a SECOND or later entry of a head walker (position >= Gh in the head of the work list), over every order
    in which the workgroups of tile_scan_kernel (SCAN_TILES tiles each; tile order inside one) may have claimed their part of the list: those the
    owner-tile launch of raster_bwd_fast_kernel back-propagates through the p.aa_err branch of bwd_fast_tile after `rank += stride`"""
    from itertools import permutations

    heavy = (c.Gh > 0) & ((c.tc > K["FIRST_PRIMS"]) | (c.ec > K["FIRST_PRIMS"]))
    blocks = [np.arange(b0, min(b0 + K["SCAN_TILES"], c.ntiles)) for b0 in range(0, c.ntiles, K["SCAN_TILES"])]
    fewest = None
    for order in permutations(range(len(blocks))):
        listed = np.concatenate([blocks[b][heavy[blocks[b]]] for b in order])
        n = int((c.ec[listed[c.Gh :]] == 0).sum())
        fewest = n if fewest is None else min(fewest, n)
    return fewest


def entries_of_busiest_walker(n_entries, stride):
    """entries the walker with the most of them takes from a list of n_entries dealt rank, rank + stride, ... (fwd_tiles, raster_bwd_fast_kernel)"""
    return -(-n_entries // stride) if stride > 0 else 0


# ---------------------------------------------------------------------------------------------------------------- scenes


def views_of(s, n):
    """n views of one topology: view v is `s` moved by (0.37 v, 0.21 v) pixels"""
    out = []
    for v in range(n):
        c = copy.copy(s)
        c.ij = np.asarray(s.ij) + np.array([0.37 * v, 0.21 * v])
        out.append(c)
    return out


REPLAY_W, REPLAY_H, REPLAY_PIXEL, REPLAY_FAR, REPLAY_ASIDE = 40, 48, (14, 21), 20, 12


def replay_scene(d, textured=True, seed=7):
    """A 40 x 48 frame whose nearest triangle has a flagged edge from (10, 20 + d) to (30, 25 + d): the pixel centres (14, 21), (18, 22), (22, 23),
    (26, 24) lie just outside it, d 4 / sqrt(17) pixels from its line -- the edge's transparency there at sigma = 1.  REPLAY_FAR farther triangles
    each have ONE flagged edge that passes 0.15 - 0.85 pixels from (14, 21), at random angles, with the pixel outside: pixel (14, 21) is
    background under REPLAY_FAR + 1 drawn edges, the near one the last of the sweep.  Shuffled among them in depth, REPLAY_ASIDE triangles whose
    flagged edge passes 2.5 - 4.5 pixels from that pixel, on the side of its tile's interior: edges of the same tile that are NOT drawn over the
    pixel, so that the masks tm[] of the tile's batches differ at the pixel and a replay that read the wrong batch would blend the wrong edges.
    textured: every third far triangle is textured (the replay's texture taps); else no texture at all (the untextured instance of the kernel).
    -> the scene; scene.replay_drawn: per edge of the pixel's tile in blending order (far -> near, the near edge left out) whether it is drawn
    over the pixel."""
    rs = np.random.RandomState(seed)
    px, py = REPLAY_PIXEL
    pieces = [twc.tri([(10.0, 20.0 + d), (30.0, 25.0 + d), (18.0, 40.0)], flag=[(0, 1)])]
    touches = rs.permutation([True] * REPLAY_FAR + [False] * REPLAY_ASIDE)
    for k, touch in enumerate(touches):
        theta, r = (rs.uniform(0, 2 * np.pi), rs.uniform(0.15, 0.85)) if touch else (rs.uniform(np.pi, 1.5 * np.pi), rs.uniform(2.5, 4.5))
        n, t = np.array([np.cos(theta), np.sin(theta)]), np.array([-np.sin(theta), np.cos(theta)])
        foot = np.array([px, py]) + r * n
        uvmap = (3.25, 0.35, 2.25, 0.3) if (textured and k % 3 == 0) else None
        pieces.append(twc.tri([foot - rs.uniform(4, 7) * t, foot + rs.uniform(4, 7) * t, foot + rs.uniform(4, 7) * n], uvmap, flag=[(0, 1)]))
    s = twc.build_scene(REPLAY_W, REPLAY_H, pieces, 24, 24, C=3, seed=seed)
    if not textured:
        s.texture = np.zeros((0, 0))
    s.replay_drawn = [bool(v) for v in touches[::-1]]  # (build_scene: the depth grows with the piece's index, and the sweep starts at the farthest)
    return s


def replay_reads_every_batch(drawn):
    """the replay of the near edge (edge len(drawn) of the tile's blending order) runs over more than one batch, and at the pixel the masks of
    the batches differ: for some edge q >= TB, bit q % TB of the first batch says otherwise than the edge's own"""
    return len(drawn) > TB and any(drawn[q] != drawn[q % TB] for q in range(TB, len(drawn)))


REPLAY_D, UNBLEND_D = 2.0**-21, 2.0**-10
REPLAY_T = lambda d: d * 4 / np.sqrt(17.0)  # transparency of the near edge at the four pixel centres (sigma = 1)


def sphere(**kw):
    return scenes.sphere_scene(angle=0.1, **kw)


def soup(**kw):
    return scenes.soup_scene(seed=2, **kw)


# name -> (constructor, sigma, number of views); a scene is built once per process
CASES = {
    "chunked_mixed": (lambda: sphere(size=180, nu=40, n_rings=32, nb_colors=4), 1.0, 1),
    "chunked_mixed_textured": (lambda: sphere(size=180, nu=40, n_rings=32, nb_colors=3, depth_channel=False, textured=True, texture_size=32), 1.0, 1),
    "chunked_mixed_sigma0": (lambda: sphere(size=180, nu=40, n_rings=32, nb_colors=4), 0.0, 1),
    "chunked_fine_mesh": (lambda: sphere(size=180, nu=80, n_rings=64, nb_colors=4), 1.0, 1),
    "chunked_head_twice": (lambda: soup(n_tri=200, width=256, height=128), 1.0, 1),
    "chunked_head_twice_textured": (lambda: soup(n_tri=200, width=256, height=128, textured_ratio=0.5), 1.0, 1),
    "edge_pool_and_emax": (lambda: soup(n_tri=1500, width=256, height=128, textured_ratio=0.5), 3.0, 1),
    "beyond_emax": (lambda: soup(n_tri=600, width=64, height=64, textured_ratio=0.5), 3.0, 1),
    "more_tiles_than_waves": (lambda: soup(n_tri=400, width=264, height=256), 1.0, 1),
    "few_channels_1": (lambda: sphere(size=96, nu=30, n_rings=24, nb_colors=1), 1.0, 1),
    "few_channels_2": (lambda: sphere(size=96, nu=30, n_rings=24, nb_colors=2), 1.5, 1),
    "replay": (lambda: replay_scene(REPLAY_D), 1.0, 1),
    "replay_untextured": (lambda: replay_scene(REPLAY_D, textured=False), 1.0, 1),
    "unblend_twin": (lambda: replay_scene(UNBLEND_D), 1.0, 1),
    "views": (lambda: soup(n_tri=200, width=256, height=128, textured_ratio=0.5), 1.0, 3),
}

_BUILT = {}


def case(name):
    """-> (views: list of Scene2D, sigma, [census of every view])"""
    if name not in _BUILT:
        make, sigma, n = CASES[name]
        views = views_of(make(), n)
        _BUILT[name] = (views, sigma, [census(v, sigma, n) for v in views])
    return _BUILT[name]


def tile_of(x, y, s):
    return (y // TILE) * -(-s.width // TILE) + x // TILE


def assert_regime(name):
    """The facts the case exists for (module docstring); raises AssertionError with the census if the scene has left its regime."""
    views, sigma, cs = case(name)
    for s, c in zip(views, cs):
        what = (name, {k: v for k, v in vars(c).items() if k not in ("tc", "ec")})
        tc, ec = c.tc, c.ec
        if name == "chunked_fine_mesh":
            # a head of more entries than head walkers in which edge-free tiles are second entries whatever the order of the scan's workgroups (the
            # adjoint's owner-tile launch takes them after `rank += stride`); tiles of more than K_TRI triangles (the triangle pool)
            assert c.ntiles == 529 and (c.G, c.Gh) == (512, 128) and c.Gh < c.head <= 2 * c.Gh, what
            assert later_entries_without_edges(c) >= 10 and int(tc.max()) > K["K_TRI"] and c.edge_tiles > 0 and c.beyond == 0, what
        elif name.startswith("chunked_mixed"):
            assert s.width % TILE != 0 and c.ntiles == 529 and (c.G, c.Gh) == (512, 128) and c.chunked, what
            if sigma == 0:  # no edge anywhere: every tile with work through the owner-tile kernel, on a chunked list with a head
                assert c.edge_tiles == 0 and c.head > 0 and c.other > 0 and c.empty > 0, what
            else:  # empty, edge-free and edge tiles, every edge list in use, a head and a rest
                assert (c.empty, c.edge_free, c.edge_tiles) == (321, 119, 89) and c.lists == (73, 11, 5), what
                assert 0 < c.head and 0 < c.other, what
        elif name.startswith("chunked_head_twice") or name == "views":
            assert c.ntiles == 512 and (c.G, c.Gh) == (512, 128) and c.chunked, what
            # head walkers take a second AND a third entry
            assert c.head > 2 * c.Gh and entries_of_busiest_walker(c.head, c.Gh) >= 3, what
            if name != "views":  # (the moved views keep the regime, not the counts)
                assert c.head == 290 and int((ec == TB).sum()) == 10 and int((ec == TB + 1).sum()) == 7, what
            else:
                assert int((ec > TB).sum()) > 0, what
            assert c.beyond == 0, what
        elif name == "edge_pool_and_emax":
            assert c.chunked and c.Gh == 128 and c.pooled == 385 and c.at_emax == 1 and c.beyond == 0, what
            assert int(tc.max()) == 91 > K["K_TRI"], what  # (the triangle pool too)
        elif name == "beyond_emax":
            assert c.ntiles == 64 and not c.chunked and c.G == 64, what
            # the ordered-search branch of the forward and the un-staged adjoint inside bwd_err_tile, next to tiles exactly at EMAX and pooled ones
            assert c.beyond == 13 and int(ec.max()) == 141 and c.at_emax == 2 and c.pooled == 46, what
            assert int(tc.max()) == K["K_TRI"], what  # (exactly the inline triangle slots: no pool)
        elif name == "more_tiles_than_waves":
            assert c.ntiles == 1056 and c.edge_tiles == c.ntiles > K["EDGE_WAVES"], what  # walkers of raster_bwd_edge_err_kernel take a second tile
            assert c.beyond == 0, what
        elif name.startswith("few_channels"):
            P = max(3, s.nb_colors)  # (KParams L.P: planes per primitive)
            assert s.nb_colors < 3 and 3 * s.nb_colors < 12 and 3 * P <= 12, what  # the mask `lane < 3 * P` / the channel loops `cc < C` bite
            assert c.lists[2] == 4 and c.beyond == 0, what  # tiles of more than one batch of edges
        elif name in ("replay", "replay_untextured", "unblend_twin"):
            t = tile_of(*REPLAY_PIXEL, s)
            # every far edge is binned into the pixel's tile (their blending order is then the order of scene.replay_drawn), and the replay of
            # the near one reads the masks of more than one batch of tm[], which differ at the pixel
            assert TB < ec[t] == REPLAY_FAR + REPLAY_ASIDE + 1 <= EMAX and len(s.replay_drawn) == ec[t] - 1, what
            assert replay_reads_every_batch(s.replay_drawn) and sum(s.replay_drawn) == REPLAY_FAR, what
            assert c.beyond == 0, what
        else:
            raise KeyError(name)
    return cs


# ------------------------------------------------------------------------------------------------- inputs and the reference


def inputs(name, seed=5):
    """(obs [n, H, W, C], err_buffer_b [n, H, W]) of a case: what the CPU test feeds the checker with and the GPU test both sides"""
    views, _sigma, _cs = case(name)
    s = views[0]
    rs = np.random.RandomState(seed)
    return rs.rand(len(views), s.height, s.width, s.nb_colors), rs.rand(len(views), s.height, s.width) + 0.1


def checker(api):
    """the repaired checker (defects D1, D2 of DESIGN.md section 6): the reference's build where there is one, else the restatement"""
    return api.ref(fixed=True) or api.port(fixed=True)


_REFERENCE = {}


def reference(api, name):
    """Per view (image, z, err, gradients) of the repaired checker; computed once per process, shared by the tests and never written to"""
    if name not in _REFERENCE:
        views, sigma, _cs = case(name)
        obs, err_b = inputs(name)
        out = []
        for i, s in enumerate(views):
            fixed = checker(api)
            image, z, err = fixed.render(s, sigma, True, obs[i])
            g = fixed.grads(s, sigma, image, z, None, True, obs[i], err, err_b[i])
            for a in (image, z, err, *g.values()):
                a.setflags(write=False)
            out.append((image, z, err, g))
        _REFERENCE[name] = out
    return _REFERENCE[name]
