"""Scenes of one or a few tiles for the texture-gradient window of owner_adjoint (deodr_amd/csrc/dr_backward.h), and a predictor of the path a tile
takes there.  No GPU: tests/test_texture_window_cases.py proves every case to be in the regime it is named for, tests/test_texture_window_gpu.py runs them.

A scene is a list of pieces (triangles, or rectangles of two triangles) in a frame of 8 x 8-pixel tiles.  The texture coordinates at the vertices
are an affine function of the vertex position, ``u = a + su x``, ``v = b + sv y``, chosen per piece: the rasterizer interpolates them exactly,
so the first texel of the footprint of pixel (x, y) is ``floor(a + su x), floor(b + sv y)`` (clamped), and offsets such as .25 keep it away from
the integers where rounding would decide.  Every triangle has a depth of its own, constant over it: the owner of a pixel is read back from the
checker's z-buffer.

The predictor replays the rule of owner_adjoint on what the CHECKER rendered (coverage and owner from its z-buffer, never the library's output):
per tile the packed or unpacked bounds of the clamped first texels of its textured pixels, the window ``(hi - lo + 2)`` per side, one window if
``ww wh C <= capacity``, else one per 4 x 4-pixel quadrant (each fits, scatters or is empty) when both texture sides are at most 65 535, else none.
The two capacities are read from the kernel sources."""

import os
import re
from types import SimpleNamespace

import numpy as np

from deodr_amd.differentiable_renderer import Scene2D

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deodr_amd", "csrc")
TILE = 8
PACKED_MAX = 0xFFFF  # texture sides up to which owner_adjoint packs (u, v) into one word and has quadrants


def constants():
    """The numbers of the kernel sources the cases are placed at: the two window capacities, and what the scan kernel's pairing rule and the
    two-kernel form of the textured forward read."""
    with open(os.path.join(CSRC, "dr_forward.h")) as f:
        fwd = f.read()
    with open(os.path.join(CSRC, "dr_workspace.h")) as f:
        wsp = f.read()
    found = {}
    for text in (fwd, wsp):
        for stmt in re.findall(r"constexpr\s+int\s+([^;()]+);", text):
            found.update({k: int(v) for k, v in re.findall(r"(\w+)\s*=\s*(\d+)\s*(?:,|$)", stmt.strip())})
    m = re.search(r"static_assert\(WIN_CAP_WAVE_LDS\s*==\s*(\d+)\s*,", fwd)
    assert m, "the static_assert that pins WIN_CAP_WAVE_LDS was not found in dr_forward.h"
    found["WIN_CAP_WAVE_LDS"] = int(m.group(1))
    missing = [k for k in ("WIN_CAP_DEFAULT", "WIN_CAP_WAVE_LDS", "WORK_CHUNK", "FIRST_PRIMS", "ENTRY_IDS", "TEX_TWO_KERNELS", "TB") if k not in found]
    assert not missing, f"constants not found in the kernel headers: {missing}"
    return found


K = constants()
CAP_EDGE, CAP_FREE = K["WIN_CAP_DEFAULT"], K["WIN_CAP_WAVE_LDS"]  # 384: two-call kernels, tiles with edges, bwd_err_tile; 768: edge-free tiles of a fit step


# ---------------------------------------------------------------------------------------------------------------- scenes


def tri(verts, uvmap=None, flag=()):
    """one triangle; uvmap (a, su, b, sv) makes it textured, None leaves it to its vertex colours; flag: pairs (i, j) of its vertices whose edge is flagged"""
    return SimpleNamespace(verts=np.asarray(verts, dtype=np.float64), uvmap=uvmap, flag=tuple(flag))


def rect(x0, x1, y0, y1, uvmap=None, flag_right=False):
    """the rectangle [x0, x1] x [y0, y1] as two triangles; flag_right: its side x = x1 is a flagged (silhouette) edge -- slanted by 0.3 pixels
    over its length, still between the same two pixel columns: the reference's span of an edge divides by the slope of its ends (H.h:2620-2648)
    and draws nothing of an exactly vertical one"""
    slant = 0.15 if flag_right else 0.0
    a, b, c, d = (x0, y0), (x1 - slant, y0), (x1 + slant, y1), (x0, y1)
    return [tri([a, b, c], uvmap, [(1, 2)] if flag_right else ()), tri([a, c, d], uvmap)]


def tile_box(W, H, tx=0, ty=0, last_col=7, first_col=0, first_row=0, last_row=7):
    """bounds of a rectangle that covers the pixel columns first_col .. last_col and rows first_row .. last_row of tile (tx, ty): between
    pixel centres inside the frame, with a margin beyond it where the tile touches the frame's border"""
    def lo(first, origin, margin):
        return origin - margin if (first == 0 and origin == 0) else origin + first - 0.45

    def hi(last, origin, size):
        return origin + TILE + 1.3 if (last == 7 and origin + TILE == size) else origin + last + 0.4

    ox, oy = tx * TILE, ty * TILE
    # (different margins in x and y: the diagonal of the rectangle then passes through no pixel centre)
    return lo(first_col, ox, 2.3), hi(last_col, ox, W), lo(first_row, oy, 2.7), hi(last_row, oy, H)


def build_scene(W, H, pieces, tex_w, tex_h, C=3, seed=0, clockwise=False):
    """Scene2D of `pieces` (every triangle with vertices of its own, so that two triangles of a tile can carry different maps), culled back
    faces with the matching winding, a depth per triangle, random texture / shades / colours / background."""
    rs = np.random.RandomState(seed)
    T = len(pieces)
    ij, uv = np.zeros((T, 3, 2)), np.zeros((T, 3, 2))
    edgeflags = np.zeros((T, 3), dtype=bool)
    textured = np.zeros(T, dtype=bool)
    front_sign = 1.0 if clockwise else -1.0  # (signedArea convention of the reference, H.h:391-398)
    for t, piece in enumerate(pieces):
        p, order = piece.verts, [0, 1, 2]
        e1, e2 = p[1] - p[0], p[2] - p[0]
        if (e1[0] * e2[1] - e1[1] * e2[0]) * front_sign < 0:
            order = [2, 1, 0]
        ij[t] = p[order]
        for i, j in piece.flag:  # edge n joins the vertices n and (n + 1) % 3 (H.h:2822)
            i, j = order.index(i), order.index(j)
            n = [n for n in range(3) if {n, (n + 1) % 3} == {i, j}]
            edgeflags[t, n[0]] = True
        if piece.uvmap is not None:
            a, su, b, sv = piece.uvmap
            textured[t] = True
            uv[t, :, 0] = a + su * ij[t, :, 0]
            uv[t, :, 1] = b + sv * ij[t, :, 1]
    depths = np.repeat(1.0 + 0.125 * np.arange(T), 3)  # distinct, exact in float32
    colors = np.where(np.repeat(textured, 3)[:, None], 0.0, 0.2 + 0.8 * rs.rand(3 * T, C))
    shade = np.where(np.repeat(textured, 3), 0.5 + 0.5 * rs.rand(3 * T), 0.0)
    faces = np.arange(3 * T, dtype=np.uint32).reshape(-1, 3)
    return Scene2D(
        faces=faces, faces_uv=faces.copy(), ij=ij.reshape(-1, 2), depths=depths, textured=textured, uv=uv.reshape(-1, 2), shade=shade,
        colors=colors, shaded=textured.copy(), edgeflags=edgeflags, height=H, width=W, nb_colors=C,
        texture=0.1 + 0.9 * rs.rand(tex_h, tex_w, C), background_image=None, background_color=0.1 + 0.8 * rs.rand(C), clockwise=clockwise,
        backface_culling=True, strict_edge=True, perspective_correct=False, integer_pixel_centers=True,
    )  # fmt: skip


# ------------------------------------------------------------------------------------------------------------- predictor


def owners(s, z_ref):
    """the triangle that owns each pixel (-1: background), from the checker's z-buffer and the triangles' distinct constant depths"""
    tri_depth = np.asarray(s.depths)[np.asarray(s.faces, dtype=np.int64)]
    assert (tri_depth == tri_depth[:, :1]).all() and len(set(tri_depth[:, 0])) == len(tri_depth), "a constant depth per triangle, all distinct"
    covered = np.isfinite(z_ref)
    dist = np.abs(np.where(covered, z_ref, 0.0)[..., None] - tri_depth[:, 0])
    assert (dist.min(axis=-1)[covered] < 1e-9).all(), "every covered pixel has the depth of one triangle"
    return np.where(covered, dist.argmin(axis=-1), -1)


def first_texels(s, z_ref):
    """Per pixel of the frame: (textured [H, W] bool, fu, fv [H, W] int: the clamped first texel of bilinear_tap, out [H, W, 2] bool, margin: the
    smallest distance of an un-clamped u or v from an integer) of the pixels whose owner -- the triangle whose depth the checker's z-buffer
    holds -- is textured and shaded."""
    H, W = s.height, s.width
    faces, faces_uv = np.asarray(s.faces, dtype=np.int64), np.asarray(s.faces_uv, dtype=np.int64)
    owner = owners(s, z_ref)
    tex = np.zeros((H, W), dtype=bool)
    fuv = np.zeros((H, W, 2), dtype=np.int64)
    out = np.zeros((H, W, 2), dtype=bool)
    size = np.array([s.texture.shape[1], s.texture.shape[0]])
    margin = np.inf
    ys, xs = np.mgrid[0:H, 0:W]
    for t in np.flatnonzero(np.asarray(s.textured, dtype=bool) & np.asarray(s.shaded, dtype=bool)):
        m = owner == t
        if not m.any():
            continue
        A = np.column_stack([np.asarray(s.ij)[faces[t]], np.ones(3)])
        coef = np.linalg.solve(A, np.asarray(s.uv)[faces_uv[t]])  # uv = [x, y, 1] coef
        val = np.stack([xs[m], ys[m], np.ones(m.sum())], axis=1) @ coef
        fp = np.floor(val).astype(np.int64)
        o = (fp < 0) | (fp > size - 2)
        if (~o).any():
            margin = min(margin, float(np.abs(val - np.round(val))[~o].min()))
        tex[m], fuv[m], out[m] = True, np.clip(fp, 0, size - 2), o
    return tex, fuv[..., 0], fuv[..., 1], out, margin


def _window(fu, fv, C, cap):
    ww, wh = int(fu.max() - fu.min()) + 2, int(fv.max() - fv.min()) + 2
    return dict(u0=int(fu.min()), v0=int(fv.min()), ww=ww, wh=wh, rowlen=ww * C, fits=ww * wh * C <= cap)


def tile_regime(s, z_ref, cap, tx=0, ty=0):
    """What owner_adjoint does in tile (tx, ty) with a window of `cap` entries -> dict: mode 'untextured' (no textured pixel: nothing to do),
    'one' (+ the window: u0, v0, ww, wh, rowlen = ww C), 'quadrants' (+ quadrants: per quadrant 'fits' / 'scatters' / 'empty', in the kernel's
    order (x & 4) | (y & 4) >> 1 ..., and windows: the quadrants' own) or 'none' (unpacked bounds, window too large: every tap is scattered)."""
    tex, fu, fv, _out, _margin = first_texels(s, z_ref)
    C = s.nb_colors
    tex_h, tex_w = s.texture.shape[:2]
    sl = (slice(ty * TILE, min((ty + 1) * TILE, s.height)), slice(tx * TILE, min((tx + 1) * TILE, s.width)))
    t, u, v = tex[sl], fu[sl], fv[sl]
    if not t.any():
        return dict(mode="untextured")
    full = _window(u[t], v[t], C, cap)
    packed = tex_w <= PACKED_MAX and tex_h <= PACKED_MAX
    if full["fits"]:
        return dict(mode="one", packed=packed, **full)
    if not packed:
        return dict(mode="none", packed=False, **full)
    quadrants, windows = [], []
    for qd in range(4):  # qd & 1: the right half, qd >> 1: the lower half (owner_adjoint's my_q)
        q = (slice((qd >> 1) * 4, (qd >> 1) * 4 + 4), slice((qd & 1) * 4, (qd & 1) * 4 + 4))
        if not t[q].any():
            quadrants.append("empty"), windows.append(None)
            continue
        w = _window(u[q][t[q]], v[q][t[q]], C, cap)
        quadrants.append("fits" if w["fits"] else "scatters"), windows.append(w)
    return dict(mode="quadrants", packed=True, quadrants=quadrants, windows=windows, **full)


def fwd_tile_blocks(ntiles, n_views, dealt_fill):
    """fwd_tile_blocks of dr_forward.h: walkers per view of the forward raster"""
    unit = 8 * K["WORK_CHUNK"]
    div = 6 if (dealt_fill and n_views >= 8) else 4
    g = ((ntiles // div + unit - 1) // unit) * unit
    return g if 0 < g <= ntiles else ntiles


def chunked_frame(s, n_views, sigma):
    """tile_scan_kernel forms classes of tiles (a head, pairs) only where the walkers come in whole units of 8 WORK_CHUNK: a tiny frame is one plain list"""
    ntiles = -(-s.width // TILE) * -(-s.height // TILE)
    return fwd_tile_blocks(ntiles, n_views, sigma > 0) % (8 * K["WORK_CHUNK"]) == 0


def tile_counts(s, z_ref, tx, ty):
    """(at least, at most) triangles the set-up kernel bins into tile (tx, ty): at least the owners the checker rendered there, at most the
    front-facing triangles whose bounding box of pixels meets it; and the flagged edges of front-facing triangles anywhere in the scene."""
    faces = np.asarray(s.faces, dtype=np.int64)
    v = np.asarray(s.ij)[faces]
    sl = owners(s, z_ref)[ty * TILE : (ty + 1) * TILE, tx * TILE : (tx + 1) * TILE]
    at_least = len(set(sl[sl >= 0].tolist()))
    x0, x1 = np.ceil(v[..., 0].min(axis=1)), np.floor(v[..., 0].max(axis=1))
    y0, y1 = np.ceil(v[..., 1].min(axis=1)), np.floor(v[..., 1].max(axis=1))
    meets = (x0 <= tx * TILE + 7) & (x1 >= tx * TILE) & (y0 <= ty * TILE + 7) & (y1 >= ty * TILE)
    return at_least, int(meets.sum()), int(np.asarray(s.edgeflags).sum())


def pairs_up(s, z_ref, n_views, sigma, tx, ty):
    """tile_scan_kernel's rule for a textured pair of the tiles (tx, ty), (tx + 1, ty), tx even: a fit step with fused edge tiles (sigma > 0) of
    fewer than TEX_TWO_KERNELS views, an even number of tile columns, a chunked frame, both tiles with triangles and without edges, at most
    FIRST_PRIMS each and ENTRY_IDS together."""
    tiles_x = -(-s.width // TILE)
    (a_lo, a_hi, flagged), (b_lo, b_hi, _) = tile_counts(s, z_ref, tx, ty), tile_counts(s, z_ref, tx + 1, ty)
    return (sigma > 0 and n_views < K["TEX_TWO_KERNELS"] and tiles_x % 2 == 0 and tx % 2 == 0 and chunked_frame(s, n_views, sigma) and flagged == 0
            and a_lo > 0 and b_lo > 0 and a_hi <= K["FIRST_PRIMS"] and b_hi <= K["FIRST_PRIMS"] and a_hi + b_hi <= K["ENTRY_IDS"])  # fmt: skip


def flush_lane_split(rowlen):
    """window_flush's split of the 64 lanes over the rows of a pass, restated in numpy with IEEE float32 arithmetic -> (rows per pass, row of each
    lane, index in its row).  A copy of the formula, not the kernel: it shows that the formula is the integer division, nothing about the build."""
    lane = np.arange(64)
    if rowlen >= 64:
        return 1, np.zeros(64, dtype=np.int64), lane
    lr = ((lane.astype(np.float32) + np.float32(0.5)) * (np.float32(1.0) / np.float32(rowlen))).astype(np.int64)
    return 64 // rowlen, lr, lane - lr * rowlen


# ----------------------------------------------------------------------------------------------------------------- cases
#
# A case is (name, tile pieces builder, texture (w, h), C, what it must be at the two capacities).  `pieces(W, H, tx, ty, edge)` places the case in
# tile (tx, ty) of a W x H frame; edge = True leaves the tile's last pixel column to the background behind a flagged edge of the textured
# rectangle (a tile with a silhouette edge: capacity CAP_EDGE also in a fit step; the edge's own taps are scattered).


def span_scale(span, last):
    """scale s such that floor(.25 + s x) runs from 0 (x = 0) to `span` (x = last), .65 above the integer at the far end"""
    return (span + 0.4) / last


def cover(umap, vmap, tex=(40, 40)):
    """the whole tile under one map; umap / vmap: (offset, texels spanned over the tile's covered pixels) or (offset, None, scale)"""
    def pieces(W, H, tx=0, ty=0, edge=False):
        last = 6 if edge else 7
        ox, oy = tx * TILE, ty * TILE

        def axis(m, origin, last_px):
            off, span = m[0], m[1]
            sc = m[2] if span is None else span_scale(span, last_px)
            return off - sc * origin, sc  # the map is placed relative to the tile

        a, su = axis(umap, ox, last)
        b, sv = axis(vmap, oy, 7)
        return rect(*tile_box(W, H, tx, ty, last_col=last), uvmap=(a, su, b, sv), flag_right=edge)

    return SimpleNamespace(pieces=pieces, tex=tex)


def mixed(scale=12.0, tex=(96, 96)):
    """quadrant 0 under a magnified map (fits), quadrant 1 under a second rectangle with a minified one (scatters), quadrant 2 under an untextured
    rectangle, quadrant 3 background"""
    def pieces(W, H, tx=0, ty=0, edge=False):
        ox, oy = tx * TILE, ty * TILE
        last = 6 if edge else 7
        q0 = rect(*tile_box(W, H, tx, ty, first_col=0, last_col=3, first_row=0, last_row=3), uvmap=(2.25 - 0.5 * ox, 0.5, 2.25 - 0.5 * oy, 0.5))
        q1 = rect(*tile_box(W, H, tx, ty, first_col=4, last_col=last, first_row=0, last_row=3), uvmap=(0.25 - scale * ox, scale, 0.25 - scale * oy, scale), flag_right=edge)
        q2 = rect(*tile_box(W, H, tx, ty, first_col=0, last_col=3, first_row=4, last_row=7))
        return q0 + q1 + q2

    return SimpleNamespace(pieces=pieces, tex=tex)


def one(ww, wh, C):
    return dict(mode="one", ww=ww, wh=wh, rowlen=ww * C)


def quads(*status):
    return dict(mode="quadrants", quadrants=list(status))


ALL_FIT = quads("fits", "fits", "fits", "fits")

# name -> (builder, C, expected at CAP_FREE, expected at CAP_EDGE); windows written as (span + 2)
CASES = {}


def case(name, builder, C, free, edge_cap):
    assert name not in CASES
    CASES[name] = SimpleNamespace(name=name, builder=builder, C=C, expect={CAP_FREE: free, CAP_EDGE: edge_cap})


# one window well inside either capacity
case("inside", cover((3.25, None, 0.5), (3.25, None, 0.5)), 3, one(5, 5, 3), one(5, 5, 3))
# exactly at a capacity, and the twin one texel wider (quadrants that all fit), for every channel count: (C, ww, wh) with ww wh C = capacity
AT_CAPACITY = {CAP_FREE: {1: (32, 24), 2: (24, 16), 3: (16, 16), 4: (16, 12)}, CAP_EDGE: {1: (24, 16), 2: (16, 12), 3: (16, 8), 4: (12, 8)}}
for _cap, _sizes in AT_CAPACITY.items():
    for _C, (_ww, _wh) in _sizes.items():
        assert _ww * _wh * _C == _cap, "the table above is placed at the capacities of the kernel sources"
        _tex = (_ww + 8, _wh + 8)
        _at, _wide = one(_ww, _wh, _C), ALL_FIT
        # (at the smaller capacity the window of the larger one is a quadrant case; at the larger one the window of the smaller one simply fits)
        case(f"cap{_cap}_c{_C}", cover((0.25, _ww - 2), (0.25, _wh - 2), _tex), _C, _at, _at if _cap == CAP_EDGE else ALL_FIT)
        case(f"cap{_cap}_c{_C}_wider", cover((0.25, _ww - 1), (0.25, _wh - 2), _tex), _C, _wide if _cap == CAP_FREE else one(_ww + 1, _wh, _C), _wide)
# quadrants mixed in one tile, every channel count
for _C in (1, 2, 3, 4):
    case(f"mixed_c{_C}", mixed(), _C, quads("fits", "scatters", "empty", "empty"), quads("fits", "scatters", "empty", "empty"))
# every quadrant scatters
case("all_scatter", cover((0.25, None, 8.0), (0.25, None, 8.0), (64, 64)), 3, quads(*["scatters"] * 4), quads(*["scatters"] * 4))
# flush row lengths ww C: several rows per pass (also lengths that do not divide 64), one row per pass with idle lanes, exactly 64, above 64.
# Anisotropic maps; the rows of the window: 11 where the larger capacity holds them (rows touched: 0-3, 4-7, 8-10: every pass of a short row) -- at the
# smaller capacity the longest of those rows (63 and more) are quadrant cases, every quadrant fits -- and a variant of 5 or 6 rows that also fits
# the smaller one.
ROW_LENGTHS = [(6, 3), (9, 3), (12, 3), (12, 4), (20, 4), (21, 3), (31, 1), (33, 3), (33, 1), (63, 3), (64, 4), (64, 1), (65, 1), (66, 3)]
for _R, _C in ROW_LENGTHS:
    _ww = _R // _C
    assert _ww * _C == _R and _ww >= 2
    _tex = (_ww + 6, 16)
    assert _R * 11 <= CAP_FREE
    case(f"row{_R}_c{_C}_h11", cover((1.25, _ww - 2), (1.25, 9), _tex), _C, one(_ww, 11, _C), one(_ww, 11, _C) if _R * 11 <= CAP_EDGE else ALL_FIT)
    _wh = 6 if _R * 6 <= CAP_EDGE else 5
    assert _R * _wh <= CAP_EDGE
    case(f"row{_R}_c{_C}_h{_wh}", cover((1.25, _ww - 2), (1.25, _wh - 2), _tex), _C, one(_ww, _wh, _C), one(_ww, _wh, _C))
# borders: the window touches texel 0 and the last texel on each side (no clamping); uv beyond the texture on all four sides; a 2 x 2 texture
case("border_touch", cover((0.25, 7), (0.25, 7), (9, 9)), 3, one(9, 9, 3), one(9, 9, 3))
case("border_beyond", cover((-2.75, None, 1.5), (-2.75, None, 1.5), (6, 6)), 3, one(6, 6, 3), one(6, 6, 3))
case("texture_2x2", cover((-1.75, None, 0.5), (-1.75, None, 0.5), (2, 2)), 3, one(2, 2, 3), one(2, 2, 3))
# texture sides around 65 535 (one channel keeps them small): packed with u at the far end; unpacked (a side above 65 535), a window that fits and
# one that must scatter, the long side along u and along v
case("side_65535_far_end", cover((65526.25, 7), (0.25, None, 0.1), (65535, 3)), 1, one(9, 2, 1), one(9, 2, 1))
case("side_65537_u_fits", cover((65528.25, 7), (0.25, None, 0.1), (65537, 3)), 1, one(9, 2, 1), one(9, 2, 1))
case("side_65537_u_scatters", cover((60000.25, None, 200.0), (0.25, None, 0.1), (65537, 3)), 1, dict(mode="none"), dict(mode="none"))
case("side_65537_v_fits", cover((0.25, None, 0.1), (65528.25, 7), (3, 65537)), 1, one(2, 9, 1), one(2, 9, 1))
case("side_65537_v_scatters", cover((0.25, None, 0.1), (60000.25, None, 200.0), (3, 65537)), 1, dict(mode="none"), dict(mode="none"))

# the cases that also run with a flagged edge in the tile (a narrower covered strip: their own expectations, at CAP_EDGE on every path)
EDGE_CASES = {}


def edge_case(name, builder, C, expect):
    EDGE_CASES[name] = SimpleNamespace(name=name, builder=builder, C=C, expect={CAP_EDGE: expect, CAP_FREE: None})


edge_case("inside", cover((3.25, None, 0.5), (3.25, None, 0.5)), 3, one(5, 5, 3))
for _C, (_ww, _wh) in AT_CAPACITY[CAP_EDGE].items():
    edge_case(f"cap{CAP_EDGE}_c{_C}", cover((0.25, _ww - 2), (0.25, _wh - 2), (_ww + 8, _wh + 8)), _C, one(_ww, _wh, _C))
    edge_case(f"cap{CAP_EDGE}_c{_C}_wider", cover((0.25, _ww - 1), (0.25, _wh - 2), (_ww + 8, _wh + 8)), _C, ALL_FIT)
for _C in (1, 2, 3, 4):
    edge_case(f"mixed_c{_C}", mixed(), _C, quads("fits", "scatters", "empty", "empty"))
edge_case("all_scatter", cover((0.25, None, 8.0), (0.25, None, 8.0), (64, 64)), 3, quads(*["scatters"] * 4))
for _R, _C in [(9, 3), (33, 3), (64, 4), (66, 3)]:
    edge_case(f"row{_R}_c{_C}", cover((1.25, _R // _C - 2), (1.25, 3), (_R // _C + 6, 16)), _C, one(_R // _C, 5, _C))
edge_case("border_beyond", cover((-2.75, None, 1.5), (-2.75, None, 1.5), (6, 6)), 3, one(6, 6, 3))
edge_case("side_65537_u_fits", cover((65528.25, 7), (0.25, None, 0.1), (65537, 3)), 1, one(9, 2, 1))
edge_case("side_65537_u_scatters", cover((60000.25, None, 200.0), (0.25, None, 0.1), (65537, 3)), 1, dict(mode="none"))


def single_tile_scene(c, edge=False, C=None, seed=3):
    """the case alone in an 8 x 8 frame: an edge-free tile that cannot pair (one tile column), or a tile with a flagged textured edge"""
    C = c.C if C is None else C
    return build_scene(TILE, TILE, c.builder.pieces(TILE, TILE, 0, 0, edge), c.builder.tex[0], c.builder.tex[1], C, seed)


# A frame of 512 tiles is the smallest the scan kernel chunks (pairs, a head of the work list, the two-kernel form): the scene sits in its first two tiles
CHUNKED_W, CHUNKED_H = 256, 128


def two_tile_scene(builder_a, builder_b, tex, C=3, edge_b=False, seed=5):
    """tile (0, 0) under one case and tile (1, 0) under another (sharing one texture) in the smallest chunked frame, the other 510 tiles empty"""
    pieces = builder_a.pieces(CHUNKED_W, CHUNKED_H, 0, 0, False) + builder_b.pieces(CHUNKED_W, CHUNKED_H, 1, 0, edge_b)
    return build_scene(CHUNKED_W, CHUNKED_H, pieces, tex[0], tex[1], C, seed)


def matches(regime, expect):
    """the predictor's answer against a case's expectation (the keys the expectation names)"""
    return all(regime.get(k) == v for k, v in expect.items())
