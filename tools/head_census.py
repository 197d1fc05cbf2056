"""Entries of the forward's work list of view 0 -- head (many-primitive tiles / tiles with edges, walked by one workgroup in heavy_share) and
the rest -- for the bench workload and for configs[4]: how many entries a head walker walks one after the other.  GPU box.
    python tools/head_census.py [--lib path]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deodr_amd import hip_renderer as hr
from deodr_amd import scenes
from deodr_amd.hip_renderer import DeviceScene, HipRasterizer

if "--lib" in sys.argv:
    hr.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
dev = torch.device("cuda:0")


def walkers(ntiles, n_views, dealt_fill, fuse_edges):
    """(walkers per view, head walkers per view): fwd_tile_blocks and heavy_share_for of dr_forward.h"""
    unit = 512
    g = -(-(ntiles // (6 if dealt_fill and n_views >= 8 else 4)) // unit) * unit
    G = g if 0 < g <= ntiles else ntiles
    if G % unit:
        return G, 0
    want = -(-n_views * G // (4096 if fuse_edges else 2048))
    share = 4
    while not (fuse_edges and want <= 8) and share < 16 and share < want:
        share *= 2
    return G, G // share


def census(name, views):
    s0 = views[0]
    stack = lambda n: np.stack([np.asarray(getattr(v, n)) for v in views])
    tex = s0.texture if np.size(s0.texture) else None
    ds = DeviceScene(s0.faces, s0.faces_uv, s0.textured, s0.shaded, s0.uv, stack("ij"), stack("depths"), stack("colors"), stack("shade"),
                     stack("edgeflags"), s0.height, s0.width, texture=tex, background_color=s0.background_color, clockwise=s0.clockwise,
                     vertex_dtype=torch.float64, pixel_dtype=torch.float32, device=dev)  # fmt: skip
    r = HipRasterizer.for_scene(ds)
    n, H, W, C = ds.n_views, ds.height, ds.width, ds.nb_colors
    obs = torch.rand((n, H, W, C), dtype=torch.float32, device=dev)
    for fit in (False, True):
        if fit:
            r.render_fit(ds, obs, 1.0, clear_grads=True)
        else:
            r.render(ds, 1.0, check_overflow=True)
        torch.cuda.synchronize()
        ws = r.workspace.view(torch.uint8).cpu().numpy()
        words = np.stack([ws[v * (r.nbytes // n) :][:64].view(np.uint32) for v in range(n)])  # WsHeader of every view (dr_workspace.h)
        G, Gh = walkers((H // 8) * (W // 8), n, fit, fit)  # (sigma > 0: a fit step fuses its edge tiles, textured or not)
        rows = lambda count, stride: int(-(-int(count) // stride)) if stride else 0  # the longest run of entries one walker gets
        print(f"{name}, {n} view(s), {'fit step' if fit else 'render'}: head entries {words[:, 13].tolist()}, other entries {words[:, 14].tolist()}, tiles {(H // 8) * (W // 8)}, "
              f"{G} walkers per view, {Gh} on the head: at most {rows(words[:, 13].max(), Gh)} head entries and {rows(words[:, 14].max(), G - Gh)} other entries per walker, "
              f"census {hr.tile_census(r, ds)}", flush=True)  # fmt: skip


for nv in (1, 8):
    census("configs[2] sphere 20k", [scenes.sphere_scene(size=1024, angle=float(a)) for a in np.linspace(-0.5, 0.5, nv)])
big = dict(size=2048, nu=224, n_rings=224, nb_colors=3, textured=True, texture_size=1024)
for nv in (1, 8):
    census("configs[4] shape", [scenes.sphere_scene(angle=float(a), **big) for a in np.linspace(-0.5, 0.5, nv)])
