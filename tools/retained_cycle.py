"""python tools/retained_cycle.py -- a fit loop whose tiles flip at every step: the 8-view benchmark scene in 8 slightly different poses, cycled.  Step time with and without
retain_frames, and the share of bitmap words (32 tiles) in which a tile that held a covered pixel in the previous pose holds none in this one
(tiles by finite depth: a lower bound of `received a primitive` by the tiles a bounding box touches without covering a pixel)."""
import sys, os, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deodr_amd import scenes
from deodr_amd.hip_renderer import DeviceScene, HipRasterizer
B, S, POSES = 8, 1024, 8


def main():
    dev = torch.device("cuda:0")
    def pose(k):
        views = [scenes.sphere_scene(size=S, angle=float(a) + 0.004 * k) for a in np.linspace(-0.5, 0.5, B)]
        s0 = views[0]
        stack = lambda n: np.stack([np.asarray(getattr(v, n)) for v in views])
        return DeviceScene(s0.faces, s0.faces_uv, s0.textured, s0.shaded, s0.uv, stack("ij"), stack("depths"), stack("colors"), stack("shade"), stack("edgeflags"),
                           S, S, texture=None, background_color=s0.background_color, clockwise=s0.clockwise, vertex_dtype=torch.float64, pixel_dtype=torch.float32, device=dev)
    dss = [pose(k) for k in range(POSES)]
    for d in dss[1:]:
        d.background_color = dss[0].background_color  # one background tensor
    C = dss[0].nb_colors
    obs = torch.rand((B, S, S, C), dtype=torch.float32, device=dev)
    image = torch.empty((B, S, S, C), dtype=torch.float32, device=dev)
    z = torch.empty((B, S, S), dtype=torch.float32, device=dev)
    grads = dss[0].zero_grads()
    def words(zz):
        t = torch.isfinite(zz).reshape(B, S // 8, 8, S // 8, 8).any(dim=4).any(dim=2).reshape(B, -1)  # [B, tiles]
        return t.reshape(B, -1, 32)
    res = {}
    for retain in (True, False, True, False):
        r = HipRasterizer.for_scene(dss[0], retain_frames=retain)
        r.render(dss[0], 1.0, out=(image, z), check_overflow=True)
        step = [0]
        def fit():
            r.render_fit(dss[step[0] % POSES], obs, 1.0, grads=grads, out=(image, z), check_overflow=False, clear_grads=True)
            step[0] += 1
        for _ in range(200):
            fit()
        best = 1e9
        for _ in range(5):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(200):
                fit()
            torch.cuda.synchronize(); best = min(best, (time.perf_counter() - t0) / 200)
        res.setdefault(retain, []).append(best * 1e3)
        print(f"retain_frames={retain}: {best * 1e3:.4f} ms / step over {POSES} cycled poses", flush=True)
    # words that needed a fill, pose k - 1 -> pose k
    r = HipRasterizer.for_scene(dss[0], retain_frames=False)
    prev, shares, tiles_flip = None, [], []
    for k in list(range(POSES)) + [0]:
        r.render_fit(dss[k], obs, 1.0, grads=grads, out=(image, z), check_overflow=False, clear_grads=True)
        torch.cuda.synchronize()
        cur = words(z)
        if prev is not None:
            need = (prev & ~cur)
            shares.append(float(need.any(dim=2).float().mean())); tiles_flip.append(int(need.sum()))
        prev = cur
    print(f"share of bitmap words with a tile to fill, per step: mean {np.mean(shares):.4f} (min {min(shares):.4f}, max {max(shares):.4f}); tiles to fill per step: mean {np.mean(tiles_flip):.0f} of {B * (S // 8) ** 2}")
    print("summary", {k: [round(x, 4) for x in v] for k, v in res.items()})


if __name__ == "__main__":
    main()
