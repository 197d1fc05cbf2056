"""Timings of texture estimation, all in ONE process and GPU visit, variants alternated after a warm-up (prints; redirect into profiles/texture_fit_times.txt):
  1. deodr_hip_texture_smoothness and deodr_hip_texture_step at 256^2 x 3 and 1024^2 x 3, float32: us per launch from device events, the bytes each moves
     by its shape over that time, next to deodr_hip_copy_probe's copy of the same number of bytes per array and of 256 MiB;
  2. one MeshTextureFitterMultiFrame iteration at the sizes of the benchmark's 8-view textured configuration (configs[4]: 2048^2, 224 x 224 sphere, 1024^2
     texture): eager, as a graph replay, and with the texture update written as torch ops (the only way before these kernels); the update's share.
"""
import os, sys, time, statistics
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deodr_amd import scenes, hip_renderer as hr
from deodr_amd import mesh_fitter as mf

arg = lambda name, default: type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
dev = torch.device("cuda:0")


def event_us(fn, reps):
    """us per call of `fn` from a device event pair around `reps` back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def alternate(fns, measure, rounds=7, warm=30):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(measure(fn))
    return out


def wall_ms(fn, steps=100):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


# ---- 1. the two kernels ----------------------------------------------------------------------------------------------------------------
L = hr.lib()
big = 256 << 20
big_src, big_dst = torch.empty(big, dtype=torch.uint8, device=dev), torch.empty(big, dtype=torch.uint8, device=dev)
for size in (256, 1024):
    t = torch.rand(size, size, 3, device=dev)
    g, s = torch.randn_like(t), torch.zeros_like(t)
    e = torch.zeros(1, dtype=torch.float64, device=dev)
    nbytes = t.numel() * 4
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = hr._stream(dev)
    fns = {
        "texture_smoothness": lambda: hr.texture_smoothness(t, g, 1e-3, e),
        "texture_step": lambda: hr.texture_step(t, s, g, 1e-3, None, 0.9, 0.05, (0.0, 1.0)),
        "copy_probe same size": lambda: L.deodr_hip_copy_probe(dst.data_ptr(), src.data_ptr(), nbytes, 0, 1, stream),
        "copy_probe 256 MiB": lambda: L.deodr_hip_copy_probe(big_dst.data_ptr(), big_src.data_ptr(), big, 0, 1, stream),
    }
    moved = {"texture_smoothness": 3 * nbytes, "texture_step": 5 * nbytes, "copy_probe same size": 2 * nbytes, "copy_probe 256 MiB": 2 * big}
    reps = {k: (20 if "256 MiB" in k else 400) for k in fns}
    res = alternate(fns, None, rounds=0)  # warm-up only
    out = {k: [] for k in fns}
    for _ in range(7):
        for k, fn in fns.items():
            out[k].append(event_us(fn, reps[k]))
    for k, v in out.items():
        us = statistics.median(v)
        print(f"{size}^2 x 3 float32  {k}: median {us:.2f} us / launch (min {min(v):.2f}, max {max(v):.2f}), {moved[k] / 1e6:.2f} MB by shape -> {moved[k] / us / 1e6:.3f} TB/s",
              flush=True)

# ---- 2. one fitter iteration at configs[4] sizes -----------------------------------------------------------------------------------------
S, NU, TEX, B = arg("--size", 2048), arg("--nu", 224), arg("--texture", 1024), arg("--views", 8)
vertices, faces = scenes.bumpy_sphere(NU, NU)
angles = [2 * np.pi * k / B for k in range(B)]
s0 = scenes.sphere_scene(S, NU, NU, nb_colors=3, textured=True, texture_size=TEX, angle=0.0)
cameras = [scenes.fit_camera(S, S, 60.0, vertices, scenes.rotx(0.37) @ scenes.roty(0.23 + a)) for a in angles]
obs = np.random.RandomState(0).rand(B, S, S, 3).astype(np.float32)


def fitter():
    f = mf.MeshTextureFitterMultiFrame(vertices, faces.astype(np.int64), s0.uv, faces.astype(np.int64), np.full((TEX, TEX, 3), 0.5), [-0.1, -0.5, -0.4], 0.6,
                                       cameras=cameras, clockwise=bool(s0.clockwise), device=dev, pixel_dtype=torch.float32)
    f.set_background_color(np.asarray(s0.background_color))
    f.set_images(obs)
    return f


class TorchUpdate(mf.MeshTextureFitterMultiFrame):
    """the same iteration with the texture update as torch ops on the device"""

    def step_device(self):
        ds, r, grads, out = self._direct
        image, _z, _g = r.render_fit(ds, self._obs, self.scene.sigma, grads=grads, out=out, clear_grads=True, loss_out=self.e_data, weights=self.weights)
        self.e_smooth.copy_(mf.texture_smoothness_torch(self.texture, grads["texture_b"], self.smoothness).reshape(1))
        mf.texture_step_torch(self.texture, self.momentum.speed["texture"], grads["texture_b"], self.step_factor_texture, self.step_max, self.inertia,
                              self.damping, self.clamp)
        torch.add(self.e_data, self.e_smooth, out=self._energy)
        self.iter += 1
        return self._energy, image


eager, torch_ops = fitter(), fitter()
torch_ops.__class__ = TorchUpdate
graphed = mf.GraphedStep(fitter())
ds, r, grads, out_buffers = eager._direct
raster_only = lambda: r.render_fit(ds, eager._obs, 1.0, grads=grads, out=out_buffers, clear_grads=True, loss_out=eager.e_data)


def update_only():
    hr.texture_smoothness(eager.texture, grads["texture_b"], eager.smoothness, eager.e_smooth, scratch=eager._scratch)
    hr.texture_step(eager.texture, eager.momentum.speed["texture"], grads["texture_b"], 0.0, None, 0.9, 0.05, (0.0, 1.0))


fns = {"iteration, eager": eager.step_device, "iteration, graph replay": graphed.step_device, "iteration, update as torch ops": torch_ops.step_device,
       "rasterizer fit step alone": raster_only, "texture update alone (2 launches)": update_only}
res = alternate(fns, wall_ms, rounds=5, warm=20)
med = {k: statistics.median(v) for k, v in res.items()}
for k, v in res.items():
    print(f"{B} views {S}^2, texture {TEX}^2 x 3 float32  {k}: median {med[k]:.4f} ms (min {min(v):.4f}, max {max(v):.4f})", flush=True)
print(f"share of the texture update in an eager iteration: {100 * med['texture update alone (2 launches)'] / med['iteration, eager']:.1f} %; "
      f"torch-op update costs {med['iteration, update as torch ops'] - med['iteration, eager']:.4f} ms more per iteration", flush=True)
