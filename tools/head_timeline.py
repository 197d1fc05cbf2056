"""The two bounds of the fused forward raster of the bench workload, from a -DDR_WAVE_TRACE build of the library (tools/build_variants.sh wavetrace):
  * the span of the kernel (first start to last end of its workgroups),
  * the life of the longest head walker, how many entries it walked, and the longest life of a head walker that walked ONE entry,
  * the time at which the last walker of the rest of the list ends, and the last fill workgroup.
The trace is indexed by workgroup; the fill workgroups carry a role bit, and the walkers are numbered in workgroup order (raster_fwd_fast_kernel), so
walker b -> (view, q) -> head or rest -> rank as in fwd_tiles; the head counts come from the views' workspace headers.  GPU box.
    python tools/head_timeline.py --lib tools/variants/libdeodr_hip_wavetrace.so [--views 8]"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deodr_amd import hip_renderer as hr
from deodr_amd import scenes
from deodr_amd.hip_renderer import DeviceScene, HipRasterizer

hr.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
B = int(sys.argv[sys.argv.index("--views") + 1]) if "--views" in sys.argv else 8
S, WORK_CHUNK = 1024, 64
dev = torch.device("cuda:0")
views = [scenes.sphere_scene(size=S, angle=float(a)) for a in np.linspace(-0.5, 0.5, B)]
s0 = views[0]
stack = lambda n: np.stack([np.asarray(getattr(v, n)) for v in views])
ds = DeviceScene(s0.faces, s0.faces_uv, s0.textured, s0.shaded, s0.uv, stack("ij"), stack("depths"), stack("colors"), stack("shade"),
                 stack("edgeflags"), S, S, texture=None, background_color=s0.background_color, clockwise=s0.clockwise,
                 vertex_dtype=torch.float64, pixel_dtype=torch.float32, device=dev)  # fmt: skip
r = HipRasterizer.for_scene(ds)
obs = torch.rand((B, S, S, ds.nb_colors), dtype=torch.float32, device=dev)
grads = ds.zero_grads()
for _ in range(20):
    r.render_fit(ds, obs, 1.0, grads=grads, clear_grads=True)
torch.cuda.synchronize()
L = hr.lib()
buf = np.zeros((3, 1 << 18, 2), dtype=np.uint64)
hw = np.zeros((3, 1 << 18, 2), dtype=np.uint32)
L.deodr_hip_debug_wave_trace.argtypes = [C.c_void_p, C.c_size_t]
L.deodr_hip_debug_wave_hw.argtypes = [C.c_void_p, C.c_size_t]
assert L.deodr_hip_debug_wave_trace(buf.ctypes.data, buf.nbytes) == 0 and L.deodr_hip_debug_wave_hw(hw.ctypes.data, hw.nbytes) == 0
assert r.nbytes % B == 0
ws = r.workspace.view(torch.uint8).cpu().numpy()
hdr = np.stack([ws[v * (r.nbytes // B):][:64].view(np.uint32) for v in range(B)])
n_head, n_rest = hdr[:, 13].astype(np.int64), hdr[:, 14].astype(np.int64)  # WsHeader::work_count (dr_workspace.h)

t = buf[2].astype(np.int64)
live = t[:, 1] > 0
live &= t[:, 0] > t[live, 0].max() - 20000  # the last launch only (200 us; entries of earlier, larger grids stay in the buffer)
idx = np.flatnonzero(live)
assert len(idx) == idx[-1] + 1, "the workgroups of the last launch are the first entries of the trace"
t0 = t[idx, 0].min()
start, end = (t[idx, 0] - t0) * 0.01, (t[idx, 1] - t0) * 0.01
fill = (hw[2][idx, 0] >> 31).astype(bool)
b = np.cumsum(~fill) - 1  # index among the walkers
ntiles = (S // 8) * (S // 8)
n_walk = int((~fill).sum())
G = n_walk // B
assert G * B == n_walk and G % (8 * WORK_CHUNK) == 0
want, share = (B * G + 4095) // 4096, 4  # heavy_share_for of a fit step with fused edge tiles (dr_forward.h)
while want > 8 and share < 16 and share < want:
    share *= 2
Gh = G // share
g8 = b >> 3
view, q = g8 % B, (g8 // B) * 8 + (b & 7)
head = ~fill & (q < Gh)
rest = ~fill & (q >= Gh)
qq = np.where(head, q, q - Gh)
stride = np.where(head, Gh, G - Gh)
chunk_here = stride % (8 * WORK_CHUNK) == 0
rank = np.where(chunk_here, (((qq >> 3) // WORK_CHUNK) * 8 + (qq & 7)) * WORK_CHUNK + (qq >> 3) % WORK_CHUNK, qq)
count = np.where(head, n_head[view], n_rest[view])
entries = np.where(rank < count, (count - rank + stride - 1) // stride, 0)
life = end - start
print(f"{os.path.basename(hr.LIB_PATH)}: {B} views, {len(idx)} workgroups ({int(fill.sum())} fill), G = {G} walkers per view, {Gh} of them on the head (1/{share})")
print(f"   head entries per view {n_head.tolist()}, other entries {n_rest.tolist()}")
print(f"   head walkers by entries walked: " + ", ".join(f"{k}: {int((entries[head] == k).sum())}" for k in range(0, int(entries[head].max()) + 1)))
print(f"   rest walkers by entries walked: " + ", ".join(f"{k}: {int((entries[rest] == k).sum())}" for k in range(0, int(entries[rest].max()) + 1)))
print(f"kernel span {end.max():.1f} us")
i = np.flatnonzero(head)[np.argmax(life[head])]
print(f"longest head walker: life {life[i]:.1f} us (start {start[i]:.1f}, end {end[i]:.1f}), view {view[i]}, rank {rank[i]}, {entries[i]} entries")
one = head & (entries == 1)
if one.any():
    i = np.flatnonzero(one)[np.argmax(life[one])]
    print(f"longest head walker with ONE entry: life {life[i]:.1f} us (start {start[i]:.1f}, end {end[i]:.1f}), view {view[i]}, rank {rank[i]}")
for k in range(1, int(entries[head].max()) + 1):
    m = head & (entries == k)
    if m.any():
        print(f"   head walkers with {k} entries: life mean {life[m].mean():.1f} p90 {np.percentile(life[m], 90):.1f} p99 {np.percentile(life[m], 99):.1f} max {life[m].max():.1f} us, last end {end[m].max():.1f}")
print(f"last head walker ends at {end[head].max():.1f} us (last start {start[head].max():.1f})")
print(f"last walker of the rest ends at {end[rest].max():.1f} us (last start {start[rest].max():.1f}; life mean {life[rest].mean():.1f} max {life[rest].max():.1f})")
if fill.any():
    print(f"last fill workgroup ends at {end[fill].max():.1f} us")
late = np.argsort(-end)[:8]
print("last to end (class, start, life, entries):", [("fill" if fill[i] else "head" if head[i] else "rest", round(float(start[i]), 1), round(float(life[i]), 1), int(entries[i])) for i in late])
print(f"slot-time: head {life[head].sum() / 5120:.1f} us, rest {life[rest].sum() / 5120:.1f} us, fill {life[fill].sum() / 5120:.1f} us of 5 120 wave slots")
