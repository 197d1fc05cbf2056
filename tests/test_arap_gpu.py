"""GPU checks of the as-rigid-as-possible kernels (include/deodr_hip_arap.h, deodr_amd/csrc/dr_arap.h): energy, gradient and rotations against the
long-double restatement of tests/arap_reference.py within 8 x the measured float64 error, on every mesh x deformation of the tables at n = 1, 2, 3
poses; strips at every V where the exported launch rule changes the geometry; the two exact cases bit for bit; ``rotations = NULL``; outputs and
scratch between guards, the scratch pre-filled with NaN; two calls bit-identical; a captured graph replayed over overwritten vertices; the autograd
op through ``Scene3DDevice.render_l2``; an eager and a ``GraphedStep`` fit."""

import numpy as np
import pytest
import torch

import arap_reference as ar
from test_basis_gpu import Arena, host

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD_BYTES, GUARD_BYTE = 4096, 0xA5


class GuardedScratch:
    """exactly deodr_hip_arap_scratch_bytes bytes filled with NaN, between two guards in the same allocation"""

    def __init__(self, V, n):
        from deodr_amd.hip_renderer import lib

        self.nbytes = int(lib().deodr_hip_arap_scratch_bytes(V, n))
        assert self.nbytes == 64 + 8 * (5 * n * V + ar.MAX_BLOCKS * n + (n + 1) // 2)
        self.buffer = torch.full((self.nbytes + 2 * GUARD_BYTES,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.front = self.buffer[GUARD_BYTES : GUARD_BYTES + self.nbytes]
        self.front.view(torch.float64).fill_(float("nan"))
        assert self.front.data_ptr() % 8 == 0

    def check(self):
        assert bool((self.buffer[:GUARD_BYTES] == GUARD_BYTE).all()), "the memory in front of the scratch was written"
        assert bool((self.buffer[GUARD_BYTES + self.nbytes :] == GUARD_BYTE).all()), "the scratch was written beyond deodr_hip_arap_scratch_bytes"


def u32(a):
    return torch.as_tensor(np.ascontiguousarray(a).astype(np.uint32).view(np.int32), device=DEV)


def run(c, calls=2, rotations=True):
    """``calls`` calls of the library on the case, outputs and scratch guarded -> [(energy, gradient, rotations)]"""
    from deodr_amd import hip_renderer as hr

    n, V = c["p"].shape[:2]
    arena = Arena()
    offsets, cols = u32(c["offsets"]), u32(c["cols"])
    weights, q, p = arena.carve(c["weights"]), arena.carve(c["q"]), arena.carve(c["p"])
    scratch = GuardedScratch(V, n)
    outs = []
    for _ in range(calls):
        energy, gradient = arena.carve(shape=(n,)), arena.carve(shape=(n, V, 3))
        quats = arena.carve(shape=(n, V, 4)) if rotations else None
        got = hr.arap_energy(offsets, cols, weights, q, p, c["cregu"], energy=energy, gradient=gradient, rotations=quats, scratch=scratch.front)
        assert got[0] is energy and got[1] is gradient and got[2] is quats
        outs.append((energy, gradient, quats))
    torch.cuda.synchronize()
    arena.check(), scratch.check()
    return outs


def check_parity(c):
    first, second = run(c)
    for a, b in zip(first, second):
        assert torch.equal(a, b)  # bit-identical from run to run
    e, g, r = ar.errors(c, host(first[0]), host(first[1]), host(first[2]))
    assert not np.isnan(host(first[1])).any() and np.all(host(first[2])[..., 3] >= 0)
    print(f"{c['name']} {c['hows']}: energy / e_scale {e:.2e}, gradient / g_scale {g:.2e}, quaternions {r:.2e}")
    assert e <= ar.TOL_ENERGY and g <= ar.TOL_GRADIENT and r <= ar.TOL_QUATERNION, (c["name"], c["hows"], e, g, r)
    return first


@pytest.mark.parametrize("name", ar.MESHES)
def test_kernels_against_long_double(name):
    """every deformation of the tables, in groups of n = 1, 2, 3, 3 poses; the fans bring the valences 7, 8, 9, 16, 17 and 40, "vertex" V = 1 with
    nnz = 0"""
    for hows in ar.POSE_GROUPS:
        c = ar.case(name, hows)
        assert c["p"].shape[0] == len(hows) and (name != "vertex" or (len(c["cols"]) == 0 and len(c["q"]) == 1))
        check_parity(c)
    if name.startswith("fan"):
        assert int(np.diff(ar.mesh(name)[2][0].astype(np.int64)).max()) == int(name[3:])


def boundary_sizes():
    from deodr_amd import hip_renderer as hr

    return ar.boundary_sizes(hr.arap_blocks, hr.ARAP_BLOCK, hr.ARAP_MAX_BLOCKS)


@pytest.mark.parametrize("which", range(5))
def test_strips_where_the_launch_geometry_changes(which):
    """one below, at and one above a workgroup's worth of vertices, the first V whose partials take grid_sum's last workgroup a second round, the first
    V beyond the grid cap (the threads stride): the sizes come from the exported rule"""
    from deodr_amd import hip_renderer as hr

    V = boundary_sizes()[which]
    assert which != 3 or hr.arap_blocks(V) == ar.FH_BLOCK + 1
    assert which != 4 or (hr.arap_blocks(V) == hr.ARAP_MAX_BLOCKS and V > hr.ARAP_BLOCK * hr.ARAP_MAX_BLOCKS)
    check_parity(ar.case(f"strip{V}", ("bend", "noise1") if which < 3 else ("bend",)))  # (one pose at the two large sizes: the long-double reference takes seconds)


def test_the_two_exact_cases_bitwise():
    identity = np.array([0.0, 0, 0, 1])
    for name in ar.MESHES + ("strip257",):
        c = ar.case(name, ("rest", "coincident"))
        (energy, gradient, quats), _ = run(c)
        assert np.array_equal(host(quats), np.broadcast_to(identity, quats.shape)), name
        assert float(energy[0]) == 0.0 and not bool(gradient[0].any()), name
        assert abs(float(energy[1]) - float(c["energy"][1])) <= ar.TOL_ENERGY * float(c["e_scale"][1])
    q, faces, (offsets, cols, w) = ar.mesh("fan9")  # weights that are all zero: S = 0, R = identity, zeros
    c = dict(ar.case("fan9", ("noise30",)), weights=0 * w)
    (energy, gradient, quats), _ = run(c)
    assert np.array_equal(host(quats), np.broadcast_to(identity, quats.shape)) and float(energy[0]) == 0.0 and not bool(gradient.any())


def test_rotations_may_be_null():
    c = ar.case("icosphere162", ("bend", "noise1", "noise30"))
    (e0, g0, none), _ = run(c, rotations=False)
    (e1, g1, quats), _ = run(c)
    assert none is None and quats is not None and torch.equal(e0, e1) and torch.equal(g0, g1)


def test_a_replayed_graph_sees_the_vertices_of_the_moment():
    from deodr_amd import hip_renderer as hr

    c = ar.case("icosphere162", ("noise30", "bend"))
    others = [ar.case("icosphere162", hows) for hows in (("mirror", "rigid170"), ("noise1", "coincident"), ("rest", "translation"))]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    o, cl, w, q, p = u32(c["offsets"]), u32(c["cols"]), t(c["weights"]), t(c["q"]), t(c["p"])
    scratch = hr.arap_scratch(len(c["q"]), 2, DEV)
    energy, gradient, quats = hr.arap_energy(o, cl, w, q, p, c["cregu"], scratch=scratch, want_rotations=True)  # eager: allocates the outputs
    call = lambda: hr.arap_energy(o, cl, w, q, p, c["cregu"], energy=energy, gradient=gradient, rotations=quats, scratch=scratch)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        call()
    for other in others:  # three replays, the vertices overwritten in place between them: each equal to the eager call on the same data
        p.copy_(t(other["p"]))
        energy.zero_(), gradient.zero_(), quats.zero_()
        graph.replay()
        torch.cuda.synchronize()
        replayed = (energy.clone(), gradient.clone(), quats.clone())
        eager = hr.arap_energy(o, cl, w, q, p, c["cregu"], scratch=scratch, want_rotations=True)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(replayed, eager))
        e, g, r = ar.errors(other, host(replayed[0]), host(replayed[1]), host(replayed[2]))
        assert e <= ar.TOL_ENERGY and g <= ar.TOL_GRADIENT and r <= ar.TOL_QUATERNION


def hand():
    import os

    from conftest import GOLDEN
    from deodr_amd import scenes

    return scenes.load_hand_mesh(os.path.join(GOLDEN, "hand_mesh.npz"))[:2]


def test_op_through_render_l2_against_the_torch_fallback():
    from deodr_amd.arap import ArapEnergyDevice
    from deodr_amd.scene3d import DeviceCamera, DeviceMesh, Scene3DDevice

    vertices, faces = hand()
    rs = np.random.RandomState(4)
    rot = np.array([[1.0, 0, 0], [0, -1, 0], [0, 0, -1]])
    cam_center = vertices.mean(axis=0) + np.array([0, 0, 7.0]) * np.max(np.std(vertices, axis=0))
    camera = DeviceCamera(np.column_stack((rot, -rot.T.dot(cam_center))), np.array([[128.0, 0, 32], [0, 128.0, 32], [0, 0, 1]]), 64, 64)
    obs = torch.as_tensor(rs.rand(1, 64, 64, 3)).cuda()
    colors = rs.rand(len(vertices), 3)
    moved = vertices + 0.02 * np.std(vertices) * rs.randn(*vertices.shape)
    arap = ArapEnergyDevice(faces, vertices, 50.0, "cotangent", device=DEV)

    def gradient(with_arap):
        v = torch.tensor(moved, device=DEV, requires_grad=True)
        scene = Scene3DDevice()
        scene.set_mesh(DeviceMesh(faces, v, colors=colors))
        scene.set_light(np.array([-0.1, -0.5, -0.4]), 0.6)
        scene.set_background_color([0.5, 0.6, 0.7])
        loss, _ = scene.render_l2(camera, obs)
        energy = arap.evaluate(v)[0] if with_arap else 0.0
        (g,) = torch.autograd.grad(loss + 0.5 * energy, v)
        return g, energy

    assert arap.uses_kernel(torch.tensor(moved, device=DEV)) and not arap.uses_kernel(torch.tensor(moved)) and not arap.uses_kernel(torch.tensor(moved, device=DEV).float())
    g_both, energy = gradient(True)
    g_render, _ = gradient(False)
    cpu = ArapEnergyDevice(faces, vertices, 50.0, "cotangent", device="cpu")
    e_torch, g_torch = cpu.evaluate(torch.tensor(moved))
    scale = float(g_torch.abs().max())
    # the rasterizer's gradient comes from double atomics whose order is not fixed: 1e-10 of the larger gradient between two renders; the fallback's
    # SVD rotations: 1e-12
    assert abs(float(energy.detach()) - float(e_torch)) <= 1e-12 * float(e_torch) and float(e_torch) > 0
    assert float(((g_both - g_render).cpu() - 0.5 * g_torch).abs().max()) <= 1e-10 * max(scale, float(g_render.abs().max())) and scale > 0
    e32, g32 = arap.evaluate(torch.tensor(moved, device=DEV).float())  # what the kernels do not take goes through the torch ops
    assert e32.dtype == torch.float32 and abs(float(e32) - float(e_torch)) <= 1e-3 * float(e_torch)


def test_arap_depth_fit_eager_and_graphed():
    """eager steps of ``MeshDepthFitter(rigidity="arap")`` on the hand equal the steps under ``GraphedStep`` (the rasterizer's gradient accumulators
    are double atomics whose order is not fixed: 1e-6 of the first energy, as the other graphed fits are held to)"""
    from deodr_amd.arap import ArapEnergyDevice
    from deodr_amd.mesh_fitter import GraphedStep
    from test_basis_gpu import depth_fitter

    eager = depth_fitter(rigidity="arap")
    assert eager._direct_iteration(1, False) is None and type(eager.rigid_energy) is ArapEnergyDevice and eager.rigid_energy.uses_kernel(eager.vertices)
    e_eager = [float(eager.step_device()[0]) for _ in range(10)]
    print("eager:", e_eager)
    assert e_eager[-1] < e_eager[0]
    f = depth_fitter(rigidity="arap")
    graphed = GraphedStep(f, warmup=3)  # 3 + 1 eager steps and 1 on the capture stream: iterations 0 .. 4
    assert f.iter == 5
    e_graph = [float(graphed.step_device()[0]) for _ in range(5)]  # iterations 5 .. 9
    print("graphed:", e_graph)
    assert np.abs(np.array(e_graph) - np.array(e_eager[5:])).max() <= 1e-6 * e_eager[0]
    assert torch.allclose(f.vertices, eager.vertices, rtol=0, atol=1e-9)
