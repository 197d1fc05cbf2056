"""The vertex-side kernels of a fit iteration (deodr_amd/csrc/dr_fronthalf.h, dr_fititer.h) where their launch geometry changes, against
the long-double NumPy reference tests/fititer_reference.py: the grid cap and the strided trips of fit_pose_project_b_kernel, the rounds of
its last workgroup's sum, the trips of its loop over the views (up to FIT_MAX_VIEWS), grid_sum with more workgroups than threads (rigid
energy, vertex_shade_b1, the momentum update's mean_out), gather lists of 8, 9, 16 and 17 entries, wavefronts of vertex_shade_b1 that span
two views, the tiniest inputs, and the frame sums at their chunk and stride boundaries.

Tolerances.  tests/test_fititer_reference.py measures, over every shape below, how far float64 arithmetic of the same formulas (np.sum
order) lies from the long-double reference: sums in units of eps64 * sum |term|, elementwise outputs in units of eps64 * max |reference|:

    E_sum  = 2.93  (the column mean of vertices_b of a one-vertex cloud)        recorded below as E_SUM  = 3
    E_elem = 183.7 (posed_b of the shading adjoint at the 128-face poles)       recorded below as E_ELEM = 184

The kernels are held to max(16, 8 E) of the same units, TOL_SUM = 24 and TOL_ELEM = 1472: 8 is the margin for their different order of
additions and for FMA contraction.  A workgroup's partial, a vertex or a view that goes missing is at least 1/N of sum |term|, about 1e-5:
eight orders of magnitude above either bound.

Every case: the scratch has exactly deodr_hip_fit_scratch_bytes(V, n) bytes and is followed by a guard pattern; the outputs are carved out
of NaN-filled buffers whose surroundings must stay NaN; the 16 counter words are zero afterwards; the call is made twice on one scratch and
gives the same bits (all but the q_b / t_b of rigid_transform_b_kernel, which leave through atomics).  Cases that exist for a regime assert,
from the constants of the kernel headers, that they are in it."""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fititer_reference as fr
from fititer_reference import LD

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not fr.longdouble_is_extended(), reason="np.longdouble is not wider than float64 here: no reference")]

E_SUM = 3
E_ELEM = 184
TOL_SUM, TOL_ELEM = max(16, 8 * E_SUM), max(16, 8 * E_ELEM)

K = fr.kernel_constants()
F32, F64 = torch.float32, torch.float64
DEV = "cuda"
PAD = 64  # elements either side of a carved output (a multiple of 32 bytes for every dtype here: the carved tensor keeps the alignment)
GUARD_BYTES, GUARD_BYTE = 4096, 0xA5


def dev(a, dtype=F64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


class Arena:
    """outputs carved out of larger buffers filled with NaN (0xA5 for bytes)"""

    def __init__(self):
        self.made = []

    def out(self, *shape, dtype=F64):
        numel = int(np.prod(shape))
        fill = GUARD_BYTE if dtype == torch.uint8 else float("nan")
        buffer = torch.full((2 * PAD + numel,), fill, dtype=dtype, device=DEV)
        self.made.append((buffer, numel, shape))
        return buffer[PAD : PAD + numel].view(*shape)

    def check(self, all_written=True):
        for buffer, numel, shape in self.made:
            around = torch.cat((buffer[:PAD], buffer[PAD + numel :]))
            assert bool((around == GUARD_BYTE).all() if buffer.dtype == torch.uint8 else around.isnan().all()), f"written outside an output of shape {shape}"
            if all_written and buffer.dtype != torch.uint8:
                assert not bool(buffer[PAD : PAD + numel].isnan().any()), f"an output of shape {shape} was not written everywhere"

    def nothing_written(self):
        for buffer, _numel, shape in self.made:
            assert bool((buffer == GUARD_BYTE).all() if buffer.dtype == torch.uint8 else buffer.isnan().all()), shape


class Scratch:
    """exactly deodr_hip_fit_scratch_bytes(V, n) bytes, zero-filled, followed in the same allocation by a guard pattern"""

    def __init__(self, V, n):
        from deodr_amd.hip_renderer import lib

        self.nbytes = int(lib().deodr_hip_fit_scratch_bytes(int(V), int(n)))
        assert self.nbytes > 64
        self.buffer = torch.zeros(self.nbytes + GUARD_BYTES, dtype=torch.uint8, device=DEV)
        self.buffer[self.nbytes :] = GUARD_BYTE
        self.front = self.buffer[: self.nbytes]

    def check(self):
        assert bool((self.buffer[self.nbytes :] == GUARD_BYTE).all()), "the scratch was written beyond deodr_hip_fit_scratch_bytes"
        assert int(self.front[:64].view(torch.int32).abs().sum()) == 0, "a counter word did not come back to zero"


def close_elem(got, ref, what):
    d = fr.elem_distance(host(got) if torch.is_tensor(got) else got, ref)
    print(f"{what}: {d:.2f} eps64 max|ref|")
    assert d <= TOL_ELEM, (what, d)


def close_sum(got, pair, what):
    d = fr.sum_distance(host(got) if torch.is_tensor(got) else got, pair)
    print(f"{what}: {d:.2f} eps64 sum|term|")
    assert d <= TOL_SUM, (what, d)


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def camera(d, n, distortion):
    from deodr_amd.scene3d import DeviceCamera

    return DeviceCamera(d["extrinsic"], d["intrinsic"], 96, 128, d["distortion"] if distortion else None, DEV)


def assert_point_regime(V, n):
    """the regime a case of the table is there for, from the constants of the headers"""
    g = fr.pose_b_geometry(V, n, K)
    lanes, block = K["GATHER_LANES"], K["FH_BLOCK"]
    if (V, n) == (1025, 17):
        assert fr.ceil_div(V * lanes, block) > (block // 64) * 8 and g["sum_rounds"] == 2 and g["view_trips"] == 3 and n % lanes == 1
    if (V, n) == (2049, 2):
        assert fr.ceil_div(V * lanes, block) > K["POSE_B_BLOCKS"] and g["strided_trips"] == 2 and V - g["grid"] * g["per_block"] == 1
    if (V, n) == (4100, 64):
        assert n == K["FIT_MAX_VIEWS"] and g["view_trips"] == K["FIT_MAX_VIEWS"] // lanes and g["strided_trips"] == 3 and g["sum_rounds"] == 2
    if (V, n) == (16385, 1):
        assert g["lanes"] == 1 and fr.ceil_div(V, block) > K["POSE_B_BLOCKS"] and g["strided_trips"] == 2 and g["sum_rounds"] == 2
    if (V, n) in ((31, 3), (32, 8), (33, 9)):
        assert g["wanted"] == (2 if V == 33 else 1) and g["view_trips"] == (2 if n == 9 else 1) and (V * lanes - block) in (-8, 0, 8)
    if (V, n) in ((255, 1), (256, 1), (257, 1)):
        assert g["lanes"] == 1 and g["wanted"] == (2 if V == 257 else 1) and abs(V - block) <= 1


@functools.lru_cache(maxsize=2)
def point_case(V, n):
    return fr.point_inputs(V, n)


# ---- A. point clouds -----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("oname", list(fr.POINT_OPTIONS))
@pytest.mark.parametrize("V,n", fr.POINT_CASES)
def test_pose_and_projection_of_a_point_cloud(V, n, oname):
    """fit_pose_project, fit_pose_project_b and views_gradient_sum"""
    from deodr_amd import fronthalf

    assert_point_regime(V, n)
    options, d = fr.POINT_OPTIONS[oname], point_case(V, n)
    ref = fr.point_reference(V, n, options, LD, d)
    assert 5 < float(ref["depths"].min()) and float(ref["depths"].max()) < 12
    cam = camera(d, n, options["distortion"])
    q, t = dev(d["quaternions"]), dev(d["translations"])
    mean = dev(d["vertices"].mean(axis=0)) if options["centre"] else None
    # ---- forward
    arena, runs = Arena(), []
    vertices = arena.out(V, 3)
    posed, ij, depths = arena.out(n, V, 3), arena.out(n, V, 2), arena.out(n, V)
    depth_colors = arena.out(n, V) if options["centre"] else None
    for _ in range(2):
        vertices.copy_(dev(d["vertices"]))  # (centred in place)
        fronthalf.fit_pose_project(vertices, mean, q, t, cam, posed, ij, depths, depth_colors=depth_colors, depth_scale=fr.DEPTH_SCALE)
        runs.append([x.clone() for x in (vertices, posed, ij, depths)] + ([depth_colors.clone()] if options["centre"] else []))
    arena.check()
    assert same_bits(*runs)
    for key, got in zip(("centred", "posed", "ij", "depths", "depth_colors"), runs[0]):
        close_elem(got, ref[key], key)
    # ---- adjoint of pose and projection
    C_ = options["C"]
    ij_b = dev(d["ij_b"])
    depths_b = dev(d["depths_b"]) if options["depths_b"] else None
    posed_b = dev(d["posed_b"]) if options["posed_b"] else None
    colors_b = dev(d["colors_b"][..., :C_]) if C_ else None
    arena, scratch, runs = Arena(), Scratch(V, n), []
    vertices_b, out = arena.out(V, 3), arena.out(3 + 7 * n)
    colors_sum = arena.out(V, C_) if C_ else None
    for _ in range(2):
        fronthalf.fit_pose_project_b(vertices, q, posed, cam, posed_b, ij_b, depths_b, vertices_b, out, scratch.front, depths_b_scale=fr.DEPTHS_B_SCALE,
                                     colors_b=colors_b, colors_sum=colors_sum)  # fmt: skip
        runs.append([x.clone() for x in (vertices_b, out)] + ([colors_sum.clone()] if C_ else []))
        scratch.check()
    arena.check()
    assert same_bits(*runs)
    close_elem(vertices_b, ref["vertices_b"], "vertices_b")
    close_sum(out[:3], ref["mean"], "mean of vertices_b")
    close_sum(out[3 : 3 + 4 * n].view(n, 4), ref["q_b"], "quaternion adjoints")
    close_sum(out[3 + 4 * n :].view(n, 3), ref["t_b"], "translation adjoints")
    if C_:
        close_elem(colors_sum, ref["colors_sum"], "colors_sum")
    # ---- what the views share: the camera adjoints summed over the views
    arena, runs = Arena(), []
    shared_b = arena.out(V, 3)
    shared_colors = arena.out(V, C_) if C_ else None
    for _ in range(2):
        fronthalf.views_gradient_sum(posed, cam, ij_b, shared_b, depths_b=depths_b, depths_b_scale=fr.DEPTHS_B_SCALE, colors_b=colors_b, colors_sum=shared_colors)
        runs.append([shared_b.clone()] + ([shared_colors.clone()] if C_ else []))
    arena.check()
    assert same_bits(*runs)
    close_elem(shared_b, ref["views_sum"], "views_gradient_sum")
    if C_:
        assert torch.equal(shared_colors, colors_sum)  # (the same sums in the same order over the views)


@pytest.mark.parametrize("V,n", fr.POINT_CASES)
def test_autograd_ops_of_a_point_cloud(V, n):
    """RigidTransformFunc and ProjectPointsFunc, values and adjoints (the quaternion and translation adjoints of the former leave through
    atomics: equal to rounding from run to run, everything else bit for bit)"""
    from deodr_amd import fronthalf

    d = point_case(V, n)
    ref = fr.autograd_ops_reference(V, n, LD, d)
    runs = []
    for _ in range(2):
        x, q, t = (dev(a).requires_grad_(True) for a in (d["vertices"], ref["unit_quaternions"], d["translations"]))
        posed = fronthalf.RigidTransformFunc.apply(x, q, t)
        gx, gq, gt = torch.autograd.grad((posed * dev(d["posed_b"])).sum(), [x, q, t])
        p = dev(ref["points"]).requires_grad_(True)
        cam = camera(d, n, True)
        ij, depths = fronthalf.ProjectPointsFunc.apply(p, cam.extrinsic, cam.intrinsic, cam.distortion)
        (gp,) = torch.autograd.grad((ij * dev(d["ij_b"])).sum() + (depths * dev(d["depths_b"])).sum(), [p])
        runs.append([posed.detach(), gx, ij.detach(), depths.detach(), gp])
        close_sum(gq, ref["q_b"], "q_b")
        close_sum(gt, ref["t_b"], "t_b")
    assert same_bits(*runs)
    for key, got in zip(("posed", "vertices_b", "ij", "depths", "points_b"), runs[0]):
        close_elem(got, ref[key], key)


@pytest.mark.parametrize("distortion", [False, True], ids=["plain", "distorted"])
@pytest.mark.parametrize("V,n", [(33, 9), (257, 1)])
def test_fused_and_plain_kernels_share_their_algebra(V, n, distortion):
    """The pose, the projection and its adjoint exist once in the device code (dr_fronthalf.h), so the fused kernels of a fit iteration and the
    plain ones give the same BITS: (33, 9) has eight lanes per vertex, two trips over the views and a part-filled second workgroup, (257, 1)
    the one-lane instances with one vertex past a workgroup."""
    from deodr_amd import fronthalf
    from deodr_amd.hip_renderer import _launch, _ptr, lib

    assert_point_regime(V, n)
    d = point_case(V, n)
    cam = camera(d, n, distortion)
    q, t, mean = dev(d["quaternions"]), dev(d["translations"]), dev(d["vertices"].mean(axis=0))
    arena = Arena()
    vertices = arena.out(V, 3)
    posed, ij, depths = arena.out(n, V, 3), arena.out(n, V, 2), arena.out(n, V)
    vertices.copy_(dev(d["vertices"]))  # (centred in place)
    fronthalf.fit_pose_project(vertices, mean, q, t, cam, posed, ij, depths)
    # the projection of the fused kernel = project_points_kernel on the posed vertices it wrote
    ij_plain, depths_plain = arena.out(n, V, 2), arena.out(n, V)
    fronthalf.project_points(posed, cam.extrinsic, cam.intrinsic, cam.distortion, ij_plain, depths_plain)
    assert torch.equal(ij, ij_plain) and torch.equal(depths, depths_plain)
    # its pose = rigid_transform_kernel with the quaternions normalised as load_unit_quaternion does: every component DIVIDED by the norm
    x, y, z, w = (d["quaternions"][:, i] for i in range(4))
    norm = np.sqrt(((x * x + y * y) + z * z) + w * w)
    unit_q = dev(d["quaternions"] / norm[:, None])
    posed_plain = arena.out(n, V, 3)
    _launch(lib().deodr_hip_rigid_transform, posed.device, _ptr(vertices), _ptr(unit_q), _ptr(t), _ptr(posed_plain), V, n)
    assert torch.equal(posed, posed_plain)
    if n == 1:  # one view: the sum over the views of the camera adjoints is project_points_b_kernel's one
        ij_b, depths_b = dev(d["ij_b"]), dev(d["depths_b"])
        shared_b, points_b = arena.out(V, 3), arena.out(n, V, 3)
        fronthalf.views_gradient_sum(posed, cam, ij_b, shared_b, depths_b=depths_b, depths_b_scale=fr.DEPTHS_B_SCALE)
        scaled = depths_b * fr.DEPTHS_B_SCALE  # (one IEEE multiply, as in the kernel)
        _launch(lib().deodr_hip_project_points_b, posed.device, _ptr(posed), _ptr(cam.extrinsic), _ptr(cam.intrinsic), _ptr(cam.distortion), _ptr(ij_b),
                _ptr(scaled), _ptr(points_b), V, n)  # fmt: skip
        assert torch.equal(shared_b, points_b[0])
    arena.check()


def test_more_views_than_fit_max_views_are_refused():
    from deodr_amd import fronthalf

    V, n = 8, K["FIT_MAX_VIEWS"] + 1
    d = fr.point_inputs(V, n)
    cam = camera(d, n, True)
    arena, scratch = Arena(), Scratch(V, n)
    vertices_b, out, colors_sum = arena.out(V, 3), arena.out(3 + 7 * n), arena.out(V, 3)
    posed = dev(np.broadcast_to(d["vertices"], (n, V, 3)) + np.array([0, 0, 1.0]))
    with pytest.raises(RuntimeError, match=f"at most {K['FIT_MAX_VIEWS']} views per call"):
        fronthalf.fit_pose_project_b(dev(d["vertices"]), dev(d["quaternions"]), posed, cam, dev(d["posed_b"]), dev(d["ij_b"]), dev(d["depths_b"]), vertices_b, out,
                                     scratch.front, colors_b=dev(d["colors_b"][..., :3]), colors_sum=colors_sum)  # fmt: skip
    torch.cuda.synchronize()
    arena.nothing_written()
    scratch.check()
    assert not bool(scratch.front.any())


# ---- B. meshes -----------------------------------------------------------------------------------------------------------------------


def assert_mesh_regime(name, V, n, faces):
    lanes, block = K["GATHER_LANES"], K["FH_BLOCK"]
    valence = np.bincount(faces.reshape(-1), minlength=V)
    if name.startswith("fan"):
        hub = int(name[3:])
        assert int(valence[0]) == hub and hub - (hub // lanes) * lanes in (0, 1) and hub // lanes in (1, 2)  # full rounds of the lanes, plus at most one entry
    if name == "sphere_7_4":
        assert V == 30 and V % lanes and n == 3 and n * V * lanes > 64  # a wavefront of vertex_shade_b1 spans two views
    if name == "sphere_33_31":
        assert V == 1025 and V % lanes and n == 3 and fr.ceil_div(n * V * lanes, block) > 1
    if name == "sphere_128_65":
        assert V == 8322 and fr.ceil_div(V * lanes, block) > block and int(valence.max()) == 128  # grid_sum's second trip; lists of 16 rounds
    if name == "triangle":
        assert V == 3 and len(faces) == 1 and V < lanes


@pytest.mark.parametrize("clockwise", [False, True])
@pytest.mark.parametrize("name", list(fr.MESH_CASES))
def test_shading_rigid_energy_and_flags_of_a_mesh(name, clockwise):
    """vertex_shade, vertex_shade_b, rigid_energy, silhouette_flags; fit_front against those three, bit for bit"""
    from deodr_amd import fronthalf
    from deodr_amd.scene3d import MeshTopology

    d = fr.mesh_inputs(name)
    V, n, T = len(d["vertices"]), d["n"], len(d["faces"])
    assert_mesh_regime(name, V, n, d["faces"])
    topo = MeshTopology(d["faces"], V, clockwise=clockwise, device=DEV)
    posed, light, ambient, color = dev(d["posed"]), dev(d["light"]), dev(d["ambient"]), dev(d["color"])
    scratch = Scratch(V, n)
    # ---- shading
    arena, runs = Arena(), []
    lum, colors = arena.out(n, V), arena.out(n, V, 3)
    for _ in range(2):
        fronthalf.vertex_shade(posed, topo, light, ambient, color, luminosity=lum, colors=colors)
        runs.append([lum.clone(), colors.clone()])
    arena.check()
    assert same_bits(*runs)
    ref = fr.shade(d["posed"], d["faces"], d["light"], d["ambient"], d["color"], clockwise, LD)
    close_elem(lum, ref["luminosity"], "luminosity")
    close_elem(colors, ref["colors"], "colors")
    assert 0.2 <= float((lum > ambient).double().mean()) <= 0.8  # lit and unlit vertices both present
    for what, lum_b, colors_b, col in (("luminosity_b and colors_b", d["luminosity_b"], d["colors_b"], d["color"]), ("luminosity_b", d["luminosity_b"], None, None)):
        arena, runs = Arena(), []
        nc = 0 if col is None else len(col)
        posed_b, out = arena.out(n, V, 3), arena.out(4 + nc)
        for _ in range(2):
            fronthalf.vertex_shade_b(posed, topo, light, ambient, None if col is None else color, dev(lum_b), None if colors_b is None else dev(colors_b),
                                     posed_b, out, scratch.front)  # fmt: skip
            runs.append([posed_b.clone(), out.clone()])
            scratch.check()
        arena.check()
        assert same_bits(*runs)
        ref = fr.shade_b(d["posed"], d["faces"], d["light"], d["ambient"], col, clockwise, lum_b, colors_b, LD)
        close_elem(posed_b, ref["posed_b"], f"posed_b ({what})")
        close_sum(out[:3], ref["light_b"], f"light_b ({what})")
        close_sum(out[3], ref["ambient_b"], f"ambient_b ({what})")
        if nc:
            close_sum(out[4:], ref["color_b"], "color_b")
    # ---- rigid energy, with the total energy on the way
    x, x_ref, data = dev(d["x"]), dev(d["ref"]), dev([fr.MESH_DATA_ENERGY])
    arena, runs = Arena(), []
    grad, energy = arena.out(V, 3), arena.out(2)
    for _ in range(2):
        fronthalf.rigid_energy(x, x_ref, topo, fr.MESH_CREGU, grad, energy, scratch.front, data_energy=data, data_weight=fr.MESH_DATA_WEIGHT)
        runs.append([grad.clone(), energy.clone()])
        scratch.check()
    arena.check()
    assert same_bits(*runs)
    off, cols, vals = (host(a) for a in topo._m_csr)
    ref = fr.rigid(d["x"], d["ref"], off.view(np.uint32), cols.view(np.uint32), vals, fr.MESH_CREGU, LD)
    close_elem(grad, ref["gradient"], "rigid gradient")
    close_sum(energy[0], ref["energy"], "rigid energy")
    assert float(ref["energy"][0]) > 0
    close_elem(energy[1:], np.array([LD(fr.MESH_DATA_WEIGHT) * LD(fr.MESH_DATA_ENERGY) + LD(float(energy[0]))]), "energy[1]")
    # ---- silhouette flags
    ij = dev(d["ij"])
    arena = Arena()
    flags = arena.out(n, T, 3, dtype=torch.uint8)
    fronthalf.silhouette_flags(ij, topo._faces_u32, topo._edge_faces, clockwise, out=flags)
    arena.check()
    flags_ref, _cr = fr.silhouette(d["ij"], d["faces"], clockwise, LD)
    assert np.array_equal(host(flags), flags_ref) and 0 < int(flags_ref.sum()) < flags_ref.size
    # ---- the three in one launch
    fronthalf.rigid_energy(x, x_ref, topo, fr.MESH_CREGU, grad, energy, scratch.front)  # (energy[1] untouched by fit_front: compare energy[0])
    for want_flags, want_shade, want_rigid in ((1, 1, 1), (0, 0, 1), (1, 1, 0)):
        arena = Arena()
        flags2, lum2, colors2, grad2, energy2 = arena.out(n, T, 3, dtype=torch.uint8), arena.out(n, V), arena.out(n, V, 3), arena.out(V, 3), arena.out(2)
        for _ in range(2):
            fronthalf.fit_front(topo, n, scratch.front, ij=ij, flags=flags2 if want_flags else None, posed=posed, light=light, ambient=ambient, color=color,
                                luminosity=lum2 if want_shade else None, colors=colors2 if want_shade else None, vertices=x, vertices_ref=x_ref,
                                cregu=fr.MESH_CREGU, gradient=grad2 if want_rigid else None, energy=energy2)  # fmt: skip
            scratch.check()
        arena.check(all_written=False)
        assert torch.equal(flags2, flags) if want_flags else bool((flags2 == GUARD_BYTE).all())
        assert (torch.equal(lum2, lum) and torch.equal(colors2, colors)) if want_shade else bool(lum2.isnan().all() and colors2.isnan().all())
        if want_rigid:
            assert torch.equal(grad2, grad) and float(energy2[0]) == float(energy[0]) and bool(energy2[1].isnan())
        else:
            assert bool(grad2.isnan().all() and energy2.isnan().all())


# ---- C. momentum update --------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(fr.MOMENTUM_LAUNCHES))
def test_momentum_update(name):
    """one launch for all the tensors, three consecutive steps, every step from the device's own state: x and speed elementwise, mean_out
    as a sum, energy[1]; a second copy of the state updated through the same scratch gives the same bits"""
    from deodr_amd import fronthalf

    (Vs, ns), entries, with_energy = fr.MOMENTUM_LAUNCHES[name]
    most = max(int(np.prod(e["shape"])) for e in entries)
    if name == "one":
        assert len(entries) == 1
    if name == "eight":
        assert len(entries) == K["MOMENTUM_MAX"] and sorted(int(np.prod(e["shape"])) for e in entries if not e["rows"]) == [1, 3, K["FH_BLOCK"] - 1, K["FH_BLOCK"], K["FH_BLOCK"] + 1]
        assert sorted(e["shape"][0] for e in entries if e["rows"]) == [1, 64, 300]
    if name == "wide":
        assert fr.ceil_div(most, K["FH_BLOCK"]) == K["FH_BLOCK"] + 1 and [int(np.prod(e["shape"])) for e in entries] == [most, 3] and all(e["mean_out"] for e in entries)
    x0, steps = fr.momentum_inputs(name)
    scratch, arena = Scratch(Vs, ns), Arena()
    state = []
    for copy in range(2):
        xs = [arena.out(*e["shape"]) for e in entries]
        speeds = [arena.out(*e["shape"]) for e in entries]
        means = [arena.out(3) if e["mean_out"] else None for e in entries]
        energy = arena.out(2)
        for x, s, a in zip(xs, speeds, x0):
            x.copy_(dev(a))
            s.zero_()
        state.append((xs, speeds, means, energy))
    data = dev([fr.MESH_DATA_ENERGY])
    cut = np.zeros(3, dtype=np.int64)
    for step, given in enumerate(steps):
        before = [(host(x).copy(), host(s).copy()) for x, s in zip(state[0][0], state[0][1])]
        for xs, speeds, means, energy in state:
            energy.copy_(dev([1.75 + step, float("nan")]))
            rows = [(xs[k], speeds[k], dev(g["grad"]), None if g["grad2"] is None else dev(g["grad2"]), e["factor"], e["step_max"], e["rows"], e["grad_scale"],
                     None if g["grad_mean"] is None else dev(g["grad_mean"]), means[k]) for k, (e, g) in enumerate(zip(entries, given))]  # fmt: skip
            fronthalf.momentum_update(rows, fr.MOMENTUM_INERTIA, fr.MOMENTUM_DAMPING, scratch=scratch.front, energy=energy if with_energy else None,
                                      data_energy=data if with_energy else None, data_weight=fr.MESH_DATA_WEIGHT)  # fmt: skip
            scratch.check()
        for a, b in zip(state[0][:3], state[1][:3]):
            assert all(x is None or torch.equal(x, y) for x, y in zip(a, b))
        xs, speeds, means, energy = state[0]
        for k, (e, g) in enumerate(zip(entries, given)):
            ref = fr.momentum_reference(e, before[k][0], before[k][1], g, LD)
            close_elem(xs[k], ref["x"], f"step {step} x[{k}]")
            close_elem(speeds[k], ref["speed"], f"step {step} speed[{k}]")
            if e["mean_out"]:
                close_sum(means[k], ref["mean"], f"step {step} mean_out[{k}]")
            if e["rows"]:
                assert float((xs[k].norm(dim=-1) - 1).abs().max()) < 1e-15 * 4
            if e["step_max"] is not None:
                cut += (ref["clamped"][0], ref["clamped"][1], before[k][0].size - sum(ref["clamped"]))
        if with_energy:
            assert float(energy[0]) == 1.75 + step
            close_elem(energy[1:], np.array([LD(fr.MESH_DATA_WEIGHT) * LD(fr.MESH_DATA_ENERGY) + LD(1.75 + step)]), "energy[1]")
        else:
            assert bool(energy[1].isnan())
    arena.check(all_written=False)
    assert cut.min() > 0, cut  # step_max hit on both sides, and not hit


def test_more_tensors_than_momentum_max_are_refused():
    from deodr_amd import fronthalf
    from deodr_amd.hip_renderer import _stream, lib

    k = K["MOMENTUM_MAX"] + 1
    arena = Arena()
    xs, speeds = [arena.out(5) for _ in range(k)], [arena.out(5) for _ in range(k)]
    grads = [dev(np.ones(5)) for _ in range(k)]
    with pytest.raises(AssertionError):
        fronthalf.momentum_update([(x, s, g, None, 0.1, None, 0) for x, s, g in zip(xs, speeds, grads)], 0.9, 0.05)
    ptrs = lambda ts: (C.c_void_p * k)(*[t.data_ptr() for t in ts])
    ones, counts, none = (C.c_double * k)(*[1.0] * k), (C.c_int * k)(*[5] * k), (C.c_void_p * k)(*[None] * k)
    rc = lib().deodr_hip_momentum_update(k, ptrs(xs), ptrs(speeds), ptrs(grads), none, ones, ones, counts, (C.c_int * k)(*[0] * k), 0.9, 0.05, ones, none, none,
                                         None, None, 1.0, None, 0, _stream(torch.device(DEV)))  # fmt: skip
    assert rc != 0 and f"at most {K['MOMENTUM_MAX']} tensors".encode() in lib().deodr_hip_last_error()
    torch.cuda.synchronize()
    arena.nothing_written()


# ---- D. frame sums -------------------------------------------------------------------------------------------------------------------


def np_type(dt):
    return np.float32 if dt == F32 else np.float64


def frame_pair(arena, count, dt, seed, offset=0):
    """two seeded frames of `count` values carved out of NaN-filled buffers (offset: the frames start that many elements later)"""
    rs = np.random.RandomState(seed)
    a, b = rs.rand(count).astype(np_type(dt)), rs.rand(count).astype(np_type(dt))
    out = []
    for values in (a, b):
        buffer = arena.out(count + offset, dtype=dt)
        buffer.fill_(0.5)
        t = buffer[offset:]
        t.copy_(dev(values, dt))
        out.append(t)
    return a, b, out[0], out[1]


@pytest.mark.parametrize("dt", [F32, F64], ids=["float32", "float64"])
def test_l2_loss_at_the_chunk_and_stride_boundaries(dt):
    from deodr_amd import fronthalf

    itemsize = 4 if dt == F32 else 8
    counts = fr.l2_counts(itemsize, K)
    g1, g2 = fr.l2_geometry(counts["beyond_one_stride"], itemsize, K), fr.l2_geometry(counts["beyond_a_round"], itemsize, K)
    assert g1["chunks"] > g1["stride"] and g1["tail"] and g2["chunks"] > K["L2_ROUND"] * g2["stride"] and g2["tail"]
    assert [counts[c] for c in ("one", "W-1", "W", "W+1")] == [1, 32 // itemsize - 1, 32 // itemsize, 32 // itemsize + 1]
    scratch = Scratch(100, 1)
    for cname, count in counts.items():
        arena = Arena()
        a, b, image, obs = frame_pair(arena, count, dt, count % 1000)
        out, again = arena.out(1), arena.out(1)
        fronthalf.l2_loss(image, obs, out, scratch.front)
        fronthalf.l2_loss(image, obs, again, scratch.front)
        scratch.check()
        arena.check()
        assert torch.equal(out, again)
        close_sum(out[0], fr.l2(a, b, dtype=LD), f"l2_loss {cname} = {count}")
    # frames that start one element into their allocation are not 32-byte aligned: refused before any launch
    arena = Arena()
    a, b, image, obs = frame_pair(arena, counts["beyond_one_stride"], dt, 7, offset=1)
    out = arena.out(1)
    with pytest.raises(RuntimeError, match="32-byte aligned"):
        fronthalf.l2_loss(image, obs, out, scratch.front)
    torch.cuda.synchronize()
    assert bool(out.isnan().all())
    scratch.check()


@pytest.mark.parametrize("dt", [F32, F64], ids=["float32", "float64"])
def test_depth_residual_at_the_stride_boundaries(dt):
    """the same counts, one beyond the grid cap of its own launch (a thread's second trip), and frames that start one element into their allocation"""
    from deodr_amd import fronthalf

    itemsize = 4 if dt == F32 else 8
    counts = dict(fr.l2_counts(itemsize, K))
    counts["beyond_the_cap"] = K["L2_BLOCKS"] * K["FH_BLOCK"] * 4 + 3
    assert fr.ceil_div(counts["beyond_the_cap"], K["FH_BLOCK"] * 4) > K["L2_BLOCKS"]
    scratch = Scratch(100, 1)
    for cname, count in counts.items():
        for offset in (0, 1) if cname in ("W+1", "beyond_one_stride") else (0,):
            arena = Arena()
            rs = np.random.RandomState(count % 1000 + offset)
            image_np = (rs.rand(count) * 1.4 - 0.2).astype(np_type(dt))  # some below 0, some above max_depth
            image_np[:2] = (0.0, 1.0)[: min(2, count)]  # the ends of the clamp pass the gradient
            obs_np = rs.rand(count)
            whole_image, whole_obs = arena.out(count + offset, dtype=dt), arena.out(count + offset)
            whole_image.fill_(0.5), whole_obs.fill_(0.5)
            image, obs = whole_image[offset:], whole_obs[offset:]
            image.copy_(dev(image_np, dt)), obs.copy_(dev(obs_np))
            runs = []
            depth, diff, image_b, loss = arena.out(count), arena.out(count), arena.out(count, dtype=dt), arena.out(1)
            for _ in range(2):
                fronthalf.depth_residual(image, obs, 1.0, depth, diff, image_b, loss, scratch.front)
                runs.append([x.clone() for x in (depth, diff, image_b, loss)])
                scratch.check()
            arena.check()
            assert same_bits(*runs)
            ref = fr.depth_residual(image_np, obs_np, 1.0, LD)
            assert np.array_equal(host(depth), ref["depth"]) and np.array_equal(host(image_b), ref["image_b"])
            close_elem(diff, ref["diff"], f"diff {cname}")
            close_sum(loss[0], ref["loss"], f"depth_residual {cname} = {count}{' offset' if offset else ''}")
            if count > 100:
                assert float((image_b == 0).double().mean()) > 0.1


def weighted_frames(itemsize, nb_colors):
    """(height, width) of the frames of the weighted sum: a few pixels, and the smallest frames whose H W C values go beyond one grid stride and
    beyond L2_ROUND strides of chunks with a ragged tail"""
    W = 32 // itemsize
    frames = [(1, p) for p in sorted({1, max(1, (W - 1) // nb_colors), fr.ceil_div(W, nb_colors), fr.ceil_div(W + 1, nb_colors)})]
    plain = fr.l2_counts(itemsize, K)
    for cname, key, least in (("beyond_one_stride", "strides", 1), ("beyond_a_round", "trips", 1)):
        height = 1 if plain[cname] < 16384 else 511  # (odd: H W C is then not always a multiple of the chunk)
        first = fr.ceil_div(plain[cname], nb_colors * height)
        ragged = nb_colors % W != 0  # (whole pixels of W channels' worth never leave a tail: float64 with four channels)
        geometry = lambda w: fr.l2_geometry(height * w * nb_colors, itemsize, K)
        frames.append((height, [w for w in range(first, first + 64) if geometry(w)[key] > least and (geometry(w)["tail"] or not ragged)][0]))
    return frames


@pytest.mark.parametrize("nb_colors", [1, 3, 4])
@pytest.mark.parametrize("dt", [F32, F64], ids=["float32", "float64"])
def test_weighted_l2_loss_of_a_fit_step(dt, nb_colors):
    """l2_loss_weighted_kernel, through the fit step of the un-staged kernels (the loss is then one pass over the finished frame): the sum of
    weight * (image - obs)^2 over the frame the step returned.  (The rasterizer owns that launch's scratch: no guard here.)  The weights start
    one element into their allocation in one case: they are read value by value."""
    from deodr_amd import hip_renderer as hr
    from deodr_amd.hip_renderer import DeviceScene, HipRasterizer

    itemsize = 4 if dt == F32 else 8
    frames = weighted_frames(itemsize, nb_colors)
    g1, g2 = (fr.l2_geometry(h * w * nb_colors, itemsize, K) for h, w in frames[-2:])
    ragged = nb_colors % (32 // itemsize) != 0
    assert g1["chunks"] > g1["stride"] and g2["chunks"] > K["L2_ROUND"] * g2["stride"] and (not ragged or (g1["tail"] and g2["tail"]))
    hr.force_generic(True)
    try:
        for number, (H, W) in enumerate(frames):
            rs = np.random.RandomState(H * W)
            ij = np.array([[[0.2 * W, 0.1 * H], [0.9 * W, 0.3 * H], [0.4 * W, 0.95 * H]]])
            ds = DeviceScene(np.array([[0, 1, 2]]), np.array([[0, 1, 2]]), np.zeros(1), np.zeros(1), np.zeros((3, 2)), ij, np.ones((1, 3)), rs.rand(1, 3, nb_colors),
                             np.zeros((1, 3)), np.ones((1, 1, 3)), H, W, background_color=rs.rand(nb_colors), pixel_dtype=dt)  # fmt: skip
            r = HipRasterizer.for_scene(ds)
            obs = dev(rs.rand(1, H, W, nb_colors), dt)
            offset = 1 if number == len(frames) - 2 else 0
            whole = dev(2 * rs.rand(H * W + offset), dt)
            weights = whole[offset:].view(1, H, W)
            losses = []
            for _ in range(2):
                loss = torch.full((1,), float("nan"), dtype=F64, device=DEV)
                image, _z, _g = r.render_fit(ds, obs, 1.0, check_overflow=True, clear_grads=True, loss_out=loss, weights=weights)
                losses.append(loss)
            torch.cuda.synchronize()
            assert torch.equal(losses[0], losses[1])
            close_sum(losses[0][0], fr.l2(host(image), host(obs), host(weights), nb_colors, None, LD), f"weighted l2 {H} x {W} x {nb_colors}")
    finally:
        hr.force_generic(False)
