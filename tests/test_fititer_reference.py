"""Pins tests/fititer_reference.py, the NumPy reference of tests/test_fititer_shapes_gpu.py (no GPU):

* at three small shapes the float64 and the long-double restatements equal the project's torch formulas on CPU float64 tensors
  (``mesh_fitter.qrot``, ``DeviceCamera.project_points``, ``MeshTopology.vertex_normals`` / ``edge_on_silhouette``,
  ``LaplacianRigidEnergyDevice``, ``_Momentum``: what runs when ``fronthalf.usable`` is false), gradients by autograd, within the tolerances
  the GPU tests of the same kernels use against those formulas (tests/test_hip_round3.py);
* at EVERY shape of the GPU case tables: the distance of the float64 restatement from the long-double one, sums in units of
  eps64 * sum |term|, elementwise outputs in units of eps64 * max |reference|.  The largest of each, E_sum and E_elem, are what the GPU
  tolerances max(16, 8 E) derive from; they are recorded in the GPU test file, may not exceed 1024, and the inputs are checked for what
  would make them large (depths outside [5, 12], |x|, |y| beyond 0.5 under distortion, a luminosity or a signed area on its kink);
* every regime case of the GPU tables is in its regime by the constants of the kernel headers.
"""

import os
import re

import numpy as np
import pytest
import torch

import fititer_reference as fr
from fititer_reference import LD

pytestmark = pytest.mark.skipif(not fr.longdouble_is_extended(), reason="np.longdouble is not wider than float64 here: no reference")

F64 = np.float64
E_CAP = 1024


def rel(a, b):
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def tt(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=F64), requires_grad=grad)


def recorded_constants():
    with open(os.path.join(fr.HERE, "test_fititer_shapes_gpu.py")) as f:
        text = f.read()
    return {k: float(v) for k, v in re.findall(r"^(E_SUM|E_ELEM) = ([0-9.]+)", text, flags=re.M)}


# ---- 1. the restatements equal the torch formulas ------------------------------------------------------------------------------------


@pytest.mark.parametrize("V,n", [(1, 2), (33, 9), (257, 1)])
@pytest.mark.parametrize("dtype", [F64, LD], ids=["float64", "longdouble"])
def test_pose_and_projection_equal_the_torch_formulas(V, n, dtype):
    from deodr_amd.mesh_fitter import qrot
    from deodr_amd.scene3d import DeviceCamera

    d = fr.point_inputs(V, n)
    for options in fr.POINT_OPTIONS.values():
        got = fr.point_reference(V, n, options, dtype, d)
        cam = DeviceCamera(d["extrinsic"], d["intrinsic"], 96, 128, d["distortion"] if options["distortion"] else None, "cpu")
        x, q, t = tt(d["vertices"], True), tt(d["quaternions"], True), tt(d["translations"], True)
        centred = x - x.mean(dim=0, keepdim=True) if options["centre"] else x
        posed = qrot(q / q.norm(dim=-1, keepdim=True), centred[None].expand(n, -1, -1)) + t[:, None, :]
        ij, depths = cam.project_points(posed)
        loss = (ij * tt(d["ij_b"])).sum()
        if options["depths_b"]:
            loss = loss + fr.DEPTHS_B_SCALE * (depths * tt(d["depths_b"])).sum()
        if options["posed_b"]:
            loss = loss + (posed * tt(d["posed_b"])).sum()
        gx, gq, gt = torch.autograd.grad(loss, [x, q, t])
        assert rel(got["posed"], posed.detach()) < 1e-13 and rel(got["ij"], ij.detach()) < 1e-13 and rel(got["depths"], depths.detach()) < 1e-14
        vertices_b = np.asarray(got["vertices_b"], dtype=F64)
        if options["centre"]:  # (autograd went through the centring: the projection on zero-mean displacements)
            vertices_b = vertices_b - np.asarray(got["mean"][0], dtype=F64)
        assert rel(vertices_b, gx) < 1e-11
        assert rel(got["q_b"][0], gq) < 1e-10 and rel(got["t_b"][0], gt) < 1e-11
        if options["C"]:
            assert rel(got["colors_sum"], d["colors_b"][..., : options["C"]].sum(axis=0)) < 1e-15
        # the camera adjoint alone, summed over the views
        p = posed.detach().clone().requires_grad_(True)
        ij2, depths2 = cam.project_points(p)
        loss = (ij2 * tt(d["ij_b"])).sum() + (fr.DEPTHS_B_SCALE * (depths2 * tt(d["depths_b"])).sum() if options["depths_b"] else 0)
        assert rel(got["views_sum"], torch.autograd.grad(loss, [p])[0].sum(dim=0)) < 1e-10
    # the autograd ops: unit quaternions taken as they are
    got = fr.autograd_ops_reference(V, n, dtype, d)
    x, q, t = tt(d["vertices"], True), tt(got["unit_quaternions"], True), tt(d["translations"], True)
    posed = qrot(q, x[None].expand(n, -1, -1)) + t[:, None, :]
    gx, gq, gt = torch.autograd.grad((posed * tt(d["posed_b"])).sum(), [x, q, t])
    assert rel(got["posed"], posed.detach()) < 1e-14
    assert rel(got["vertices_b"], gx) < 1e-12 and rel(got["q_b"][0], gq) < 1e-12 and rel(got["t_b"][0], gt) < 1e-12
    cam = DeviceCamera(d["extrinsic"], d["intrinsic"], 96, 128, d["distortion"], "cpu")
    p = tt(got["points"], True)
    ij, depths = cam.project_points(p)
    (gp,) = torch.autograd.grad((ij * tt(d["ij_b"])).sum() + (depths * tt(d["depths_b"])).sum(), [p])
    assert rel(got["ij"], ij.detach()) < 1e-13 and rel(got["depths"], depths.detach()) < 1e-14 and rel(got["points_b"], gp) < 1e-11


@pytest.mark.parametrize("name", ["tetrahedron", "fan9", "sphere_7_4"])
@pytest.mark.parametrize("clockwise", [False, True])
@pytest.mark.parametrize("dtype", [F64, LD], ids=["float64", "longdouble"])
def test_shading_rigid_energy_and_flags_equal_the_torch_formulas(name, clockwise, dtype):
    from deodr_amd.scene3d import LaplacianRigidEnergyDevice, MeshTopology

    d = fr.mesh_inputs(name)
    topo = MeshTopology(d["faces"], len(d["vertices"]), clockwise=clockwise, device="cpu")
    posed, light, amb, color = tt(d["posed"], True), tt(d["light"], True), tt(d["ambient"], True), tt(d["color"], True)
    lum = torch.relu(-(topo.vertex_normals(posed) * light).sum(-1)) + amb
    colors = lum[..., None] * color
    got = fr.shade(d["posed"], d["faces"], d["light"], d["ambient"], d["color"], clockwise, dtype)
    assert rel(got["luminosity"], lum.detach()) < 1e-13 and rel(got["colors"], colors.detach()) < 1e-13
    g = torch.autograd.grad((lum * tt(d["luminosity_b"])).sum() + (colors * tt(d["colors_b"])).sum(), [posed, light, amb, color])
    got = fr.shade_b(d["posed"], d["faces"], d["light"], d["ambient"], d["color"], clockwise, d["luminosity_b"], d["colors_b"], dtype)
    for key, ref in zip(("posed_b", "light_b", "ambient_b", "color_b"), g):
        assert rel(got[key] if key == "posed_b" else got[key][0], ref) < 1e-11, key
    # rigid energy
    off, cols, vals = (a.numpy() for a in topo._m_csr)
    energy = LaplacianRigidEnergyDevice(topo, d["ref"], fr.MESH_CREGU)
    x = tt(d["x"], True)
    e, grad = energy.evaluate(x)
    got = fr.rigid(d["x"], d["ref"], off.view(np.uint32), cols.view(np.uint32), vals, fr.MESH_CREGU, dtype)
    assert abs(float(got["energy"][0]) - float(e.detach())) <= 1e-12 * abs(float(e.detach())) and rel(got["gradient"], grad.detach()) < 1e-12
    assert rel(got["gradient"], torch.autograd.grad(e, [x])[0]) < 1e-12
    # silhouette flags
    flags, _cr = fr.silhouette(d["ij"], d["faces"], clockwise, dtype)
    assert np.array_equal(flags, topo.edge_on_silhouette(tt(d["ij"])).numpy())


@pytest.mark.parametrize("name", list(fr.MOMENTUM_LAUNCHES))
@pytest.mark.parametrize("dtype", [F64, LD], ids=["float64", "longdouble"])
def test_momentum_equals_the_torch_formula(name, dtype):
    from deodr_amd.mesh_fitter import _Momentum

    _size, entries, _energy = fr.MOMENTUM_LAUNCHES[name]
    x0, steps = fr.momentum_inputs(name)
    mom = _Momentum(fr.MOMENTUM_INERTIA, fr.MOMENTUM_DAMPING)
    x_t = [tt(x) for x in x0]
    x_n, speed = [np.asarray(x, dtype=dtype) for x in x0], [np.zeros(np.shape(x), dtype=dtype) for x in x0]
    for given in steps:
        rows = []
        for k, (e, g) in enumerate(zip(entries, given)):
            grad = tt(g["grad"])
            if g["grad_mean"] is not None:
                grad = grad - tt(g["grad_mean"])
            rows.append((str(k), x_t[k], grad * e["grad_scale"], None if g["grad2"] is None else tt(g["grad2"]), e["factor"], e["step_max"], e["rows"]))
        x_t = mom.update_all(rows)
        for k, (e, g) in enumerate(zip(entries, given)):
            out = fr.momentum_reference(e, x_n[k], speed[k], g, dtype)
            x_n[k], speed[k] = out["x"], out["speed"]
            assert rel(out["x"], x_t[k]) < 1e-14, (name, k)
            if "mean" in out and len(np.shape(x0[k])) == 2:
                assert rel(out["mean"][0], x_t[k].mean(dim=0)) < 1e-13


# ---- 2. how far float64 arithmetic of the same formulas lies from the reference, at every shape of the GPU tables ----------------------


class Distances:
    def __init__(self):
        self.sum, self.elem, self.worst_sum, self.worst_elem = 0.0, 0.0, None, None

    def sums(self, what, got, ref):
        d = fr.sum_distance(got[0], ref)
        if d > self.sum:
            self.sum, self.worst_sum = d, what

    def elems(self, what, got, ref):
        d = fr.elem_distance(got, ref)
        if d > self.elem:
            self.elem, self.worst_elem = d, what


def measure_points(D):
    for V, n in fr.POINT_CASES:
        d = fr.point_inputs(V, n)
        for oname, options in fr.POINT_OPTIONS.items():
            lo, hi = fr.point_reference(V, n, options, F64, d), fr.point_reference(V, n, options, LD, d)
            assert 5 < float(hi["depths"].min()) and float(hi["depths"].max()) < 12, (V, n)
            for key in ("centred", "posed", "ij", "depths", "depth_colors", "views_sum", "vertices_b") + (("colors_sum",) if options["C"] else ()):
                D.elems(("points", V, n, oname, key), lo[key], hi[key])
            for key in ("mean", "q_b", "t_b"):
                D.sums(("points", V, n, oname, key), lo[key], hi[key])
        # under distortion |x|, |y| stay below 0.5
        (cx, cy, cz), _E = fr._camera_space(hi["posed"], d["extrinsic"], LD)
        assert float(np.abs(cx / cz).max()) < 0.5 and float(np.abs(cy / cz).max()) < 0.5
        lo, hi = fr.autograd_ops_reference(V, n, F64, d), fr.autograd_ops_reference(V, n, LD, d)
        for key in ("posed", "vertices_b", "ij", "depths", "points_b"):
            D.elems(("ops", V, n, key), lo[key], hi[key])
        for key in ("q_b", "t_b"):
            D.sums(("ops", V, n, key), lo[key], hi[key])


def measure_meshes(D):
    from deodr_amd.scene3d import MeshTopology

    for name in fr.MESH_CASES:
        d = fr.mesh_inputs(name)
        topo = MeshTopology(d["faces"], len(d["vertices"]), device="cpu")
        off, cols, vals = (a.numpy() for a in topo._m_csr)
        off, cols = off.view(np.uint32), cols.view(np.uint32)
        lo, hi = (fr.rigid(d["x"], d["ref"], off, cols, vals, fr.MESH_CREGU, t) for t in (F64, LD))
        D.elems((name, "gradient"), lo["gradient"], hi["gradient"])
        D.sums((name, "energy"), lo["energy"], hi["energy"])
        for clockwise in (False, True):
            lo, hi = (fr.shade(d["posed"], d["faces"], d["light"], d["ambient"], d["color"], clockwise, t) for t in (F64, LD))
            # no vertex on the kink of max(0, .), lit and unlit vertices both there
            assert float(np.abs(hi["d"]).min()) > 1e-9, (name, float(np.abs(hi["d"]).min()))
            assert 0.2 <= float((hi["d"] > 0).mean()) <= 0.8, (name, clockwise)
            for key in ("luminosity", "colors"):
                D.elems((name, clockwise, key), lo[key], hi[key])
            for lum_b, colors_b, color in ((d["luminosity_b"], d["colors_b"], d["color"]), (d["luminosity_b"], None, None)):
                lo, hi = (fr.shade_b(d["posed"], d["faces"], d["light"], d["ambient"], color, clockwise, lum_b, colors_b, t) for t in (F64, LD))
                D.elems((name, clockwise, "posed_b"), lo["posed_b"], hi["posed_b"])
                for key in ("light_b", "ambient_b") + (("color_b",) if color is not None else ()):
                    D.sums((name, clockwise, key), lo[key], hi[key])
            flags_lo, _ = fr.silhouette(d["ij"], d["faces"], clockwise, F64)
            flags_hi, cr = fr.silhouette(d["ij"], d["faces"], clockwise, LD)
            assert np.array_equal(flags_lo, flags_hi) and 0 < int(flags_hi.sum()) < flags_hi.size
            assert float(np.abs(cr).min()) > 1e-9 * float(np.abs(cr).max()), name  # no face edge-on in the image


def measure_momentum(D):
    for name, (_size, entries, _energy) in fr.MOMENTUM_LAUNCHES.items():
        x0, steps = fr.momentum_inputs(name)
        x, speed = [np.array(a) for a in x0], [np.zeros_like(a) for a in x0]
        cut = np.zeros(3, dtype=np.int64)
        for given in steps:
            for k, (e, g) in enumerate(zip(entries, given)):
                lo, hi = fr.momentum_reference(e, x[k], speed[k], g, F64), fr.momentum_reference(e, x[k], speed[k], g, LD)
                for key in ("x", "speed"):
                    D.elems((name, k, key), lo[key], hi[key])
                if e["mean_out"]:
                    D.sums((name, k, "mean"), lo["mean"], hi["mean"])
                if e["step_max"] is not None:
                    cut += (hi["clamped"][0], hi["clamped"][1], x[k].size - sum(hi["clamped"]))
                x[k], speed[k] = lo["x"], lo["speed"]  # (the state a float64 kernel would carry on with)
        assert cut.min() > 0, (name, cut)  # step_max hit on both sides, and not hit


def measure_frames(D):
    for np_type in (np.float32, np.float64):
        for cname, count in fr.l2_counts(np.dtype(np_type).itemsize).items():
            rs = np.random.RandomState(count % 1000)
            a, b, w = rs.rand(count).astype(np_type), rs.rand(count).astype(np_type), rs.rand(count).astype(np_type)
            D.sums(("l2", cname, np_type.__name__), fr.l2(a, b, dtype=F64), fr.l2(a, b, dtype=LD))
            D.sums(("l2 weighted", cname, np_type.__name__), fr.l2(a, b, w, 1, (0.1, 0.8), F64), fr.l2(a, b, w, 1, (0.1, 0.8), LD))
            lo, hi = fr.depth_residual(a * 1.4 - 0.2, b.astype(F64), 1.0, F64), fr.depth_residual(a * 1.4 - 0.2, b.astype(F64), 1.0, LD)
            D.sums(("depth", cname, np_type.__name__), lo["loss"], hi["loss"])
            D.elems(("depth diff", cname, np_type.__name__), lo["diff"], hi["diff"])


def test_float64_distance_from_the_reference_at_every_gpu_shape():
    """E_sum / E_elem: the largest distance of the float64 restatement (np.sum order) from the long-double one over all the GPU cases.
    Both within the cap, and within what the GPU test file records (its tolerances derive from the recorded values)."""
    D = Distances()
    for measure in (measure_points, measure_meshes, measure_momentum, measure_frames):
        measure(D)
    print(f"E_sum = {D.sum:.3f} at {D.worst_sum}; E_elem = {D.elem:.3f} at {D.worst_elem}")
    assert D.sum <= E_CAP and D.elem <= E_CAP, "badly conditioned inputs: rechoose them, do not loosen the bound"
    recorded = recorded_constants()
    assert set(recorded) == {"E_SUM", "E_ELEM"}
    assert D.sum <= recorded["E_SUM"] <= E_CAP and D.elem <= recorded["E_ELEM"] <= E_CAP, (D.sum, D.elem, recorded)


# ---- 3. the regime cases are in their regimes ------------------------------------------------------------------------------------------


def test_case_tables_enter_the_regimes_they_are_there_for():
    k = fr.kernel_constants()
    geo = lambda V, n: fr.pose_b_geometry(V, n, k)
    assert (1025, 17) in fr.POINT_CASES and geo(1025, 17)["sum_rounds"] > 1 and geo(1025, 17)["view_trips"] == 3 and 17 % k["GATHER_LANES"] == 1
    assert (2049, 2) in fr.POINT_CASES and geo(2049, 2)["wanted"] > k["POSE_B_BLOCKS"] and geo(2049, 2)["strided_trips"] == 2
    assert 2049 - geo(2049, 2)["grid"] * geo(2049, 2)["per_block"] == 1  # one vertex in the second strided trip
    assert (4100, 64) in fr.POINT_CASES and k["FIT_MAX_VIEWS"] == 64 and geo(4100, 64)["strided_trips"] > 2
    assert (16385, 1) in fr.POINT_CASES and geo(16385, 1)["lanes"] == 1 and geo(16385, 1)["strided_trips"] == 2
    assert geo(33, 9)["view_trips"] == 2 and geo(32, 8)["view_trips"] == 1 and geo(31, 3)["idle_lanes"] > 0
    assert geo(32, 8)["wanted"] == 1 and geo(33, 9)["wanted"] == 2 and geo(256, 1)["wanted"] == 1 and geo(257, 1)["wanted"] == 2
    blocks = lambda count: fr.ceil_div(count, k["FH_BLOCK"])
    V = len(fr.mesh_inputs("sphere_128_65")["vertices"])
    assert V == 8322 and blocks(V * k["GATHER_LANES"]) > k["FH_BLOCK"]  # grid_sum's second trip: rigid energy and vertex_shade_b1
    V, n = len(fr.mesh_inputs("sphere_33_31")["vertices"]), fr.MESH_CASES["sphere_33_31"][1]
    assert V == 1025 and V % k["GATHER_LANES"] and n == 3
    V = len(fr.mesh_inputs("sphere_7_4")["vertices"])
    assert V == 30 and V % k["GATHER_LANES"] and (3 * V * k["GATHER_LANES"]) > 64  # wavefronts of b1 span views
    for hub in (8, 9, 16, 17):
        d = fr.mesh_inputs(f"fan{hub}")
        assert int((d["faces"] == 0).sum()) == hub and hub in (k["GATHER_LANES"], k["GATHER_LANES"] + 1, 2 * k["GATHER_LANES"], 2 * k["GATHER_LANES"] + 1)
    assert int(np.bincount(fr.mesh_inputs("sphere_128_65")["faces"].reshape(-1)).max()) == 128
    wide = fr.MOMENTUM_LAUNCHES["wide"][1]
    assert blocks(int(np.prod(wide[0]["shape"]))) == k["FH_BLOCK"] + 1 and wide[1]["shape"] == (1, 3) and wide[1]["mean_out"]
    assert len(fr.MOMENTUM_LAUNCHES["eight"][1]) == k["MOMENTUM_MAX"] and len(fr.MOMENTUM_LAUNCHES["one"][1]) == 1
    for itemsize in (4, 8):
        c = fr.l2_counts(itemsize, k)
        g1, g2 = fr.l2_geometry(c["beyond_one_stride"], itemsize, k), fr.l2_geometry(c["beyond_a_round"], itemsize, k)
        assert g1["strides"] == 2 and g1["tail"] and g2["trips"] == 2 and g2["tail"]
