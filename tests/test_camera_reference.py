"""Pins tests/camera_reference.py, the NumPy reference of tests/test_camera_gpu.py (no GPU):

* at three small shapes the float64 and the long-double restatements equal the project's torch formulas on CPU float64 tensors (the fallback of
  ``DeviceCamera.project_points``, the fallback of ``DeviceCamera.from_pose``), gradients by autograd; ``torch.autograd.gradcheck`` on both;
* at EVERY shape of the GPU case tables: the distance of the float64 restatement from the long-double one, sums in units of eps64 * sum |term|,
  elementwise outputs in units of eps64 * max |reference|.  The largest of each, E_sum and E_elem, are what the GPU tolerances max(16, 8 E) derive
  from; they are recorded in the GPU test file and may not exceed 1024; the inputs are checked for what would make them large (depths outside
  [5, 12], |x|, |y| beyond 0.5 under distortion)."""

import math
import os
import re

import numpy as np
import pytest
import torch

import camera_reference as cr
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
    with open(os.path.join(fr.HERE, "test_camera_gpu.py")) as f:
        text = f.read()
    return {k: float(v) for k, v in re.findall(r"^(E_SUM|E_ELEM) = ([0-9.]+)", text, flags=re.M)}


def blocks_of(V, n):
    from deodr_amd import hip_renderer as hr

    return hr.camera_blocks(V, n)


# ---- 1. the restatements equal the torch formulas ------------------------------------------------------------------------------------


@pytest.mark.parametrize("V,n", cr.SMALL_SHAPES)
@pytest.mark.parametrize("dtype", [F64, LD], ids=["float64", "longdouble"])
def test_the_full_adjoint_equals_autograd_through_the_torch_projection(V, n, dtype):
    from deodr_amd.scene3d import DeviceCamera

    d = cr.project_inputs(V, n)
    for options in cr.OPTIONS.values():
        got = cr.project_reference(V, n, dict(options, accumulate=False), dtype, d)
        E, K = tt(d["extrinsic"], True), tt(d["intrinsic"], True)
        D = tt(d["distortion"], True) if options["distortion"] else None
        cam = DeviceCamera(E, K, 96, 128, D, "cpu")
        p = tt(d["points"], True)
        ij, depths = cam.project_points(p)
        loss = (ij * tt(d["ij_b"])).sum() + ((depths * tt(d["depths_b"])).sum() if options["depths_b"] else 0)
        grads = torch.autograd.grad(loss, [p, E, K] + ([D] if options["distortion"] else []))
        assert rel(got["points_b"], grads[0]) < 1e-11
        assert rel(got["extrinsic_b"][0], grads[1]) < 1e-11
        assert rel(got["intrinsic_b"][0], grads[2][:, :2]) < 1e-11 and float(grads[2][:, 2].abs().max()) == 0
        if options["distortion"]:
            assert rel(got["distortion_b"][0], grads[3]) < 1e-11
        else:
            assert got["distortion_b"] is None


@pytest.mark.parametrize("n,shared,distortion", [(1, True, True), (2, False, True), (9, True, False), (9, False, True), (9, True, True)])
@pytest.mark.parametrize("dtype", [F64, LD], ids=["float64", "longdouble"])
def test_assemble_and_its_adjoint_equal_the_torch_formulas(n, shared, distortion, dtype):
    from deodr_amd.mesh_fitter import qrot
    from deodr_amd.scene3d import DeviceCamera

    d = cr.assemble_inputs(n)
    q, t, f, c, dist = cr.assemble_arguments(d, shared, distortion)
    E, K, D = cr.assemble(q, t, f, c, dist, shared, dtype)
    tq, ttr, tf, tc = tt(q, True), tt(t, True), tt(f, True), tt(c, True)
    td = tt(dist, True) if distortion else None
    cam = DeviceCamera.from_pose(tq, ttr, tf, tc, 96, 128, td, shared_intrinsics=shared, device="cpu")
    assert rel(E, cam.extrinsic.detach()) < 1e-14 and rel(K, cam.intrinsic.detach()) < 1e-15
    assert (cam.distortion is None) == (not distortion) and (not distortion or rel(D, cam.distortion.detach()) == 0)
    # R p + t == qrot(q / |q|, p) + t
    p = torch.tensor(np.random.RandomState(n).randn(n, 7, 3))
    unit = tq.detach() / tq.detach().norm(dim=-1, keepdim=True)
    assert rel((p @ cam.extrinsic[:, :, :3].transpose(1, 2) + cam.extrinsic[:, None, :, 3]).detach(), qrot(unit, p) + ttr.detach()[:, None, :]) < 1e-14
    loss = (cam.extrinsic * tt(d["extrinsic_b"])).sum() + (cam.intrinsic * tt(d["intrinsic_b"])).sum()
    if distortion:
        loss = loss + (cam.distortion * tt(d["distortion_b"])).sum()
    grads = torch.autograd.grad(loss, [tq, ttr, tf, tc] + ([td] if distortion else []))
    got = cr.assemble_b(q, d["extrinsic_b"], d["intrinsic_b"], d["distortion_b"] if distortion else None, shared, dtype)
    assert rel(got["quaternions_b"], grads[0]) < 1e-12 and rel(got["translations_b"], grads[1]) == 0
    assert rel(got["focal_b"][0], grads[2]) < 1e-14 and rel(got["center_b"][0], grads[3]) < 1e-14
    if distortion:
        assert rel(got["distortion_b"][0], grads[4]) < 1e-14


def test_gradcheck_of_the_two_fallbacks():
    from deodr_amd.scene3d import DeviceCamera

    d = cr.project_inputs(5, 2)
    for dist in (None, d["distortion"]):
        inputs = [tt(d["points"], True), tt(d["extrinsic"], True), tt(d["intrinsic"], True)] + ([] if dist is None else [tt(dist, True)])

        def project(p, E, K, D=None):
            return DeviceCamera(E, K, 96, 128, D, "cpu").project_points(p)

        assert torch.autograd.gradcheck(project, inputs, eps=1e-6, atol=1e-6, rtol=1e-6)
    a = cr.assemble_inputs(3)
    for shared in (True, False):
        args = [tt(x, True) for x in cr.assemble_arguments(a, shared, True)]

        def pose(q, t, f, c, dd):
            cam = DeviceCamera.from_pose(q, t, f, c, 96, 128, dd, shared_intrinsics=shared, device="cpu")
            return cam.extrinsic, cam.intrinsic, cam.distortion

        assert torch.autograd.gradcheck(pose, args, eps=1e-6, atol=1e-6, rtol=1e-6)


# ---- 2. the float64 error of the formulas at every shape of the GPU tables -----------------------------------------------------------


def test_float64_error_of_the_formulas_at_every_gpu_shape():
    e_sum, e_elem, where_sum, where_elem = 0.0, 0.0, None, None

    def sum_(got, pair, what):
        nonlocal e_sum, where_sum
        v = fr.sum_distance(np.asarray(got[0], dtype=F64), pair)
        if v > e_sum:
            e_sum, where_sum = v, what

    def elem(got, ref, what):
        nonlocal e_elem, where_elem
        v = fr.elem_distance(np.asarray(got, dtype=F64), ref)
        if v > e_elem:
            e_elem, where_elem = v, what

    for V, n, _why in cr.project_cases(blocks_of).values():
        d = cr.project_inputs(V, n)
        for oname, options in cr.OPTIONS.items():
            ref, f64 = cr.project_reference(V, n, options, LD, d), cr.project_reference(V, n, options, F64, d)
            assert 5 < float(ref["depths"].min()) and float(ref["depths"].max()) < 12, (V, n)
            if options["distortion"]:  # (the distorted normalised point: a little larger than |x|, |y| themselves)
                xy = np.asarray(d["points"], dtype=LD)
                (cx, cy, cz), _ = fr._camera_space(xy, d["extrinsic"], LD)
                assert float(np.abs(cx / cz).max()) <= 0.5 and float(np.abs(cy / cz).max()) <= 0.5, (V, n)
            elem(f64["points_b"], ref["points_b"], ("points_b", V, n, oname))
            for key in ("extrinsic_b", "intrinsic_b", "distortion_b"):
                if ref[key] is not None:
                    sum_(f64[key], ref[key], (key, V, n, oname))
    for n, shared, distortion in cr.ASSEMBLE_CASES:
        d = cr.assemble_inputs(n)
        q, t, f, c, dist = cr.assemble_arguments(d, shared, distortion)
        for key, got, ref in zip("EKD", cr.assemble(q, t, f, c, dist, shared, F64), cr.assemble(q, t, f, c, dist, shared, LD)):
            if ref is not None:
                elem(got, ref, ("assemble " + key, n, shared))
        db = d["distortion_b"] if distortion else None
        got, ref = (cr.assemble_b(q, d["extrinsic_b"], d["intrinsic_b"], db, shared, dt) for dt in (F64, LD))
        elem(got["quaternions_b"], ref["quaternions_b"], ("quaternions_b", n, shared))
        elem(got["translations_b"], ref["translations_b"], ("translations_b", n, shared))
        for key in ("focal_b", "center_b", "distortion_b"):
            if ref[key] is not None:
                sum_(got[key], ref[key], (key, n, shared))
    print(f"E_sum = {e_sum:.3f} at {where_sum}; E_elem = {e_elem:.3f} at {where_elem}")
    assert e_sum <= E_CAP and e_elem <= E_CAP
    recorded = recorded_constants()
    assert recorded == {"E_SUM": float(math.ceil(e_sum)), "E_ELEM": float(math.ceil(e_elem))}, (e_sum, e_elem, recorded)


def test_the_case_table_is_where_the_launch_geometry_changes():
    k = cr.kernel_constants()
    cases = list(cr.project_cases(blocks_of, k).values())
    shapes = {(V, n) for V, n, _ in cases}
    assert {V for V, _ in shapes} >= set(cr.SMALL_V) and {n for _, n in shapes} == set(cr.VIEWS)
    for V, n, why in cases:
        b = blocks_of(V, n)
        assert 1 <= b <= k["CAMERA_MAX_BLOCKS"]
        if why == "small" or why == "one workgroup":
            assert b == 1
        if why == "second workgroup":
            assert b == 2 and blocks_of(V - 2, n) == 1
        if why == "below the cap":
            assert b == k["CAMERA_MAX_BLOCKS"] - 1
        if why == "cap":
            assert b == k["CAMERA_MAX_BLOCKS"] == blocks_of(1 << 24, n)
        if why == "cap of 64 views":
            assert b == blocks_of(1 << 24, n) and blocks_of(V - 1, n) == b - 1
        if why == "several trips":
            assert b == 3 and 2 * b * k["FH_BLOCK"] < V
