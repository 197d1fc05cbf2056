"""Pins tests/lighting_reference.py, the NumPy reference of tests/test_lighting_gpu.py (no GPU):

* the float64 and the long-double restatements equal the project's torch formulas on CPU float64 tensors (``lighting.sh_shade_torch``, the fallback of
  ``fronthalf.sh_shade``), gradients by autograd, under every entry of the option table;
* the nine Y_k are orthonormal: a quadrature over the sphere in long double (Gauss-Legendre in z with 8 nodes refined by Newton steps in long
  double, 16 equally spaced longitudes: exact for polynomials of degree <= 15 in (x, y, z)) gives delta_kl.  The quadrature's measured accuracy
  is 1.3e-18: its largest error over the 35 monomials x^a y^b z^c of degree <= 4, whose integrals 4 pi (a-1)!! (b-1)!! (c-1)!! / (a+b+c+1)!! (0 with
  an odd exponent) are known -- 12 eps of the 80-bit long double on integrals up to 4 pi.  The test holds the monomials and the 81 pairs
  |integral Y_k Y_l - delta_kl| (measured: 1.1e-18) to 8 times that, QUADRATURE_BOUND;
* ``lighting.sh_from_directional`` equals its restatement, approximates max(0, -N . L) + ambient as an order-2 expansion does, and is exactly constant
  without a directional light;
* a finite-difference check of the adjoint in long double;
* at EVERY shape of the GPU case table under every option: the distance of the float64 restatement from the long-double one, sums in units of
  eps64 * sum |term|, elementwise outputs in units of eps64 * max |reference|.  The largest of each, E_sum and E_elem, are what the GPU tolerances
  max(16, 8 E) derive from; they are recorded in the GPU test file and may not exceed 1024.

The finite-difference checks (of grad Y_k and of the adjoint) exercise tests/lighting_reference.py alone: they pin the test reference, not the product,
and pass whatever the package holds."""

import math
import os
import re

import numpy as np
import pytest
import torch

import fititer_reference as fr
import lighting_reference as lr
from fititer_reference import LD

pytestmark = pytest.mark.skipif(not fr.longdouble_is_extended(), reason="np.longdouble is not wider than float64 here: no reference")

F64 = np.float64
E_CAP = 1024
QUADRATURE_MEASURED = 1.3e-18
QUADRATURE_BOUND = 8 * QUADRATURE_MEASURED
SMALL_CASES = ("triangle_n2", "fan9", "v33")


def rel(a, b):
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def tt(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=F64), requires_grad=grad)


def recorded_constants():
    with open(os.path.join(fr.HERE, "test_lighting_gpu.py")) as f:
        text = f.read()
    return {k: float(v) for k, v in re.findall(r"^(E_SUM|E_ELEM) = ([0-9.]+)", text, flags=re.M)}


# ---- 1. the restatements equal the torch formulas ------------------------------------------------------------------------------------


@pytest.mark.parametrize("oname", list(lr.OPTIONS))
@pytest.mark.parametrize("case", SMALL_CASES)
@pytest.mark.parametrize("dtype", [F64, LD], ids=["float64", "longdouble"])
def test_forward_and_adjoint_equal_autograd_through_the_torch_formulas(case, oname, dtype):
    from deodr_amd import lighting
    from deodr_amd.scene3d import MeshTopology

    d, o = lr.inputs(case, oname), lr.OPTIONS[oname]
    got = lr.reference(case, oname, dtype, d=dict(d))
    topology = MeshTopology(d["faces"], d["V"], o["clockwise"], device="cpu")
    posed, sh = tt(d["posed"], True), tt(d["sh"], True)
    albedo = None if d["albedo"] is None else tt(d["albedo"], True)
    assert rel(got["normals"], topology.vertex_normals(posed).detach().numpy()) < 1e-13
    assert rel(got["Y"], lighting.sh_basis(topology.vertex_normals(posed)).detach().numpy()) < 1e-13
    loss = 0
    if d["luminosity_b"] is not None:
        lum = lighting.sh_shade_torch(posed, topology, sh, None)
        assert rel(got["luminosity"], lum.detach().numpy()) < 1e-13
        loss = loss + (lum * tt(d["luminosity_b"])).sum()
    if albedo is not None:
        colors = lighting.sh_shade_torch(posed, topology, sh, albedo)
        assert rel(got["colors"], colors.detach().numpy()) < 1e-13
        loss = loss + (colors * tt(d["colors_b"])).sum()
    loss.backward()
    before = lambda key: np.asarray(d[key + "0"], dtype=F64) if o["accumulate"] else 0.0
    assert rel(got["posed_b"], posed.grad.numpy()) < 1e-11
    assert rel(np.asarray(got["sh_b"][0], dtype=F64) - before("sh_b"), sh.grad.numpy()) < 1e-11
    if albedo is not None:
        assert rel(np.asarray(got["albedo_b"][0], dtype=F64) - before("albedo_b"), albedo.grad.numpy()) < 1e-11


def test_sh_shade_falls_back_to_the_torch_formulas_on_cpu_tensors():
    from deodr_amd import fronthalf, lighting
    from deodr_amd.scene3d import MeshTopology

    d = lr.inputs("fan9", "c3-s3-vertex")
    topology = MeshTopology(d["faces"], d["V"], False, device="cpu")
    posed, sh, albedo = tt(d["posed"]), tt(d["sh"]), tt(d["albedo"])
    assert torch.equal(fronthalf.sh_shade(posed, sh, albedo, topology), lighting.sh_shade_torch(posed, topology, sh, albedo))
    assert torch.equal(fronthalf.sh_shade(posed[0], sh[:, 0], None, topology), lighting.sh_shade_torch(posed[0], topology, sh[:, 0], None))
    assert torch.autograd.gradcheck(lambda p, s, a: fronthalf.sh_shade(p, s, a, topology), (tt(d["posed"][:1], True), tt(d["sh"], True), tt(d["albedo"], True)),
                                    eps=1e-6, atol=1e-6, rtol=1e-6)  # fmt: skip


# ---- 2. the basis ------------------------------------------------------------------------------------------------------------------------


def gauss_legendre(n):
    """nodes and weights of the n-point rule on [-1, 1] in long double: float64 nodes refined by Newton steps on P_n"""
    x = np.asarray(np.polynomial.legendre.leggauss(n)[0], dtype=LD)
    for _ in range(4):
        p0, p1 = np.ones_like(x), x
        for k in range(2, n + 1):
            p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
        dp = n * (x * p1 - p0) / (x * x - 1)
        x = x - p1 / dp
    p0, p1 = np.ones_like(x), x
    for k in range(2, n + 1):
        p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
    dp = n * (x * p1 - p0) / (x * x - 1)
    return x, 2 / ((1 - x * x) * dp * dp)


def test_the_basis_is_orthonormal_on_the_sphere():
    z, w = gauss_legendre(8)
    phi = 2 * lr.pi(LD) * np.arange(16, dtype=LD) / 16
    r = np.sqrt(1 - z * z)
    N = np.stack((r[:, None] * np.cos(phi), r[:, None] * np.sin(phi), z[:, None] * np.ones_like(phi)), axis=-1)  # [8,16,3]
    # the quadrature itself, on monomials with known integrals
    def odd_factorial(k):  # k!! for odd k (1 for k <= 1)
        return math.prod(range(k, 1, -2)) if k > 1 else 1

    worst = 0.0
    for a in range(5):
        for b in range(5 - a):
            for c in range(5 - a - b):
                got = np.einsum("zp,z->", N[..., 0] ** a * N[..., 1] ** b * N[..., 2] ** c, w) * (2 * lr.pi(LD) / 16)
                even = not (a % 2 or b % 2 or c % 2)
                exact = 4 * lr.pi(LD) * LD(odd_factorial(a - 1) * odd_factorial(b - 1) * odd_factorial(c - 1)) / LD(odd_factorial(a + b + c + 1)) if even else LD(0)
                worst = max(worst, abs(float(got - exact)))
    print(f"largest error of the quadrature on the monomials of degree <= 4 = {worst:.3e}")
    assert worst <= QUADRATURE_BOUND
    Y = lr.basis(N, LD)
    gram = np.einsum("zpk,zpl,z->kl", Y, Y, w) * (2 * lr.pi(LD) / 16)
    error = float(np.abs(gram - np.eye(9, dtype=LD)).max())
    print(f"largest |integral Y_k Y_l - delta_kl| = {error:.3e}")
    assert error <= QUADRATURE_BOUND
    # the float64 basis of the package is the same functions
    from deodr_amd import lighting

    assert rel(lighting.sh_basis(tt(N.reshape(-1, 3))).numpy(), Y.reshape(-1, 9)) < 1e-15


def test_basis_gradient_by_finite_differences():
    rs = np.random.RandomState(3)
    N = np.asarray(rs.randn(20, 3), dtype=LD)
    h = LD(1e-9)
    dY = lr.basis_gradient(N, LD)
    for axis in range(3):
        step = np.zeros(3, dtype=LD)
        step[axis] = h
        numeric = (lr.basis(N + step, LD) - lr.basis(N - step, LD)) / (2 * h)
        assert float(np.abs(numeric - dY[..., axis]).max()) < 1e-9


def test_sh_from_directional():
    from deodr_amd import lighting

    light, ambient = np.array([0.3, -0.5, 0.6]), 0.25
    got = lighting.sh_from_directional(tt(light), ambient)
    assert rel(got.numpy(), lr.from_directional(light, ambient, LD)) < 1e-15
    assert rel(lr.from_directional(light, ambient, F64), lr.from_directional(light, ambient, LD)) < 1e-15
    # what it approximates: with t = -N . L / |L| the expansion is 1/4 + t/2 + 5/32 (3 t^2 - 1); its distance from max(t, 0) is largest at the
    # terminator t = 0, where it is 1/4 - 5/32 = 3/32 (1/16 at t = +-1, 0.04 at the inner extremum t = -8/15)
    rs = np.random.RandomState(0)
    N = rs.randn(2000, 3)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    exact = np.maximum(-(N @ light), 0) + ambient
    approx = lighting.sh_basis(tt(N)).numpy() @ got.numpy()
    assert np.abs(approx - exact).max() <= 3 / 32 * np.linalg.norm(light) + 1e-12
    assert np.abs(approx - exact).max() > 0.08 * np.linalg.norm(light)  # (and it is reached: 2000 directions come close to the terminator)
    # differentiable in both
    assert torch.autograd.gradcheck(lighting.sh_from_directional, (tt(light, True), tt(ambient, True)), eps=1e-6, atol=1e-7, rtol=1e-6)
    # ambient only: exactly constant
    for zero in (None, tt(np.zeros(3))):
        sh = lighting.sh_from_directional(zero, 0.4)
        assert sh.shape == (9,) and bool((sh[1:] == 0).all())
        E = lighting.sh_basis(tt(N)) @ sh.to(torch.float64)
        assert bool((E == E[0]).all()) and abs(float(E[0]) - 0.4) < 1e-15


# ---- 3. the adjoint by finite differences, in long double -------------------------------------------------------------------------------


@pytest.mark.parametrize("oname", ["lum", "c3-s1-single", "c3-s3-vertex", "c3-s1-vertex-lum"])
def test_adjoint_by_finite_differences_in_long_double(oname):
    case = "fan9"
    d, o = lr.inputs(case, oname), lr.OPTIONS[oname]
    back = lr.backward(d["posed"], d["faces"], d["sh"], d["albedo"], o["clockwise"], d["luminosity_b"], d["colors_b"], LD)

    def loss(posed, sh, albedo):
        f = lr.forward(posed, d["faces"], sh, albedo, o["clockwise"], LD)
        total = LD(0)
        if d["luminosity_b"] is not None:
            total = total + (f["luminosity"] * np.asarray(d["luminosity_b"], dtype=LD)).sum()
        if albedo is not None:
            total = total + (f["colors"] * np.asarray(d["colors_b"], dtype=LD)).sum()
        return total

    h = LD(1e-7)
    rs = np.random.RandomState(5)
    args = [np.asarray(d["posed"], dtype=LD), np.asarray(d["sh"], dtype=LD), None if d["albedo"] is None else np.asarray(d["albedo"], dtype=LD)]
    grads = [back["posed_b"], back["sh_b"][0], back["albedo_b"][0] if d["albedo"] is not None else None]
    for i, (x, g) in enumerate(zip(args, grads)):
        if x is None:
            continue
        for _ in range(4):  # random directions
            direction = np.asarray(rs.randn(*x.shape), dtype=LD)
            plus, minus = list(args), list(args)
            plus[i], minus[i] = x + h * direction, x - h * direction
            numeric = (loss(*plus) - loss(*minus)) / (2 * h)
            analytic = (np.asarray(g, dtype=LD).reshape(x.shape) * direction).sum()
            assert abs(float(numeric - analytic)) <= 1e-9 * max(1.0, abs(float(analytic))), (i, float(numeric), float(analytic))


# ---- 4. the float64 error of the formulas at every shape of the GPU table ----------------------------------------------------------------


def test_float64_error_of_the_formulas_at_every_gpu_shape():
    from deodr_amd import hip_renderer as hr

    e_sum, e_elem, where_sum, where_elem = 0.0, 0.0, None, None
    k = lr.kernel_constants()
    for case in lr.CASES:
        build, n, _why = lr.CASES[case]
        assert 1 <= hr.sh_blocks(len(build()[0]), n) <= k["SH_MAX_BLOCKS"], case  # (a shape of the table is one the library launches)
        for oname in lr.OPTIONS:
            d = lr.inputs(case, oname)
            ref, f64 = lr.reference(case, oname, LD, d=d), lr.reference(case, oname, F64, d=d)
            assert float(ref["acc_len"].min()) > 0.5, (case, oname)  # (no vertex whose normals cancel: the normalisation is well conditioned)
            for key in ("luminosity", "colors", "posed_b"):
                if key in ref and (key != "luminosity" or d["luminosity_b"] is not None):
                    v = fr.elem_distance(np.asarray(f64[key], dtype=F64), ref[key])
                    if v > e_elem:
                        e_elem, where_elem = v, (key, case, oname)
            for key in ("sh_b", "albedo_b"):
                if key in ref:
                    v = fr.sum_distance(np.asarray(f64[key][0], dtype=F64), ref[key])
                    if v > e_sum:
                        e_sum, where_sum = v, (key, case, oname)
    print(f"E_sum = {e_sum:.3f} at {where_sum}; E_elem = {e_elem:.3f} at {where_elem}")
    assert e_sum <= E_CAP and e_elem <= E_CAP
    recorded = recorded_constants()
    assert recorded == {"E_SUM": float(math.ceil(e_sum)), "E_ELEM": float(math.ceil(e_elem))}, (e_sum, e_elem, recorded)


def test_the_case_table_is_where_the_launch_geometry_changes():
    from deodr_amd import hip_renderer as hr

    k = lr.kernel_constants()
    per_block = k["FH_BLOCK"] // k["GATHER_LANES"]
    shape = {case: (len(build()[0]), n) for case, (build, n, _why) in lr.CASES.items()}
    assert shape["triangle_n1"] == (3, 1) and hr.sh_blocks(3, 1) == 1
    assert shape["v32"] == (per_block, 1) and hr.sh_blocks(*shape["v32"]) == 1 and hr.sh_blocks(*shape["v33"]) == 2
    assert {n for _, n in shape.values()} == {1, 2, k["FIT_MAX_VIEWS"]}
    for valence in (7, 8, 9, 16, 17):
        vertices, faces = lr.CASES[f"fan{valence}"][0]()
        assert np.bincount(faces.reshape(-1)).max() == valence
    assert shape["v8193_n1"] == (8193, 1) and hr.sh_blocks(8193, 1) == k["FH_BLOCK"] + 1
    assert shape["v129_n64"] == (129, 64) and hr.sh_blocks(129, 64) > k["FH_BLOCK"]
    V, n = shape["past_cap"]
    cap = k["SH_MAX_BLOCKS"]
    assert hr.sh_blocks(V, n) == cap == hr.sh_blocks(1 << 24, 64) and fr.ceil_div(V * n, per_block) > cap >= fr.ceil_div((V - 1) * n, per_block)
