"""GPU tests of linear bases: ``deodr_hip_basis_apply`` / ``deodr_hip_basis_apply_b`` against NumPy in long double where their launch geometry or
their loops change, the autograd op between the coefficients and the rasterizer, and the fitters with ``shape_basis`` / ``texture_basis`` -- eager, and
replayed as a HIP graph.

Tolerances are derived, not measured.  A sum of n terms taken in ANY order, with or without FMA contraction, lies within
(n + 2) 2^-53 sum |term| of the exact value.  Forward: n = K + 1 terms, mean_j and c_k B_kj.  Adjoint: n = N terms B_kj g_j (one more with
``accumulate``: the value coeffs_b held).  The rounding of the store is added on top: 2^-53 |value| (float64), 2^-24 |value| (float32).  Every
element is checked against its own bound.  A term, a row, a segment's partial or a tail element that goes missing is of the order of
sum |term| / n: twelve orders of magnitude above the bound.

Every call: outputs and scratch are carved out of larger buffers with guard patterns on both sides (NaN; 0xA5 behind the scratch, which has
exactly deodr_hip_basis_scratch_bytes bytes), checked after the call; the scratch's counter words are zero again; the same call into fresh outputs
gives the same bits, and so does a call on a second zero-filled scratch.  The shapes come from the constants of csrc/dr_basis.h (read from the
file) and from deodr_hip_basis_segments (asked, never written down)."""

import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

LD = np.longdouble
F32, F64 = torch.float32, torch.float64
DEV = "cuda"
PAD = 64  # elements either side of a carved tensor: a multiple of 16 bytes for every dtype here
GUARD_BYTES, GUARD_BYTE = 4096, 0xA5
U = 2.0**-53


@functools.lru_cache(maxsize=None)
def constants():
    """the constexpr ints of csrc/dr_basis.h (+ FH_BLOCK of dr_fronthalf.h)"""
    out = {}
    for name in ("dr_basis.h", "dr_fronthalf.h"):
        text = open(os.path.join(ROOT, "deodr_amd", "csrc", name)).read()
        for m in re.finditer(r"constexpr int ([^;]*);", text):
            for item in m.group(1).split(","):
                key, value = (s.strip() for s in item.split("="))
                if re.fullmatch(r"\d+", value):
                    out[key] = int(value)
    assert np.finfo(LD).eps < 2e-19, "np.longdouble is not wider than float64 here: no reference"
    return out


def vec(dtype):
    return 16 // (8 if dtype == F64 else 4)


def first_n_with(K, segments):
    """the smallest N at which deodr_hip_basis_segments(K, N) reaches ``segments`` (the function is non-decreasing in N: bisection)"""
    from deodr_amd import hip_renderer as hr

    lo, hi = 1, 2
    while hr.basis_segments(K, hi) < segments:
        lo, hi = hi, 2 * hi
        assert hi <= 2**24, "the segment rule never cuts a row of this K"
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if hr.basis_segments(K, mid) >= segments else (mid + 1, hi)
    assert hr.basis_segments(K, lo) == segments and (lo == 1 or hr.basis_segments(K, lo - 1) == segments - 1)
    return lo


class Arena:
    """tensors carved out of larger NaN-filled buffers, on a 16-byte boundary or (``misalign``) one element behind it"""

    def __init__(self, misalign=False):
        self.made, self.misalign = [], misalign

    def carve(self, values=None, shape=None, dtype=F64):
        shape = tuple(values.shape) if values is not None else tuple(shape)
        numel = int(np.prod(shape))
        start = PAD + (1 if self.misalign else 0)
        buffer = torch.full((2 * PAD + numel + 1,), float("nan"), dtype=dtype, device=DEV)
        t = buffer[start : start + numel].view(*shape)
        assert t.data_ptr() % 16 == (t.element_size() if self.misalign else 0)
        if values is not None:
            t.copy_(torch.as_tensor(np.ascontiguousarray(values)).to(dtype))
        self.made.append((buffer, start, numel, shape, values is None))
        return t

    def check(self):
        for buffer, start, numel, shape, is_output in self.made:
            around = torch.cat((buffer[:start], buffer[start + numel :]))
            assert bool(around.isnan().all()), f"written outside a tensor of shape {shape}"
            if is_output:
                assert not bool(buffer[start : start + numel].isnan().any()), f"an output of shape {shape} was not written everywhere"


class Scratch:
    """exactly deodr_hip_basis_scratch_bytes(K, N, batch) bytes, zero-filled, followed in the same allocation by a guard pattern"""

    def __init__(self, K, N, batch):
        from deodr_amd.hip_renderer import lib

        k = constants()
        self.nbytes = int(lib().deodr_hip_basis_scratch_bytes(K, N, batch))
        groups = -(-batch // k["BASIS_CHUNK"]) * -(-K // k["BASIS_ROW_TILE"])  # one counter word per (chunk of the batch, row tile)
        self.counter_bytes = -(-4 * groups // 64) * 64
        assert self.nbytes > self.counter_bytes
        self.buffer = torch.zeros(self.nbytes + GUARD_BYTES, dtype=torch.uint8, device=DEV)
        self.buffer[self.nbytes :] = GUARD_BYTE
        self.front = self.buffer[: self.nbytes]

    def check(self):
        assert bool((self.buffer[self.nbytes :] == GUARD_BYTE).all()), "the scratch was written beyond deodr_hip_basis_scratch_bytes"
        assert int(self.front[: self.counter_bytes].view(torch.int32).abs().sum()) == 0, "a counter word did not come back to zero"


def host(t):
    return t.detach().cpu().numpy()


def problem(K, N, batch, basis_dtype, other_dtype, seed):
    """values as they are stored (float32 values are exact in long double)"""
    rs = np.random.RandomState(seed)
    to = lambda a, dtype: a.astype(np.float32 if dtype == F32 else np.float64)
    return dict(B=to(rs.randn(K, N), basis_dtype), mean=to(rs.randn(N), basis_dtype), c=rs.randn(batch, K), g=to(rs.randn(batch, N), other_dtype),
                c0=rs.randn(batch, K))  # fmt: skip


def check_forward(K, N, batch, basis_dtype, y_dtype, with_mean, misalign, seed=0):
    from deodr_amd import hip_renderer as hr

    p = problem(K, N, batch, basis_dtype, y_dtype, seed)
    arena = Arena(misalign)
    B, c = arena.carve(p["B"], dtype=basis_dtype), arena.carve(p["c"])
    mean = arena.carve(p["mean"], dtype=basis_dtype) if with_mean else None
    y, again = arena.carve(shape=(batch, N), dtype=y_dtype), arena.carve(shape=(batch, N), dtype=y_dtype)
    assert hr.basis_apply(B, mean, c, out=y) is y
    hr.basis_apply(B, mean, c, out=again)
    torch.cuda.synchronize()
    arena.check()
    assert torch.equal(y, again)  # bit-identical from run to run
    Bl, cl, ml = p["B"].astype(LD), p["c"].astype(LD), (p["mean"].astype(LD) if with_mean else np.zeros(N, dtype=LD))
    ref = ml[None] + cl @ Bl
    magnitude = np.abs(ml)[None] + np.abs(cl) @ np.abs(Bl)
    bound = (K + 1 + 2) * U * magnitude + (2.0**-24 if y_dtype == F32 else U) * np.abs(ref)
    err = np.abs(host(y).astype(LD) - ref)
    assert np.all(err <= bound), (K, N, batch, basis_dtype, y_dtype, with_mean, float((err / bound).max()), np.argwhere(err > bound)[:4])
    return float((err / bound).max())


def check_adjoint(K, N, batch, basis_dtype, g_dtype, accumulate, misalign, seed=0):
    from deodr_amd import hip_renderer as hr

    p = problem(K, N, batch, basis_dtype, g_dtype, seed)
    arena = Arena(misalign)
    B, g = arena.carve(p["B"], dtype=basis_dtype), arena.carve(p["g"], dtype=g_dtype)
    outs = [arena.carve(p["c0"]) if accumulate else arena.carve(shape=(batch, K)) for _ in range(3)]
    if accumulate:
        arena.made = [m[:4] + (True,) for m in arena.made]  # (nothing of them may be NaN afterwards either)
    scratch, other = Scratch(K, N, batch), Scratch(K, N, batch)
    for out, s in zip(outs, (scratch, scratch, other)):  # twice on one scratch, once on a second zero-filled one
        assert hr.basis_apply_b(B, g, out=out, accumulate=accumulate, scratch=s.front) is out
        torch.cuda.synchronize()
        s.check()  # the counter words are zero again after every call
    arena.check()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    Bl, gl = p["B"].astype(LD), p["g"].astype(LD)
    ref = gl @ Bl.T + (p["c0"].astype(LD) if accumulate else 0)
    magnitude = np.abs(gl) @ np.abs(Bl).T + (np.abs(p["c0"]).astype(LD) if accumulate else 0)
    bound = (N + (1 if accumulate else 0) + 2) * U * magnitude + U * np.abs(ref)
    err = np.abs(host(outs[0]).astype(LD) - ref)
    assert np.all(err <= bound), (K, N, batch, basis_dtype, g_dtype, accumulate, float((err / bound).max()), np.argwhere(err > bound)[:4])
    return float((err / bound).max())


def shape_cases():
    """(K, N, batch): the smallest shapes at which each kernel's loops, tails and launch geometry change"""
    k = constants()
    unroll, tile, chunk, block, segment = k["BASIS_UNROLL"], k["BASIS_ROW_TILE"], k["BASIS_CHUNK"], k["FH_BLOCK"], k["BASIS_SEGMENT"]
    cases = []
    for v in (vec(F32), vec(F64)):
        cases += [(3, n, 1) for n in (1, v - 1, v, v + 1)]  # below, at and behind one piece
        cases += [(3, block * v + d, 1) for d in (-1, 0, 1)]  # one workgroup's span of j
    two, three = first_n_with(3, 2), first_n_with(3, 3)
    assert (two - 1) % segment == 0 and (three - 1) % segment == 0  # (a segment is a whole number of BASIS_SEGMENT elements but for the last: ...
    cases += [(3, two - 1, 1), (3, two, 1), (3, three, 1), (3, 3 * segment + 1, 2)]  # ... so the last segment of `two`, `three` and this one holds ONE element)
    cases += [(K, 2 * block + 3, 1) for K in sorted({1, unroll - 1, unroll, unroll + 1, tile - 1, tile, tile + 1, 2 * tile + 1})]
    cases += [(1024, 5, 1), (1024, 5, chunk + 1)]
    cases += [(tile + 1, block * 4 + 3, b) for b in (chunk, chunk + 1, 64)] + [(3, two + 2, chunk + 1)]
    return sorted(set(c for c in cases if c[1] >= 1))


def storage_combinations(index):
    """all four for the forward (basis x output) and the adjoint (basis x gradient); which of them gets the mean / accumulate rotates with the case"""
    return [(b, o, (index + i) % 2 == 0) for i, (b, o) in enumerate(((F32, F32), (F32, F64), (F64, F32), (F64, F64)))]


def pytest_generate_tests(metafunc):
    if "shape_case" in metafunc.fixturenames:  # (the segment rule is a host function of the library: asked at collection, needs no GPU)
        metafunc.parametrize("shape_case", shape_cases(), ids=lambda c: "K{}_N{}_b{}".format(*c))


def test_kernels_at_the_shapes_where_they_change(shape_case):
    K, N, batch = shape_case
    index = shape_cases().index(shape_case)
    worst = [0.0, 0.0]
    for basis_dtype, other_dtype, flag in storage_combinations(index):
        worst[0] = max(worst[0], check_forward(K, N, batch, basis_dtype, other_dtype, with_mean=flag, misalign=False, seed=index))
        worst[1] = max(worst[1], check_adjoint(K, N, batch, basis_dtype, other_dtype, accumulate=flag, misalign=False, seed=index))
    print(f"K = {K}, N = {N}, batch = {batch}: largest error / bound: forward {worst[0]:.3f}, adjoint {worst[1]:.3f}")


def test_the_regimes_the_shapes_are_meant_for():
    """the cases above are in the regime they exist for, by the library's own rule and the kernels' constants"""
    from deodr_amd import hip_renderer as hr

    k = constants()
    cases = shape_cases()
    segments = {hr.basis_segments(K, N) for K, N, _b in cases}
    assert {1, 2, 3, 4} <= segments
    two = first_n_with(3, 2)
    assert (3, two, 1) in cases and (3, two - 1, 1) in cases and hr.basis_segments(3, two - 1) == 1
    assert {b for _K, _N, b in cases} >= {1, k["BASIS_CHUNK"], k["BASIS_CHUNK"] + 1, 64}
    assert {K for K, _N, _b in cases} >= {1, k["BASIS_UNROLL"] - 1, k["BASIS_UNROLL"] + 1, k["BASIS_ROW_TILE"] - 1, k["BASIS_ROW_TILE"] + 1, 1024}
    assert k["BASIS_SEGMENT"] % (k["FH_BLOCK"] * vec(F32)) == 0 and k["FH_BLOCK"] == 256


@pytest.mark.parametrize("shape", [(9, 1030, 1), (9, 1030, 5), (3, 4099, 2)], ids=lambda c: "K{}_N{}_b{}".format(*c))
def test_tensors_one_element_off_a_16_byte_boundary(shape):
    """every tensor of the call is a slice that starts one element behind a 16-byte boundary; all storage combinations, mean on and off,
    accumulate on and off"""
    K, N, batch = shape
    worst = 0.0
    for basis_dtype, other_dtype, _flag in storage_combinations(0):
        for flag in (False, True):
            worst = max(worst, check_forward(K, N, batch, basis_dtype, other_dtype, with_mean=flag, misalign=True, seed=7))
            worst = max(worst, check_adjoint(K, N, batch, basis_dtype, other_dtype, accumulate=flag, misalign=True, seed=7))
    print(f"misaligned, K = {K}, N = {N}, batch = {batch}: largest error / bound {worst:.3f}")


def test_host_wrappers_refuse_what_the_library_would_misread():
    from deodr_amd import hip_renderer as hr

    B, c, g = torch.zeros(4, 10, device=DEV), torch.zeros(2, 4, dtype=F64, device=DEV), torch.zeros(2, 10, device=DEV)
    for call, bad, what in (
        (hr.basis_apply, dict(basis=torch.zeros(10, 4, device=DEV).T), "contiguous"), (hr.basis_apply, dict(coeffs=c.float()), "float64"),
        (hr.basis_apply, dict(mean=torch.zeros(10, dtype=F64, device=DEV)), "mean must be float32"), (hr.basis_apply, dict(coeffs=c[0]), "shape"),
        (hr.basis_apply, dict(out=torch.zeros(2, 11, device=DEV)), "out must have shape"), (hr.basis_apply, dict(coeffs=c.cpu()), "ROCm tensor"),
        (hr.basis_apply_b, dict(g=g[:, :9]), "shape"), (hr.basis_apply_b, dict(g=g.half()), "float32 or float64"), (hr.basis_apply_b, dict(accumulate=True), "needs out"),
        (hr.basis_apply_b, dict(out=torch.zeros(2, 4, device=DEV)), "out must be float64"),
    ):  # fmt: skip
        arguments = dict(basis=B, mean=None, coeffs=c) if call is hr.basis_apply else dict(basis=B, g=g)
        arguments.update(bad)
        with pytest.raises(ValueError, match=what):
            call(**arguments)
    with pytest.raises(RuntimeError, match="scratch too small"):  # (the library's own refusals, through the wrapper)
        hr.basis_apply_b(B, g, scratch=torch.zeros(8, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="y must not overlap basis, mean or coeffs"):
        square = torch.zeros(4, 4, dtype=F64, device=DEV)
        hr.basis_apply(square, None, square, out=square)
    fresh = hr.basis_apply(B, None, c, out_dtype=F32)  # without out: fresh tensors
    assert fresh.shape == (2, 10) and fresh.dtype == F32 and hr.basis_apply_b(B, g).shape == (2, 4)


def test_kernel_equals_the_torch_fallback_and_autograd_runs_the_adjoint_kernel(monkeypatch):
    from deodr_amd import hip_renderer as hr
    from deodr_amd.basis import LinearBasis

    rs = np.random.RandomState(3)
    K, shape, batch = 11, (37, 3), 3
    N = int(np.prod(shape))
    launched = []
    apply_b = hr.basis_apply_b
    monkeypatch.setattr(hr, "basis_apply_b", lambda *a, **kw: launched.append("b") or apply_b(*a, **kw))
    for dtype in (F32, F64):
        components, mean = rs.randn(K, *shape), rs.randn(*shape)
        kernel, fallback = LinearBasis(components, mean, device=DEV, dtype=dtype), LinearBasis(components, mean, device=DEV, dtype=dtype)
        fallback.uses_kernel = lambda x: False
        for c0 in (rs.randn(K), rs.randn(batch, K)):
            w = torch.as_tensor(rs.randn(*c0.shape[:-1], *shape), device=DEV)
            results = []
            for basis in (kernel, fallback):
                c = torch.tensor(c0, device=DEV, requires_grad=True)
                assert basis.uses_kernel(c) == (basis is kernel)
                del launched[:]
                y = basis.apply(c)
                (c_b,) = torch.autograd.grad((y * w).sum(), c)
                assert launched == (["b"] if basis is kernel else [])  # autograd ran the adjoint kernel
                assert y.shape == (*c0.shape[:-1], *shape) and c_b.shape == c0.shape and y.dtype == F64 and c_b.dtype == F64
                results.append((host(y).reshape(-1, N), host(c_b).reshape(-1, K)))
            # each path is within its bound of the exact value: the two are within twice that of each other
            Bs, ms = host(kernel.components).astype(np.float64), host(kernel.mean).astype(np.float64)
            c2, w2 = np.atleast_2d(c0), host(w).reshape(-1, N)
            bound_y = 2 * ((K + 3) * U * (np.abs(ms)[None] + np.abs(c2) @ np.abs(Bs)) + U * np.abs(results[0][0]))
            bound_c = 2 * ((N + 2) * U * (np.abs(w2) @ np.abs(Bs).T) + U * np.abs(results[0][1]))
            assert np.all(np.abs(results[0][0] - results[1][0]) <= bound_y) and np.all(np.abs(results[0][1] - results[1][1]) <= bound_c)
    # float32 out: the pixel-typed output of the texture fitter
    y32 = kernel.apply(torch.tensor(rs.randn(K), device=DEV), out_dtype=F32)
    assert y32.dtype == F32 and y32.shape == shape


# ---- through the rasterizer, and the fitters


def fixture(name):
    return np.load(os.path.join(GOLDEN, name))


def hand():
    d = fixture("hand_mesh.npz")
    return d["vertices"], d["faces"].astype(np.int64)


def hand_modes(K=4, seed=0):
    """K smooth displacement fields of the hand [K,526,3] with orthonormal rows: low-frequency waves along random directions"""
    vertices, _faces = hand()
    rs = np.random.RandomState(seed)
    centred = (vertices - vertices.mean(axis=0)) / np.abs(vertices - vertices.mean(axis=0)).max()
    fields = [np.sin(centred @ rs.randn(3) * 2.0 + rs.rand() * 6.0)[:, None] * rs.randn(3)[None, :] for _ in range(K)]
    q, _r = np.linalg.qr(np.stack(fields).reshape(K, -1).T)
    return q.T.reshape(K, *vertices.shape).copy()


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_gradients_reach_the_coefficients_through_the_rasterizer():
    """the same hand rendered twice on a 128 x 128 frame -- as basis.apply(c), and as a plain mesh of the same vertices: equal frames, and
    d loss / d c = the contraction of B with d loss / d vertices"""
    from deodr_amd.basis import LinearBasis
    from deodr_amd.scene3d import DeviceCamera, DeviceMesh, Scene3DDevice

    vertices, faces = hand()
    rs = np.random.RandomState(4)
    B = hand_modes(4)
    basis = LinearBasis(B, vertices, dtype=F64)
    rot = np.array([[1.0, 0, 0], [0, -1, 0], [0, 0, -1]])
    cam_center = vertices.mean(axis=0) + np.array([0, 0, 7.0]) * np.max(np.std(vertices, axis=0))
    camera = DeviceCamera(np.column_stack((rot, -rot.T.dot(cam_center))), np.array([[256.0, 0, 64], [0, 256.0, 64], [0, 0, 1]]), 128, 128)
    obs = torch.as_tensor(rs.rand(1, 128, 128, 3)).cuda()
    colors = rs.rand(526, 3)

    def loss_of(mesh):
        scene = Scene3DDevice()
        scene.set_mesh(mesh)
        scene.set_light(np.array([-0.1, -0.5, -0.4]), 0.6)
        scene.set_background_color([0.5, 0.6, 0.7])
        return scene.render_l2(camera, obs)

    c = torch.tensor(0.05 * float(np.abs(vertices).max()) * rs.randn(4), device=DEV, requires_grad=True)
    assert basis.uses_kernel(c)
    derived = basis.apply(c)
    loss, image = loss_of(DeviceMesh(faces, derived, colors=colors))
    loss.backward()
    plain_vertices = derived.detach().clone().requires_grad_(True)
    loss_plain, image_plain = loss_of(DeviceMesh(faces, plain_vertices, colors=colors))
    loss_plain.backward()
    assert torch.equal(image, image_plain) and float(image.std()) > 0.01
    expected = B.reshape(4, -1) @ host(plain_vertices.grad).reshape(-1)
    # the two renders start from the same bits; their vertex gradients are sums of double atomics in whatever order the wavefronts arrive: relative
    # differences of the order of 2^-53 times the number of contributions per vertex -- 1e-12 leaves four orders of magnitude
    print(f"c.grad against B . vertices.grad: {rel(host(c.grad), expected):.3e}")
    assert float(np.abs(expected).max()) > 0 and rel(host(c.grad), expected) <= 1e-12


def depth_fitter(**keywords):
    from deodr_amd.mesh_fitter import MeshDepthFitter

    d = fixture("depth_hand_fit.npz")
    depth = d["depth_raw_f32"].astype(np.float64)
    depth[depth == 0] = float(d["max_depth"])
    vertices, faces = hand()
    f = MeshDepthFitter(vertices, faces, d["euler_init"], d["translation_init"], cregu=1000, **keywords)
    f.set_image(depth / float(d["max_depth"]), focal=241, distortion=d["distortion"])
    f.set_max_depth(1)
    f.set_depth_scale(float(d["depth_scale"]))
    return f


def test_depth_fit_of_the_hand_with_a_shape_basis_eager_and_graphed():
    """The eager and the replayed iteration are the same launches on the same values but for one thing: the rasterizer's gradient accumulators
    are double atomics, whose order is not fixed (tests/test_subdivision_gpu.py holds the subdivided fit to 1e-6 of the first energy for the same
    reason).  So the energies agree step for step within that bound, not bit for bit."""
    from deodr_amd.mesh_fitter import GraphedStep

    B = hand_modes(4)
    keywords = dict(shape_basis=B, coefficient_regu=1.0, sigmas=np.array([1.0, 2.0, 1.0, 0.5]))
    eager = depth_fitter(**keywords)
    assert eager.coefficients.shape == (4,) and eager._direct_iteration(1, False) is None and eager.shape_basis.uses_kernel(eager.coefficients)
    e_eager = [float(eager.step_device()[0]) for _ in range(12)]
    print("eager:", e_eager)
    assert e_eager[11] < e_eager[0] and float(eager.coefficients.abs().max()) > 0
    rendered = host(eager.coefficients - eager.momentum.speed["coefficients"])  # the coefficients of the last step, before its update
    assert rel(host(eager.vertices), hand()[0] + np.tensordot(rendered, B, axes=1)) <= 1e-12  # the derived vertices, refreshed every step
    f = depth_fitter(**keywords)
    graphed = GraphedStep(f, warmup=3)  # 3 + 1 eager steps and 1 on the capture stream: iterations 0 .. 4
    assert f.iter == 5 and ("attr", "coefficients") in graphed.state
    e_graph = [float(graphed.step_device()[0]) for _ in range(7)]  # iterations 5 .. 11
    print("graphed:", e_graph)
    assert np.abs(np.array(e_graph) - np.array(e_eager[5:])).max() <= 1e-6 * e_eager[0]
    assert rel(host(f.coefficients), host(eager.coefficients)) <= 1e-6


def texture_modes(K, shape, seed=0):
    """K smooth random fields [K, *shape] with orthonormal rows"""
    rs = np.random.RandomState(seed)
    ys, xs = np.meshgrid(np.linspace(0, 1, shape[0]), np.linspace(0, 1, shape[1]), indexing="ij")
    fields = [np.stack([np.sin(2 * np.pi * (rs.rand() * xs * 1.5 + rs.rand() * ys * 1.5) + 6 * rs.rand()) for _ in range(shape[2])], axis=-1) for _ in range(K)]
    q, _r = np.linalg.qr(np.stack(fields).reshape(K, -1).T)
    return q.T.reshape(K, *shape).copy()


TEXTURE_FIT = dict(smoothness=0.2, inertia=0.9, damping=0.05, step_max=0.3)


@functools.lru_cache(maxsize=None)
def texture_problem():
    """K = 4 modes of a 32 x 32 x 3 texture on the bumpy sphere, 2 views of 64 x 64; the photographs are rendered from known coefficients"""
    import cpu_raster_texture as crt
    from deodr_amd.scene3d import DeviceCamera, DeviceMesh, Scene3DDevice

    v = crt.sphere_views(n_views=2, size=64, texture_size=32, nu=30, n_rings=20)
    shape = v["texture"].shape
    assert shape == (32, 32, 3)
    B, mean = texture_modes(4, shape), np.full(shape, 0.5)
    truth = mean + np.tensordot(np.array([12.0, -9.0, 7.0, 5.0]), B, axes=1)
    mesh = DeviceMesh(v["faces"], v["vertices"], clockwise=v["clockwise"], uv=v["uv"], faces_uv=v["faces"], texture=truth, device=DEV)
    scene = Scene3DDevice(pixel_dtype=F64)
    scene.set_mesh(mesh)
    scene.set_light(v["light"], v["ambient"])
    scene.set_background_color(v["background"])
    with torch.no_grad():
        obs = host(scene.render(DeviceCamera.stack(v["cameras"], DEV))).astype(np.float64)
    return v, B, mean, obs


def texture_fitter(pixel_dtype, **keywords):
    from deodr_amd.pytorch import MeshTextureFitterMultiFrame

    v, B, mean, obs = texture_problem()
    f = MeshTextureFitterMultiFrame(v["vertices"], v["faces"], v["uv"], v["faces"], mean, v["light"], v["ambient"], cameras=v["cameras"], clockwise=v["clockwise"],
                                    pixel_dtype=pixel_dtype, texture_basis=B, coefficient_regu=0.05, sigmas=np.array([1.0, 2.0, 0.5, 1.0]), **TEXTURE_FIT,
                                    **keywords)  # fmt: skip
    f.set_background_color(v["background"])
    f.set_images(obs)
    return f


def checked_texture_step(fitter, step, stored, what):
    """one iteration by ``step()``; its coefficient update against the formula evaluated in NumPy from THAT step's own texture_b (which holds the data +
    smoothness gradient after the step): c_b = B . texture_b + prior, then the momentum rule.  The contraction is held to the adjoint's derived bound
    (N + 1 terms: the prior is one); the update adds a few roundings of c and of the speed.  -> (energy, coefficients the step rendered)"""
    regu, sigmas, N = 0.05, np.array([1.0, 2.0, 0.5, 1.0]), stored.shape[1]
    c, s = host(fitter.coefficients).copy(), host(fitter.momentum.speed["coefficients"]).copy()
    energy = float(step()[0])
    texture_b = host(fitter._direct[2]["texture_b"]).astype(np.float64).reshape(-1)
    prior = 2 * regu * c / sigmas**2
    c_b = stored @ texture_b + prior
    bound_c_b = (N + 3) * U * (np.abs(stored) @ np.abs(texture_b) + np.abs(prior)) + U * np.abs(c_b)
    assert np.all(np.abs(host(fitter.coefficients_b) - c_b) <= bound_c_b), what
    move = np.clip(-fitter.step_factor_coefficients * c_b, -TEXTURE_FIT["step_max"], TEXTURE_FIT["step_max"])
    s = (1 - TEXTURE_FIT["damping"]) * (TEXTURE_FIT["inertia"] * s + (1 - TEXTURE_FIT["inertia"]) * move)
    bound_c = fitter.step_factor_coefficients * bound_c_b + 8 * U * (np.abs(c) + np.abs(s))
    assert np.all(np.abs(host(fitter.coefficients) - (c + s)) <= bound_c), what
    return energy, c


@pytest.mark.parametrize("pixel_dtype", [F32, F64], ids=["f32", "f64"])
def test_texture_basis_fit_eager_and_graphed(pixel_dtype):
    from deodr_amd.mesh_fitter import GraphedStep

    _v, B, mean, _obs = texture_problem()
    eager = texture_fitter(pixel_dtype)
    assert eager.texture_basis.uses_kernel(eager.coefficients) and eager.texture_basis.dtype == pixel_dtype
    stored = host(eager.texture_basis.components).astype(np.float64)  # the basis as the device holds it (pixel dtype)
    texture_tensor, energies = eager.texture, []
    for it in range(10):
        energy, c = checked_texture_step(eager, eager.step_device, stored, ("eager", it))
        energies.append(energy)
    # the texture the last step rendered: mean + c . B in the pixel dtype, written in place, not clamped
    expected = host(eager.texture_basis.mean).astype(np.float64) + c @ stored
    assert rel(host(eager.texture).reshape(-1), expected) <= (2.0**-23 if pixel_dtype == F32 else 16 * U)
    print(f"{pixel_dtype}: energies", energies)
    assert eager.texture is texture_tensor is eager.mesh.texture and eager.iter == 10
    assert energies[-1] < energies[0]
    f = texture_fitter(pixel_dtype)
    graphed = GraphedStep(f, warmup=3)  # iterations 0 .. 4 are taken while capturing
    assert f.iter == 5 and graphed.state == []  # a fixed kernel sequence on fixed storage: nothing to rebind
    e_graph = [checked_texture_step(f, graphed.step_device, stored, ("graphed", it))[0] for it in range(5, 10)]
    print(f"{pixel_dtype}: graphed", e_graph)
    # (the texture gradient leaves the rasterizer through atomics in the pixel type, whose order is not fixed: the trajectories agree, not their bits)
    tol = 1e-4 if pixel_dtype == F32 else 1e-9
    assert np.abs(np.array(e_graph) - np.array(energies[5:])).max() <= tol * energies[0] and e_graph[-1] < energies[0]
    assert rel(host(f.coefficients), host(eager.coefficients)) <= 10 * tol
