"""GPU tests of Loop subdivision: ``deodr_hip_subdiv_apply`` (both instances) against SciPy in float64, the autograd op between the control
vertices and the rasterizer, and the fitters with ``subdivisions=k`` -- eager, and replayed as a HIP graph."""

import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
TETRAHEDRON = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def fixture(name):
    return np.load(os.path.join(GOLDEN, name))


def hand():
    d = fixture("hand_mesh.npz")
    return d["vertices"], d["faces"].astype(np.int64)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@functools.lru_cache(maxsize=None)
def subdivision(mesh, n_iter):
    """built once, shared by the tests (the tables are never written)"""
    from deodr_amd.subdivision import LoopSubdivision

    faces = TETRAHEDRON if mesh == "tetrahedron" else hand()[1]
    return LoopSubdivision(faces, 4 if mesh == "tetrahedron" else 526, n_iter)


# (mesh, levels, transposed) -> (lanes per row the host must choose, rows, shortest and longest row)
CASES = {
    ("tetrahedron", 1, False): (8, 10, 4, 4),  # fewer rows than one wavefront holds
    ("hand", 2, False): (8, 8386, 5, 17),  # rows longer than the 8 lanes that walk them
    ("hand", 2, True): (64, 526, 85, 238),  # a wavefront per row, rows longer than the wavefront
    ("hand", 1, True): (8, 526, 13, 34),
}


@pytest.mark.parametrize("case", list(CASES), ids=lambda c: f"{c[0]}{c[1]}{'T' if c[2] else ''}")
def test_subdiv_apply_against_scipy(case):
    """|y - y_ref| <= 4 L 2^-53 (|A| |x|) element-wise, L the longest row: a row's value is a sum of at most L products, each rounded once, added
    in L - 1 rounded additions (first-order bound (L + 1) u (|A| |x|), u = 2^-53; SciPy's own sum carries as much).  With ``accumulate`` the value y
    held is one more term of the sum: |A| |x| + |y0| in its place.  float32 storage: 2^-24 |y_ref| on top (the one rounding of the stored value);
    the inputs are then float32 values, converted exactly."""
    from deodr_amd import hip_renderer as hr

    mesh, n_iter, transposed = case
    lanes, n_rows, shortest, longest = CASES[case]
    sub = subdivision(mesh, n_iter)
    operator = sub._vertices
    A = operator.transposed if transposed else operator.matrix
    lengths = np.diff(A.indptr)
    assert A.shape[0] == n_rows and (lengths.min(), lengths.max()) == (shortest, longest)
    assert sub.lanes(transposed) == lanes == hr.sparse_rows_lanes(n_rows, A.nnz)  # (no parity check can see a call that fell into the slower instance)
    tables = sub.tables(transposed)
    absA = abs(A)
    rs = np.random.RandomState(0)
    worst = 0.0
    for dtype in (F64, F32):
        for batch in (1, 3):
            for D in (1, 2, 3, 4, 5):
                x = torch.as_tensor(rs.randn(batch, A.shape[1], D)).to(dtype).cuda()
                x64 = x.cpu().numpy().astype(np.float64)
                for accumulate in (False, True):
                    y0 = torch.as_tensor(rs.randn(batch, n_rows, D)).to(dtype).cuda()
                    y = y0.clone()
                    out = hr.sparse_rows_apply(*tables, x, out=y, accumulate=accumulate)
                    assert out is y
                    again = y0.clone()
                    hr.sparse_rows_apply(*tables, x, out=again, accumulate=accumulate)
                    assert torch.equal(y, again)  # bit-identical from run to run
                    y064 = y0.cpu().numpy().astype(np.float64)
                    ref = np.stack([A @ x64[b] for b in range(batch)]) + (y064 if accumulate else 0)
                    magnitude = np.stack([absA @ np.abs(x64[b]) for b in range(batch)]) + (np.abs(y064) if accumulate else 0)
                    bound = 4 * longest * 2.0**-53 * magnitude + (2.0**-24 * np.abs(ref) if dtype == F32 else 0)
                    err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
                    worst = max(worst, float((err / bound).max()))
                    assert np.all(err <= bound), (dtype, batch, D, accumulate, float((err / bound).max()))
    print(f"{case}: largest error / bound = {worst:.3f}")
    # without out: a fresh tensor
    x = torch.as_tensor(rs.randn(2, A.shape[1], 3)).cuda()
    fresh = hr.sparse_rows_apply(*tables, x)
    assert fresh.shape == (2, n_rows, 3) and rel(fresh[1].cpu().numpy(), A @ x[1].cpu().numpy()) < 1e-14


def test_host_wrapper_refuses_tensors_the_library_would_misread():
    from deodr_amd import hip_renderer as hr

    offsets, cols, vals = subdivision("tetrahedron", 1).tables()
    x = torch.zeros(1, 4, 3, dtype=F64, device="cuda")
    for bad, what in (
        (dict(x=x[:, :, :2]), "contiguous"), (dict(x=x.half()), "float32 or float64"), (dict(x=x[0]), "shape"), (dict(vals=vals.float()), "float64"),
        (dict(offsets=offsets.long()), "4-byte"), (dict(out=torch.zeros(1, 10, 3, dtype=F32, device="cuda")), "out must be"),
        (dict(out=torch.zeros(1, 9, 3, dtype=F64, device="cuda")), "out must be"), (dict(accumulate=True), "needs out"),
    ):  # fmt: skip
        arguments = dict(offsets=offsets, cols=cols, vals=vals, x=x)
        arguments.update(bad)
        with pytest.raises(ValueError, match=what):
            hr.sparse_rows_apply(**arguments)
    with pytest.raises(RuntimeError, match="y must not overlap x"):  # (the library's own refusal, through the wrapper)
        identity = (torch.arange(5, dtype=torch.int32, device="cuda"), torch.arange(4, dtype=torch.int32, device="cuda"), torch.ones(4, dtype=F64, device="cuda"))
        hr.sparse_rows_apply(*identity, x, out=x)


def test_kernel_equals_the_torch_fallback_and_autograd_runs_the_transpose():
    sub = subdivision("hand", 2)
    rs = np.random.RandomState(3)
    for dtype, tol in ((F64, 1e-14), (F32, 1e-6)):
        x = torch.as_tensor(rs.randn(2, 526, 3)).to(dtype).cuda().requires_grad_(True)
        w = torch.as_tensor(rs.randn(2, 8386, 3)).to(dtype).cuda()
        y = sub.apply(x)
        (g,) = torch.autograd.grad((y * w).sum(), x)
        xc = x.detach().cpu().requires_grad_(True)
        yc = sub.apply(xc)  # CPU tensors: the torch ops
        (gc,) = torch.autograd.grad((yc * w.cpu()).sum(), xc)
        assert rel(y.detach().cpu(), yc.detach()) < tol and rel(g.cpu(), gc) < tol
    colors = torch.as_tensor(rs.rand(526, 4)).cuda()
    assert rel(sub.apply_colors(colors).cpu(), sub.colors_matrix @ colors.cpu().numpy()) < 1e-15
    assert sub.apply(torch.zeros(526, 0, dtype=F64, device="cuda")).shape == (8386, 0)  # (no values per vertex: nothing to launch)


def test_gradients_reach_the_control_vertices_through_the_rasterizer():
    """the same fine mesh rendered twice on a 128 x 128 frame -- as S control, and as a plain mesh of the same vertices: equal losses, and
    d loss / d control = S^T (d loss / d fine vertices)"""
    from deodr_amd.scene3d import DeviceCamera, DeviceMesh, Scene3DDevice

    vertices, faces = hand()
    rs = np.random.RandomState(4)
    rot = np.array([[1.0, 0, 0], [0, -1, 0], [0, 0, -1]])
    cam_center = vertices.mean(axis=0) + np.array([0, 0, 7.0]) * np.max(np.std(vertices, axis=0))
    camera = DeviceCamera(np.column_stack((rot, -rot.T.dot(cam_center))), np.array([[256.0, 0, 64], [0, 256.0, 64], [0, 0, 1]]), 128, 128)
    obs = torch.as_tensor(rs.rand(1, 128, 128, 3)).cuda()

    def loss_of(mesh):
        scene = Scene3DDevice()
        scene.set_mesh(mesh)
        scene.set_light(np.array([-0.1, -0.5, -0.4]), 0.6)
        scene.set_background_color([0.5, 0.6, 0.7])
        return scene.render_l2(camera, obs)

    control = torch.tensor(vertices, device="cuda", requires_grad=True)
    fine = DeviceMesh(faces, control, colors=rs.rand(526, 3)).subdivise(1)
    assert fine.nb_faces == 4192 and fine.vertices.requires_grad and fine.topology is fine.subdivision.topology
    loss, image = loss_of(fine)
    loss.backward()
    fine_vertices = fine.vertices.detach().clone().requires_grad_(True)
    plain = DeviceMesh(fine.subdivision.faces_fine, fine_vertices, colors=fine.vertices_colors.detach())
    loss_plain, image_plain = loss_of(plain)
    loss_plain.backward()
    # the rasterizer's inputs are the same bits in the two renders: the same frames; the loss is the sum of the squared residuals of at most 128^2
    # pixels added by double atomics in whatever order the wavefronts arrive, so two sums differ by at most 2 N 2^-53 of it (N = 128^2 terms)
    print(f"losses: {float(loss)!r}, {float(loss_plain)!r}")
    assert torch.equal(image, image_plain) and float(image.std()) > 0.01
    assert abs(float(loss) - float(loss_plain)) <= 2 * 128 * 128 * 2.0**-53 * float(loss_plain)
    expected = fine.subdivision.matrix.T @ fine_vertices.grad.cpu().numpy()
    print(f"control.grad against S^T fine.grad: {rel(control.grad.cpu(), expected):.3e}")
    assert float(np.abs(expected).max()) > 0 and rel(control.grad.cpu(), expected) <= 1e-12


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


def test_depth_fit_of_a_subdivided_hand_eager_and_graphed():
    from deodr_amd.mesh_fitter import GraphedStep

    eager = depth_fitter(subdivisions=1)
    assert eager.vertices.shape == (526, 3) and eager.mesh.nb_faces == 4192 and eager._direct_iteration(1, False) is None
    e_eager = [float(eager.step_device()[0]) for _ in range(12)]
    print("eager:", e_eager)
    assert e_eager[11] < e_eager[0] and eager.vertices.shape == (526, 3)
    f = depth_fitter(subdivisions=1)
    graphed = GraphedStep(f, warmup=3)  # 3 + 1 eager steps and 1 on the capture stream: iterations 0 .. 4
    assert f.iter == 5
    e_graph = [float(graphed.step_device()[0]) for _ in range(7)]  # iterations 5 .. 11
    print("graphed:", e_graph)
    assert np.abs(np.array(e_graph) - np.array(e_eager[5:])).max() <= 1e-6 * e_eager[0]


def test_subdivisions_zero_takes_the_path_of_today():
    plain, zero = depth_fitter(), depth_fitter(subdivisions=0)
    assert plain._direct_iteration(1, False) is not None and zero._direct_iteration(1, False) is not None  # the fixed kernel sequence, both
    assert zero.mesh is zero.control_mesh
    e_plain, e_zero = ([float(f.step_device()[0]) for _ in range(3)] for f in (plain, zero))
    # (the same launches on the same bits; from the second step on the gradients' atomic sums may arrive in another order)
    assert np.abs(np.array(e_plain) - np.array(e_zero)).max() <= 1e-9 * e_plain[0]


def test_rgb_fit_of_a_twice_subdivided_hand():
    from deodr_amd.mesh_fitter import MeshRGBFitterWithPose

    r = fixture("rgb_hand_fit.npz")
    image = r["image_u8"].astype(np.float64) / 255
    rows, columns = (np.linspace(0, image.shape[i] - 1, 128).round().astype(int) for i in (0, 1))  # the photograph at 128 x 128 (nearest pixel)
    image = image[rows][:, columns]
    _, faces = hand()
    f = MeshRGBFitterWithPose(r["vertices_centered"], faces, np.zeros(3), r["translation_init"], r["default_color"], r["default_light_directional"],
                              float(r["default_light_ambient"]), cregu=1000, subdivisions=2)  # fmt: skip
    f.set_image(image)
    f.set_background_color(r["background_color"])
    assert f.mesh.nb_faces == 16768 and f.mesh.nb_vertices == 8386 and f.vertices.shape == (526, 3)
    for _ in range(3):
        energy, rendered, diff = f.step()
    assert np.isfinite(energy) and rendered.shape == (128, 128, 3) and diff.shape == (128, 128) and rendered.std() > 0.01
    assert f.vertices.shape == (526, 3) and f.iter == 3


def test_colored_trimesh_subdivise_on_the_device():
    from test_subdivision import check_colored_trimesh_subdivise

    check_colored_trimesh_subdivise("cuda")
