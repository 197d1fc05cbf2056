"""CPU checks of Loop subdivision (deodr_amd/subdivision.py): the tables against the reference's ``loop_subdivision`` (tests/golden/loop_subdivision.npz,
written by tests/golden/make_loop_subdivision.py), the boundary rules, the refusals, the torch fallback of the differentiable map (what the kernel
is tested against in tests/test_subdivision_gpu.py), ``ColoredTriMesh.subdivise`` and the ``subdivisions=k`` keyword of the fitters on the
checker-backed rasterizer of tests/cpu_raster.py."""

import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

EPS = float(np.finfo(np.float64).eps)


def fixture(name="loop_subdivision.npz"):
    return np.load(os.path.join(GOLDEN, name))


def hand():
    d = fixture("hand_mesh.npz")
    return d["vertices"], d["faces"].astype(np.int64)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def dense_of_tables(tables, shape):
    """(offsets u32, cols u32, vals) as MeshTopology-style int32 bit patterns -> a dense matrix"""
    offsets, cols, vals = (t.cpu().numpy() for t in tables)
    offsets, cols = offsets.view(np.uint32).astype(np.int64), cols.view(np.uint32).astype(np.int64)
    assert offsets.shape == (shape[0] + 1,) and offsets[0] == 0 and offsets[-1] == len(cols) == len(vals)
    out = np.zeros(shape)
    for r in range(shape[0]):
        assert np.all(np.diff(cols[offsets[r] : offsets[r + 1]]) > 0)  # columns sorted within a row, no duplicates
        out[r, cols[offsets[r] : offsets[r + 1]]] = vals[offsets[r] : offsets[r + 1]]
    return out


FAN_VERTICES = np.array([[0.0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]])
FAN_FACES = np.array([[0, 1, 3], [0, 3, 2], [0, 2, 4], [0, 4, 1]])


def grid_strip():
    """an open strip of 2 x 3 quads (12 triangles, 12 vertices of which 2 are interior), not flat"""
    ys, xs = np.meshgrid(np.arange(3), np.arange(4), indexing="ij")
    vertices = np.column_stack((xs.ravel() * 1.0, ys.ravel() * 1.0, 0.3 * np.sin(1.0 + xs.ravel() + 2 * ys.ravel())))
    faces = []
    for y in range(2):
        for x in range(3):
            a, b, c, d = 4 * y + x, 4 * y + x + 1, 4 * (y + 1) + x, 4 * (y + 1) + x + 1
            faces += [[a, b, d], [a, d, c]]
    return vertices, np.array(faces)


# ---- tables against the reference


def test_tables_equal_the_reference_on_the_octahedron_and_the_hand():
    from deodr_amd.subdivision import LoopSubdivision

    d = fixture()
    vertices, faces = hand()
    for n_iter in (1, 2):
        s = LoopSubdivision(d["octa_faces"], 6, n_iter, device="cpu")
        assert np.array_equal(s.faces_fine, d[f"octa{n_iter}_faces"]) and s.nb_vertices_fine == len(d[f"octa{n_iter}_vertices"])
        for got, expected in ((s.matrix @ d["octa_vertices"], d[f"octa{n_iter}_vertices"]), (s.colors_matrix @ d["octa_colors"], d[f"octa{n_iter}_colors"])):
            err, bound = np.abs(got - expected).max(), 8 * EPS * np.abs(expected).max()
            print(f"octahedron, {n_iter} levels: max error {err:.3e} (bound {bound:.3e})")
            assert err <= bound
        # the tables that go to the device, and their transposes, are the matrices (compared dense)
        for operator, m in ((s._vertices, s.matrix), (s._colors, s.colors_matrix)):
            assert m.has_sorted_indices and m.shape == (s.nb_vertices_fine, 6)
            assert np.array_equal(dense_of_tables(operator.csr_tables(False, "cpu"), m.shape), m.toarray())
            assert np.array_equal(dense_of_tables(operator.csr_tables(True, "cpu"), m.shape[::-1]), m.toarray().T)
        h = LoopSubdivision(faces, len(vertices), n_iter, device="cpu")
        assert h.faces_fine.shape == (1048 * 4**n_iter, 3) and h.matrix.shape == (h.nb_vertices_fine, 526)
        if n_iter == 1:
            assert np.array_equal(h.faces_fine, d["hand1_faces"])
        else:
            assert hashlib.sha256(np.ascontiguousarray(h.faces_fine.astype(np.int64)).tobytes()).hexdigest() == str(d["hand2_faces_sha256"])
        expected = d[f"hand{n_iter}_vertices"]
        err, bound = np.abs(h.matrix @ vertices - expected).max(), 8 * EPS * np.abs(expected).max()
        print(f"hand, {n_iter} levels: max error {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        for s_ in (s, h):
            sums = np.asarray(s_.matrix.sum(axis=1)).ravel()
            assert np.abs(sums - 1).max() <= 4 * n_iter * EPS
            assert s_.matrix.data.min() > 0
    # the row lengths DESIGN.md section 4d quotes for the hand
    lengths = lambda m: (int(np.diff(m.indptr).min()), int(np.diff(m.indptr).max()), int(m.nnz))
    h1, h2 = LoopSubdivision(faces, 526, 1, device="cpu"), LoopSubdivision(faces, 526, 2, device="cpu")
    assert lengths(h1.matrix) == (4, 12, 9958) and lengths(h1._vertices.transposed) == (13, 34, 9958)
    assert lengths(h2.matrix) == (5, 17, 67930) and lengths(h2._vertices.transposed) == (85, 238, 67930)
    assert h2.topology.nb_faces == 16768 and h2.topology.nb_vertices == 8386 and h2.topology.is_closed


def test_composed_levels_equal_levels_applied_one_by_one():
    from deodr_amd.subdivision import LoopSubdivision

    vertices, faces = hand()
    once = LoopSubdivision(faces, 526, 1, device="cpu")
    again = LoopSubdivision(once.faces_fine, once.nb_vertices_fine, 1, device="cpu")
    both = LoopSubdivision(faces, 526, 2, device="cpu")
    assert np.array_equal(both.faces_fine, again.faces_fine)
    assert np.abs(both.matrix @ vertices - again.matrix @ (once.matrix @ vertices)).max() <= 8 * EPS * np.abs(vertices).max()
    with pytest.raises(ValueError, match="n_iter"):
        LoopSubdivision(faces, 526, 0, device="cpu")


# ---- boundary rules, refusals


def test_open_fan_follows_the_standard_boundary_rules():
    from deodr_amd.subdivision import LoopSubdivision

    s = LoopSubdivision(FAN_FACES, 5, 1, device="cpu")
    expected = np.array([[0, 0, 0], [0.75, 0, 0], [-0.75, 0, 0], [0, 0.75, 0], [0, -0.75, 0],  # the centre, the rim vertices
                         [0.375, 0, 0], [-0.375, 0, 0], [0, 0.375, 0], [0, -0.375, 0],  # spoke mid points (edges (0,1) .. (0,4))
                         [0.5, 0.5, 0], [0.5, -0.5, 0], [-0.5, 0.5, 0], [-0.5, -0.5, 0]])  # rim mid points (edges (1,3), (1,4), (2,3), (2,4))  # fmt: skip
    assert np.array_equal(s.matrix @ FAN_VERTICES, expected)
    assert np.array_equal(s.apply(torch.tensor(FAN_VERTICES)).numpy(), expected)
    assert s.faces_fine.shape == (16, 3) and not s.topology.is_closed and s.topology.is_manifold


@pytest.mark.parametrize("mesh", ["fan", "strip"])
def test_boundary_rules_are_affine(mesh):
    """apply(v + t) = apply(v) + t: every row sums to 1 (the reference's boundary edge point has weights that sum to 5/8, and moves by 3.75 when
    the fan is moved by 10)"""
    from deodr_amd.subdivision import LoopSubdivision

    vertices, faces = (FAN_VERTICES, FAN_FACES) if mesh == "fan" else grid_strip()
    t = np.array([10.0, -7.0, 3.0])
    for n_iter in (1, 2):
        s = LoopSubdivision(faces, len(vertices), n_iter, device="cpu")
        moved = s.apply(torch.tensor(vertices + t)).numpy()
        still = s.apply(torch.tensor(vertices)).numpy()
        err, bound = np.abs(moved - (still + t)).max(), 4 * np.spacing(np.linalg.norm(t))
        print(f"{mesh}, {n_iter} levels: |apply(v + t) - apply(v) - t| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        assert np.abs(np.asarray(s.matrix.sum(axis=1)).ravel() - 1).max() <= 4 * n_iter * EPS


def test_meshes_that_are_refused():
    from deodr_amd.subdivision import LoopSubdivision

    with pytest.raises(ValueError, match="more than two faces"):
        LoopSubdivision(np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]]), 5, device="cpu")  # two triangles glued to a third along the edge (0,1)
    with pytest.raises(ValueError, match="more than two boundary edges"):
        LoopSubdivision(np.array([[0, 1, 2], [0, 3, 4]]), 5, device="cpu")  # a bow tie: two triangles that share vertex 0 only
    tetrahedron = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    with pytest.raises(ValueError, match="vertex 4 is referenced by no face"):
        LoopSubdivision(tetrahedron, 5, device="cpu")
    assert LoopSubdivision(tetrahedron, 4, device="cpu").matrix.shape == (10, 4)


def test_textured_meshes_are_refused_with_the_reference_message():
    from deodr_amd import ColoredTriMesh
    from deodr_amd.scene3d import DeviceMesh

    uv, texture = np.random.RandomState(0).rand(5, 2) * 7, np.zeros((8, 8, 3))
    mesh = ColoredTriMesh(FAN_FACES, vertices=FAN_VERTICES, faces_uv=FAN_FACES, uv=uv, texture=texture, device="cpu")
    with pytest.raises(BaseException, match=r"^Textured mesh not supported yet in subdivision\.$"):
        mesh.subdivise(1)
    device_mesh = DeviceMesh(FAN_FACES, FAN_VERTICES, uv=uv, faces_uv=FAN_FACES, texture=texture, device="cpu")
    with pytest.raises(BaseException, match=r"^Textured mesh not supported yet in subdivision\.$"):
        device_mesh.subdivise(1)


# ---- the differentiable map (torch fallback)


def test_gradcheck_of_the_torch_fallback():
    from deodr_amd.subdivision import LoopSubdivision

    s = LoopSubdivision(fixture()["octa_faces"], 6, 2, device="cpu")
    rs = np.random.RandomState(0)
    x = torch.tensor(rs.randn(6, 3), requires_grad=True)
    assert torch.autograd.gradcheck(s.apply, (x,)) and torch.autograd.gradcheck(s.apply_colors, (x,))
    xb = torch.tensor(rs.randn(2, 3, 6, 2), requires_grad=True)  # leading dimensions are a batch
    assert s.apply(xb).shape == (2, 3, 66, 2) and torch.autograd.gradcheck(s.apply, (xb,))
    assert np.abs(s.apply(xb).detach().numpy()[1, 2] - s.matrix @ xb.detach().numpy()[1, 2]).max() < 1e-15
    with pytest.raises(ValueError, match=r"expected \[\.\.\., 6, D\]"):
        s.apply(torch.zeros(5, 3))


def test_backward_is_the_transposed_matrix():
    from deodr_amd.subdivision import LoopSubdivision

    vertices, faces = hand()
    s = LoopSubdivision(faces, 526, 1, device="cpu")
    rs = np.random.RandomState(1)
    x, y = torch.tensor(rs.randn(526, 3), requires_grad=True), torch.tensor(rs.randn(2098, 3))
    sx = s.apply(x)
    (st_y,) = torch.autograd.grad(sx, x, y)
    lhs, rhs = float((sx.detach() * y).sum()), float((x.detach() * st_y).sum())
    bound = 1e-13 * float(sx.detach().norm()) * float(y.norm())
    print(f"<S x, y> - <x, S^T y> = {lhs - rhs:.3e} (bound {bound:.3e})")
    assert abs(lhs - rhs) <= bound
    assert rel(st_y.numpy(), s.matrix.T @ y.numpy()) < 1e-14
    assert rel(s.apply(x.detach().float()).numpy(), s.matrix @ x.detach().numpy()) < 1e-6  # another dtype: same map, in that dtype


# ---- the NumPy-level drop-in


def check_colored_trimesh_subdivise(device):
    from deodr_amd import ColoredTriMesh

    d = fixture()
    mesh = ColoredTriMesh(d["octa_faces"], vertices=d["octa_vertices"], colors=d["octa_colors"], device=device)
    assert mesh.subdivise(0) is mesh
    for n_iter in (1, 2):
        fine = mesh.subdivise(n_iter)
        assert isinstance(fine, ColoredTriMesh) and fine is not mesh and fine.nb_colors == 3
        assert np.array_equal(fine.faces, d[f"octa{n_iter}_faces"])
        assert np.abs(fine.vertices - d[f"octa{n_iter}_vertices"]).max() <= 8 * EPS and np.abs(fine.vertices_colors - d[f"octa{n_iter}_colors"]).max() <= 8 * EPS
        assert fine.adjacencies.is_closed and fine.adjacencies.nb_faces == 8 * 4**n_iter
    assert ColoredTriMesh(d["octa_faces"], vertices=d["octa_vertices"], nb_colors=0, device=device).subdivise(1).vertices_colors is None


def test_colored_trimesh_subdivise_cpu():
    check_colored_trimesh_subdivise("cpu")


def test_device_mesh_subdivise_cpu():
    from deodr_amd.scene3d import DeviceMesh

    d = fixture()
    control = torch.tensor(d["octa_vertices"], requires_grad=True)
    mesh = DeviceMesh(d["octa_faces"], control, colors=d["octa_colors"], device="cpu")
    assert mesh.subdivise(0) is mesh
    fine = mesh.subdivise(2)
    assert fine.nb_vertices == 66 and fine.nb_faces == 128 and np.array_equal(fine.faces_np, d["octa2_faces"])
    assert np.abs(fine.vertices.detach().numpy() - d["octa2_vertices"]).max() <= 8 * EPS
    assert np.abs(fine.vertices_colors.numpy() - d["octa2_colors"]).max() <= 8 * EPS
    w = torch.tensor(np.random.RandomState(2).randn(66, 3))
    (fine.vertices * w).sum().backward()  # gradients reach the control vertices
    assert rel(control.grad.numpy(), fine.subdivision.matrix.T @ w.numpy()) < 1e-14


# ---- the fitters


def reduced_depth_inputs(factor=4):
    d = fixture("depth_hand_fit.npz")
    depth = d["depth_raw_f32"].astype(np.float64)
    depth[depth == 0] = float(d["max_depth"])
    return d, (depth / float(d["max_depth"]))[::factor, ::factor].copy(), 241.0 / factor


def depth_fitter(d, image, focal, **keywords):
    from deodr_amd.mesh_fitter import MeshDepthFitter

    vertices, faces = hand()
    f = MeshDepthFitter(vertices, faces, d["euler_init"], d["translation_init"], cregu=1000, device="cpu", **keywords)
    f.set_image(image, focal=focal, distortion=d["distortion"])
    f.set_max_depth(1)
    f.set_depth_scale(float(d["depth_scale"]))
    return f


def test_depth_fitter_with_one_subdivision_on_the_checker(oracle_api):
    import cpu_raster

    d, image, focal = reduced_depth_inputs()
    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        f = depth_fitter(d, image, focal, subdivisions=1)
        assert f.vertices.shape == (526, 3) and f.mesh.nb_faces == 4192 and f.mesh.nb_vertices == 2098 and f.control_mesh.nb_faces == 1048
        assert f.rigid_energy.topology is f.control_mesh.topology and f._direct_iteration(1, False) is None
        # d data / d control is S^T (d data / d fine), through the step's own graph
        leaf = f._leaves()[0]
        e_data = f.energy()[0]
        g_leaf, g_control, g_fine = torch.autograd.grad(e_data, [leaf, f.last_vertices["control"], f.last_vertices["fine"]])
        assert g_fine.shape == (2098, 3) and float(g_fine.abs().max()) > 0
        expected = f.subdivision.matrix.T @ g_fine.numpy()
        print(f"d data / d control against S^T (d data / d fine): {rel(g_control.numpy(), expected):.3e}")
        assert rel(g_control.numpy(), expected) <= 1e-12
        assert rel(g_leaf.numpy(), expected - expected.mean(axis=0)) <= 1e-12  # the centring: projected on zero-mean displacements
        energies = [f.step()[0] for _ in range(11)]
        print("energies:", energies)
        assert f.vertices.shape == (526, 3) and f.iter == 11
        assert energies[10] < energies[0]


def test_subdivisions_zero_changes_nothing(oracle_api):
    import cpu_raster

    d, image, focal = reduced_depth_inputs()
    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        plain, zero = depth_fitter(d, image, focal), depth_fitter(d, image, focal, subdivisions=0)
        assert zero.mesh is zero.control_mesh and zero.subdivision is None
        assert plain._direct_iteration(1, False) is None and zero._direct_iteration(1, False) is None  # CPU tensors: autograd, both
        assert [plain.step()[0] for _ in range(3)] == [zero.step()[0] for _ in range(3)]
        assert torch.equal(plain.vertices, zero.vertices)
