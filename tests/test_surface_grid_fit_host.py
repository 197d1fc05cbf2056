"""CPU checks (torch fallback) of ``PointSurfaceTerm(search="grid")`` and ``MeshPointCloudFitter(metric="surface", surface_search="grid")``: on CPU
tensors the energies and gradients are those of ``search="brute"`` with the same finite ``max_distance``, bit for bit, and the correspondences are
the restatement's (tests/surface_grid_reference.py): -1 and zero barycentric coordinates where no face lies within ``max_distance``; the
refusals; the defaults build what they build today."""

import numpy as np
import pytest
import torch

import surface_grid_reference as sg
from test_chamfer_fit_host import hand
from test_surface_fit_host import surface_fitter


def test_grid_term_equals_the_brute_term_on_cpu_tensors():
    from deodr_amd.surface import PointSurfaceTerm

    for directions, mask in (("both", 3), ("points_to_mesh", 1), ("mesh_to_points", 2)):
        c = sg.case(F=90, P=300, n=3, seed=4, max_distance="mid", cell_size=0.05, directions=mask)
        keywords = dict(point_weights=c["point_weights"], vertex_weights=c["vertex_weights"], directions=directions, max_distance=c["params"][2],
                        mix=c["params"][:2], normalise=False, device="cpu")  # fmt: skip
        grid, brute = PointSurfaceTerm(c["faces"], 37, c["points"], search="grid", cell_size=0.05, **keywords), PointSurfaceTerm(c["faces"], 37, c["points"], **keywords)
        assert grid.search == "grid" and brute.search == "brute" and grid.cell_size == 0.05 and brute.cell_size is None
        v = torch.tensor(c["vertices"], requires_grad=True)
        (lg, tg), (lb, tb) = grid.evaluate(v), brute.evaluate(v)
        assert torch.equal(lg, lb) and torch.equal(tg, tb)
        assert torch.equal(torch.autograd.grad(lg.sum(), v)[0], torch.autograd.grad(lb.sum(), v)[0])
        ref = c["ref_grid"]
        got, theirs = grid.correspondences(v.detach()), brute.correspondences(v.detach())
        for g, t, want in zip(got, theirs, (ref["nearest_face"], ref["barycentric"], ref["nearest_point"])):
            assert (g is None) == (want is None) == (t is None)
        if mask & 1:
            face, bary = got[0].numpy(), got[1].numpy()
            assert got[0].dtype == torch.int64 and np.array_equal(face, ref["nearest_face"]) and np.array_equal(bary.view(np.int64), ref["barycentric"].view(np.int64))
            assert (face < 0).any() and (face >= 0).any() and not bary[face < 0].any()
            assert bool((got[0][got[0] >= 0] == theirs[0][got[0] >= 0]).all())
        if mask & 2:
            assert np.array_equal(got[2].numpy(), ref["nearest_point"])
        assert sg.mixed(c)


def test_default_cell_size_is_the_clouds_and_the_defaults_build_what_they_build_today():
    from deodr_amd.chamfer import default_cell_size
    from deodr_amd.surface import PointSurfaceTerm

    rs = np.random.RandomState(0)
    faces, cloud = np.array([[0, 1, 2], [1, 2, 3]]), rs.rand(200, 3)
    assert PointSurfaceTerm(faces, 4, cloud, max_distance=0.5, search="grid", device="cpu").cell_size == default_cell_size([cloud])
    plain = PointSurfaceTerm(faces, 4, cloud, device="cpu")
    assert plain.search == "brute" and plain.cell_size is None and float(plain.params[2]) == float("inf")
    f = surface_fitter(count=50)
    assert f.surface_search == "brute" and f.search == "brute" and f.term.search == "brute" and f.term.cell_size is None


@pytest.mark.parametrize("name", ["plain", "subdivisions=1", 'rigidity="arap"', "points_to_mesh"])
def test_grid_fit_gives_the_energies_of_the_brute_fit(name):
    tau = 2 * hand()[0].std()
    keywords = {"plain": {}, "subdivisions=1": dict(subdivisions=1), 'rigidity="arap"': dict(rigidity="arap"), "points_to_mesh": dict(directions="points_to_mesh")}[name]
    grid, brute = surface_fitter(count=600, surface_search="grid", max_distance=tau, **keywords), surface_fitter(count=600, max_distance=tau, **keywords)
    assert grid.term.search == "grid" and grid.surface_search == "grid" and grid.search == "brute" and brute.surface_search == "brute" and grid.term.cell_size > 0
    e_grid, e_brute = [grid.step()[0] for _ in range(6)], [brute.step()[0] for _ in range(6)]
    assert e_grid == e_brute and e_grid[-1] < e_grid[0]  # (the same torch ops: the same bits)
    face, bary, _ = grid.term.correspondences(grid._transformed(grid.vertices_leaf).detach())
    assert face.dtype == torch.int64 and int(face.min()) >= -1 and bary.shape == face.shape + (3,)
    assert surface_fitter(count=50, surface_search="grid", max_distance=tau, cell_size=0.25).term.cell_size == 0.25


def test_refusals():
    from deodr_amd.pytorch import MeshPointCloudFitter
    from deodr_amd.surface import PointSurfaceTerm

    faces, cloud = np.array([[0, 1, 2], [1, 2, 3]]), np.random.RandomState(0).rand(30, 3)
    term = lambda **kw: PointSurfaceTerm(faces, 4, cloud, device="cpu", **kw)
    with pytest.raises(ValueError, match='search="grid" needs a finite max_distance'):
        term(search="grid")
    with pytest.raises(ValueError, match='search="grid" needs a finite max_distance'):
        term(search="grid", max_distance=float("inf"))
    with pytest.raises(ValueError, match='search must be "brute" or "grid"'):
        term(search="tree", max_distance=1.0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="cell_size must be finite and > 0"):
            term(search="grid", max_distance=1.0, cell_size=bad)
    with pytest.raises(ValueError, match='cell_size belongs to search="grid"'):
        term(max_distance=1.0, cell_size=0.1)
    t = term(search="grid", max_distance=1.0)
    v = torch.zeros((4, 3), dtype=torch.float64)
    t.evaluate(v)
    t.params.copy_(torch.tensor([1.0, 1.0, float("inf")], dtype=torch.float64))  # copy_-ed in later, where the host can see it
    with pytest.raises(ValueError, match='search="grid" needs a finite max_distance'):
        t.evaluate(v)
    vertices, hand_faces = hand()
    make = lambda **kw: MeshPointCloudFitter(vertices, hand_faces, np.zeros(3), np.zeros(3), device="cpu", **kw)
    with pytest.raises(ValueError, match='does not go with metric="surface".*surface_search'):
        make(search="grid", metric="surface", max_distance=1.0)
    with pytest.raises(ValueError, match='surface_search must be "brute" or "grid"'):
        make(metric="surface", surface_search="tree")
    with pytest.raises(ValueError, match='surface_search="grid" belongs to metric="surface"'):
        make(surface_search="grid", max_distance=1.0)
    with pytest.raises(ValueError, match='cell_size belongs to surface_search="grid"'):  # (not to search="grid", which the surface metric refuses)
        make(metric="surface", cell_size=0.1)
    with pytest.raises(ValueError, match='cell_size belongs to search="grid"'):
        make(cell_size=0.1)
    with pytest.raises(ValueError, match='search="grid" needs a finite max_distance'):
        make(metric="surface", surface_search="grid").set_point_cloud(cloud)
    with pytest.raises(ValueError, match="cell_size must be finite and > 0"):
        make(metric="surface", surface_search="grid", max_distance=1.0, cell_size=-2.0).set_point_cloud(cloud)
    assert make(metric="surface").surface_search == "brute" and make().surface_search == "brute"
