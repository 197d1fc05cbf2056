"""CPU checks (torch fallback) of ``search="grid"``: on CPU tensors ``PointCloudTerm(search="grid")`` equals ``search="brute"`` bit for bit in loss,
terms and gradient, with -1 correspondences exactly beyond ``max_distance``; ``MeshPointCloudFitter(search="grid")`` gives the energies of the
brute-force fit, also with ``subdivisions``, ``rigidity="arap"`` and points -> mesh alone; the default cell size is a function of the clouds alone;
and the refusals: an infinite ``max_distance`` at construction and ``copy_``-ed in later, ``metric="surface"``, a bad ``cell_size``, a bad
``search``."""

import numpy as np
import pytest
import torch

import chamfer_grid_reference as gr
from test_chamfer_fit_host import cloud_fitter, hand


def test_grid_term_equals_the_brute_term_on_cpu_tensors():
    from deodr_amd.chamfer import PointCloudTerm

    for directions in ("both", "points_to_mesh", "mesh_to_points"):
        c = gr.case(90, 300, n=3, seed=4, max_distance="mid", cell_size=0.05)
        keywords = dict(point_weights=c["point_weights"], vertex_weights=c["vertex_weights"], directions=directions, max_distance=c["params"][2],
                        mix=c["params"][:2], normalise=False, device="cpu")  # fmt: skip
        grid, brute = PointCloudTerm(c["points"], search="grid", cell_size=0.05, **keywords), PointCloudTerm(c["points"], **keywords)
        assert grid.search == "grid" and brute.search == "brute" and grid.cell_size == 0.05 and brute.cell_size is None
        v = torch.tensor(c["vertices"], requires_grad=True)
        (lg, tg), (lb, tb) = grid.evaluate(v), brute.evaluate(v)
        assert torch.equal(lg, lb) and torch.equal(tg, tb)
        assert torch.equal(torch.autograd.grad(lg.sum(), v)[0], torch.autograd.grad(lb.sum(), v)[0])
        ref = gr.case(90, 300, n=3, seed=4, max_distance="mid", cell_size=0.05, directions={"both": 3, "points_to_mesh": 1, "mesh_to_points": 2}[directions])
        for got, theirs, want in zip(grid.correspondences(v.detach()), brute.correspondences(v.detach()), (ref["ref_grid"]["nearest_vertex"], ref["ref_grid"]["nearest_point"])):
            assert (got is None) == (want is None) == (theirs is None)
            if got is not None:
                assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want) and 0.1 < float((got < 0).double().mean()) < 0.9  # (the median is over both directions)
                assert bool((got[got >= 0] == theirs[got >= 0]).all())


def test_default_cell_size_depends_on_the_clouds_alone():
    from deodr_amd.chamfer import PointCloudTerm, default_cell_size

    rs = np.random.RandomState(0)
    a, b = rs.rand(400, 3) * [1.0, 2.0, 0.5], rs.rand(100, 3)
    want = max(2 * np.sqrt((1 * 2 + 2 * 0.5 + 1 * 0.5) / 400), 2 * np.sqrt(3.0 / 100))
    assert abs(default_cell_size([a, b]) - want) < 0.05 * want
    assert default_cell_size([np.zeros((7, 3))]) == 1.0  # no extent
    for tau in (0.1, 10.0):
        assert PointCloudTerm([a, b], max_distance=tau, search="grid", device="cpu").cell_size == default_cell_size([a, b])


@pytest.mark.parametrize("name", ["plain", "subdivisions=1", 'rigidity="arap"', "points_to_mesh"])
def test_grid_fit_gives_the_energies_of_the_brute_fit(name):
    tau = 2 * hand()[0].std()
    keywords = {"plain": {}, "subdivisions=1": dict(subdivisions=1), 'rigidity="arap"': dict(rigidity="arap"), "points_to_mesh": dict(directions="points_to_mesh")}[name]
    grid, brute = cloud_fitter(search="grid", max_distance=tau, **keywords), cloud_fitter(max_distance=tau, **keywords)
    assert grid.term.search == "grid" and grid.search == "grid" and brute.search == "brute" and grid.term.cell_size > 0
    e_grid, e_brute = [grid.step()[0] for _ in range(8)], [brute.step()[0] for _ in range(8)]
    assert e_grid == e_brute and e_grid[-1] < e_grid[0]  # (the same torch ops: the same bits)
    nv, npt = grid.term.correspondences(grid._transformed(grid.vertices_leaf).detach())
    assert nv.dtype == torch.int64 and int(nv.min()) >= -1


def test_refusals():
    from deodr_amd.chamfer import PointCloudTerm
    from deodr_amd.pytorch import MeshPointCloudFitter

    cloud = np.random.RandomState(0).rand(30, 3)
    with pytest.raises(ValueError, match='search="grid" needs a finite max_distance'):
        PointCloudTerm(cloud, search="grid", device="cpu")
    with pytest.raises(ValueError, match='search="grid" needs a finite max_distance'):
        PointCloudTerm(cloud, search="grid", max_distance=float("inf"), device="cpu")
    with pytest.raises(ValueError, match='search must be "brute" or "grid"'):
        PointCloudTerm(cloud, search="tree", max_distance=1.0, device="cpu")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="cell_size must be finite and > 0"):
            PointCloudTerm(cloud, search="grid", max_distance=1.0, cell_size=bad, device="cpu")
    with pytest.raises(ValueError, match='cell_size belongs to search="grid"'):
        PointCloudTerm(cloud, max_distance=1.0, cell_size=0.1, device="cpu")
    term = PointCloudTerm(cloud, search="grid", max_distance=1.0, device="cpu")
    v = torch.zeros((7, 3), dtype=torch.float64)
    term.evaluate(v)
    term.params.copy_(torch.tensor([1.0, 1.0, float("inf")], dtype=torch.float64))  # copy_-ed in later, where the host can see it
    with pytest.raises(ValueError, match='search="grid" needs a finite max_distance'):
        term.evaluate(v)
    vertices, faces = hand()
    make = lambda **kw: MeshPointCloudFitter(vertices, faces, np.zeros(3), np.zeros(3), device="cpu", **kw)
    with pytest.raises(ValueError, match='does not go with metric="surface"'):
        make(search="grid", metric="surface", max_distance=1.0)
    with pytest.raises(ValueError, match='search must be "brute" or "grid"'):
        make(search="auto")
    with pytest.raises(ValueError, match='cell_size belongs to search="grid"'):
        make(cell_size=0.1)
    with pytest.raises(ValueError, match='search="grid" needs a finite max_distance'):
        make(search="grid").set_point_cloud(cloud)
    with pytest.raises(ValueError, match="cell_size must be finite and > 0"):
        make(search="grid", max_distance=1.0, cell_size=-2.0).set_point_cloud(cloud)
    assert make().search == "brute" and make().term is None
