"""CPU checks of the per-pixel weights of the fit step (DeodrHipFitOptions::weights): the options struct on both sides of the C ABI, the
ABI version, and the shape checks of the Python layers -- which must refuse a wrong shape BEFORE anything reaches the library."""

import ctypes
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# DeodrHipFitOptions of include/deodr_hip.h, written out
FIT_OPTIONS_FIELDS = [("tile_loss", ctypes.c_void_p), ("loss", ctypes.c_void_p), ("loss_scratch", ctypes.c_void_p), ("clamp", ctypes.c_int),
                      ("clamp_lo", ctypes.c_double), ("clamp_hi", ctypes.c_double), ("done_flag", ctypes.c_void_p), ("done_value", ctypes.c_uint32),
                      ("weights", ctypes.c_void_p)]  # fmt: skip


def test_fit_options_struct_matches_header():
    """names, order, types, offsets and size of the ctypes mirror (derived from the header by deodr_amd/_abi.py) == the list above and == what
    the C compiler makes of the header"""
    from deodr_amd.hip_renderer import _FitOptionsC
    from sim_util import assert_layout_is_the_compilers

    fields = FIT_OPTIONS_FIELDS
    assert [n for n, _ in fields] == [n for n, _ in _FitOptionsC._fields_]
    assert [t for _, t in fields] == [t for _, t in _FitOptionsC._fields_]
    assert fields[-1] == ("weights", ctypes.c_void_p)  # appended: a zero-initialised struct of an older caller means "no weights"
    mirror = type("Mirror", (ctypes.Structure,), {"_fields_": fields})
    assert ctypes.sizeof(mirror) == ctypes.sizeof(_FitOptionsC)
    for name, _ in fields:
        assert getattr(mirror, name).offset == getattr(_FitOptionsC, name).offset, name
    assert _FitOptionsC().weights is None
    assert_layout_is_the_compilers(_FitOptionsC, "DeodrHipFitOptions", fields)


def test_abi_version_13_on_both_sides():
    import __graft_entry__ as g
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    assert _abi.HEADER.defines["DEODR_HIP_ABI_VERSION"] == 13 == hr.ABI_VERSION
    assert ctypes.CDLL(g.build_hip()).deodr_hip_abi_version() == 13


def test_render_fit_refuses_a_wrong_weights_shape_before_the_library(monkeypatch):
    from deodr_amd import hip_renderer as hr

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(hr, "lib", no_library)
    cpu = torch.device("cpu")
    ds = types.SimpleNamespace(n_views=2, height=24, width=40, nb_colors=3, nb_triangles=5, device=cpu, pixel_dtype=torch.float32)
    r = hr.HipRasterizer.__new__(hr.HipRasterizer)
    r.dims, r.device, r._weights_cache = (5, 24, 40, 3, 2), cpu, None  # (all the shape checks and the conversion touch)
    obs = torch.zeros(2, 24, 40, 3)
    for shape in [(2, 24, 40, 3), (2, 24, 40, 1), (3, 24, 40), (40, 24), (2, 40, 24), (24,), ()]:
        with pytest.raises(ValueError, match="weights"):
            r.render_fit(ds, obs, weights=torch.ones(shape))
        with pytest.raises(ValueError, match="weights"):
            r.render_fit(ds, obs, weights=np.ones(shape))
    # the accepted shapes: converted to [n, H, W] in the scene's pixel dtype, contiguous; a tensor that already is all that is passed through
    w = r._fit_weights(ds, np.full((24, 40), 0.5))
    assert tuple(w.shape) == (2, 24, 40) and w.dtype == torch.float32 and w.is_contiguous() and float(w.min()) == 0.5
    good = torch.rand(2, 24, 40)
    assert r._fit_weights(ds, good) is good
    w64 = torch.rand(2, 24, 40, dtype=torch.float64)
    first = r._fit_weights(ds, w64)
    assert first.dtype == torch.float32 and r._fit_weights(ds, w64) is first  # converted once
    w64.mul_(2)
    again = r._fit_weights(ds, w64)
    assert again is not first and torch.equal(again, w64.float())  # modified in place: converted again


def _hand():
    d = np.load(os.path.join(GOLDEN, "hand_mesh.npz"))
    return d["vertices"], d["faces"].astype(np.int64)


def test_fitters_check_the_weights_shape():
    from deodr_amd.mesh_fitter import MeshDepthFitter, MeshRGBFitterWithPose, MeshRGBFitterWithPoseMultiFrame

    vertices, faces = _hand()
    H, W = 30, 44
    f = MeshDepthFitter(vertices, faces, np.zeros(3), np.zeros(3), device="cpu")
    f.set_image(np.ones((H, W)))
    assert f.weights is None and f._fit_weights() is None
    for bad in (np.ones((W, H)), np.ones((H, W, 1)), np.ones((2, H, W)), np.ones(H)):
        with pytest.raises(ValueError, match="weights"):
            f.set_image(np.ones((H, W)), weights=bad)
    f.set_image(np.ones((H, W)), weights=torch.full((H, W), 0.25))
    assert tuple(f.weights.shape) == (1, H, W) and f.weights.dtype == torch.float64
    assert f._fit_weights().dtype == f.scene.pixel_dtype and f._fit_weights() is f._fit_weights()
    f.set_image(np.ones((H, W)))  # a new image without weights: an unweighted fit again
    assert f.weights is None

    color, light = np.array([0.5, 0.5, 0.5]), np.array([0.0, 0.0, -1.0])
    g = MeshRGBFitterWithPose(vertices, faces, np.zeros(3), np.zeros(3), color, light, 0.1, device="cpu")
    for bad in (np.ones((H, W, 3)), np.ones((W, H)), np.ones((2, H, W))):
        with pytest.raises(ValueError, match="weights"):
            g.set_image(np.ones((H, W, 3)), weights=bad)
    g.set_image(np.ones((H, W, 3)), weights=np.ones((H, W)))
    assert tuple(g.weights.shape) == (1, H, W)

    m = MeshRGBFitterWithPoseMultiFrame(vertices, faces, np.zeros((3, 3)), np.zeros((3, 3)), color, light, 0.1, device="cpu")
    images = [np.ones((H, W, 3))] * 3
    for bad in (np.ones((2, H, W)), np.ones((3, H, W, 3)), np.ones((3, W, H))):
        with pytest.raises(ValueError, match="weights"):
            m.set_images(images, weights=bad)
    w = np.arange(3.0)[:, None, None] * np.ones((3, H, W))
    m.set_images(images, weights=w)
    assert tuple(m.weights.shape) == (3, H, W) and [float(x) for x in m.weights[:, 0, 0]] == [0.0, 1.0, 2.0]  # one plane per view, in the views' order
    m.set_images(images, weights=np.full((H, W), 2.0))  # [H, W]: every view
    assert tuple(m.weights.shape) == (3, H, W) and float(m.weights.min()) == 2.0


def test_sharded_multi_frame_fit_shards_the_weights_with_the_images(monkeypatch):
    """under torch.distributed every rank keeps the weights of ITS views (distributed.shard_views), like the images"""
    import torch.distributed as dist

    from deodr_amd import distributed as dd
    from deodr_amd.mesh_fitter import MeshRGBFitterWithPoseMultiFrame

    vertices, faces = _hand()
    H, W, n = 12, 16, 5
    images = [np.full((H, W, 3), float(i)) for i in range(n)]
    w = np.arange(float(n))[:, None, None] * np.ones((n, H, W))
    for rank in range(2):
        monkeypatch.setattr(dist, "is_initialized", lambda: True)
        monkeypatch.setattr(dist, "get_rank", lambda group=None: rank)
        monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
        m = MeshRGBFitterWithPoseMultiFrame(vertices, faces, np.zeros((n, 3)), np.zeros((n, 3)), np.ones(3), np.array([0.0, 0.0, -1.0]), 0.1, device="cpu")
        mine = list(dd.shard_views(n, rank, 2))
        assert m.my_views == mine and 0 < len(mine) < n
        m.set_images(images, weights=w)
        assert [float(x) for x in m.weights[:, 0, 0]] == [float(i) for i in mine]
        assert [float(x) for x in m.mesh_image[:, 0, 0, 0]] == [float(i) for i in mine]
