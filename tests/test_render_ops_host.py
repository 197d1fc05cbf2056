"""CPU tests of deodr_amd/render_ops.py -- the one implementation of the rasterizer's autograd ops -- under tests/fake_hip.py: every route into it
computes the same thing, bit for bit (the emulation is deterministic); two forwards in one graph on one scene / workspace each get their own gradients;
what a None per-view input leaves alone; gradient dtypes; library calls per op; and the emulation's own handling of per-pixel weights."""

import ctypes

import numpy as np
import pytest
import torch

import fake_hip
import render_ops_cases as cases

PIXEL_DTYPES = [torch.float64, torch.float32]


@pytest.fixture
def fake(oracle_api):
    with fake_hip.emulate(oracle_api.ref() or oracle_api.port(), oracle_api.ref(fixed=True) or oracle_api.port(fixed=True)) as lib:
        yield lib


def assert_same_gradients(got, expected):
    assert sorted(got) == sorted(expected)
    for k in expected:
        assert expected[k] is not None and float(expected[k].abs().max()) > 0, k
        assert got[k].dtype == expected[k].dtype and torch.equal(got[k], expected[k]), k


@pytest.mark.parametrize("shared", [("texture",), ("texture", "uv")], ids="+".join)
@pytest.mark.parametrize("pixel_dtype", PIXEL_DTYPES)
def test_every_route_is_the_same_computation(fake, pixel_dtype, shared):
    ds, r, obs, _weights, seed = cases.prepared(pixel_dtype)
    (image_a, grads_a), (image_b, grads_b) = cases.render_routes(ds, r, seed, shared)
    assert torch.equal(image_a, image_b)
    assert_same_gradients(grads_a, grads_b)
    (loss_a, image_a, grads_a), (loss_b, image_b, grads_b) = cases.l2_routes(ds, r, obs, None, shared)
    assert torch.equal(image_a, image_b)
    assert_same_gradients(grads_a, grads_b)
    print(f"loss from the frame {loss_a!r}, from the library {loss_b!r}")
    assert abs(loss_a - loss_b) <= 1e-12 * abs(loss_b)  # (library loss against frame loss: the bound of tests/test_hip_round3.py)


def assert_each_forward_got_its_own(alone, together):
    for one, both in zip(alone, together):
        assert_same_gradients(both, one)
    moved = "ij" if "ij" in alone[0] else "vertices"
    assert not torch.equal(alone[0][moved], alone[1][moved])  # (the two forwards do differ)


def test_two_forwards_in_one_graph_render_2d(fake):
    assert_each_forward_got_its_own(*cases.stale_2d())


@pytest.mark.parametrize("pixel_dtype", PIXEL_DTYPES)
def test_two_forwards_in_one_graph_render_views(fake, pixel_dtype):
    ds, r, _obs, _weights, seed = cases.prepared(pixel_dtype)
    assert_each_forward_got_its_own(*cases.stale_views(ds, r, seed))


@pytest.mark.parametrize("pixel_dtype", PIXEL_DTYPES)
def test_two_forwards_in_one_graph_scene3d_render(fake, pixel_dtype):
    assert_each_forward_got_its_own(*cases.stale_scene3d(pixel_dtype, "cpu"))


@pytest.mark.parametrize("pixel_dtype", PIXEL_DTYPES)
def test_per_view_inputs_that_are_none_are_left_alone(fake, pixel_dtype):
    from deodr_amd.pytorch import TorchDifferentiableRenderViews

    ds, r, _obs, _weights, _seed = cases.prepared(pixel_dtype)
    before = ds.shade, ds.depths, ds.edgeflags
    x = cases.leaves(ds, ())
    image = TorchDifferentiableRenderViews(x["ij"], x["colors"], ds, r)
    assert ds.shade is before[0] and ds.depths is before[1] and ds.edgeflags is before[2]
    saved = image.grad_fn.saved_tensors
    assert len(saved) == 2 and saved[0].data_ptr() == x["ij"].data_ptr() and saved[1].data_ptr() == x["colors"].data_ptr()
    assert not {t.data_ptr() for t in saved} & {t.data_ptr() for t in before}


@pytest.mark.parametrize("pixel_dtype", PIXEL_DTYPES)
def test_float32_leaves_receive_float32_gradients(fake, pixel_dtype):
    """the scene's vertex arrays are float64, and so are the library's gradients: each is cast to the dtype of its input"""
    from deodr_amd.pytorch import TorchDifferentiableRenderViews, TorchRenderViewsL2Loss
    from deodr_amd.render_ops import RenderViewsFunc, RenderViewsL2Func

    ds, r, obs, _weights, seed = cases.prepared(pixel_dtype)
    per_view = ds.shade.clone(), ds.depths.clone(), ds.edgeflags.clone()
    entries = {
        "TorchDifferentiableRenderViews": lambda x: (TorchDifferentiableRenderViews(x["ij"], x["colors"], ds, r, 1.0, texture=x["texture"]) * seed).sum(),
        "TorchRenderViewsL2Loss": lambda x: TorchRenderViewsL2Loss(x["ij"], x["colors"], obs, ds, r, 1.0, texture=x["texture"]),
        "RenderViewsFunc": lambda x: (RenderViewsFunc.apply(x["ij"], x["colors"], *per_view, ds, r, 1.0, x["texture"])[0] * seed).sum(),
        "RenderViewsL2Func": lambda x: RenderViewsL2Func.apply(x["ij"], x["colors"], *per_view, obs, ds, r, 1.0, None, x["texture"])[0],
    }
    for name, entry in entries.items():
        x = {k: cases.leaf(t.float()) for k, t in cases.leaves(ds, ("texture",)).items()}
        entry(x).backward()
        for k, t in x.items():
            assert t.grad is not None and t.grad.dtype == torch.float32 and float(t.grad.abs().max()) > 0, (name, k)


def test_library_calls_per_op(fake):
    """one render_scene per forward and one render_scene_b per backward of the render op -- also when the forward state is stale: the library
    recomputes it inside that call (have_forward_state = 0), which the rasterizer stamps as a new generation --; one render_scene_fit per forward
    of the L2 op and nothing in its backward"""
    from deodr_amd.pytorch import TorchDifferentiableRenderViews, TorchRenderViewsL2Loss

    ds, r, obs, _weights, seed = cases.prepared(torch.float64)
    inputs = lambda offset: [cases.leaf(ds.ij + offset), cases.leaf(ds.colors)]
    render = lambda offset=0.0: TorchDifferentiableRenderViews(*inputs(offset), ds, r)
    fit = lambda: TorchRenderViewsL2Loss(*inputs(0.0), obs, ds, r)
    render().backward(seed), fit().backward()  # (the first call on a workspace sizes its spill pool with a forward of its own)

    def calls(f):
        before, generation = dict(fake.calls), r.generation
        out = f()
        return out, tuple(fake.calls[k] - before[k] for k in ("render_scene", "render_scene_b", "render_scene_fit")), r.generation - generation

    image, forward, stamps = calls(render)
    assert (forward, stamps) == ((1, 0, 0), 1)
    assert calls(lambda: image.backward(seed))[1:] == ((0, 1, 0), 0)
    first, second = render(), render(0.25)
    assert calls(lambda: first.backward(seed))[1:] == ((0, 1, 0), 1)  # stale
    loss, forward, stamps = calls(fit)
    assert (forward, stamps) == ((0, 0, 1), 1)
    assert calls(loss.backward)[1:] == ((0, 0, 0), 0)
    del second


@pytest.mark.parametrize("pixel_dtype", PIXEL_DTYPES)
def test_the_emulation_honours_weights(fake, pixel_dtype):
    """DeodrHipFitOptions::weights under tests/fake_hip.py: the residual a weighted fit step back-propagates is 2 w (image - obs) and the loss it
    writes is sum w (image - obs)^2 -- in the values the library is handed (frame, observation and weights in the pixel dtype)"""
    from deodr_amd.pytorch import TorchRenderViewsL2Loss
    from deodr_amd.render_ops import RenderViewsL2Func

    ds, r, obs, weights, _seed = cases.prepared(pixel_dtype)
    x = cases.leaves(ds, ())
    TorchRenderViewsL2Loss(x["ij"], x["colors"], obs, ds, r, 1.0, weights=weights).backward()
    image = r.last_fit[0]
    image_b = (2 * weights.double()[..., None] * (image.double() - obs.double())).numpy()
    sc, arrays, _pd = fake._scene(ctypes.byref(ds.c_struct()))
    for i in range(2):
        view = fake._view_scene(sc, arrays, i)  # (the checker's scene of view i, from the arrays the library reads)
        frame, z = fake.checker.render(view, 1.0)
        g = fake.repaired.grads(view, 1.0, frame, z, image_b[i])
        for k in ("ij", "colors"):
            expected = np.nan_to_num(g[k + "_b"])
            assert np.abs(expected).max() > 0 and np.abs(x[k].grad[i].numpy() - expected).max() <= 1e-12 * np.abs(expected).max(), (i, k)
    expected = float((weights.double()[..., None] * (image.double() - obs.double()) ** 2).sum())
    loss = RenderViewsL2Func.apply(x["ij"], x["colors"], ds.shade, ds.depths, ds.edgeflags, obs, ds, r, 1.0, weights, None, None, True)[0]
    assert abs(float(loss.detach()) - expected) <= 1e-12 * expected
    unweighted = float(((image.double() - obs.double()) ** 2).sum())
    assert abs(unweighted - expected) > 0.1 * expected  # (the weights do matter here)
