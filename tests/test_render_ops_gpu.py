"""GPU tests of deodr_amd/render_ops.py with the real library: the cases of tests/render_ops_cases.py (every route into the one implementation; two
forwards in one graph on one scene / workspace).  The adjoint accumulates with atomics, so gradients are compared to the bounds the suite already uses
for two runs of the same adjoint: 1e-5 of the largest entry with float32 frames (tests/test_hip_parity.py, the L2 op against render + loss), 1e-9 with
float64 frames (tests/test_hip_round3.py, the fit step with and without its loss); a loss to 1e-9 (tests/test_hip_parity.py)."""

import pytest
import torch

import render_ops_cases as cases
from hip_util import rel_err

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
GRADIENT_BOUND = {F32: 1e-5, F64: 1e-9}


def assert_close_gradients(got, expected, bound, what):
    assert sorted(got) == sorted(expected)
    for k in expected:
        assert float(expected[k].abs().max()) > 0 and got[k].dtype == expected[k].dtype, (what, k)
        err = rel_err(got[k].cpu().numpy(), expected[k].cpu().numpy())
        print(f"{what}: {k}_b differs by {err:.3e} of the largest entry (bound {bound:g})")
        assert err <= bound, (what, k)


@pytest.mark.parametrize("shared", [("texture",), ("texture", "uv")], ids="+".join)
@pytest.mark.parametrize("pixel_dtype", [F32, F64])
def test_every_route_is_the_same_computation(pixel_dtype, shared):
    ds, r, obs, weights, seed = cases.prepared(pixel_dtype)
    (image_a, grads_a), (image_b, grads_b) = cases.render_routes(ds, r, seed, shared)
    assert torch.equal(image_a, image_b)
    assert_close_gradients(grads_a, grads_b, GRADIENT_BOUND[pixel_dtype], "render")
    (loss_a, image_a, grads_a), (loss_b, image_b, grads_b) = cases.l2_routes(ds, r, obs, weights, shared)
    assert torch.equal(image_a, image_b)
    assert_close_gradients(grads_a, grads_b, GRADIENT_BOUND[pixel_dtype], "weighted L2")
    print(f"weighted loss from the frame {loss_a!r}, from the library {loss_b!r}: {abs(loss_a - loss_b) / loss_b:.3e} apart")
    assert abs(loss_a - loss_b) <= 1e-9 * abs(loss_b)


def assert_each_forward_got_its_own(alone, together, bound, what):
    for i, (one, both) in enumerate(zip(alone, together)):
        assert_close_gradients(both, one, bound, f"{what}, forward {i}")
    moved = "ij" if "ij" in alone[0] else "vertices"
    assert rel_err(alone[0][moved].cpu().numpy(), alone[1][moved].cpu().numpy()) > 1e-3  # (the two forwards do differ)


def test_two_forwards_in_one_graph_render_2d():
    assert_each_forward_got_its_own(*cases.stale_2d(), GRADIENT_BOUND[F64], "TorchDifferentiableRender2D")


@pytest.mark.parametrize("pixel_dtype", [F32, F64])
def test_two_forwards_in_one_graph_render_views(pixel_dtype):
    ds, r, _obs, _weights, seed = cases.prepared(pixel_dtype)
    assert_each_forward_got_its_own(*cases.stale_views(ds, r, seed), GRADIENT_BOUND[pixel_dtype], "TorchDifferentiableRenderViews")


@pytest.mark.parametrize("pixel_dtype", [F32, F64])
def test_two_forwards_in_one_graph_scene3d_render(pixel_dtype):
    assert_each_forward_got_its_own(*cases.stale_scene3d(pixel_dtype, "cuda"), GRADIENT_BOUND[pixel_dtype], "Scene3DDevice.render")
