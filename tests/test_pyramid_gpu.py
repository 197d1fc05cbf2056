"""GPU tests of the multi-scale L2 data term: ``deodr_hip_pyramid_l2`` against the long-double restatement of tests/pyramid_reference.py over its case
table (the smallest shapes at which the kernels can go wrong and the shapes at which their launch geometry changes), the autograd op against the
torch formulas on the same tensors, a captured call replayed with another schedule of level weights, and the term behind the rasterizer: the vertex
gradient of ``Scene3DDevice.render_pyramid_l2`` and a multi-view fit, eager and replayed as a HIP graph.

The tolerance is derived in tests/pyramid_reference.py: every element of every output lies within TOLERANCE = 16 x (the largest float64 error of the
NumPy restatement, relative to the scale) of the long-double value, relative to that element's own scale; a float32 ``image_b`` gets 2^-24 of its
value for the one rounding when it is stored.

Every call of the case table: the outputs are carved out of larger NaN-filled buffers and the scratch has exactly deodr_hip_pyramid_scratch_bytes
bytes, filled with a pattern (the header: it need not be zeroed), followed by a guard; all checked after the call.  A second call gives the same bits,
and a call without ``image_b`` the same ``terms`` and ``loss``."""

import functools

import numpy as np
import pytest
import torch

import pyramid_reference as pr
from test_basis_gpu import Arena, host

pytestmark = pytest.mark.gpu

LD = pr.LD
DEV = "cuda"
GUARD_BYTES, GUARD_BYTE, FILL_BYTE = 4096, 0xA5, 0x7F
TORCH = {np.float32: torch.float32, np.float64: torch.float64}


@functools.lru_cache(maxsize=None)
def reference(name, variant, dtype):
    """-> (case, its long-double restatement), computed once"""
    case = pr.make_case(name, variant, dtype)
    return case, pr.restate(case["image"], case["obs"], case["weights"], case["levels"], case["lam"])


class GuardedScratch:
    """exactly deodr_hip_pyramid_scratch_bytes bytes filled with a pattern, followed in the same allocation by a guard"""

    def __init__(self, n, H, W, C, levels):
        from deodr_amd.hip_renderer import lib

        self.nbytes = int(lib().deodr_hip_pyramid_scratch_bytes(n, H, W, C, levels))
        assert self.nbytes >= 64 + 8 * 4 * 1024
        self.buffer = torch.full((self.nbytes + GUARD_BYTES,), FILL_BYTE, dtype=torch.uint8, device=DEV)
        self.buffer[self.nbytes :] = GUARD_BYTE
        self.front = self.buffer[: self.nbytes]

    def check(self):
        assert bool((self.buffer[self.nbytes :] == GUARD_BYTE).all()), "the scratch was written beyond deodr_hip_pyramid_scratch_bytes"
        assert bool((self.front[:8] == 0).all()), "the counter words of the scratch were not left at zero"


def within(got, ref, key, f32_output=False):
    value, scale = np.asarray(ref[key]), np.asarray(ref[key + "_scale"])
    err = np.abs(np.asarray(got).astype(LD) - value)
    bound = pr.TOLERANCE * scale + (pr.F32_ROUNDING * np.abs(value) if f32_output else 0)
    assert np.all(err <= bound), (key, float((err / np.maximum(scale, LD(1e-300))).max()), np.argwhere(err > bound)[:4])
    return float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0


@pytest.mark.parametrize("dtype", pr.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("variant", pr.VARIANTS)
@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_kernels_against_long_double(name, variant, dtype):
    from deodr_amd import hip_renderer as hr

    case, ref = reference(name, variant, dtype)
    levels, pix = case["levels"], TORCH[dtype]
    n, H, W, C = case["image"].shape
    arena = Arena()
    image, obs = arena.carve(case["image"], dtype=pix), arena.carve(case["obs"], dtype=pix)
    weights = None if case["weights"] is None else arena.carve(case["weights"], dtype=pix)
    lam = arena.carve(case["lam"])
    outs = [(arena.carve(shape=(levels + 1,)), arena.carve(shape=(1,)), arena.carve(shape=(n, H, W, C), dtype=pix) if with_b else None) for with_b in (True, True, False)]
    scratch = GuardedScratch(n, H, W, C, levels)
    for terms, loss, image_b in outs:
        got = hr.pyramid_l2(image, obs, weights, levels, lam, terms=terms, loss=loss, image_b=image_b, scratch=scratch.front, want_gradient=image_b is not None)
        assert got[0] is terms and got[1] is loss and got[2] is image_b
    torch.cuda.synchronize()
    arena.check(), scratch.check()
    (terms, loss, image_b), (terms2, loss2, image_b2), (terms3, loss3, _) = outs
    assert torch.equal(terms, terms2) and torch.equal(loss, loss2) and torch.equal(image_b, image_b2)  # a second call gives the same bits
    assert torch.equal(terms, terms3) and torch.equal(loss, loss3)  # image_b = NULL gives the same terms
    worst = dict(terms=within(host(terms), ref, "terms"), loss=within(host(loss)[0], ref, "loss"),
                 image_b=within(host(image_b), ref, "image_b", f32_output=dtype == np.float32))  # fmt: skip
    print(f"{case['name']}: largest error relative to the scale " + "  ".join(f"{k} {e:.2e}" for k, e in worst.items()) + f"  (tolerance {pr.TOLERANCE:.2e})")
    assert bool(torch.isfinite(image_b).all())
    if weights is not None:
        assert bool((image_b[weights == 0] == 0).all())  # the gradient is exactly 0 where the weight is
    assert float(terms[0]) > 0 or name == "1x1x1x1_L3"


def test_results_and_scratch_where_none_are_given():
    """the smallest ragged two-tile frame of the three-launch path with nothing but the inputs: the wrapper allocates the results, ``want_gradient=False``
    leaves ``image_b`` None with the same ``terms`` and ``loss``, and the scratch is the one per stream that a larger frame made before"""
    from deodr_amd import hip_renderer as hr

    case = pr.make_case("1x9x8x4_L4", "holes", np.float64)
    image, obs, weights, lam = (torch.as_tensor(case[k], device=DEV) for k in ("image", "obs", "weights", "lam"))
    larger = torch.rand((2, 20, 24, 4), dtype=torch.float64, device=DEV)
    hr.pyramid_l2(larger, larger.flip(0), None, 5, torch.ones(6, dtype=torch.float64, device=DEV))
    key = ("pyramid", image.device, torch.cuda.current_stream(image.device).cuda_stream)
    cached = hr._scratch_cache[key]
    assert cached.numel() >= int(hr.lib().deodr_hip_pyramid_scratch_bytes(2, 20, 24, 4, 5)) > int(hr.lib().deodr_hip_pyramid_scratch_bytes(1, 9, 8, 4, 4))
    terms, loss, image_b = hr.pyramid_l2(image, obs, weights, case["levels"], lam)
    terms2, loss2, none = hr.pyramid_l2(image, obs, weights, case["levels"], lam, want_gradient=False)
    assert hr._scratch_cache[key] is cached  # (neither call made another)
    own = hr.pyramid_l2(image, obs, weights, case["levels"], lam, scratch=hr.pyramid_scratch(1, 9, 8, 4, 4, DEV))
    assert none is None and image_b.shape == image.shape and image_b.dtype == image.dtype and terms.shape == (5,) and loss.shape == (1,)
    assert torch.equal(terms2, terms) and torch.equal(loss2, loss)
    assert torch.equal(own[0], terms) and torch.equal(own[1], loss) and torch.equal(own[2], image_b)
    assert bool((cached[:8] == 0).all())  # the counter is left at zero


def test_op_against_the_torch_formulas_on_the_same_tensors():
    from deodr_amd.pyramid import pyramid_l2, pyramid_l2_torch, pyramid_terms, uses_kernel

    for dtype in pr.DTYPES:
        case, ref = reference("3x17x23x4_L5", "holes", dtype)
        t = lambda a: torch.as_tensor(a, device=DEV)
        obs, weights, lam = t(case["obs"]), t(case["weights"]), t(case["lam"])
        image, image2 = t(case["image"]).requires_grad_(True), t(case["image"]).requires_grad_(True)
        assert uses_kernel(image, obs, weights, lam)
        loss, expected = pyramid_l2(image, obs, weights, 5, lam), pyramid_l2_torch(image2, obs, weights, 5, lam)
        assert loss.shape == expected.shape == () and loss.dtype == torch.float64
        (g,), (g2,) = torch.autograd.grad(3.5 * loss, image), torch.autograd.grad(3.5 * expected, image2)  # a non-unit incoming gradient
        # the kernels within TOLERANCE of the exact value and the torch formulas, another float64 evaluation whose sums the device orders as it likes,
        # within the same (tests/test_pyramid_reference.py holds them to it on the CPU), both relative to the scale
        bound = 2 * pr.TOLERANCE
        assert abs(float(loss.detach()) - float(expected.detach())) <= bound * float(ref["loss_scale"])
        within(float(loss.detach()), ref, "loss")
        err = np.abs(host(g).astype(LD) - 3.5 * ref["image_b"])
        if dtype == np.float64:
            assert np.all(np.abs(host(g).astype(LD) - host(g2).astype(LD)) <= 3.5 * bound * ref["image_b_scale"])
            assert np.all(err <= 3.5 * pr.TOLERANCE * ref["image_b_scale"] + 2.0**-52 * np.abs(3.5 * ref["image_b"]))
        else:  # stored once by the kernel, multiplied by the incoming scalar in float32: two roundings of the value
            assert np.all(err <= 3.5 * pr.TOLERANCE * ref["image_b_scale"] + 2 * pr.F32_ROUNDING * np.abs(3.5 * ref["image_b"]))
        within(host(pyramid_terms(image, obs, weights, 5)), ref, "terms")
        # what the kernels do not take goes through the torch formulas: a non-contiguous image, mixed dtypes
        strided = t(np.ascontiguousarray(case["image"].transpose(0, 2, 1, 3))).transpose(1, 2)
        assert not uses_kernel(strided, obs, weights, lam) and abs(float(pyramid_l2(strided, obs, weights, 5, lam)) - float(expected.detach())) <= bound * float(ref["loss_scale"])
        other = torch.float32 if dtype == np.float64 else torch.float64
        assert not uses_kernel(image, obs.to(other), weights, lam)
        # no gradient asked for: the same value
        assert float(pyramid_l2(image.detach(), obs, weights, 5, lam)) == float(loss.detach())


def test_a_replayed_graph_sees_the_level_weights_of_the_moment():
    from deodr_amd import hip_renderer as hr

    case, ref = reference("2x64x64x3_L6", "holes", np.float32)
    t = lambda a: torch.as_tensor(a, device=DEV)
    image, obs, weights, lam = t(case["image"]), t(case["obs"]), t(case["weights"]), t(case["lam"])
    scratch = hr.pyramid_scratch(2, 64, 64, 3, 6, DEV)
    terms, loss, image_b = hr.pyramid_l2(image, obs, weights, 6, lam, scratch=scratch)  # eager: allocates the outputs
    eager = (loss.clone(), image_b.clone())
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hr.pyramid_l2(image, obs, weights, 6, lam, terms=terms, loss=loss, image_b=image_b, scratch=scratch)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        hr.pyramid_l2(image, obs, weights, 6, lam, terms=terms, loss=loss, image_b=image_b, scratch=scratch)
    loss.zero_(), image_b.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, eager[0]) and torch.equal(image_b, eager[1])
    schedule = np.array([0.0, 0.0, 0.5, 0.0, 3.0, 0.0, 1.25])
    lam.copy_(t(schedule))  # in place: the graph holds the address
    graph.replay()
    torch.cuda.synchronize()
    again = pr.restate(case["image"], case["obs"], case["weights"], 6, schedule)
    within(host(loss)[0], again, "loss"), within(host(image_b), again, "image_b", f32_output=True), within(host(terms), again, "terms")
    assert not torch.equal(image_b, eager[1])


def hand_scene(pixel_dtype, n_views):
    """the hand of the colour fit in ``n_views`` 64 x 64 views, started 3 pixels off its target, with ``pyramid_levels=3``"""
    from test_pyramid_fit_host import hand_fitter

    return hand_fitter(n_views, DEV, pixel_dtype, shift_pixels=(3, -2), pyramid_levels=3)


@pytest.mark.parametrize("pixel_dtype, tolerance", [(torch.float32, 1e-4), (torch.float64, 1e-8)], ids=["float32", "float64"])
def test_vertex_gradient_through_the_rasterizer(pixel_dtype, tolerance):
    """``Scene3DDevice.render_pyramid_l2`` on a 64 x 64 view of the hand against ``render`` + ``pyramid_l2_torch`` through autograd"""
    from deodr_amd.pyramid import pyramid_l2_torch

    f = hand_scene(pixel_dtype, 1)
    lam = torch.as_tensor([1.0, 0.5, 2.0, 0.25], device=DEV)
    weights = torch.rand(1, 64, 64, device=DEV, dtype=pixel_dtype, generator=torch.Generator(DEV).manual_seed(0))
    grads = []
    for use_kernel in (True, False):
        f._leaves(f._appearance_leaves())
        f._pose_scene()
        if use_kernel:
            loss, image = f.scene.render_pyramid_l2(f.camera, f._observation(), 3, weights=weights, level_weights=lam)
        else:
            image = f.scene.render(f.camera)
            loss = pyramid_l2_torch(image, f._observation(), weights, 3, lam)
        assert image.dtype == pixel_dtype and image.shape == (1, 64, 64, 3)
        grads.append((float(loss), torch.autograd.grad(loss, f.vertices_leaf)[0]))
    (loss, g), (loss_torch, g_torch) = grads
    print(f"loss {loss:.6f} / {loss_torch:.6f}; largest vertex gradient {float(g_torch.abs().max()):.3e}, largest difference {float((g - g_torch).abs().max()):.3e}")
    assert abs(loss - loss_torch) <= tolerance * abs(loss_torch) and float(g_torch.abs().max()) > 0
    assert float((g - g_torch).abs().max()) <= tolerance * float(g_torch.abs().max())


def test_multiview_fit_eager_and_graphed():
    """five eager steps of ``MeshRGBFitterWithPoseMultiFrame(pyramid_levels=3)`` on two 64 x 64 views equal five steps under ``GraphedStep``; a schedule
    copied into ``pyramid_weights`` reaches the replayed step"""
    from deodr_amd.mesh_fitter import GraphedStep, MeshRGBFitterWithPoseMultiFrame

    eager = hand_scene(torch.float64, 2)
    assert eager._direct_iteration(3, True) is None and eager.pyramid_weights.device.type == "cuda"
    assert isinstance(eager, MeshRGBFitterWithPoseMultiFrame) and eager.mesh_image.shape == (2, 64, 64, 3)
    e_eager = [float(eager.step_device()[0]) for _ in range(10)]
    f = hand_scene(torch.float64, 2)
    graphed = GraphedStep(f, warmup=3)  # 3 + 1 eager steps and 1 on the capture stream: iterations 0 .. 4
    assert f.iter == 5
    e_graph = [float(graphed.step_device()[0]) for _ in range(5)]  # iterations 5 .. 9
    print("eager:", e_eager, "graphed:", e_graph)
    assert np.abs(np.array(e_graph) - np.array(e_eager[5:])).max() <= 1e-6 * e_eager[0]
    assert torch.allclose(f.vertices, eager.vertices, rtol=0, atol=1e-9)
    # a schedule copied into the tensor (in place: the graph holds its address) reaches the next replay as it reaches the next eager step
    for fitter in (eager, f):
        fitter.pyramid_weights.copy_(torch.tensor([2.0, 0.0, 4.0, 0.5], dtype=torch.float64))
    e_after, g_after = float(eager.step_device()[0]), float(graphed.step_device()[0])
    print("after the new schedule: eager", e_after, "graphed", g_after)
    assert abs(g_after - e_after) <= 1e-6 * e_eager[0] and abs(e_after - e_eager[-1]) > 0.1 * e_eager[-1]
