"""GPU tests of the structural (SSIM) data term: ``deodr_hip_ssim_l2`` against the long-double restatement of tests/ssim_reference.py over its case
table (built for the kernels' tile of 16 x 32 pixels, ssim_reference.TILE: frames inside the window, one tile exactly and one pixel either side of
it, two tiles by two, more tiles than the capped grid), the autograd op against the torch formulas on the same tensors, a captured call replayed
with another mix, and the term behind the rasterizer: the vertex gradient of ``Scene3DDevice.render_ssim_l2`` and a multi-view fit, eager and
replayed as a HIP graph.

The tolerance is derived in tests/ssim_reference.py: TOLERANCE = 8 x (the largest float64 error of the torch formulas, relative to the scale),
relative to ``max |image_b|`` of the case for the gradient, to the term's own value for the two terms and to ``|alpha| term_0 + |beta| term_1`` for
the loss; a float32 ``image_b`` gets 2^-23 of its value for the one rounding when it is stored.

Every call of the case table: the outputs are carved out of larger NaN-filled buffers and the scratch has exactly deodr_hip_ssim_scratch_bytes bytes,
filled with a pattern (the header: it need not be zeroed), followed by a guard; all checked after the call.  A second call gives the same bits, and a
call without ``image_b`` the same ``terms`` and ``loss``."""

import numpy as np
import pytest
import torch

import ssim_reference as sr
from test_basis_gpu import Arena, host

pytestmark = pytest.mark.gpu

LD = sr.LD
DEV = "cuda"
GUARD_BYTES, GUARD_BYTE, FILL_BYTE = 4096, 0xA5, 0x7F
TORCH = {np.float32: torch.float32, np.float64: torch.float64}


class GuardedScratch:
    """exactly deodr_hip_ssim_scratch_bytes bytes filled with a pattern, followed in the same allocation by a guard"""

    def __init__(self, n, H, W, C):
        from deodr_amd.hip_renderer import lib

        self.nbytes = int(lib().deodr_hip_ssim_scratch_bytes(n, H, W, C))
        assert self.nbytes == 64 + 8 * (2 * sr.GRID_CAP + 3 * n * H * W * C)
        self.buffer = torch.full((self.nbytes + GUARD_BYTES,), FILL_BYTE, dtype=torch.uint8, device=DEV)
        self.buffer[self.nbytes :] = GUARD_BYTE
        self.front = self.buffer[: self.nbytes]

    def check(self):
        assert bool((self.buffer[self.nbytes :] == GUARD_BYTE).all()), "the scratch was written beyond deodr_hip_ssim_scratch_bytes"
        assert bool((self.front[:8] == 0).all()), "the counter words of the scratch were not left at zero"


def within(got, ref, key, f32_output=False, factor=1.0):
    """every element of ``got`` within TOLERANCE x the scale of ``key`` (x ``factor``) of the reference; -> the largest error relative to the scale"""
    value = np.asarray(ref[key])
    err = np.abs(np.asarray(got).astype(LD) - factor * value)
    scale = factor * np.broadcast_to(np.asarray(ref[key + "_scale"]), err.shape)
    bound = sr.TOLERANCE * scale + (sr.F32_ROUNDING * np.abs(factor * value) if f32_output else 0)
    assert np.all(err <= bound), (key, float((err / np.maximum(scale, LD(1e-300))).max()), np.argwhere(err > bound)[:4])
    return float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0


@pytest.mark.parametrize("combo", sr.every_case(), ids=sr.case_id)
def test_kernels_against_long_double(combo):
    from deodr_amd import hip_renderer as hr

    case, ref = sr.reference(*combo)
    dtype, pix = combo[2], TORCH[combo[2]]
    n, H, W, C = case["image"].shape
    arena = Arena()
    image, obs = arena.carve(case["image"], dtype=pix), arena.carve(case["obs"], dtype=pix)
    weights = None if case["weights"] is None else arena.carve(case["weights"], dtype=pix)
    mix = arena.carve(np.array(case["mix"]))
    outs = [(arena.carve(shape=(2,)), arena.carve(shape=(1,)), arena.carve(shape=(n, H, W, C), dtype=pix) if with_b else None) for with_b in (True, True, False)]
    scratch = GuardedScratch(n, H, W, C)
    for terms, loss, image_b in outs:
        got = hr.ssim_l2(image, obs, weights, mix, case["data_range"], terms=terms, loss=loss, image_b=image_b, scratch=scratch.front,
                         want_gradient=image_b is not None)  # fmt: skip
        assert got[0] is terms and got[1] is loss and got[2] is image_b
    torch.cuda.synchronize()
    arena.check(), scratch.check()
    (terms, loss, image_b), (terms2, loss2, image_b2), (terms3, loss3, _) = outs
    assert torch.equal(terms, terms2) and torch.equal(loss, loss2) and torch.equal(image_b, image_b2)  # a second call gives the same bits
    assert torch.equal(terms, terms3) and torch.equal(loss, loss3)  # image_b = NULL gives the same terms
    worst = dict(terms=within(host(terms), ref, "terms"), loss=within(host(loss)[0], ref, "loss"),
                 image_b=within(host(image_b), ref, "image_b", f32_output=dtype == np.float32))  # fmt: skip
    print(f"{case['name']}: largest error relative to the scale " + "  ".join(f"{k} {e:.2e}" for k, e in worst.items()) + f"  (tolerance {sr.TOLERANCE:.2e})")
    assert bool(torch.isfinite(image_b).all())
    if combo[1] == "zero":
        assert float(terms.abs().sum()) == 0 and float(image_b.abs().sum()) == 0
    elif case["weights"] is None or (case["weights"] > 0).any():  # (the one pixel of the 1 x 1 frame may have drawn a weight of 0)
        assert float(terms[0]) > 0 and float(terms[1]) > 0


def test_results_and_scratch_where_none_are_given():
    """the ragged 2 x 2 tiles with nothing but the inputs: the wrapper allocates the results, ``want_gradient=False`` leaves ``image_b`` None with the
    same ``terms`` and ``loss``, and the scratch is the one per stream that a larger frame made before"""
    from deodr_amd import hip_renderer as hr

    case = sr.make_case("2x2 tiles ragged 1x29x53x5", "holes255", np.float64)
    image, obs, weights = (torch.as_tensor(case[k], device=DEV) for k in ("image", "obs", "weights"))
    mix = torch.as_tensor(case["mix"], dtype=torch.float64, device=DEV)
    larger = torch.rand((2, 40, 70, 5), dtype=torch.float64, device=DEV)
    hr.ssim_l2(larger, larger.flip(0), None, mix)
    key = ("ssim", image.device, torch.cuda.current_stream(image.device).cuda_stream)
    cached = hr._scratch_cache[key]
    assert cached.numel() >= int(hr.lib().deodr_hip_ssim_scratch_bytes(2, 40, 70, 5)) > int(hr.lib().deodr_hip_ssim_scratch_bytes(1, 29, 53, 5))
    terms, loss, image_b = hr.ssim_l2(image, obs, weights, mix, case["data_range"])
    terms2, loss2, none = hr.ssim_l2(image, obs, weights, mix, case["data_range"], want_gradient=False)
    assert hr._scratch_cache[key] is cached  # (neither call made another)
    own = hr.ssim_l2(image, obs, weights, mix, case["data_range"], scratch=hr.ssim_scratch(1, 29, 53, 5, DEV))
    assert none is None and image_b.shape == image.shape and image_b.dtype == image.dtype and terms.shape == (2,) and loss.shape == (1,)
    assert torch.equal(terms2, terms) and torch.equal(loss2, loss)
    assert torch.equal(own[0], terms) and torch.equal(own[1], loss) and torch.equal(own[2], image_b)
    assert bool((cached[:8] == 0).all())  # the counter is left at zero


def test_op_against_the_torch_formulas_on_the_same_tensors():
    from deodr_amd.ssim import ssim_l2, ssim_l2_torch, ssim_terms, uses_kernel

    for dtype in sr.DTYPES:
        case, ref = sr.reference("2x2 tiles ragged 1x29x53x5", "holes255", dtype)
        t = lambda a: torch.as_tensor(a, device=DEV)
        obs, weights, mix, R = t(case["obs"]), t(case["weights"]), t(np.array(case["mix"])), case["data_range"]
        image, image2 = t(case["image"]).requires_grad_(True), t(case["image"]).requires_grad_(True)
        assert uses_kernel(image, obs, weights, mix)
        loss, expected = ssim_l2(image, obs, weights, mix, R), ssim_l2_torch(image2, obs, weights, mix, R)
        assert loss.shape == expected.shape == () and loss.dtype == torch.float64
        (g,), (g2,) = torch.autograd.grad(3.5 * loss, image), torch.autograd.grad(3.5 * expected, image2)  # a non-unit incoming gradient
        # the kernels within TOLERANCE of the exact value, and the torch formulas -- another float64 evaluation whose sums the device orders as it
        # likes -- within the same, both relative to the scale
        within(float(loss.detach()), ref, "loss"), within(float(expected.detach()), ref, "loss")
        if dtype == np.float64:
            within(host(g2), ref, "image_b", factor=3.5)
            err = np.abs(host(g).astype(LD) - 3.5 * ref["image_b"])
            assert np.all(err <= 3.5 * sr.TOLERANCE * ref["image_b_scale"] + 2.0**-52 * np.abs(3.5 * ref["image_b"]))
        else:  # stored once by the kernel, multiplied by the incoming scalar in float32: two roundings of the value
            err = np.abs(host(g).astype(LD) - 3.5 * ref["image_b"])
            assert np.all(err <= 3.5 * sr.TOLERANCE * ref["image_b_scale"] + 2 * sr.F32_ROUNDING * np.abs(3.5 * ref["image_b"]))
        within(host(ssim_terms(image, obs, weights, R)), ref, "terms")
        # what the kernels do not take goes through the torch formulas: a non-contiguous image, mixed dtypes
        strided = t(np.ascontiguousarray(case["image"].transpose(0, 2, 1, 3))).transpose(1, 2)
        assert not uses_kernel(strided, obs, weights, mix)
        within(float(ssim_l2(strided, obs, weights, mix, R)), ref, "loss")
        other = torch.float32 if dtype == np.float64 else torch.float64
        assert not uses_kernel(image, obs.to(other), weights, mix)
        # no gradient asked for: the same value
        assert float(ssim_l2(image.detach(), obs, weights, mix, R)) == float(loss.detach())


def test_a_replayed_graph_sees_the_mix_of_the_moment():
    from deodr_amd import hip_renderer as hr

    case, ref = sr.reference("2x2 tiles 3x32x64x3", "plain", np.float32)
    t = lambda a: torch.as_tensor(a, device=DEV)
    image, obs, mix = t(case["image"]), t(case["obs"]), t(np.array(case["mix"]))
    scratch = hr.ssim_scratch(3, 32, 64, 3, DEV)
    terms, loss, image_b = hr.ssim_l2(image, obs, None, mix, scratch=scratch)  # eager: allocates the outputs
    eager = (loss.clone(), image_b.clone())
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hr.ssim_l2(image, obs, None, mix, terms=terms, loss=loss, image_b=image_b, scratch=scratch)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        hr.ssim_l2(image, obs, None, mix, terms=terms, loss=loss, image_b=image_b, scratch=scratch)
    loss.zero_(), image_b.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, eager[0]) and torch.equal(image_b, eager[1])
    mix.copy_(t(np.array([0.25, 1.5])))  # in place: the graph holds the address
    graph.replay()
    torch.cuda.synchronize()
    again = sr.restate(case["image"], case["obs"], None, (0.25, 1.5), 1.0)
    within(host(loss)[0], again, "loss"), within(host(image_b), again, "image_b", f32_output=True), within(host(terms), again, "terms")
    assert not torch.equal(image_b, eager[1])


def hand_scene(pixel_dtype, n_views, **keywords):
    """the hand of the colour fit in ``n_views`` 64 x 64 views, started 3 pixels off its target, with ``ssim_weight=0.2``"""
    from test_pyramid_fit_host import hand_fitter

    return hand_fitter(n_views, DEV, pixel_dtype, shift_pixels=(3, -2), ssim_weight=0.2, **keywords)


@pytest.mark.parametrize("pixel_dtype, tolerance", [(torch.float32, 1e-4), (torch.float64, 1e-8)], ids=["float32", "float64"])
def test_vertex_gradient_through_the_rasterizer(pixel_dtype, tolerance):
    """``Scene3DDevice.render_ssim_l2`` on a 64 x 64 view of the hand against ``render`` + ``ssim_l2_torch`` through autograd (the bounds are those of
    the same comparison of the multi-scale term: what float32 and float64 frames leave of a gradient that passes the rasterizer's adjoint)"""
    from deodr_amd.ssim import ssim_l2_torch

    f = hand_scene(pixel_dtype, 1)
    mix = torch.as_tensor([0.6, 0.4], device=DEV)
    weights = torch.rand(1, 64, 64, device=DEV, dtype=pixel_dtype, generator=torch.Generator(DEV).manual_seed(0))
    grads = []
    for use_kernel in (True, False):
        f._leaves(f._appearance_leaves())
        f._pose_scene()
        if use_kernel:
            loss, image = f.scene.render_ssim_l2(f.camera, f._observation(), weights=weights, mix=mix)
        else:
            image = f.scene.render(f.camera)
            loss = ssim_l2_torch(image, f._observation(), weights, mix)
        assert image.dtype == pixel_dtype and image.shape == (1, 64, 64, 3)
        grads.append((float(loss.detach()), torch.autograd.grad(loss, f.vertices_leaf)[0]))
    (loss, g), (loss_torch, g_torch) = grads
    print(f"loss {loss:.6f} / {loss_torch:.6f}; largest vertex gradient {float(g_torch.abs().max()):.3e}, largest difference {float((g - g_torch).abs().max()):.3e}")
    assert abs(loss - loss_torch) <= tolerance * abs(loss_torch) and float(g_torch.abs().max()) > 0
    assert float((g - g_torch).abs().max()) <= tolerance * float(g_torch.abs().max())


def test_multiview_fit_eager_and_graphed():
    """three eager steps of ``MeshRGBFitterWithPoseMultiFrame(ssim_weight=0.2)`` on two 64 x 64 views after the warm-up equal three steps under
    ``GraphedStep``; a mix copied into ``ssim_mix`` reaches the replayed step"""
    from deodr_amd.mesh_fitter import GraphedStep, MeshRGBFitterWithPoseMultiFrame

    eager = hand_scene(torch.float64, 2)
    assert eager._direct_iteration(3, True) is None and eager.ssim_mix.device.type == "cuda" and eager.ssim_mix.tolist() == [0.8, 0.2]
    assert isinstance(eager, MeshRGBFitterWithPoseMultiFrame) and eager.mesh_image.shape == (2, 64, 64, 3)
    e_eager = [float(eager.step_device()[0]) for _ in range(8)]
    f = hand_scene(torch.float64, 2)
    graphed = GraphedStep(f, warmup=3)  # 3 + 1 eager steps and 1 on the capture stream: iterations 0 .. 4
    assert f.iter == 5
    e_graph = [float(graphed.step_device()[0]) for _ in range(3)]  # iterations 5 .. 7
    print("eager:", e_eager, "graphed:", e_graph)
    assert np.abs(np.array(e_graph) - np.array(e_eager[5:])).max() <= 1e-6 * e_eager[0]
    assert torch.allclose(f.vertices, eager.vertices, rtol=0, atol=1e-9)
    # a mix copied into the tensor (in place: the graph holds its address) reaches the next replay as it reaches the next eager step
    for fitter in (eager, f):
        fitter.ssim_mix.copy_(torch.tensor([0.0, 1.0], dtype=torch.float64))
    e_after, g_after = float(eager.step_device()[0]), float(graphed.step_device()[0])
    print("after the new mix: eager", e_after, "graphed", g_after)
    assert abs(g_after - e_after) <= 1e-6 * e_eager[0] and abs(e_after - e_eager[-1]) > 0.1 * e_eager[-1]
