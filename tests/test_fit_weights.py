"""Per-pixel weights in the one-call fit step (DeodrHipFitOptions::weights, HipRasterizer.render_fit(weights=...)): GPU parity tests.

    L = sum_p w[p] sum_c (f(image) - obs)^2,    dL/dimage = w[p] * 2 (f(image) - obs)   (f: identity or the clamp)

Expected values come from the unmodified reference (the `oracle_api` checker; the repaired one for texture_b, defect D1, as in the existing
parity tests): `image, z = ref.render(scene, sigma)`, `image_b = 2 w (clip(image) - obs)` with zeros where `image` is outside the clamp
interval, `ref.grads(scene, sigma, image, z, image_b)`.  Tolerances are the project's (README "Parity"): image / z 1e-5 and gradients 1e-4
with float32 pixel buffers, 1e-9 / 1e-8 with float64; no pixel may change owner.  The loss is compared with
sum(w (clip(image_returned) - obs)^2) formed in float64 from the returned frame, at the tolerance of the existing `loss_out` tests (1e-12
relative with float64 frames, 1e-9 with float32).  The cases are arranged by tile class: a residual site that ignores the weight shows up
as a wrong gradient in one of them only.
"""

import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from deodr_amd import scenes

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
TOL = {F32: (1e-5, 1e-4), F64: (1e-9, 1e-8)}
LOSS_TOL = {F32: 1e-9, F64: 1e-12}
HAND = os.path.join(GOLDEN, "hand_mesh.npz")


def checker(api, fixed=False):
    return api.ref(fixed=fixed) or api.port(fixed=fixed)


def smooth_weights(n, H, W, seed=0):
    """random smooth weights in [0, 2]: a coarse random grid, bilinearly enlarged"""
    rs = np.random.RandomState(seed)
    coarse = torch.as_tensor(2 * rs.rand(n, 1, max(H // 16, 2), max(W // 16, 2)))
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)[:, 0].clamp(0, 2).numpy()


def mask_weights(n, H, W):
    """a binary mask: zeros over whole 8 x 8 tiles of the frame's border (empty tiles: the loss table), over a slanted band through the
    middle (parts of non-empty tiles) and, with several views, over the whole of view 1"""
    w = np.ones((n, H, W))
    w[:, : 16 if H > 64 else 8, :] = 0
    w[:, :, W - 8 * (W // 8 // 4) :] = 0
    i, j = np.mgrid[0:H, 0:W]
    w[:, np.abs(i - 0.7 * j - 0.1 * H) < 0.06 * H] = 0
    if n > 1:
        w[1] = 0
    return w


def run_fit(views, dt, sigma, w, clamp=None, obs_seed=5, **kw):
    from hip_util import device_scene
    from deodr_amd.hip_renderer import HipRasterizer

    ds = device_scene(views, dt)
    r = HipRasterizer.for_scene(ds)
    shape = (ds.n_views, ds.height, ds.width, ds.nb_colors)
    obs = torch.as_tensor(np.random.RandomState(obs_seed).rand(*shape), device=ds.device).to(dt)
    w_t = None if w is None else torch.as_tensor(w, device=ds.device).to(dt).contiguous()
    loss = torch.zeros(1, dtype=torch.float64, device=ds.device)
    image, z, g = r.render_fit(ds, obs, sigma, check_overflow=True, clear_grads=True, loss_out=loss, clamp=clamp, weights=w_t, **kw)
    torch.cuda.synchronize()
    return ds, r, obs, w_t, image, z, g, loss


def expected_loss(image, obs, w_t, clamp):
    v = image.double()
    if clamp is not None:
        v = v.clamp(*clamp)
    r2 = ((v - obs.double()) ** 2).sum(dim=-1)
    return float((r2 if w_t is None else w_t.double() * r2).sum())


def check_against_reference(api, views, dt, sigma, w, clamp=None, grad_tol=None, clamp_cuts=True, **kw):
    """one weighted fit step of `views` against the reference, view by view; -> the gradients"""
    from hip_util import image_report, rel_err

    views = views if isinstance(views, (list, tuple)) else [views]
    n = len(views)
    ds, r, obs, w_t, image, z, g, loss = run_fit(views, dt, sigma, w, clamp, **kw)
    ref, fixed = checker(api), checker(api, fixed=True)
    tol_img, tol_g = TOL[dt][0], grad_tol or TOL[dt][1]
    uv_sum, tex_sum = 0.0, 0.0
    for i, s in enumerate(views):
        img_ref, z_ref = ref.render(s, sigma)
        im, zz = image[i].cpu().numpy().astype(np.float64), z[i].cpu().numpy().astype(np.float64)
        err, flipped = image_report(im, img_ref, zz, z_ref, tol_img)
        print(f"view {i}: max |image - ref| = {err:.3e}, pixels that changed owner = {flipped}")
        assert flipped == 0 and err < tol_img
        fin = np.isfinite(z_ref)
        assert np.array_equal(np.isfinite(zz), fin)
        if fin.any():
            assert np.abs(zz[fin] - z_ref[fin]).max() < tol_img * max(1.0, np.abs(z_ref[fin]).max())
        o = obs[i].cpu().numpy().astype(np.float64)
        wi = np.asarray(w[i], dtype=np.float64) if w_t is None else w_t[i].cpu().numpy().astype(np.float64)
        if clamp is None:
            image_b = 2 * wi[..., None] * (img_ref - o)
        else:
            inside = (img_ref >= clamp[0]) & (img_ref <= clamp[1])
            assert not clamp_cuts or 0.02 < inside.mean() < 0.98  # (the interval does cut through the frame)
            image_b = 2 * wi[..., None] * (np.clip(img_ref, *clamp) - o) * inside
        gr = ref.grads(s, sigma, img_ref, z_ref, image_b)
        uv_sum = uv_sum + gr["uv_b"]
        if g["texture_b"] is not None and np.size(s.texture):
            tex_sum = tex_sum + fixed.grads(s, sigma, img_ref, z_ref, image_b)["texture_b"]
        for k in ("ij_b", "colors_b", "shade_b"):
            e = rel_err(g[k][i].cpu().numpy(), gr[k])
            print(f"view {i}: rel err {k} = {e:.3e}")
            assert e < tol_g or (np.abs(gr[k]).max() == 0 and np.abs(g[k][i].cpu().numpy()).max() == 0), (k, i, e)
    e = rel_err(g["uv_b"].cpu().numpy(), uv_sum)
    print(f"rel err uv_b = {e:.3e}")
    assert e < tol_g  # (an untextured scene: the reference's uv_b is zero, and rel_err is then 0 only for a uv_b that is exactly zero too)
    if g["texture_b"] is not None and np.size(views[0].texture):
        e = rel_err(g["texture_b"].cpu().numpy(), tex_sum)
        print(f"rel err texture_b = {e:.3e}")
        assert e < tol_g
    want = expected_loss(image, obs, w_t, clamp)
    print(f"loss = {float(loss)!r}, from the returned frame = {want!r}")
    assert abs(float(loss) - want) <= LOSS_TOL[dt] * max(want, 1e-300)
    return g


def both_kinds(n, H, W):
    return [("mask", mask_weights(n, H, W)), ("smooth", smooth_weights(n, H, W, seed=n))]


# ---- 1. edge-free tiles and tile pairs -----------------------------------------------------------------------------------------


@pytest.mark.parametrize("dt", [F32, F64])
def test_weights_edge_free_tiles_and_pairs(oracle_api, dt):
    s = scenes.sphere_scene(size=256, nu=40, n_rings=40)  # C = 4, untextured; sigma = 0: no silhouette edge anywhere
    for _name, w in both_kinds(1, 256, 256):
        check_against_reference(oracle_api, s, dt, 0.0, w)


# ---- 2. tiles with silhouette edges, untextured -------------------------------------------------------------------------------


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("sigma", [1.0, 2.5])
@pytest.mark.parametrize("n_views", [1, 8])
def test_weights_edge_tiles_untextured(oracle_api, n_views, sigma, dt):
    views = [scenes.sphere_scene(size=256, nu=40, n_rings=40, angle=float(a)) for a in np.linspace(-0.4, 0.4, n_views)]
    kind = both_kinds(n_views, 256, 256)[0 if sigma == 1.0 else 1]
    check_against_reference(oracle_api, views, dt, sigma, kind[1])


# ---- 3. textured scenes: the fused edge sweep ---------------------------------------------------------------------------------


@pytest.mark.parametrize("n_views", [1, 2, 8])
def test_weights_textured_fused_edge_sweep(oracle_api, n_views):
    tex = dict(size=256, nu=40, n_rings=40, nb_colors=3, textured=True, texture_size=64)
    views = [scenes.sphere_scene(angle=float(a), **tex) for a in np.linspace(-0.4, 0.4, n_views)]
    for dt, (_name, w) in zip((F32, F64), both_kinds(n_views, 256, 256)):
        check_against_reference(oracle_api, views, dt, 1.0, w)


def test_weights_textured_hand(oracle_api):
    views = [scenes.hand_scene(HAND, size=256, angle=a) for a in (-0.3, 0.4)]
    check_against_reference(oracle_api, views, F32, 1.0, smooth_weights(2, 256, 256, seed=3))
    check_against_reference(oracle_api, views[:1], F64, 0.0, mask_weights(1, 256, 256))  # sigma = 0: the textured instance without the edge adjoint


# ---- 4. mixed soup, a frame whose sides are no multiples of the tile -----------------------------------------------------------


@pytest.mark.parametrize("dt", [F32, F64])
def test_weights_mixed_soup_ragged_frame(oracle_api, dt):
    s = scenes.soup_scene(n_tri=150, width=203, height=117, seed=3, textured_ratio=0.5)
    for _name, w in both_kinds(1, 117, 203):
        check_against_reference(oracle_api, s, dt, 1.0, w)
    s = scenes.soup_scene(n_tri=30, width=53, height=37, seed=6, textured_ratio=0.5, flat=False, texture_size=16)
    s.depths = s.depths + 0.05 * np.random.RandomState(6).rand(s.depths.shape[0]) + 0.2
    check_against_reference(oracle_api, s, dt, 1.5, smooth_weights(1, 37, 53))


# ---- 5. a depth image: one channel, clamp and weights together ----------------------------------------------------------------


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("sigma", [0.0, 1.0])
def test_weights_with_clamp_depth_image(oracle_api, sigma, dt):
    s = scenes.sphere_scene(size=256, nu=40, n_rings=40, nb_colors=1)  # the colour IS the scaled depth: 0.48 .. 0.74 in the frame, background 0.5
    assert s.nb_colors == 1
    for _name, w in both_kinds(1, 256, 256):
        check_against_reference(oracle_api, s, dt, sigma, w, clamp=(0.0, 0.55))  # the interval cuts through the sphere
    check_against_reference(oracle_api, s, dt, sigma, smooth_weights(1, 256, 256), clamp=(0.0, 1.0), clamp_cuts=False)  # the depth fitter's: (0, max_depth)


def test_weights_with_clamp_textured_and_four_channels(oracle_api):
    """the clamp-capable weighted instances of the other scene kinds"""
    s = scenes.sphere_scene(size=128, nu=30, n_rings=30)
    check_against_reference(oracle_api, s, F64, 1.0, smooth_weights(1, 128, 128), clamp=(0.2, 0.65))
    s = scenes.sphere_scene(size=128, nu=30, n_rings=30, nb_colors=3, textured=True, texture_size=32)
    check_against_reference(oracle_api, s, F64, 1.0, mask_weights(1, 128, 128), clamp=(0.2, 0.65))


# ---- 6. the un-staged family: more than 4 channels, the deterministic mode -----------------------------------------------------


@pytest.mark.parametrize("dt", [F32, F64])
def test_weights_six_channels(oracle_api, dt):
    s = scenes.sphere_scene(size=128, nu=30, n_rings=30, nb_colors=6, depth_channel=False)
    for _name, w in both_kinds(1, 128, 128):
        check_against_reference(oracle_api, s, dt, 1.0, w)
    check_against_reference(oracle_api, s, dt, 1.0, smooth_weights(1, 128, 128), clamp=(0.1, 0.6))


@pytest.mark.parametrize("dt", [F32, F64])
def test_weights_deterministic_mode(oracle_api, dt):
    from deodr_amd import hip_renderer as hr

    s = scenes.soup_scene(n_tri=60, width=96, height=80, seed=4, textured_ratio=0.5)
    w = smooth_weights(1, 80, 96, seed=2)
    hr.set_deterministic(True)
    try:
        # (contributions are rounded to 2^-32 in this mode: the project's bound for it is 1e-4 / 1e-6, tests/test_hip_round4.py)
        runs = [check_against_reference(oracle_api, s, dt, 1.0, w, grad_tol=1e-4 if dt == F32 else 1e-6) for _ in range(2)]
    finally:
        hr.set_deterministic(False)
    for k, v in runs[0].items():
        assert v is None or torch.equal(v, runs[1][k]), k


# ---- 8. identities -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize(
    "scene",
    [
        lambda: scenes.sphere_scene(size=256, nu=40, n_rings=40),
        lambda: scenes.sphere_scene(size=256, nu=40, n_rings=40, nb_colors=3, textured=True, texture_size=64),
        lambda: scenes.soup_scene(n_tri=150, width=203, height=117, seed=3, textured_ratio=0.5),
        lambda: scenes.sphere_scene(size=128, nu=30, n_rings=30, nb_colors=6, depth_channel=False),
    ],
    ids=["untextured", "textured", "soup", "six_channels"],
)
@pytest.mark.parametrize("dt", [F32, F64])
def test_weight_zero_and_weight_one(scene, dt):
    from hip_util import rel_err

    s = scene()
    H, W = s.height, s.width
    for sigma in (0.0, 1.0):
        _ds, _r, _obs, _w, image0, z0, g0, loss0 = run_fit([s], dt, sigma, None)
        _ds, _r, _obs, _w, image, z, g, loss = run_fit([s], dt, sigma, np.zeros((1, H, W)))
        assert torch.equal(image, image0) and torch.equal(z, z0)  # pixels of weight 0 are still rendered
        assert float(loss) == 0.0
        for k, v in g.items():
            assert v is None or not bool(v.any()), k
        _ds, _r, _obs, _w, image, z, g, loss = run_fit([s], dt, sigma, np.ones((1, H, W)))
        assert torch.equal(image, image0) and torch.equal(z, z0)
        assert abs(float(loss) - float(loss0)) <= LOSS_TOL[dt] * float(loss0)
        for k, v in g.items():
            if v is not None:
                assert rel_err(v.cpu().numpy(), g0[k].cpu().numpy()) < TOL[dt][1], k


def test_weight_one_is_bit_identical_in_deterministic_mode():
    from deodr_amd import hip_renderer as hr

    s = scenes.soup_scene(n_tri=60, width=96, height=80, seed=4, textured_ratio=0.5)
    hr.set_deterministic(True)
    try:
        g0, loss0 = run_fit([s], F64, 1.0, None)[6:]
        g1, loss1 = run_fit([s], F64, 1.0, np.ones((1, 80, 96)))[6:]
    finally:
        hr.set_deterministic(False)
    assert float(loss0) == float(loss1)
    for k, v in g0.items():
        assert v is None or torch.equal(v, g1[k]), k


def test_unweighted_call_after_a_weighted_one(oracle_api):
    """the loss-table cache of the rasterizer is keyed by the weights: None after a weighted call gives the unweighted loss, another
    weights tensor (or the same one modified in place) another table"""
    from hip_util import rel_err

    s = scenes.sphere_scene(size=256, nu=40, n_rings=40)
    ds, r, obs, w_t, image, z, g, loss = run_fit([s], F64, 1.0, mask_weights(1, 256, 256))
    assert abs(float(loss) - expected_loss(image, obs, w_t, None)) <= 1e-12 * float(loss)
    g_w = {k: v.clone() for k, v in g.items() if v is not None}
    image, z, g = r.render_fit(ds, obs, 1.0, clear_grads=True, loss_out=loss)
    assert abs(float(loss) - expected_loss(image, obs, None, None)) <= 1e-12 * float(loss)
    fresh = run_fit([s], F64, 1.0, None)[6]
    for k, v in g.items():
        if v is not None:
            assert rel_err(v.cpu().numpy(), fresh[k].cpu().numpy()) < 1e-8, k
    assert rel_err(g["ij_b"].cpu().numpy(), g_w["ij_b"].cpu().numpy()) > 1e-3  # (the mask did matter)
    w2 = torch.as_tensor(smooth_weights(1, 256, 256), device=ds.device)
    image, z, g = r.render_fit(ds, obs, 1.0, clear_grads=True, loss_out=loss, weights=w2)
    assert abs(float(loss) - expected_loss(image, obs, w2, None)) <= 1e-12 * float(loss)
    w2.mul_(0.5)  # same address, new version
    image, z, g = r.render_fit(ds, obs, 1.0, clear_grads=True, loss_out=loss, weights=w2)
    assert abs(float(loss) - expected_loss(image, obs, w2, None)) <= 1e-12 * float(loss)
    # [H, W] weights are expanded over the views
    image, z, g2 = r.render_fit(ds, obs, 1.0, clear_grads=True, loss_out=loss, weights=w2[0])
    assert abs(float(loss) - expected_loss(image, obs, w2, None)) <= 1e-12 * float(loss)


# ---- 9. accumulation and the step-done flag ------------------------------------------------------------------------------------


@pytest.mark.parametrize("textured", [False, True])
def test_weights_clear_grads_and_done_flag(textured):
    from hip_util import device_scene, rel_err
    from deodr_amd import hip_renderer as hr
    from deodr_amd.hip_renderer import HipRasterizer

    kw = dict(nb_colors=3, textured=True, texture_size=64) if textured else {}
    views = [scenes.sphere_scene(size=256, nu=40, n_rings=40, angle=a, **kw) for a in (-0.2, 0.3)]
    ds = device_scene(views, F64)
    r = HipRasterizer.for_scene(ds)
    obs = torch.as_tensor(np.random.RandomState(6).rand(2, 256, 256, ds.nb_colors), device=ds.device)
    w = torch.as_tensor(smooth_weights(2, 256, 256), device=ds.device)
    once = r.render_fit(ds, obs, 1.0, check_overflow=True, clear_grads=True, weights=w)[2]
    once = {k: v.clone() for k, v in once.items() if v is not None}
    g = ds.zero_grads()
    for _ in range(2):
        r.render_fit(ds, obs, 1.0, grads=g, clear_grads=False, weights=w)  # accumulated into
    for k, v in once.items():
        assert rel_err(g[k].cpu().numpy(), 2 * v.cpu().numpy()) < 1e-9, k
    r.render_fit(ds, obs, 1.0, grads=g, clear_grads=True, weights=w)  # cleared first
    for k, v in once.items():
        assert rel_err(g[k].cpu().numpy(), v.cpu().numpy()) < 1e-9, k
    flag = torch.zeros(1, dtype=torch.int32, device=ds.device)
    status = torch.zeros(1, dtype=torch.int32, device=ds.device)
    side = torch.cuda.Stream()
    for step in (1, 2, 3):
        r.render_fit(ds, obs, 1.0, grads=g, clear_grads=True, check_overflow=False, done_flag=(flag, step), weights=w)
        with torch.cuda.stream(side):
            hr.wait_flag(flag, step, status=status, timeout=5.0)
            copy = g["ij_b"].clone()
        side.synchronize()
        assert rel_err(copy.cpu().numpy(), once["ij_b"].cpu().numpy()) < 1e-9
    torch.cuda.synchronize()
    assert int(flag.item()) == 3 and int(status.item()) == 0


# ---- 10. the layers above ------------------------------------------------------------------------------------------------------


def test_autograd_l2_loss_op_with_weights():
    from hip_util import device_scene, rel_err
    from deodr_amd.hip_renderer import HipRasterizer
    from deodr_amd.pytorch import TorchDifferentiableRenderViews, TorchRenderViewsL2Loss

    views = [scenes.hand_scene(HAND, size=128, angle=a, textured=False) for a in (-0.3, 0.4)]
    ds = device_scene(views, F32)
    r = HipRasterizer.for_scene(ds)
    obs = torch.as_tensor(np.random.RandomState(4).rand(2, 128, 128, 3).astype(np.float32), device=ds.device)
    w = torch.as_tensor(mask_weights(2, 128, 128) * smooth_weights(2, 128, 128), device=ds.device).float()
    grads = []
    for fused in (True, False):
        ij = ds.ij.clone().requires_grad_(True)
        colors = ds.colors.clone().requires_grad_(True)
        if fused:
            loss = TorchRenderViewsL2Loss(ij, colors, obs, ds, r, 1.0, weights=w)
        else:
            loss = (w.double()[..., None] * (TorchDifferentiableRenderViews(ij, colors, ds, r, 1.0).double() - obs.double()) ** 2).sum()
        (3.0 * loss).backward()
        grads.append((float(loss.detach()), ij.grad.cpu().numpy(), colors.grad.cpu().numpy()))
    assert abs(grads[0][0] - grads[1][0]) <= 1e-9 * abs(grads[1][0])
    assert rel_err(grads[0][1], grads[1][1]) < 1e-5 and rel_err(grads[0][2], grads[1][2]) < 1e-5  # (the bound of the unweighted twin of this test)


@pytest.mark.parametrize("textured", [False, True])
def test_scene3d_render_l2_with_weights(textured):
    from deodr_amd.scene3d import DeviceCamera, DeviceMesh, Scene3DDevice

    d = np.load(HAND)
    vertices, faces = d["vertices"], d["faces"].astype(np.int64)
    rot = np.array([[1.0, 0, 0], [0, -1, 0], [0, 0, -1]])
    radius = np.max(np.std(vertices, axis=0))
    ext = []
    for shift in (np.array([0, 0, 9.0]), np.array([2.5, 1.0, 7.0])):
        center = vertices.mean(axis=0) + shift * radius
        ext.append(np.column_stack((rot, -rot.T.dot(center))))
    cam = DeviceCamera(np.stack(ext), np.tile(np.array([[260.0, 0, 64], [0, 260.0, 64], [0, 0, 1]]), (2, 1, 1)), 128, 128)
    rs = np.random.RandomState(1)
    obs = torch.as_tensor(rs.rand(2, 128, 128, 3), device="cuda")
    w = torch.as_tensor(mask_weights(2, 128, 128) * smooth_weights(2, 128, 128), device="cuda")
    w[1] = torch.as_tensor(smooth_weights(1, 128, 128, seed=9)[0], device="cuda")
    extra = dict(uv=rs.rand(len(vertices), 2) * 30 + 1, faces_uv=faces, texture=rs.rand(32, 32, 3)) if textured else dict(colors=rs.rand(len(vertices), 3))
    out = []
    for fused in (True, False):
        v = torch.tensor(vertices, device="cuda", requires_grad=True)
        scene = Scene3DDevice()
        scene.set_mesh(DeviceMesh(faces, v, device="cuda", **extra))
        scene.set_light(np.array([0.3, 0.2, -0.9]), 0.3)
        scene.set_background_color([0.2, 0.3, 0.4])
        if fused:
            loss, _image = scene.render_l2(cam, obs, weights=w)
        else:
            loss = (w[..., None] * (scene.render(cam) - obs) ** 2).sum()
        loss.backward()
        out.append((float(loss.detach()), v.grad.cpu().numpy()))
    assert abs(out[0][0] - out[1][0]) <= 1e-12 * abs(out[1][0])
    assert np.abs(out[0][1] - out[1][1]).max() <= 1e-8 * np.abs(out[1][1]).max()
    with pytest.raises(ValueError):
        scene.render_l2(cam, obs, weights=w[:, :64])


def _holed_depth_fitter(direct=True):
    from deodr_amd.mesh_fitter import MeshDepthFitter

    d = np.load(os.path.join(GOLDEN, "depth_hand_fit.npz"))
    depth = d["depth_raw_f32"].astype(np.float64)
    max_depth = float(d["max_depth"])
    depth[depth == 0] = max_depth
    mask = np.ones(depth.shape)
    rs, side = np.random.RandomState(0), min(depth.shape) // 12
    for _ in range(12):  # holes: the sensor returned 0 there
        i, j = rs.randint(0, depth.shape[0] - side), rs.randint(0, depth.shape[1] - side)
        depth[i : i + side, j : j + side], mask[i : i + side, j : j + side] = 0.0, 0.0
    hand = np.load(HAND)
    f = MeshDepthFitter(hand["vertices"], hand["faces"].astype(np.int64), d["euler_init"], d["translation_init"], cregu=1000)
    f.set_image(depth / max_depth, focal=241, distortion=d["distortion"], weights=mask)
    f.set_max_depth(1)
    f.set_depth_scale(float(d["depth_scale"]))
    f.direct = direct
    return f, mask


def test_depth_fitter_with_holes_and_mask():
    """MeshDepthFitter with a holed target + mask: the GraphedStep replay equals the eager direct path over 10 iterations, and the direct
    path equals the autograd path (energy within 1e-9, the bound of test_direct_fit_iteration_equals_the_autograd_iteration)"""
    from deodr_amd.mesh_fitter import GraphedStep

    eager, mask = _holed_depth_fitter()
    auto, _ = _holed_depth_fitter(direct=False)
    e_eager = []
    for step in range(15):
        out = eager.step_device()
        assert eager._direct_state is not None
        e_eager.append(float(out[0]))
        if step < 6:
            out_b = auto.step_device()
            assert auto._direct_state is None
            e_auto = float(out_b[0].detach())
            assert abs(e_eager[-1] - e_auto) <= 1e-9 * abs(e_auto), (step, e_eager[-1], e_auto)
            for name in ("vertices", "transform_quaternion", "transform_translation"):
                pa, pb = getattr(eager, name).detach().cpu().numpy(), getattr(auto, name).detach().cpu().numpy()
                assert np.abs(pa - pb).max() <= 1e-9 * np.abs(pb).max(), (step, name)
    f, _ = _holed_depth_fitter()
    g = GraphedStep(f, warmup=3)  # iterations 0 .. 4
    e_graph = [float(g.step_device()[0]) for _ in range(10)]  # iterations 5 .. 14
    assert np.abs(np.array(e_graph) - np.array(e_eager[5:15])).max() <= 1e-6 * e_eager[0]  # (the bound of the existing eager-vs-replay test of the colour fitter)
    # the mask matters: the same holed target without it is another fit
    plain, _ = _holed_depth_fitter()
    plain.set_image(plain.mesh_image.cpu().numpy(), focal=241, distortion=np.load(os.path.join(GOLDEN, "depth_hand_fit.npz"))["distortion"])
    assert abs(float(plain.step_device()[0]) - e_eager[0]) > 1e-3 * e_eager[0]
    # the difference image for display stays un-weighted: non-zero inside the holes
    _e, _depth, diff = eager.step_device()
    assert float(diff[torch.as_tensor(mask == 0, device=diff.device)].max()) > 0


@pytest.mark.parametrize("direct", [True, False])
def test_multi_frame_fit_ignores_a_view_of_weight_zero(direct):
    """three views, the middle one with weight 0 everywhere: the shared parameters move as in the fit of the two other views (same data weight)"""
    from deodr_amd.mesh_fitter import MeshRGBFitterWithPoseMultiFrame

    r = np.load(os.path.join(GOLDEN, "rgb_hand_fit.npz"))
    faces = np.load(HAND)["faces"].astype(np.int64)
    rs = np.random.RandomState(2)
    images = [np.clip(r["image_u8"].astype(np.float64) / 255 + 0.05 * rs.randn(*r["image_u8"].shape), 0, 1) for _ in range(3)]
    H, W = images[0].shape[:2]
    angles = (-0.2, 0.0, 0.2)

    def fitter(keep, weights):
        eul = np.stack([np.array([0, angles[i], 0]) for i in keep])
        f = MeshRGBFitterWithPoseMultiFrame(r["vertices_centered"], faces, eul, np.tile(r["translation_init"], (len(keep), 1)), r["default_color"],
                                            r["default_light_directional"], float(r["default_light_ambient"]), cregu=2000, cdata=len(keep) / 3)  # fmt: skip
        f.set_images([images[i] for i in keep], weights=weights)
        f.set_background_color(r["background_color"])
        f.direct = direct
        return f

    w = np.ones((3, H, W))
    w[1] = 0
    a, b = fitter((0, 1, 2), w), fitter((0, 2), None)  # (cdata / n_views is the data weight: 1 / 3 in both)
    for step in range(4):
        ea, eb = float(a.step_device()[0]), float(b.step_device()[0])
        assert (a._direct_state is not None) == direct
        assert abs(ea - eb) <= 1e-9 * abs(eb), (step, ea, eb)
        for name in ("vertices", "mesh_color", "light_directional", "light_ambient"):
            pa, pb = getattr(a, name).detach().cpu().numpy(), getattr(b, name).detach().cpu().numpy()
            assert np.abs(pa - pb).max() <= 1e-9 * np.abs(pb).max(), (step, name)
        for name in ("transform_quaternion", "transform_translation"):
            pa, pb = getattr(a, name).detach().cpu().numpy()[[0, 2]], getattr(b, name).detach().cpu().numpy()
            assert np.abs(pa - pb).max() <= 1e-9 * np.abs(pb).max(), (step, name)


# ---- the two-call entry keeps its behaviour ------------------------------------------------------------------------------------


@pytest.mark.parametrize("mode", ["six_channels", "force_generic", "deterministic", "staged"])
@pytest.mark.parametrize("residual", [True, False])
def test_render_scene_b_ignores_err_buffer_b_without_antialiase_error(mode, residual):
    """deodr_hip_render_scene_b through the C ABI with a non-NULL err_buffer_b and antialiase_error = 0 (the reference's renderScene_B always
    has that pointer): the buffer is ignored, as before the weights existed -- in particular it is not taken for per-pixel weights by the
    un-staged kernels.  Residual mode (image + obs) and image_b mode; bit-identical in the deterministic mode, to the order of the float64
    atomics (1e-12, tests/test_hip_parity2.py::test_run_to_run_determinism_bound) otherwise."""
    import ctypes as C

    from hip_util import device_scene, rel_err
    from deodr_amd import hip_renderer as hr
    from deodr_amd.hip_renderer import HipRasterizer

    kw = dict(nb_colors=6, depth_channel=False) if mode == "six_channels" else {}
    s = scenes.sphere_scene(size=128, nu=30, n_rings=30, **kw)
    ds = device_scene([s], F64)
    r = HipRasterizer.for_scene(ds)
    rs = np.random.RandomState(3)
    obs = torch.as_tensor(rs.rand(1, 128, 128, ds.nb_colors), device=ds.device)
    image_b = torch.as_tensor(rs.randn(1, 128, 128, ds.nb_colors), device=ds.device)
    junk = torch.as_tensor(5 * rs.rand(1, 128, 128), device=ds.device)  # what a caller may leave in err_buffer_b
    hr.force_generic(mode == "force_generic")
    hr.set_deterministic(mode == "deterministic")
    try:
        image, z = r.render(ds, 1.0, check_overflow=True)
        out = []
        for err_b in (None, junk):
            g = ds.zero_grads()
            sc = ds.c_struct(g)
            hr._check(hr.lib().deodr_hip_render_scene_b(C.byref(sc), hr._ptr(image), None, None if residual else hr._ptr(image_b), 1.0, 0,
                                                        hr._ptr(obs) if residual else None, None, hr._ptr(err_b), hr._ptr(r.workspace), r.nbytes, 0,
                                                        hr._stream(r.device)))  # fmt: skip
            torch.cuda.synchronize()
            out.append({k: v.clone() for k, v in g.items() if v is not None})
    finally:
        hr.force_generic(False)
        hr.set_deterministic(False)
    assert float(out[0]["ij_b"].abs().max()) > 0
    for k, v in out[0].items():
        if mode == "deterministic":
            assert torch.equal(v, out[1][k]), k
        else:
            assert rel_err(out[1][k].cpu().numpy(), v.cpu().numpy()) < 1e-12, k
