"""What the fitter-matrix tests share (tests/test_fitter_matrix_host.py on the CPU, tests/test_fitter_matrix_gpu.py on the device): the table of keyword
combinations of the three pose fitters, the builder that gives every case non-neutral starting values, the lock-step driver, and a restatement of the
composition ``basis -> skin -> minus the mean of the rest vertices -> subdivision -> pose`` and of its adjoint in NumPy (float64 or long double).  No
test functions here.

THE CASES.  fitter x shape keywords x lighting: MeshDepthFitter (the set-up of test_skinning_fit_host.rig_fitter, 64 x 64), MeshRGBFitterWithPose (one
view) and MeshRGBFitterWithPoseMultiFrame (three views) with the set-up of test_lighting_gpu.make_fitter (the hand at 64 x 64, a seeded random target);
shape keywords sub1, basis3, skin, basis3+sub1, basis3+skin; for the colour fitters the directional light, ``light_sh_init`` [9], and ``light_sh_init``
[9,3] with a per-vertex albedo and its smoothness term: 5 + 2 * 5 * 3 = 35 cases with float64 frames, and per class one case with per-pixel weights
and one with float32 frames on its richest combination (basis3+skin, SH + albedo): 41.

LOCK-STEP.  :func:`run` drives ``step_device`` three times and records, per step, every parameter and every momentum speed before it, every entry of
``momentum.update_all`` (name, gradient, second gradient), the posed vertices handed to the scene and the adjoint that comes back to them, the energy
and the image.  With ``follow=`` a recording, the parameters and speeds of that recording are loaded before each step: the two fitters then take their
gradients at EQUAL parameters, nothing is amplified from step to step, and ``step_max`` cannot hide an error behind a clamped step, because the
gradients are compared where they enter the momentum rule.  What lock-step cannot see: the stability of a free-running fit.

THE TOLERANCE OF THE COMPOSITION CHECKS.  The restatement computes, next to every value, the sum of the absolute values of its terms (the scale of
tests/skinning_reference.py, carried through the basis, the centring, S and the pose).  ``python tests/fitter_matrix_cases.py`` runs it in float64
against long double at the starting values of every case and prints the largest ``|float64 - long double| / scale``: MEASURED_CHAIN below.  The
fitters' torch formulas are held to ``skinning_reference.TOLERANCE + MEASURED_CHAIN`` of the scale: the bound of the skin alone, widened by what the
longer chain itself loses in float64."""

import contextlib
from typing import NamedTuple, Optional

import numpy as np
import torch

import fititer_reference as fr
import skinning_reference as sr

LD = np.longdouble
SIZE, STEPS, VIEWS = 64, 3, 3
SHAPES = ("sub1", "basis3", "skin", "basis3+sub1", "basis3+skin")
LIGHTS = ("directional", "sh", "sh3-albedo")
FITTERS = ("depth", "rgb", "multi")
SIGMAS = np.array([1.0, 2.0, 0.5])

# python tests/fitter_matrix_cases.py: "largest float64 error of the restatement relative to the scale" 1.516e-15 (the adjoint to the view quaternion of
# depth-basis3+sub1; the posed vertices 5.03e-16, translation 5.12e-16, vertices 9.08e-16, joint quaternions 2.32e-16, coefficients 4.99e-18)
MEASURED_CHAIN = 1.6e-15
COMPOSITION_BOUND = sr.TOLERANCE + MEASURED_CHAIN


class Case(NamedTuple):
    fitter: str
    shape: str
    light: Optional[str] = None
    weights: bool = False
    pixel_dtype: torch.dtype = torch.float64

    @property
    def name(self):
        parts = [self.fitter, self.shape] + ([self.light] if self.light else [])
        return "-".join(parts + (["weights"] if self.weights else []) + (["f32"] if self.pixel_dtype == torch.float32 else []))

    @property
    def views(self):
        return VIEWS if self.fitter == "multi" else 1

    @property
    def groups(self):
        """-> {name of every entry the case's keywords imply in ``momentum.update_all``: whether it carries a second gradient (a prior)}"""
        g = {"coefficients" if "basis3" in self.shape else "vertices": True, "quaternion": False, "translation": False}
        if "skin" in self.shape:
            g["joint_quaternions"] = True
        if self.light == "directional":
            g.update(light_directional=False, light_ambient=False, mesh_color=False)
        elif self.light is not None:
            g.update(light_sh=False, mesh_color=self.light == "sh3-albedo")
        return g


def _cases():
    table = [Case("depth", s) for s in SHAPES] + [Case(f, s, light) for f in ("rgb", "multi") for s in SHAPES for light in LIGHTS]
    for f in FITTERS:
        richest = Case(f, "basis3+skin", None if f == "depth" else "sh3-albedo")
        table += [richest._replace(weights=True), richest._replace(pixel_dtype=torch.float32)]
    return {c.name: c for c in table}


CASES = _cases()
assert len(CASES) == 41
GRAPHED = [Case(f, s, None if f == "depth" else "sh3-albedo").name for f in FITTERS for s in ("basis3+skin", "basis3+sub1")]
PARAMETERS = ("vertices", "coefficients", "transform_quaternion", "transform_translation", "joint_quaternions", "mesh_color", "light_directional",
              "light_ambient", "light_sh")  # fmt: skip
ATTRIBUTE_OF = {"quaternion": "transform_quaternion", "translation": "transform_translation"}  # (update_all's name -> the fitter's attribute, where they differ)

# the refused combinations: (fitter, shape keywords, further keywords, the message of the ValueError)
REFUSED = [(f, shape, {}, "skin with subdivisions > 0 is not supported") for f in FITTERS for shape in ("skin+sub1", "basis3+skin+sub1")]
REFUSED += [(f, "basis3", dict(vertex_albedo=True), "vertex_albedo needs light_sh_init") for f in ("rgb", "multi")]


# ---- building a case ------------------------------------------------------------------------------------------------------------------------


def joint_start():
    """-> joint_quaternions_init away from identity, as tests/test_skinning_fit_host.py::test_skin_with_a_shape_basis_and_a_joint_prior has it"""
    q = sr.hand_target_quaternions().copy()
    q[1] = sr.axis_quaternion(1, 0.2)
    return q


def shape_keywords(shape, device, with_rig=True):
    from test_basis import hand_modes

    kw = {}
    if "sub1" in shape:
        kw["subdivisions"] = 1
    if "basis3" in shape:
        kw.update(shape_basis=hand_modes(3), coefficient_regu=1.0, sigmas=SIGMAS)
    if "skin" in shape:
        kw.update(joint_quaternions_init=joint_start(), joint_regu=5.0)
        if with_rig:
            from deodr_amd.skinning import Skin

            _v, _faces, joints, parents, w = sr.hand_rig(measured_from="far")
            kw["skin"] = Skin(joints, parents, w, device=device)
    return kw


def pixel_weights(n):
    """a mask [n,H,W] with zeros (a block and scattered pixels) and fractional values"""
    rs = np.random.RandomState(77)
    w = 0.25 + 0.75 * rs.rand(n, SIZE, SIZE)
    w[rs.rand(n, SIZE, SIZE) < 0.2] = 0.0
    w[:, 20:30, 24:40] = 0.0
    return w


_depth_targets = {}


def _depth_target(f, focal, key, articulated):
    """the depth image of the fitter's own model at a moved pose (and at the articulated pose of the skin tests): made once, on the CPU reference
    (inside :func:`reference_raster`), and given to the fitter under test as it is"""
    if key not in _depth_targets:
        assert f.device.type == "cpu", "build the reference fitter of a depth case first"
        f.set_image(np.ones((SIZE, SIZE)), focal=focal)
        if articulated:
            f.joint_quaternions = torch.as_tensor(sr.hand_target_quaternions())
        f.transform_translation = f.transform_translation + torch.as_tensor(np.array([[0.06, -0.05, 0.03]]) * f.object_radius)
        f._leaves()
        with torch.no_grad():
            _depth_targets[key] = f.energy()[3].detach().numpy().copy()
        f.reset()
    return _depth_targets[key]


def set_start(f, case):
    """seeded starting values away from the neutral ones, so that no term of the energy is zero by accident: coefficients off zero (with the prior on
    unequal sigmas), joint quaternions off ``joint_quaternions_init`` (with ``joint_regu``), vertices off ``vertices_ref``, a per-vertex albedo that is
    not constant (the smoothness term has a gradient)"""
    rs = np.random.RandomState(2026 + list(CASES).index(case.name))
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=f.device)
    scale = float(f.vertices_init.abs().max())
    if f.shape_basis is not None:
        f.coefficients = t(0.05 * scale * rs.randn(f.shape_basis.K))
    else:
        f.vertices = f.vertices + t(0.002 * scale * rs.randn(*f.vertices.shape))
    if f.skin is not None:
        q = f.joint_quaternions_init.cpu().numpy() + 0.05 * rs.randn(f.skin.J, 4)
        f.joint_quaternions = t(q / np.linalg.norm(q, axis=1, keepdims=True))
    if case.light == "sh3-albedo":
        f.mesh_color = f.mesh_color + t(0.05 * rs.randn(*f.mesh_color.shape))
    return f


# The joint step of a FREE-RUNNING fit (the graph test; the lock-step and host cases keep the class default).  The default 3e-4 is sized for a depth fit
# whose first energy is 3.4 and "scales with the inverse of the energy" (mesh_fitter.py).  The depth fits of this rig start near 100 and take the 1e-4
# tests/test_skinning_fit_host.py gives the same rig.  The colour fits start near 1400: with 3e-4 they overshoot, and a free-running fit multiplies the
# rounding noise of the rasterizer's atomics by about 30 per step -- two EAGER twins on the device part by 0.6 in their twelfth energy, exactly as a
# replay and eager steps do; with 1e-4 the noise still grows (3e-10 after twelve steps), with 3e-5, 1e-5 and 1e-6 it stays at 2e-12 (measured on the
# MI355X).  1e-5: the joint quaternions then move by 2e-3 over the seven compared steps, 2000 times the bound of the comparison.
FREE_RUNNING_JOINT_STEP = {"depth": 1e-4, "rgb": 1e-5, "multi": 1e-5}


def build_free_running(case, device):
    f = build(case, device)
    if f.skin is not None:
        f.step_factor_joints = FREE_RUNNING_JOINT_STEP[case.fitter]
    return f


def build(case, device, neutral=None):
    """-> the fitter of ``case`` on ``device`` at its starting values (a depth case: the CPU one first, it renders the target).  ``neutral``: "keyword":
    the case's shape keywords at their neutral values (identity joint quaternions, no priors, coefficients zero) and the vertices at the reference
    shape; "plain": the same fitter without the shape keywords -- the pair the neutral-values tests compare"""
    kw = dict(pixel_dtype=case.pixel_dtype)
    shape = "" if neutral == "plain" else case.shape
    if case.fitter == "depth":
        from test_skinning_fit_host import rig_fitter

        kw.update(shape_keywords(shape, device, with_rig=False))
        skin = "skin" in shape
    else:
        kw.update(shape_keywords(shape, device))
    if neutral:
        kw.update({k: 0.0 for k in ("joint_regu", "coefficient_regu") if k in kw}, **({"joint_quaternions_init": None} if "skin" in shape else {}))
    if case.fitter == "depth":
        f, _rig, focal = rig_fitter(skin="rig" if skin else "omit", device=device, measured_from="far", **kw)
        target = _depth_target(f, focal, case.name + ("-neutral" if neutral else ""), skin and not neutral)
        f.set_image(target, focal=focal, weights=pixel_weights(1)[0] if case.weights else None)
    else:
        from test_lighting_gpu import MODES, make_fitter

        f = make_fitter(case.views, True, device=device, **kw, **MODES.get(case.light, {}))
        if case.weights:
            images, w = f.mesh_image.cpu().numpy(), pixel_weights(case.views)
            f.set_image(images[0], weights=w[0]) if case.fitter == "rgb" else f.set_images(list(images), weights=w)
    return f if neutral else set_start(f, case)


@contextlib.contextmanager
def reference_raster(oracle_api):
    """tests/cpu_raster.py::emulate, with a fit step that knows per-pixel weights (``sum(weights[..., None] * (image - obs)**2)``)"""
    import cpu_raster
    from deodr_amd.scene3d import Scene3DDevice

    with cpu_raster.emulate(oracle_api.ref() or oracle_api.port()):
        plain = Scene3DDevice._rasterize_l2

        def _rasterize_l2(self, camera, ij, depths, colors, shade, textured, backface_culling, obs, weights=None):
            if weights is None:
                return plain(self, camera, ij, depths, colors, shade, textured, backface_culling, obs)
            image, _z = self._rasterize(camera, ij, depths, colors, shade, textured, backface_culling)
            residual = (image.to(torch.float64) - obs.to(torch.float64)) ** 2
            return (weights.to(torch.float64)[..., None] * residual).sum(), image.detach()

        Scene3DDevice._rasterize_l2 = _rasterize_l2
        try:
            yield
        finally:
            Scene3DDevice._rasterize_l2 = plain


# ---- the lock-step driver -------------------------------------------------------------------------------------------------------------------


def host(t):
    return t.detach().to(torch.float64).cpu().numpy().copy()


def snapshot(f):
    """-> ({attribute: array} of every parameter tensor the fitter has, {name: array} of the whole ``momentum.speed``)"""
    params = {k: host(getattr(f, k)) for k in PARAMETERS if torch.is_tensor(getattr(f, k, None))}
    return params, {k: host(v) for k, v in f.momentum.speed.items()}


def load(f, params, speed):
    t = lambda a: torch.as_tensor(np.array(a), device=f.device)
    for k, a in params.items():
        setattr(f, k, t(a))
    f.momentum.speed = {k: t(a) for k, a in speed.items()}


def step_recorded(f):
    """one ``step_device`` -> dict(params, speed: before the step; entries {name: (gradient, second gradient | None)} as ``momentum.update_all`` got
    them; posed [n,V,3]: what ``_transformed`` handed to the scene, posed_b: the adjoint that came back to it; energy; image)"""
    row = {}
    row["params"], row["speed"] = snapshot(f)
    update_all, transformed = f.momentum.update_all, f._transformed

    def spy_update(entries):
        assert "entries" not in row, "momentum.update_all was called twice in one step"
        row["entries"] = {e[0]: (host(e[2]), None if e[3] is None else host(e[3])) for e in entries}
        row["shapes"] = {e[0]: (tuple(e[1].shape), tuple(e[2].shape)) for e in entries}
        return update_all(entries)

    def spy_transformed(vertices):
        posed = transformed(vertices)
        row["posed"] = host(posed)
        if posed.requires_grad:
            posed.register_hook(lambda g: row.__setitem__("posed_b", host(g)))
        return posed

    f.momentum.update_all, f._transformed = spy_update, spy_transformed
    try:
        out = f.step_device()
    finally:
        f.momentum.update_all = update_all
        del f._transformed  # (the instance attribute: the method of the class shows again)
    row["energy"], row["image"] = float(out[0].detach()), host(out[1])
    return row


def run(f, follow=None, steps=STEPS):
    """``steps`` recorded steps; ``follow``: a recording whose parameters and speeds are loaded before each step (lock-step)"""
    rows = []
    for k in range(steps):
        if follow is not None:
            load(f, follow[k]["params"], follow[k]["speed"])
        rows.append(step_recorded(f))
    return rows


def reference_recording(case, oracle_api):
    """-> (the CPU fitter after its three steps, its recording)"""
    with reference_raster(oracle_api):
        f = build(case, "cpu")
        assert f._direct_iteration(1, False) is None
        return f, run(f)


def weighted_residual_norm(case, f, image):
    """-> (|r|, data weight, largest weight): r the weighted residual ``sqrt(w) (image - target)`` of the reference's image, the factor the data term
    enters the energy with, and max w -- what the float32 energy bound of the GPU test is made of"""
    depth = case.fitter == "depth"  # (its image is [H,W], already clipped, and its target stays float64; the colour fitters compare in the pixel dtype)
    target = f.mesh_image.cpu().numpy() if depth else f._observation().to(torch.float64).cpu().numpy()
    r2 = (image - target) ** 2 if depth else ((image - target) ** 2).sum(axis=-1)
    w = np.ones(r2.shape) if f.weights is None else f.weights.cpu().numpy().reshape(r2.shape)
    return float(np.sqrt((w * r2).sum())), (1.0 if depth else float(f.data_weight)), float(w.max())


# ---- the composition, restated from the docstring of the fitters ----------------------------------------------------------------------------


def _spmv(matrix, x):
    coo = matrix.tocoo()
    out = np.zeros((matrix.shape[0],) + x.shape[1:], dtype=x.dtype)
    np.add.at(out, coo.row, coo.data.astype(x.dtype)[:, None] * x[coo.col])
    return out


def _abs_cross(a, b):
    """the sum of the absolute values of the terms of a x b, for arrays of magnitudes"""
    a, b = np.broadcast_arrays(a, b)
    return np.stack((a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]), axis=-1)


def restate(f, params, posed_b=None, dtype=LD):
    """``X = S (skin(mean + c . B, q_joints) - mean of the rest vertices)``, then ``qrot(q_view / |q_view|, X) + t_view`` -- and, for the adjoint
    ``posed_b`` [n,V,3] of the posed vertices, the data gradients of the parameters: the pose adjoint summed over the views, S^T, the skin's adjoint,
    the projection on zero-mean displacements that the subtracted mean amounts to, and the contraction with the basis (of the vertex gradient PLUS the
    rigid gradient, as the coefficients' first gradient is defined).  Every value comes with the sum of the absolute values of its terms.
    -> {name: (value, scale)} for posed, and with ``posed_b``: vertices | coefficients, quaternion, translation, joint_quaternions"""
    A = lambda a: np.asarray(a, dtype=dtype)
    mean = A(f.vertices_init.cpu().numpy())
    V = mean.shape[0]
    if f.shape_basis is not None:
        B = A(f.shape_basis.components.cpu().numpy().reshape(f.shape_basis.K, V, 3))
        c = A(params["coefficients"])
        delta, m_delta = np.tensordot(c, B, axes=1), np.tensordot(np.abs(c), np.abs(B), axes=1)
        rest, m_rest = mean + delta, np.abs(mean) + m_delta
    else:
        rest = A(params["vertices"])
        m_rest = np.abs(rest)
    skinned, m_skinned = rest, m_rest
    if f.skin is not None:
        s = f.skin
        rig = dict(vertices=rest, quaternions=A(params["joint_quaternions"])[None], joints=s.joints_np, indices=s.indices_np.astype(np.uint32),
                   parents=np.where(s.parents_np < 0, sr.ROOT_MARKER, s.parents_np).astype(np.uint32), weights=s.weights_np)  # fmt: skip
        fwd = sr.forward(rig, dtype)
        skinned, m_skinned = fwd["posed"].v[0], fwd["posed"].m[0]
    centred, m_centred = skinned - rest.mean(axis=0), m_skinned + m_rest.mean(axis=0)
    fine, m_fine = centred, m_centred
    if f.subdivisions:
        S = f.subdivision.matrix
        fine, m_fine = _spmv(S, centred), _spmv(abs(S), m_centred)
    q, t = A(params["transform_quaternion"]), A(params["transform_translation"])
    pose = fr.pose(fine, q, t, dtype=dtype)
    u, w = np.abs(pose["unit"][:, None, :3]), np.abs(pose["unit"][:, None, 3:])
    m_posed = m_fine[None] + 2 * (w * _abs_cross(u, m_fine[None]) + _abs_cross(u, _abs_cross(u, m_fine[None]))) + np.abs(t)[:, None, :]
    out = {"posed": (pose["posed"], m_posed)}
    if posed_b is None:
        return out
    g = A(posed_b)
    back = fr.pose_b(fine, q, g, dtype=dtype)
    out["quaternion"], out["translation"] = back["q_b"], back["t_b"]
    ag = np.abs(g)
    agu = _abs_cross(ag, u)
    fine_b, m_fine_b = back["vertices_b"], (ag + 2 * w * agu + 2 * _abs_cross(agu, u)).sum(axis=0)
    centred_b, m_centred_b = fine_b, m_fine_b
    if f.subdivisions:
        centred_b, m_centred_b = _spmv(S.T, fine_b), _spmv(abs(S.T), m_fine_b)
    column, m_column = centred_b.sum(axis=0) / dtype(V), m_centred_b.sum(axis=0) / dtype(V)  # (the mean of the REST vertices was subtracted)
    if f.skin is not None:
        adj = sr.adjoint(rig, centred_b[None], dtype, fwd)
        rest_b, m_rest_b = adj["vertices_b"].v - column, adj["vertices_b"].m + m_column
        out["joint_quaternions"] = (adj["quaternions_b"].v[0], adj["quaternions_b"].m[0])
    else:
        rest_b, m_rest_b = centred_b - column, m_centred_b + m_column
    if f.shape_basis is None:
        out["vertices"] = (rest_b, m_rest_b)
    else:  # the first gradient of the coefficients: the basis adjoint of the data gradient plus the rigid gradient cregu (L^T L) (rest - mean)
        topo = f.rigid_energy.topology
        rows, cols, vals = (x.cpu().numpy() for x in (topo._m_rows, topo._m_cols, topo._m_vals))
        rigid, m_rigid = np.zeros_like(delta), np.zeros_like(delta)
        np.add.at(rigid, rows, A(vals)[:, None] * delta[cols])
        np.add.at(m_rigid, rows, np.abs(A(vals))[:, None] * m_delta[cols])
        cregu = dtype(f.cregu)
        out["coefficients"] = (np.tensordot(B, rest_b + cregu * rigid, axes=([1, 2], [0, 1])), np.tensordot(np.abs(B), m_rest_b + cregu * m_rigid, axes=([1, 2], [0, 1])))
    return out


def relative_to_scale(got, pair):
    """largest |got - value| / scale over the elements of one output"""
    value, scale = pair
    err = np.abs(np.asarray(got).astype(LD).reshape(value.shape) - value)
    zero = scale == 0  # (a vertex no pixel's gradient reaches: no terms, and the value must be exactly zero)
    assert np.all(err[zero] == 0)
    return float((err[~zero] / scale[~zero]).max())


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import api

    assert fr.longdouble_is_extended(), "np.longdouble is not wider than float64 here: no reference"
    worst = {}
    for name, case in CASES.items():
        f, rows = reference_recording(case, api)
        row = rows[0]
        f64, ld = restate(f, row["params"], row["posed_b"], np.float64), restate(f, row["params"], row["posed_b"], LD)
        errors = {k: relative_to_scale(f64[k][0], ld[k]) for k in ld}
        print(f"{name:40s} " + "  ".join(f"{k} {e:.2e}" for k, e in errors.items()))
        for k, e in errors.items():
            worst[k] = max(worst.get(k, 0.0), e)
    print("per output: " + "  ".join(f"{k} {e:.2e}" for k, e in worst.items()))
    print(f"largest float64 error of the restatement relative to the scale: {max(worst.values()):.3e}")
