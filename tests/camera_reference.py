"""NumPy restatement, in float64 and in long double, of what include/deodr_hip_camera.h computes: the full adjoint of the camera projection (the
points' adjoint is tests/fititer_reference.project_b; here are the 12 + 6 + 5 sums over the vertices that are the adjoints of a view's extrinsic,
intrinsic and distortion), the map from calibration parameters to the per-view matrices and its adjoint -- and the case tables that
tests/test_camera_reference.py (CPU: pins this module, measures the float64 error) and tests/test_camera_gpu.py (the kernels) share.

Sums come as pairs (sum, sum of |term|): the second is the scale their errors are measured in (fititer_reference.sum_distance)."""

import functools
import os
import re

import numpy as np

import fititer_reference as fr
from fititer_reference import LD

F64 = np.float64


def kernel_constants():
    """``constexpr int NAME = value`` of deodr_amd/csrc/dr_camera.h (and FH_BLOCK, FIT_MAX_VIEWS of the headers before it)"""
    found = dict(fr.kernel_constants())
    with open(os.path.join(fr.CSRC, "dr_camera.h")) as f:
        found.update({k: int(v) for k, v in re.findall(r"constexpr\s+int\s+(\w+)\s*=\s*([0-9]+)\s*;", f.read())})
        f.seek(0)
        found.update({k: int(a) << int(b) for k, a, b in re.findall(r"constexpr\s+int\s+(\w+)\s*=\s*([0-9]+)\s*<<\s*([0-9]+)\s*;", f.read())})
    missing = [k for k in ("CAMERA_MAX_BLOCKS", "CAMERA_SUMS", "CAMERA_MAX_VERTICES") if k not in found]
    assert not missing, f"constants not found in dr_camera.h: {missing}"
    return found


# ---- the projection's full adjoint ---------------------------------------------------------------------------------------------------


def project_full_b(points, extrinsic, intrinsic, distortion, ij_b, depths_b=None, dtype=LD):
    """-> dict: points_b [n,V,3]; extrinsic_b, intrinsic_b (rows 0 and 1: [n,2,3]), distortion_b ([n,5] | None) as (sum, sum |term|) over the vertices.
    Every adjoint is the derivative of  sum ij_b . ij + sum depths_b . depth  written out per vertex."""
    p = np.asarray(points, dtype=dtype)
    (cx, cy, cz), _E = fr._camera_space(points, extrinsic, dtype)
    K, g = np.asarray(intrinsic, dtype=dtype), np.asarray(ij_b, dtype=dtype)
    x, y = cx / cz, cy / cz
    xd_b = K[:, None, 0, 0] * g[..., 0] + K[:, None, 1, 0] * g[..., 1]
    yd_b = K[:, None, 0, 1] * g[..., 0] + K[:, None, 1, 1] * g[..., 1]
    x_b, y_b, xd, yd, d_b = xd_b, yd_b, x, y, None
    if distortion is not None:
        k1, k2, p1, p2, k3 = (np.asarray(distortion, dtype=dtype)[:, i, None] for i in range(5))
        r2 = x * x + y * y
        radial = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
        slope = k1 + 2 * k2 * r2 + 3 * k3 * r2 * r2
        xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x_b = xd_b * (radial + 2 * x * x * slope + 2 * p1 * y + 6 * p2 * x) + yd_b * (2 * x * y * slope + 2 * p1 * x + 2 * p2 * y)
        y_b = xd_b * (2 * x * y * slope + 2 * p1 * x + 2 * p2 * y) + yd_b * (radial + 2 * y * y * slope + 6 * p1 * y + 2 * p2 * x)
        radial_b = x * xd_b + y * yd_b  # d / d radial, then radial's derivatives by k1, k2, k3: r2, r2^2, r2^3
        per_vertex = np.stack((radial_b * r2, radial_b * r2 * r2, 2 * x * y * xd_b + (r2 + 2 * y * y) * yd_b, (r2 + 2 * x * x) * xd_b + 2 * x * y * yd_b,
                               radial_b * r2 * r2 * r2), axis=-1)  # fmt: skip
        d_b = fr.sums(per_vertex, axis=1)
    c_b = [x_b / cz, y_b / cz, -(x * x_b + y * y_b) / cz]
    if depths_b is not None:
        c_b[2] = c_b[2] + np.asarray(depths_b, dtype=dtype)
    one = np.ones_like(cx)
    e_terms = np.stack([np.stack((c * p[..., 0], c * p[..., 1], c * p[..., 2], c), axis=-1) for c in c_b], axis=-2)  # [n,V,3,4]
    k_terms = np.stack([np.stack((g[..., r] * xd, g[..., r] * yd, g[..., r] * one), axis=-1) for r in range(2)], axis=-2)  # [n,V,2,3]
    return {"points_b": fr.project_b(points, extrinsic, intrinsic, distortion, ij_b, depths_b, dtype), "extrinsic_b": fr.sums(e_terms, axis=1),
            "intrinsic_b": fr.sums(k_terms, axis=1), "distortion_b": d_b}  # fmt: skip


# ---- calibration parameters <-> per-view matrices ------------------------------------------------------------------------------------


def _per_view(a, n, shared, dtype):
    a = np.asarray(a, dtype=dtype)
    return np.broadcast_to(a[None], (n,) + a.shape) if shared else a


def rotation(unit):
    """unit quaternions [n,4] = (x, y, z, w) -> R [n,3,3] with R p = qrot(q, p) = p + 2 (w u x p + u x (u x p))"""
    x, y, z, w = (unit[:, i] for i in range(4))
    return np.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), axis=-1).reshape(-1, 3, 3)  # fmt: skip


def assemble(quaternions, translations, focal, center, distortion, shared, dtype=LD):
    """-> extrinsic [n,3,4] = [R(q / |q|) | t], intrinsic [n,3,3], distortion [n,5] | None"""
    q, t = np.asarray(quaternions, dtype=dtype), np.asarray(translations, dtype=dtype)
    n = q.shape[0]
    unit = q / np.sqrt((q * q).sum(axis=-1))[:, None]
    E = np.concatenate((rotation(unit), t[:, :, None]), axis=2)
    f, c = _per_view(focal, n, shared, dtype), _per_view(center, n, shared, dtype)
    K = np.zeros((n, 3, 3), dtype=dtype)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = f[:, 0], f[:, 1], c[:, 0], c[:, 1], 1
    return E, K, (None if distortion is None else np.array(_per_view(distortion, n, shared, dtype)))


def assemble_b(quaternions, extrinsic_b, intrinsic_b, distortion_b, shared, dtype=LD):
    """adjoint of :func:`assemble` -> dict: quaternions_b [n,4] (raw quaternions), translations_b [n,3]; focal_b, center_b, distortion_b as (sum,
    sum |term|) over the views when shared ([2], [2], [5]), else the entries themselves ([n,2], [n,2], [n,5]) with their magnitudes.
    The derivative of R by each component of the unit quaternion is written out as a matrix and contracted with the adjoint of R."""
    q, Eb, Kb = (np.asarray(a, dtype=dtype) for a in (quaternions, extrinsic_b, intrinsic_b))
    norm = np.sqrt((q * q).sum(axis=-1))
    unit = q / norm[:, None]
    x, y, z, w = (unit[:, i] for i in range(4))
    o = np.zeros_like(x)
    dR = [np.stack((o, 2 * y, 2 * z, 2 * y, -4 * x, -2 * w, 2 * z, 2 * w, -4 * x), axis=-1),  # d R / d x
          np.stack((-4 * y, 2 * x, 2 * w, 2 * x, o, 2 * z, -2 * w, 2 * z, -4 * y), axis=-1),  # d R / d y
          np.stack((-4 * z, -2 * w, 2 * x, 2 * w, -4 * z, 2 * y, 2 * x, 2 * y, o), axis=-1),  # d R / d z
          np.stack((o, -2 * z, 2 * y, 2 * z, o, -2 * x, -2 * y, 2 * x, o), axis=-1)]  # d R / d w  # fmt: skip
    Rb = Eb[:, :, :3].reshape(-1, 9)
    unit_b = np.stack([(d * Rb).sum(axis=-1) for d in dR], axis=-1)
    q_b = (unit_b - unit * (unit * unit_b).sum(axis=-1)[:, None]) / norm[:, None]
    f_terms, c_terms = np.stack((Kb[:, 0, 0], Kb[:, 1, 1]), axis=-1), np.stack((Kb[:, 0, 2], Kb[:, 1, 2]), axis=-1)
    pair = (lambda a: fr.sums(a, axis=0)) if shared else (lambda a: (a, np.abs(a)))
    return {"quaternions_b": q_b, "translations_b": Eb[:, :, 3], "focal_b": pair(f_terms), "center_b": pair(c_terms),
            "distortion_b": None if distortion_b is None else pair(np.asarray(distortion_b, dtype=dtype))}  # fmt: skip


# ---- the case tables -----------------------------------------------------------------------------------------------------------------

SMALL_V = (1, 63, 64, 65, 255, 256, 257)
VIEWS = (1, 2, 9, 64)
# every option both ways
OPTIONS = {
    "dist-depth-points": dict(distortion=True, depths_b=True, points_b=True, accumulate=False),
    "plain": dict(distortion=False, depths_b=False, points_b=False, accumulate=False),
    "dist-acc": dict(distortion=True, depths_b=False, points_b=False, accumulate=True),
    "depth-points-acc": dict(distortion=False, depths_b=True, points_b=True, accumulate=True),
}
ASSEMBLE_CASES = [(n, shared, distortion) for n in (1, 2, 64) for shared in (True, False) for distortion in (True, False)]
SMALL_SHAPES = [(1, 2), (33, 9), (257, 1)]  # where the restatements are compared with the torch formulas


def first_v(blocks_of, n, wanted, top=1 << 24):
    """the smallest V at which ``blocks_of(V, n) >= wanted`` (the rule is non-decreasing in V: bisection)"""
    lo, hi = 1, top
    assert blocks_of(hi, n) >= wanted
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if blocks_of(mid, n) >= wanted else (mid + 1, hi)
    return lo


SMALL_CASES = [(V, VIEWS[i % len(VIEWS)]) for i, V in enumerate(SMALL_V)] + [(1, 64), (257, 2)]
# the names of the cases (what a parametrised test lists when it is collected); project_cases() gives their shapes when it runs
CASE_NAMES = [f"small-{V}x{n}" for V, n in SMALL_CASES] + ["second-1", "second", "second+1", "cap-1", "cap", "cap+1", "cap64", "trip-n1", "trip-n9"]


def project_cases(blocks_of, constants=None):
    """{name: (V, n, why)}: the shapes at which the launch geometry of camera_project_b_kernel changes -- asked of ``blocks_of`` =
    deodr_hip_camera_blocks and of the header's constants, never written down"""
    k = constants or kernel_constants()
    cases = {f"small-{V}x{n}": (V, n, "small") for V, n in SMALL_CASES}
    second = first_v(blocks_of, 2, 2)  # a view's second workgroup
    cases.update({"second-1": (second - 1, 2, "one workgroup"), "second": (second, 2, "second workgroup"), "second+1": (second + 1, 9, "second workgroup")})
    top = blocks_of(1 << 24, 1)
    assert top == k["CAMERA_MAX_BLOCKS"], "one view of the largest mesh is cut into the cap"
    cap = first_v(blocks_of, 1, top)
    cases.update({"cap-1": (cap - 1, 1, "below the cap"), "cap": (cap, 1, "cap"), "cap+1": (cap + 1, 1, "cap")})
    top64 = blocks_of(1 << 24, 64)  # 64 views fill the chip with fewer workgroups each
    cases["cap64"] = (first_v(blocks_of, 64, top64), 64, "cap of 64 views")
    # a thread's further strided trips in a launch of several workgroups: the first V of a view's third workgroup (more vertices than twice the
    # launch's threads)
    for n in (1, 9):
        cases[f"trip-n{n}"] = (first_v(blocks_of, n, 3), n, "several trips")
    assert list(cases) == CASE_NAMES
    return cases


@functools.lru_cache(maxsize=4)
def project_inputs(V, n):
    """seeded float64 inputs: the posed cloud of fititer_reference.point_inputs as the points, its cameras, and what accumulate adds to"""
    d = dict(fr.point_inputs(V, n))
    d["points"] = np.ascontiguousarray(fr.pose(d["vertices"], d["quaternions"], d["translations"], dtype=F64)["posed"])
    rs = np.random.RandomState(77 * n + V)
    d["extrinsic_b0"], d["intrinsic_b0"], d["distortion_b0"] = rs.randn(n, 3, 4) * 10, rs.randn(n, 3, 3) * 10, rs.randn(n, 5)
    return d


def project_reference(V, n, options, dtype=LD, inputs=None):
    """what one call of deodr_hip_camera_project_b leaves for an entry of OPTIONS -> dict (sums as pairs; with accumulate what the outputs held before
    is one more term of each sum)"""
    d = inputs or project_inputs(V, n)
    dist = d["distortion"] if options["distortion"] else None
    out = project_full_b(d["points"], d["extrinsic"], d["intrinsic"], dist, d["ij_b"], d["depths_b"] if options["depths_b"] else None, dtype)
    out["depths"] = fr.project(d["points"], d["extrinsic"], d["intrinsic"], dist, dtype)[1]
    if options["accumulate"]:
        for key, before in (("extrinsic_b", d["extrinsic_b0"]), ("intrinsic_b", d["intrinsic_b0"][:, :2]), ("distortion_b", d["distortion_b0"])):
            if out[key] is not None:
                b = np.asarray(before, dtype=dtype)
                out[key] = (out[key][0] + b, out[key][1] + np.abs(b))
    return out


def assemble_inputs(n):
    rs = np.random.RandomState(4242 + n)
    return {
        "quaternions": rs.randn(n, 4) * 0.4 + np.array([0.1, -0.2, 0.05, 1.0]), "translations": rs.randn(n, 3) + np.array([0, 0, 8.0]),
        "focal": 300 + 20 * rs.rand(n, 2), "center": np.array([64.0, 48.0]) + rs.randn(n, 2), "distortion": rs.randn(n, 5) * 0.05,
        "extrinsic_b": rs.randn(n, 3, 4), "intrinsic_b": rs.randn(n, 3, 3), "distortion_b": rs.randn(n, 5),
    }  # fmt: skip


def assemble_arguments(d, shared, distortion):
    """the parameters of a case: row 0 of the per-view inputs when one physical camera is shared"""
    pick = (lambda a: a[0]) if shared else (lambda a: a)
    return d["quaternions"], d["translations"], pick(d["focal"]), pick(d["center"]), (pick(d["distortion"]) if distortion else None)


# ---- the calibration problem the fitter tests share ----------------------------------------------------------------------------------

FIT_COLOR, FIT_LIGHT, FIT_AMBIENT, FIT_BACKGROUND = (0.8, 0.6, 0.5), (-0.3, -0.4, -0.6), 0.4, (0.1, 0.2, 0.3)
FIT_GROUPS = {"quaternions": "extrinsic", "translations": "extrinsic", "focal": "focal", "center": "center", "distortion": "distortion"}


def calibration_problem(n_views, size, update, arc=2 * np.pi):
    """the hand mesh seen by ``n_views`` cameras (deodr_amd.scenes.calibration_scene) -> dict: vertices, faces, colors, truth, start; a group that is
    not in ``update`` starts at the truth (it is not to move at all)"""
    from deodr_amd import scenes

    vertices, faces = scenes.load_hand_mesh(os.path.join(fr.HERE, "golden", "hand_mesh.npz"))
    s = scenes.calibration_scene(vertices, n_views, size, arc=arc)
    for key, group in FIT_GROUPS.items():
        if group not in update:
            s["start"][key] = s["truth"][key].copy()
    return dict(s, vertices=vertices, faces=faces.astype(np.int64), colors=np.tile(FIT_COLOR, (len(vertices), 1)))


def planar_texture(problem, size=16):
    """-> the keywords of a textured mesh instead of per-vertex colours: uv = the vertices' (x, y) stretched over a smooth ``size`` x ``size`` x 3 texture"""
    from deodr_amd import scenes

    xy = problem["vertices"][:, :2]
    uv = (xy - xy.min(axis=0)) / (xy.max(axis=0) - xy.min(axis=0)) * (size - 1)
    return dict(uv=uv, faces_uv=problem["faces"], texture=scenes.smooth_texture(size, size, 3, seed=3, passes=2))


def make_camera_fitter(problem, parameters, update, device, textured=False, **keywords):
    from deodr_amd.mesh_fitter import CameraFitterMultiFrame

    p = parameters
    keywords.update(planar_texture(problem) if textured else dict(colors=problem["colors"]))
    fitter = CameraFitterMultiFrame(problem["vertices"], problem["faces"], p["quaternions"], p["translations"], p["focal"], p["center"], p["distortion"],
                                    light_directional=np.array(FIT_LIGHT), light_ambient=FIT_AMBIENT, update=update, device=device,
                                    **keywords)  # fmt: skip
    fitter.set_background_color(np.array(FIT_BACKGROUND))
    return fitter


def photographs(problem, device, textured=False):
    """the images of the ground-truth cameras [n,H,W,3] (NumPy), through the fitter's own renderer"""
    truth = make_camera_fitter(problem, problem["truth"], (), device, textured=textured)
    truth.set_images(np.zeros((len(problem["truth"]["quaternions"]), problem["height"], problem["width"], 3)))
    return truth.gradients()[1].to("cpu").double().numpy()


def group_errors(fitter, problem):
    """distance of the fitter's parameters from the truth, per group: for the extrinsics the largest, over the views, mean distance between the mesh
    vertices in the camera frames of the estimate and of the truth (a rotation and a translation that compensate each other are not an error twice);
    the largest absolute difference for focal, centre and distortion"""
    from scipy.spatial.transform import Rotation

    v, truth = problem["vertices"], problem["truth"]
    frame = lambda q, t: np.einsum("nij,vj->nvi", Rotation.from_quat(np.asarray(q)).as_matrix(), v) + np.asarray(t)[:, None, :]
    get = lambda k: getattr(fitter, k).detach().cpu().numpy()
    out = {"extrinsic": float(np.linalg.norm(frame(get("quaternions"), get("translations")) - frame(truth["quaternions"], truth["translations"]), axis=-1).mean(axis=1).max())}
    out.update({k: float(np.abs(get(k) - truth[k]).max()) for k in ("focal", "center", "distortion")})
    return out
