"""A plain NumPy restatement of the vertex-side operations of a fit iteration (deodr_amd/csrc/dr_fronthalf.h, dr_fititer.h): no torch, no
device.  Every function takes ``dtype`` -- ``np.longdouble`` (the reference the GPU tests compare with) or ``np.float64`` (what
tests/test_fititer_reference.py measures against the former, to learn how far float64 arithmetic of the same formulas lies from them).

Every quantity the kernels obtain as a SUM OVER VERTICES -- pose_b, the column mean of vertices_b, light_b, ambient_b, color_b, the rigid
energy, mean_out of the momentum update, the frame sums -- comes back as a pair ``(sum, sum of |term|)`` over the same terms: the error of
a floating-point sum is a multiple of eps * sum |term| whatever its order of additions, so that is the scale its tolerance is stated in.
Elementwise outputs are compared on the scale eps * max |reference|.

The second half of the module holds the seeded inputs and the case tables that tests/test_fititer_reference.py (CPU) and
tests/test_fititer_shapes_gpu.py share, and the launch-geometry constants read from the kernel headers."""

import os
import re

import numpy as np

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "deodr_amd", "csrc")


def longdouble_is_extended():
    """80-bit (or wider) long doubles: what makes this module a reference for float64 kernels"""
    return bool(np.finfo(LD).eps < 2e-19)


def sums(terms, axis=None):
    """(sum, sum of |term|) over ``axis``"""
    return terms.sum(axis=axis), np.abs(terms).sum(axis=axis)


def cross(a, b):
    a, b = np.broadcast_arrays(a, b)
    return np.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), axis=-1)  # fmt: skip


def dot(a, b):
    return (a * b).sum(axis=-1)


# ---- pose: qrot(q / |q|, v - mean) + t ----------------------------------------------------------------------------------------------


def pose(vertices, quaternions, translations, mean=None, normalise=True, dtype=LD):
    """vertices [V,3], raw quaternions [n,4] = (x, y, z, w), translations [n,3] -> dict: centred [V,3], posed [n,V,3], unit [n,4], norm [n]"""
    v, q, t = (np.asarray(a, dtype=dtype) for a in (vertices, quaternions, translations))
    c = v if mean is None else v - np.asarray(mean, dtype=dtype)
    norm = np.sqrt((q * q).sum(axis=-1)) if normalise else np.ones(q.shape[0], dtype=dtype)
    unit = q / norm[:, None]
    u, w = unit[:, None, :3], unit[:, None, 3:]
    a = cross(u, c[None])
    posed = c[None] + 2 * (w * a + cross(u, a)) + t[:, None, :]
    return {"centred": c, "posed": posed, "unit": unit, "norm": norm}


def pose_b(centred, quaternions, g, normalise=True, dtype=LD):
    """adjoint of :func:`pose` for the adjoint g [n,V,3] of the posed vertices -> dict: vertices_b [V,3] (summed over the views, no mean
    subtracted), mean = (sum, abs) of its column mean [3], q_b = (sum, abs) [n,4] w.r.t. the RAW quaternions, t_b = (sum, abs) [n,3].

    r = c + 2 w (u x c) + 2 u x (u x c);  the adjoint of x -> u x x is y -> y x u."""
    c, q, g = (np.asarray(a, dtype=dtype) for a in (centred, quaternions, g))
    n, V = g.shape[0], g.shape[1]
    norm = np.sqrt((q * q).sum(axis=-1)) if normalise else np.ones(n, dtype=dtype)
    unit = q / norm[:, None]
    u, w = unit[:, None, :3], unit[:, None, 3:]
    cc = np.broadcast_to(c[None], g.shape)
    a = cross(u, cc)
    gu = cross(g, u)
    c_b = g + 2 * w * gu + 2 * cross(gu, u)
    u_b = 2 * w * cross(cc, g) + 2 * cross(a, g) + 2 * cross(cc, gu)
    w_b = 2 * dot(g, a)
    s = np.concatenate((u_b, w_b[..., None]), axis=-1)  # [n,V,4]: adjoint of the unit quaternion, per vertex
    S, A = sums(s, axis=1)
    if normalise:  # raw_b = (I - q q^T) / |raw| applied to the sum; its error scale: |that matrix| applied to the sums of |term|
        P = (np.eye(4, dtype=dtype)[None] - unit[:, :, None] * unit[:, None, :]) / norm[:, None, None]
        S, A = (P * S[:, None, :]).sum(axis=-1), (np.abs(P) * A[:, None, :]).sum(axis=-1)
    return {"vertices_b": c_b.sum(axis=0), "mean": sums(c_b.reshape(-1, 3) / dtype(V), axis=0), "q_b": (S, A), "t_b": sums(g, axis=1)}


# ---- pinhole projection with OpenCV's five distortion coefficients (k1, k2, p1, p2, k3) ----------------------------------------------


def _camera_space(points, extrinsic, dtype):
    p, E = np.asarray(points, dtype=dtype), np.asarray(extrinsic, dtype=dtype)
    return [E[:, None, i, 0] * p[..., 0] + E[:, None, i, 1] * p[..., 1] + E[:, None, i, 2] * p[..., 2] + E[:, None, i, 3] for i in range(3)], E


def project(points, extrinsic, intrinsic, distortion=None, dtype=LD):
    """points [n,V,3], extrinsic [n,3,4], intrinsic [n,3,3], distortion [n,5] | None -> ij [n,V,2], depths [n,V]"""
    (cx, cy, cz), _E = _camera_space(points, extrinsic, dtype)
    K = np.asarray(intrinsic, dtype=dtype)
    x, y = cx / cz, cy / cz
    if distortion is not None:
        k1, k2, p1, p2, k3 = (np.asarray(distortion, dtype=dtype)[:, i, None] for i in range(5))
        r2 = x * x + y * y
        radial = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
        x, y = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    ij = np.stack((K[:, None, 0, 0] * x + K[:, None, 0, 1] * y + K[:, None, 0, 2], K[:, None, 1, 0] * x + K[:, None, 1, 1] * y + K[:, None, 1, 2]), axis=-1)
    return ij, cz


def project_b(points, extrinsic, intrinsic, distortion, ij_b, depths_b=None, dtype=LD):
    """adjoint of :func:`project`: -> points_b [n,V,3], through the Jacobian of the distortion written out"""
    (cx, cy, cz), E = _camera_space(points, extrinsic, dtype)
    K, g = np.asarray(intrinsic, dtype=dtype), np.asarray(ij_b, dtype=dtype)
    x, y = cx / cz, cy / cz
    xd_b = K[:, None, 0, 0] * g[..., 0] + K[:, None, 1, 0] * g[..., 1]
    yd_b = K[:, None, 0, 1] * g[..., 0] + K[:, None, 1, 1] * g[..., 1]
    x_b, y_b = xd_b, yd_b
    if distortion is not None:
        k1, k2, p1, p2, k3 = (np.asarray(distortion, dtype=dtype)[:, i, None] for i in range(5))
        r2 = x * x + y * y
        radial = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
        slope = k1 + 2 * k2 * r2 + 3 * k3 * r2 * r2  # d radial / d r2
        xd_x = radial + 2 * x * x * slope + 2 * p1 * y + 6 * p2 * x
        xd_y = 2 * x * y * slope + 2 * p1 * x + 2 * p2 * y
        yd_x = 2 * x * y * slope + 2 * p1 * x + 2 * p2 * y
        yd_y = radial + 2 * y * y * slope + 6 * p1 * y + 2 * p2 * x
        x_b, y_b = xd_b * xd_x + yd_b * yd_x, xd_b * xd_y + yd_b * yd_y
    c_b = [x_b / cz, y_b / cz, -(x * x_b + y * y_b) / cz]
    if depths_b is not None:
        c_b[2] = c_b[2] + np.asarray(depths_b, dtype=dtype)
    return np.stack([E[:, None, 0, j] * c_b[0] + E[:, None, 1, j] * c_b[1] + E[:, None, 2, j] * c_b[2] for j in range(3)], axis=-1)


# ---- shading: vertex normals from the faces around each vertex, luminosity max(0, -N.l) + ambient, colour * luminosity ---------------


def _face_geometry(P, faces):
    p0, p1, p2 = P[:, faces[:, 0]], P[:, faces[:, 1]], P[:, faces[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    nn = cross(e1, e2)
    length = np.sqrt(dot(nn, nn))
    return e1, e2, nn / length[..., None], length


def _scatter_corners(out, faces, values):
    """out[b, faces[f, corner]] += values[corner][b, f] (a face adds to its three corners)"""
    for b in range(out.shape[0]):
        for corner in range(3):
            np.add.at(out[b], faces[:, corner], values[corner][b])
    return out


def shade(posed, faces, light, ambient, color=None, clockwise=False, dtype=LD):
    """posed [n,V,3] -> dict: normals [n,V,3], luminosity [n,V], colors [n,V,C] (with a colour [C]), d = -N.l [n,V]"""
    P, L = np.asarray(posed, dtype=dtype), np.asarray(light, dtype=dtype)
    faces = np.asarray(faces, dtype=np.int64)
    _e1, _e2, unit, _len = _face_geometry(P, faces)
    acc = _scatter_corners(np.zeros_like(P), faces, (unit, unit, unit)) * dtype(-1 if clockwise else 1)
    length = np.sqrt(dot(acc, acc))
    N = acc / length[..., None]
    d = -dot(N, L)
    lum = np.maximum(d, 0) + dtype(ambient)
    out = {"normals": N, "acc_len": length, "d": d, "luminosity": lum}
    if color is not None:
        out["colors"] = lum[..., None] * np.asarray(color, dtype=dtype)
    return out


def shade_b(posed, faces, light, ambient, color, clockwise, luminosity_b=None, colors_b=None, dtype=LD):
    """adjoint of :func:`shade` -> dict: posed_b [n,V,3], light_b = (sum, abs) [3], ambient_b = (sum, abs) [], color_b = (sum, abs) [C]"""
    P, L = np.asarray(posed, dtype=dtype), np.asarray(light, dtype=dtype)
    faces = np.asarray(faces, dtype=np.int64)
    sign = dtype(-1 if clockwise else 1)
    f = shade(posed, faces, light, ambient, color, clockwise, dtype)
    N, lum = f["normals"], f["luminosity"]
    lum_b = np.zeros_like(lum) if luminosity_b is None else np.asarray(luminosity_b, dtype=dtype).copy()
    out = {}
    if colors_b is not None:
        cb, col = np.asarray(colors_b, dtype=dtype), np.asarray(color, dtype=dtype)
        lum_b = lum_b + (cb * col).sum(axis=-1)
        out["color_b"] = sums((cb * lum[..., None]).reshape(-1, cb.shape[-1]), axis=0)
    d_b = np.where(f["d"] > 0, lum_b, 0)
    out["light_b"] = sums((-N * d_b[..., None]).reshape(-1, 3), axis=0)
    out["ambient_b"] = sums(lum_b.reshape(-1))
    N_b = -d_b[..., None] * L
    acc_b = (N_b - N * dot(N, N_b)[..., None]) / f["acc_len"][..., None]
    e1, e2, unit, length = _face_geometry(P, faces)
    unit_b = sign * (acc_b[:, faces[:, 0]] + acc_b[:, faces[:, 1]] + acc_b[:, faces[:, 2]])
    n_b = (unit_b - unit * dot(unit, unit_b)[..., None]) / length[..., None]
    e1_b, e2_b = cross(e2, n_b), cross(n_b, e1)  # n = e1 x e2
    out["posed_b"] = _scatter_corners(np.zeros_like(P), faces, (-(e1_b + e2_b), e1_b, e2_b))
    return out


# ---- rigid energy 0.5 c d^T (L^T L) d over the CSR rows of L^T L -----------------------------------------------------------------------


def rigid(vertices, vertices_ref, offsets, cols, vals, cregu, dtype=LD):
    """-> dict: gradient [V,3] = c (L^T L) d, energy = (sum, abs) of 0.5 d . gradient, d = vertices - vertices_ref"""
    d = np.asarray(vertices, dtype=dtype) - np.asarray(vertices_ref, dtype=dtype)
    offsets, cols = np.asarray(offsets, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    rows = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    grad = np.zeros_like(d)
    np.add.at(grad, rows, np.asarray(vals, dtype=dtype)[:, None] * d[cols])
    grad = grad * dtype(cregu)
    return {"gradient": grad, "energy": sums((dtype(0.5) * d * grad).reshape(-1))}


# ---- silhouette flags: an edge with exactly one front-facing face in the image -------------------------------------------------------


def silhouette(ij, faces, clockwise, dtype=LD):
    """ij [n,V,2] -> (uint8 [n,T,3] in the slot order (v0,v1), (v1,v2), (v2,v0); the signed areas [n,T] they were decided by)"""
    p, faces = np.asarray(ij, dtype=dtype), np.asarray(faces, dtype=np.int64)
    V = p.shape[1]
    u, v = p[:, faces[:, 1]] - p[:, faces[:, 0]], p[:, faces[:, 2]] - p[:, faces[:, 0]]
    cr = u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]
    visible = (cr > 0) if clockwise else (cr < 0)
    e = np.concatenate((faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]))  # slot-major
    _, edge_id = np.unique(e.min(axis=1) * V + e.max(axis=1), return_inverse=True)
    edge_id = edge_id.reshape(3, -1).T  # [T,3]
    flags = np.zeros(visible.shape + (3,), dtype=np.uint8)
    for b in range(p.shape[0]):
        count = np.zeros(int(edge_id.max()) + 1, dtype=np.int64)
        np.add.at(count, edge_id.reshape(-1), np.repeat(visible[b].astype(np.int64), 3))
        flags[b] = count[edge_id] == 1
    return flags, cr


# ---- momentum update -------------------------------------------------------------------------------------------------------------------


def momentum(x, speed, grad, factor, inertia, damping, grad2=None, step_max=None, normalize_rows=0, grad_scale=1.0, grad_mean=None, dtype=LD):
    """s = (1 - damping)(inertia s + (1 - inertia) clamp(-factor (grad_scale (grad - grad_mean) + grad2), +-step_max)), x += s, rows of
    ``normalize_rows`` values renormalised -> dict: x, speed (shape of x), mean = (sum, abs) [3] of the column mean of the new x viewed
    as [count/3, 3] (when count is a multiple of 3), clamped = (number of steps cut at -step_max, at +step_max)"""
    shape = np.shape(x)
    x, speed, grad = (np.asarray(a, dtype=dtype).reshape(-1) for a in (x, speed, grad))
    g = grad
    if grad_mean is not None:
        g = (g.reshape(-1, 3) - np.asarray(grad_mean, dtype=dtype)).reshape(-1)
    g = g * dtype(grad_scale)
    if grad2 is not None:
        g = g + np.asarray(grad2, dtype=dtype).reshape(-1)
    step = -g * dtype(factor)
    clamped = (0, 0)
    if step_max is not None:
        clamped = (int((step < -step_max).sum()), int((step > step_max).sum()))
        step = np.clip(step, dtype(-step_max), dtype(step_max))
    s = (1 - dtype(damping)) * (speed * dtype(inertia) + (1 - dtype(inertia)) * step)
    new = x + s
    if normalize_rows:
        rows = new.reshape(-1, normalize_rows)
        new = (rows / np.sqrt((rows * rows).sum(axis=-1, keepdims=True))).reshape(-1)
    out = {"x": new.reshape(shape), "speed": s.reshape(shape), "clamped": clamped}
    if new.size % 3 == 0 and not normalize_rows:
        out["mean"] = sums(new.reshape(-1, 3) / dtype(new.size // 3), axis=0)
    return out


# ---- frame sums ------------------------------------------------------------------------------------------------------------------------


def l2(image, obs, weights=None, nb_colors=1, clamp=None, dtype=LD):
    """(sum, abs) of w[pixel] (clamp(image) - obs)^2 over the values of a frame; the residual is formed in float64 as the kernel forms it
    (exact for float32 pixels), squared and added in ``dtype``"""
    v = np.asarray(image).astype(np.float64).reshape(-1)
    if clamp is not None:
        v = np.clip(v, clamp[0], clamp[1])
    r = (v - np.asarray(obs).astype(np.float64).reshape(-1)).astype(dtype)
    terms = r * r
    if weights is not None:
        terms = terms * np.repeat(np.asarray(weights).astype(np.float64).reshape(-1), nb_colors).astype(dtype)
    return sums(terms)


def depth_residual(image, obs, max_depth, dtype=LD):
    """-> dict: depth = clamp(image, 0, max_depth), diff = (depth - obs)^2, image_b = 2 (depth - obs) where the clamp passes (in the pixel
    type of ``image``), loss = (sum, abs) of diff"""
    v = np.asarray(image).astype(np.float64).reshape(-1)
    depth = np.clip(v, 0.0, max_depth)
    r = (depth - np.asarray(obs, dtype=np.float64).reshape(-1)).astype(dtype)
    diff = r * r
    image_b = np.where((v >= 0) & (v <= max_depth), 2 * r, 0).astype(np.asarray(image).dtype)
    return {"depth": depth, "diff": diff, "image_b": image_b, "loss": sums(diff)}


# ======== what the CPU and the GPU tests share: launch constants, distances, seeded inputs, case tables ================================


def kernel_constants():
    """``constexpr int NAME = value`` of the kernel headers"""
    found = {}
    for name in ("dr_fronthalf.h", "dr_fititer.h"):
        with open(os.path.join(CSRC, name)) as f:
            found.update({k: int(v) for k, v in re.findall(r"constexpr\s+int\s+(\w+)\s*=\s*(\d+)\s*;", f.read())})
    missing = [k for k in ("FH_BLOCK", "GATHER_LANES", "POSE_B_BLOCKS", "FIT_MAX_VIEWS", "MOMENTUM_MAX", "L2_BLOCKS", "L2_ROUND") if k not in found]
    assert not missing, f"constants not found in the kernel headers: {missing}"
    return found


def ceil_div(a, b):
    return -(-int(a) // int(b))


def pose_b_geometry(V, n, k=None):
    """launch geometry of fit_pose_project_b_kernel, as deodr_hip_fit_pose_project_b chooses it -> dict"""
    k = k or kernel_constants()
    lanes = 1 if n == 1 else k["GATHER_LANES"]
    per_block = k["FH_BLOCK"] // lanes
    wanted = ceil_div(V * lanes, k["FH_BLOCK"])
    grid = min(wanted, k["POSE_B_BLOCKS"])
    return {"lanes": lanes, "per_block": per_block, "wanted": wanted, "grid": grid, "strided_trips": ceil_div(V, grid * per_block),
            "sum_rounds": ceil_div(grid, (k["FH_BLOCK"] // 64) * 8), "view_trips": ceil_div(n, lanes), "idle_lanes": (-n) % lanes}  # fmt: skip


def l2_geometry(count, itemsize, k=None):
    """launch geometry of l2_loss_kernel (l2_loss_impl): chunks of 32 bytes, a thread takes L2_ROUND chunks a grid stride apart per trip"""
    k = k or kernel_constants()
    W = 32 // itemsize
    grid = min(ceil_div(count, k["FH_BLOCK"] * 32), k["L2_BLOCKS"])
    chunks, stride = count // W, grid * k["FH_BLOCK"]
    return {"W": W, "grid": grid, "chunks": chunks, "stride": stride, "tail": count - chunks * W, "strides": ceil_div(chunks, stride),
            "trips": ceil_div(chunks, stride * k["L2_ROUND"])}  # fmt: skip


def l2_counts(itemsize, k=None):
    """the element counts of the frame-sum cases for a pixel type -> {name: count}: 1, W - 1, W, W + 1 (W = 32 bytes' worth), the smallest
    count with a ragged tail whose chunks go beyond one grid stride, and the smallest beyond L2_ROUND strides (a thread's second trip)"""
    k = k or kernel_constants()
    W = 32 // itemsize
    out = {"one": 1, "W-1": W - 1, "W": W, "W+1": W + 1}
    for name, strides in (("beyond_one_stride", 1), ("beyond_a_round", k["L2_ROUND"])):
        for grid in range(1, k["L2_BLOCKS"] + 1):
            count = (strides * grid * k["FH_BLOCK"] + 1) * W + W - 1  # one chunk more than `strides` strides, and a tail of W - 1 values
            g = l2_geometry(count, itemsize, k)
            if g["grid"] == grid and g["strides"] > strides:
                out[name] = count
                break
        assert name in out, name
    return out


def sum_distance(got, ref_pair):
    """largest |got - sum| in units of eps64 * sum |term|, over the components (0 where a component has no terms at all)"""
    ref, scale = (np.asarray(a, dtype=LD) for a in ref_pair)
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    if not err.size:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        units = np.where(scale > 0, err / (EPS64 * scale), np.where(err > 0, np.inf, 0))
    return float(units.max())


def elem_distance(got, ref):
    """largest |got - ref| in units of eps64 * max |ref|"""
    ref = np.asarray(ref, dtype=LD)
    if not ref.size:
        return 0.0
    scale = np.abs(ref).max()
    err = np.abs(np.asarray(got, dtype=LD) - ref).max()
    return float(err / (EPS64 * scale)) if scale > 0 else (0.0 if err == 0 else float("inf"))


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def cameras(n):
    """n cameras looking down +z from about 8 units away: -> extrinsic [n,3,4], intrinsic [n,3,3], distortion [n,5]"""
    i = np.arange(n, dtype=np.float64)
    E = np.stack([np.column_stack((rot_x(0.1 + 0.004 * b) @ rot_y(0.01 * b), [0.05 * np.sin(b), 0.03 * np.cos(b), 8.0 + 0.5 * np.sin(1.3 * b)])) for b in i])
    K = np.stack([np.array([[300.0 + b, 0.3, 64.0], [0.0, 310.0 - 0.5 * b, 48.0 + 0.1 * b], [0.0, 0.0, 1.0]]) for b in i])
    dist = np.stack([np.array([0.1, -0.02, 0.003, -0.004, 0.01]) * (1 + 0.02 * b) for b in i])
    return E, K, dist


# A. point clouds: (V, n) and the regime each is there for
POINT_CASES = [(1, 1), (1, 2), (31, 3), (32, 8), (33, 9), (255, 1), (256, 1), (257, 1), (1025, 17), (2049, 2), (4100, 64), (16385, 1)]
# every option both ways, every number of colour channels: [distortion, depths_b, posed_b, C of colors_b | None, mean + depth_colors in the forward]
POINT_OPTIONS = {
    "dist-depth-posed-c3-mean": dict(distortion=True, depths_b=True, posed_b=True, C=3, centre=True),
    "plain": dict(distortion=False, depths_b=False, posed_b=False, C=None, centre=False),
    "dist-posed-c1": dict(distortion=True, depths_b=False, posed_b=True, C=1, centre=False),
    "depth-c4-mean": dict(distortion=False, depths_b=True, posed_b=False, C=4, centre=True),
}
DEPTHS_B_SCALE, DEPTH_SCALE = 0.7, 2.5


def point_inputs(V, n):
    """seeded float64 inputs of a point-cloud case (the cloud is not centred: its mean is an input of the forward)"""
    rs = np.random.RandomState(1000 * n + V)
    E, K, dist = cameras(n)
    return {
        "vertices": rs.rand(V, 3) - 0.5 + np.array([0.2, -0.1, 0.15]), "quaternions": rs.randn(n, 4) * 0.3 + np.array([0, 0, 0, 1.0]),
        "translations": rs.randn(n, 3) * 0.05, "extrinsic": E, "intrinsic": K, "distortion": dist, "ij_b": rs.randn(n, V, 2),
        "depths_b": rs.randn(n, V), "posed_b": rs.randn(n, V, 3), "colors_b": rs.randn(n, V, 4),
    }  # fmt: skip


def point_reference(V, n, options, dtype=LD, inputs=None):
    """everything the point-cloud calls of a case compute, for one entry of POINT_OPTIONS -> dict"""
    d = inputs or point_inputs(V, n)
    dist = d["distortion"] if options["distortion"] else None
    mean = d["vertices"].mean(axis=0)  # (a float64 input of the kernel: the same rounded value goes to both)
    f = pose(d["vertices"], d["quaternions"], d["translations"], mean if options["centre"] else None, dtype=dtype)
    ij, depths = project(f["posed"], d["extrinsic"], d["intrinsic"], dist, dtype)
    camera_b = project_b(f["posed"], d["extrinsic"], d["intrinsic"], dist, d["ij_b"], d["depths_b"] * dtype(DEPTHS_B_SCALE) if options["depths_b"] else None, dtype)
    g = camera_b + (np.asarray(d["posed_b"], dtype=dtype) if options["posed_b"] else 0)
    out = {"centred": f["centred"], "posed": f["posed"], "ij": ij, "depths": depths, "depth_colors": depths * dtype(DEPTH_SCALE), "views_sum": camera_b.sum(axis=0)}
    out.update(pose_b(f["centred"], d["quaternions"], g, dtype=dtype))
    if options["C"]:
        out["colors_sum"] = np.asarray(d["colors_b"][..., : options["C"]], dtype=dtype).sum(axis=0)
    return out


def autograd_ops_reference(V, n, dtype=LD, inputs=None):
    """RigidTransformFunc (unit quaternions given, not renormalised) and ProjectPointsFunc, values and adjoints"""
    d = inputs or point_inputs(V, n)
    q = d["quaternions"] / np.linalg.norm(d["quaternions"], axis=-1, keepdims=True)  # float64 inputs, unit to rounding
    f = pose(d["vertices"], q, d["translations"], None, normalise=False, dtype=dtype)
    out = {"unit_quaternions": q, "posed": f["posed"]}
    out.update(pose_b(f["centred"], q, d["posed_b"], normalise=False, dtype=dtype))
    posed64 = np.asarray(f["posed"], dtype=np.float64)  # the projection op is given float64 points: the same ones here
    out["points"] = posed64
    out["ij"], out["depths"] = project(posed64, d["extrinsic"], d["intrinsic"], d["distortion"], dtype)
    out["points_b"] = project_b(posed64, d["extrinsic"], d["intrinsic"], d["distortion"], d["ij_b"], d["depths_b"], dtype)
    return out


# B. meshes
def fan(k):
    """an open fan of k faces around a raised hub (vertex 0): the hub's list of faces has k entries, every rim edge is a boundary"""
    theta = 1.5 * np.pi * np.arange(k + 1) / k
    rim = np.stack(((1 + 0.1 * np.sin(3 * theta)) * np.cos(theta), (1 + 0.1 * np.sin(3 * theta)) * np.sin(theta), 0.05 * np.cos(2 * theta)), axis=-1)
    vertices = np.vstack(([[0.02, -0.03, 0.3]], rim))
    faces = np.stack((np.zeros(k, dtype=np.int64), 1 + np.arange(k), 2 + np.arange(k)), axis=-1)
    return vertices, faces


def _sphere(nu, rings):
    from deodr_amd import scenes  # (NumPy only)

    v, f = scenes.bumpy_sphere(nu, rings)
    return np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.int64)


MESH_CASES = {  # name -> (builder, number of views)
    "triangle": (lambda: (np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.05], [0.2, 0.9, -0.1]]), np.array([[0, 1, 2]])), 2),
    "tetrahedron": (lambda: (np.array([[1.0, 1.1, 0.9], [1.05, -1.0, -1.0], [-1.0, 0.95, -1.0], [-0.9, -1.0, 1.1]]), np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]])), 2),
    "fan8": (lambda: fan(8), 2),
    "fan9": (lambda: fan(9), 2),
    "fan16": (lambda: fan(16), 2),
    "fan17": (lambda: fan(17), 2),
    "sphere_7_4": (lambda: _sphere(7, 4), 3),
    "sphere_33_31": (lambda: _sphere(33, 31), 3),
    "sphere_128_65": (lambda: _sphere(128, 65), 1),
}
MESH_CREGU, MESH_DATA_ENERGY, MESH_DATA_WEIGHT = 500.0, 3.25, 0.5


def mesh_inputs(name):
    """seeded float64 inputs of a mesh case: the second view looks at the back of the mesh (lit and unlit vertices both occur)"""
    build, n = MESH_CASES[name]
    vertices, faces = build()
    V = len(vertices)
    rs = np.random.RandomState(sum(map(ord, name)))
    turn = [rot_x(0.3) @ rot_y(0.2), rot_x(0.3) @ rot_y(0.2) @ np.diag([1.0, -1.0, -1.0]), rot_x(-0.9) @ rot_y(1.7)][:n]
    posed = np.stack([(vertices * (1 + 0.03 * rs.randn(V, 1))) @ r.T + 0.01 * rs.randn(V, 3) for r in turn])
    return {
        "vertices": vertices, "faces": faces, "n": n, "posed": posed, "ij": 100 * posed[..., :2] + np.array([64.0, 48.0]),
        "light": np.array([0.3, -0.5, 0.6]), "ambient": 0.25, "color": np.array([0.7, 0.5, 0.4]), "luminosity_b": rs.randn(n, V),
        "colors_b": rs.randn(n, V, 3), "x": vertices + 0.01 * rs.randn(V, 3), "ref": vertices,
    }  # fmt: skip


# C. momentum update: launches of several tensors, three consecutive steps each
def _entry(shape, factor, step_max=None, rows=0, grad2=False, grad_scale=1.0, grad_mean=False, mean_out=False):
    return dict(shape=shape, factor=factor, step_max=step_max, rows=rows, grad2=grad2, grad_scale=grad_scale, grad_mean=grad_mean, mean_out=mean_out)


MOMENTUM_STEPS, MOMENTUM_INERTIA, MOMENTUM_DAMPING = 3, 0.96, 0.05
MOMENTUM_LAUNCHES = {  # name -> (V and n the scratch is sized for, entries, whether energy[1] is formed on the way)
    "one": ((100, 1), [_entry((257,), 0.0005, step_max=0.5)], False),
    "eight": ((400, 1), [
        _entry((1,), 0.0001), _entry((1, 3), 0.0005, grad_mean=True, mean_out=True), _entry((85, 3), 0.0005, step_max=0.5, grad2=True, mean_out=True),
        _entry((256,), 0.0005), _entry((257,), 0.0005, step_max=0.3, grad_scale=0.37), _entry((1, 4), 0.00006, step_max=0.1, rows=4),
        _entry((64, 4), 0.00006, step_max=0.1, rows=4), _entry((300, 4), 0.00006, rows=4, grad2=True)], True),
    "wide": ((21846, 1), [_entry((21846, 3), 0.0005, step_max=0.5, grad2=True, grad_scale=0.37, grad_mean=True, mean_out=True),
                          _entry((1, 3), 0.0005, mean_out=True)], True),
}  # fmt: skip


def momentum_inputs(name):
    """-> (initial x per entry, per step and entry: dict grad, grad2 | None, grad_mean | None)"""
    _size, entries, _energy = MOMENTUM_LAUNCHES[name]
    rs = np.random.RandomState(len(name))
    x0 = [rs.randn(*e["shape"]) for e in entries]
    steps = [[{"grad": rs.randn(*e["shape"]) * 1e3, "grad2": rs.randn(*e["shape"]) * 50 if e["grad2"] else None,
               "grad_mean": rs.randn(3) * 100 if e["grad_mean"] else None} for e in entries] for _ in range(MOMENTUM_STEPS)]  # fmt: skip
    return x0, steps


def momentum_reference(entry, x, speed, given, dtype=LD):
    return momentum(x, speed, given["grad"], entry["factor"], MOMENTUM_INERTIA, MOMENTUM_DAMPING, given["grad2"], entry["step_max"], entry["rows"],
                    entry["grad_scale"], given["grad_mean"], dtype)  # fmt: skip
