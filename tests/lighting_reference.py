"""NumPy restatement, in float64 and in long double, of what include/deodr_hip_lighting.h computes: vertex normals from the faces around each vertex
(tests/fititer_reference has the face geometry), the nine real SH basis functions Y_k of bands 0 - 2 and their gradients, the irradiance
E = sum_k sh[k, min(c, S-1)] Y_k(N), colours = albedo E, and the adjoint: through grad Y_k, the normalisation of the accumulated normal, the face
normals back to the corners, and the sums that are sh_b and albedo_b -- and the case tables that tests/test_lighting_reference.py (CPU: pins this
module, measures the float64 error) and tests/test_lighting_gpu.py (the kernels) share.

Sums come as pairs (sum, sum of |term|): the second is the scale their errors are measured in (fititer_reference.sum_distance)."""

import os
import re

import numpy as np

import fititer_reference as fr
from fititer_reference import LD

F64 = np.float64


def kernel_constants():
    """``constexpr int NAME = value`` of deodr_amd/csrc/dr_lighting.h (and FH_BLOCK, GATHER_LANES, FIT_MAX_VIEWS of the headers before it)"""
    found = dict(fr.kernel_constants())
    with open(os.path.join(fr.CSRC, "dr_lighting.h")) as f:
        text = f.read()
    found.update({k: int(v) for k, v in re.findall(r"constexpr\s+int\s+(\w+)\s*=\s*([0-9]+)\s*;", text)})
    found.update({k: int(a) << int(b) for k, a, b in re.findall(r"constexpr\s+int\s+(\w+)\s*=\s*([0-9]+)\s*<<\s*([0-9]+)\s*;", text)})
    missing = [k for k in ("SH_MAX_BLOCKS", "SH_COEFFS", "SH_MAX_VERTICES") if k not in found]
    assert not missing, f"constants not found in dr_lighting.h: {missing}"
    return found


# ---- the basis ------------------------------------------------------------------------------------------------------------------------


def pi(dtype=LD):
    return 4 * np.arctan(dtype(1))


def constants(dtype=LD):
    """c0 .. c4 as expressions of pi"""
    root = np.sqrt(pi(dtype))
    return (1 / (2 * root), np.sqrt(dtype(3)) / (2 * root), np.sqrt(dtype(15)) / (2 * root), np.sqrt(dtype(5)) / (4 * root), np.sqrt(dtype(15)) / (4 * root))


def basis(N, dtype=LD):
    """N [..., 3] -> Y [..., 9]"""
    N = np.asarray(N, dtype=dtype)
    c0, c1, c2, c3, c4 = constants(dtype)
    x, y, z = N[..., 0], N[..., 1], N[..., 2]
    return np.stack((c0 * np.ones_like(x), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c3 * (3 * z * z - 1), c2 * x * z, c4 * (x * x - y * y)), axis=-1)


def basis_gradient(N, dtype=LD):
    """N [..., 3] -> dY_k / d(x, y, z) [..., 9, 3], x, y, z free variables"""
    N = np.asarray(N, dtype=dtype)
    _c0, c1, c2, c3, c4 = constants(dtype)
    x, y, z = N[..., 0], N[..., 1], N[..., 2]
    o, l = np.zeros_like(x), np.ones_like(x)
    rows = [(o, o, o), (o, c1 * l, o), (o, o, c1 * l), (c1 * l, o, o), (c2 * y, c2 * x, o), (o, c2 * z, c2 * y), (o, o, 6 * c3 * z), (c2 * z, o, c2 * x),
            (2 * c4 * x, -2 * c4 * y, o)]  # fmt: skip
    return np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)


LOBE = lambda dtype: (pi(dtype), 2 * pi(dtype) / 3, pi(dtype) / 4)  # noqa: E731  the clamped cosine in zonal harmonics, per band
BAND = (0, 1, 1, 1, 2, 2, 2, 2, 2)


def from_directional(light, ambient, dtype=LD):
    """sh [9] of max(0, -N . L) + ambient to order 2: lobe_band(k) Y_k(-L / |L|) |L|, the ambient term in band 0"""
    L = np.asarray(light, dtype=dtype)
    norm = np.sqrt((L * L).sum())
    sh = np.zeros(9, dtype=dtype)
    if norm > 0:
        lobe = LOBE(dtype)
        sh = np.array([lobe[b] for b in BAND], dtype=dtype) * basis(-L / norm, dtype) * norm
    sh[0] += dtype(ambient) / constants(dtype)[0]
    return sh


# ---- forward and adjoint ----------------------------------------------------------------------------------------------------------------


def _columns(sh, dtype):
    sh = np.asarray(sh, dtype=dtype)
    return sh.reshape(9, -1)


def forward(posed, faces, sh, albedo=None, clockwise=False, dtype=LD):
    """posed [n,V,3], sh [9] | [9,S], albedo None | [C] | [V,C] -> dict: normals [n,V,3], acc_len [n,V], Y [n,V,9], E [n,V,S], luminosity [n,V]
    (S = 1), colors [n,V,C] (with an albedo)"""
    P, faces = np.asarray(posed, dtype=dtype), np.asarray(faces, dtype=np.int64)
    _e1, _e2, unit, _len = fr._face_geometry(P, faces)
    acc = fr._scatter_corners(np.zeros_like(P), faces, (unit, unit, unit)) * dtype(-1 if clockwise else 1)
    length = np.sqrt(fr.dot(acc, acc))
    N = acc / length[..., None]
    Y = basis(N, dtype)
    E = Y @ _columns(sh, dtype)
    out = {"normals": N, "acc_len": length, "Y": Y, "E": E}
    if E.shape[-1] == 1:
        out["luminosity"] = E[..., 0]
    if albedo is not None:
        out["colors"] = np.asarray(albedo, dtype=dtype) * E  # (E [n,V,1] broadcasts over the channels)
    return out


def backward(posed, faces, sh, albedo, clockwise, luminosity_b=None, colors_b=None, dtype=LD):
    """adjoint of :func:`forward` -> dict: posed_b [n,V,3]; sh_b = (sum, abs) [9,S]; albedo_b = (sum, abs) of the albedo's shape (with an albedo)"""
    P, faces = np.asarray(posed, dtype=dtype), np.asarray(faces, dtype=np.int64)
    n, V = P.shape[:2]
    sign = dtype(-1 if clockwise else 1)
    f = forward(posed, faces, sh, albedo, clockwise, dtype)
    N, Y, E, cols = f["normals"], f["Y"], f["E"], _columns(sh, dtype)
    S = cols.shape[1]
    out = {}
    if colors_b is not None:
        cb, alb = np.asarray(colors_b, dtype=dtype), np.asarray(albedo, dtype=dtype)
        C = cb.shape[-1]
        E_b = cb * alb  # [n,V,C]
        products = cb * E  # [n,V,C]
        out["albedo_b"] = fr.sums(products, axis=0) if alb.ndim == 2 else fr.sums(products.reshape(-1, C), axis=0)
    else:
        E_b = np.zeros((n, V, 1), dtype=dtype)
    if S == 1:
        g = E_b.sum(axis=-1, keepdims=True)
        if luminosity_b is not None:
            g = g + np.asarray(luminosity_b, dtype=dtype)[..., None]
        E_b = g  # [n,V,1]
    else:
        assert luminosity_b is None
    terms = Y[..., :, None] * E_b[..., None, :]  # [n,V,9,S]
    out["sh_b"] = fr.sums(terms.reshape(n * V, 9, S), axis=0)
    dY = basis_gradient(N, dtype)  # [n,V,9,3]
    N_b = np.einsum("nvs,ks,nvkd->nvd", E_b, cols, dY)
    acc_b = (N_b - N * fr.dot(N, N_b)[..., None]) / f["acc_len"][..., None]
    e1, e2, unit, length = fr._face_geometry(P, faces)
    unit_b = sign * (acc_b[:, faces[:, 0]] + acc_b[:, faces[:, 1]] + acc_b[:, faces[:, 2]])
    n_b = (unit_b - unit * fr.dot(unit, unit_b)[..., None]) / length[..., None]
    e1_b, e2_b = fr.cross(e2, n_b), fr.cross(n_b, e1)  # n = e1 x e2
    out["posed_b"] = fr._scatter_corners(np.zeros_like(P), faces, (-(e1_b + e2_b), e1_b, e2_b))
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------------------

def grid(V, w):
    """a bumpy height field of exactly V >= 2 w vertices, w per row (the last row may be shorter), two triangles per cell: every vertex has a face,
    inner vertices have six"""
    assert V >= 2 * w
    i = np.arange(V)
    x, y = (i % w).astype(F64), (i // w).astype(F64)
    vertices = np.stack((0.1 * x, 0.1 * y, 0.08 * np.sin(0.7 * x) * np.cos(0.5 * y) + 0.002 * x * y / w), axis=-1)
    faces = []
    for a in range(V - w):
        if a % w < w - 1:
            faces.append((a, a + 1, a + w))
            if a + w + 1 < V:
                faces.append((a + 1, a + w + 1, a + w))
    faces = np.array(faces, dtype=np.int64)
    assert len(np.unique(faces)) == V
    return vertices, faces


# name -> (builder of (vertices, faces), views, why).  fan(k): k + 2 vertices, the hub's list of faces has k entries.
CASES = {
    "triangle_n1": (lambda: fr.MESH_CASES["triangle"][0](), 1, "V = 3, T = 1"),
    "triangle_n2": (lambda: fr.MESH_CASES["triangle"][0](), 2, "two views"),
    "fan7": (lambda: fr.fan(7), 2, "valence GATHER_LANES - 1"),
    "fan8": (lambda: fr.fan(8), 2, "valence GATHER_LANES"),
    "fan9": (lambda: fr.fan(9), 2, "valence GATHER_LANES + 1"),
    "fan16": (lambda: fr.fan(16), 1, "valence 2 GATHER_LANES"),
    "fan17": (lambda: fr.fan(17), 2, "valence 2 GATHER_LANES + 1"),
    "v32": (lambda: fr.fan(30), 1, "V = 32: one workgroup at 8 lanes per vertex and 256 threads"),
    "v33": (lambda: fr.fan(31), 1, "V = 33: two workgroups"),
    "sphere_n64": (lambda: fr._sphere(7, 4), 64, "a closed mesh, 64 views"),
    "v8193_n1": (lambda: grid(8193, 64), 1, "257 workgroups: a second round of grid_sum"),
    "v129_n64": (lambda: grid(129, 8), 64, "258 workgroups over 64 views"),
    "past_cap": (lambda: grid(513, 16), 64, "V = 513, n = 64: 1026 workgroups wanted, the first shape past the cap of 1024"),
}

# name -> C, S, albedo (None | "single" | "vertex"), luminosity as well, clockwise, accumulate
OPTIONS = {
    "lum": dict(C=1, S=1, albedo=None, lum=True, clockwise=False, accumulate=False),
    "c1-single": dict(C=1, S=1, albedo="single", lum=False, clockwise=True, accumulate=True),
    "c3-s1-single": dict(C=3, S=1, albedo="single", lum=False, clockwise=False, accumulate=True),
    "c3-s3-single": dict(C=3, S=3, albedo="single", lum=False, clockwise=True, accumulate=False),
    "c3-s3-vertex": dict(C=3, S=3, albedo="vertex", lum=False, clockwise=False, accumulate=True),
    "c3-s1-vertex-lum": dict(C=3, S=1, albedo="vertex", lum=True, clockwise=True, accumulate=False),
    "c1-vertex": dict(C=1, S=1, albedo="vertex", lum=False, clockwise=False, accumulate=False),
}


def rotations(n):
    return [fr.rot_x(0.3 + 0.05 * b) @ fr.rot_y(0.2 + 0.37 * b) for b in range(n)]


def inputs(case, oname):
    """seeded float64 inputs of a case under an entry of OPTIONS"""
    build, n, _why = CASES[case]
    o = OPTIONS[oname]
    vertices, faces = build()
    V, C, S = len(vertices), o["C"], o["S"]
    rs = np.random.RandomState(sum(map(ord, case + oname)))
    posed = np.stack([(vertices + 0.01 * rs.randn(V, 3)) @ r.T for r in rotations(n)])  # (a tenth of the finest mesh's spacing: no face flips)
    sh = from_directional([0.3, -0.5, 0.6], 0.25, F64)[:, None] * (1 + 0.2 * rs.randn(9, S)) + 0.1 * rs.randn(9, S)
    albedo = None if o["albedo"] is None else 0.3 + 0.6 * rs.rand(*((C,) if o["albedo"] == "single" else (V, C)))
    return {
        "faces": np.asarray(faces, dtype=np.int64), "n": n, "V": V, "posed": posed, "sh": sh, "albedo": albedo,
        "luminosity_b": rs.randn(n, V) if o["lum"] else None, "colors_b": None if albedo is None else rs.randn(n, V, C),
        "sh_b0": rs.randn(9, S), "albedo_b0": None if albedo is None else rs.randn(*albedo.shape),
    }  # fmt: skip


def reference(case, oname, dtype=LD, d=None):
    """forward and adjoint of a case -> dict; with ``accumulate`` the sums include what the outputs held before (sh_b0, albedo_b0)"""
    d, o = d or inputs(case, oname), OPTIONS[oname]
    out = forward(d["posed"], d["faces"], d["sh"], d["albedo"], o["clockwise"], dtype)
    out.update(backward(d["posed"], d["faces"], d["sh"], d["albedo"], o["clockwise"], d["luminosity_b"], d["colors_b"], dtype))
    if o["accumulate"]:
        for key in ("sh_b", "albedo_b"):
            if key in out:
                before = np.asarray(d[key + "0"], dtype=dtype)
                out[key] = (out[key][0] + before, out[key][1] + np.abs(before))
    return out
