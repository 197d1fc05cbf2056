"""Low-order spherical-harmonic (SH) lighting and per-vertex albedo: the formulas as torch ops.

With ``N = (x, y, z)`` the unit vertex normal (``MeshTopology.vertex_normals``), the nine real SH basis functions of bands 0 to 2 are ::

    Y0 = c0      Y1 = c1 y    Y2 = c1 z    Y3 = c1 x
    Y4 = c2 x y  Y5 = c2 y z  Y6 = c3 (3 z^2 - 1)  Y7 = c2 x z  Y8 = c4 (x^2 - y^2)
    c0 = 1/(2 sqrt(pi))  c1 = sqrt(3)/(2 sqrt(pi))  c2 = sqrt(15)/(2 sqrt(pi))  c3 = sqrt(5)/(4 sqrt(pi))  c4 = sqrt(15)/(4 sqrt(pi))

the irradiance is ``E[b,v,c] = sum_k sh[k, min(c, S-1)] Y_k(N[b,v])`` (``sh`` [9,S], S = 1 or C; not clamped, so that a fit is differentiable
everywhere) and the colours are ``albedo[v,c] E[b,v,c]``.  The kernels of ``deodr_amd/csrc/dr_lighting.h`` (``fronthalf.SHShadeFunc``) compute the
same; what is here runs on tensors those do not take (the CPU suite) and is what they are tested against."""

import math

import torch

C0 = 1 / (2 * math.sqrt(math.pi))
C1 = math.sqrt(3) / (2 * math.sqrt(math.pi))
C2 = math.sqrt(15) / (2 * math.sqrt(math.pi))
C3 = math.sqrt(5) / (4 * math.sqrt(math.pi))
C4 = math.sqrt(15) / (4 * math.sqrt(math.pi))
# the clamped-cosine lobe max(0, cos) in zonal harmonics, per band (Ramamoorthi & Hanrahan 2001): what turns radiance coefficients into irradiance
LOBE = (math.pi, 2 * math.pi / 3, math.pi / 4)
_BAND = (0, 1, 1, 1, 2, 2, 2, 2, 2)


def sh_basis(normals):
    """normals [..., 3] -> Y [..., 9] (the normals are taken as they are: x, y, z are free variables of the polynomials)"""
    x, y, z = normals.unbind(-1)
    return torch.stack((C0 * torch.ones_like(x), C1 * y, C1 * z, C1 * x, C2 * (x * y), C2 * (y * z), C3 * (3 * (z * z) - 1), C2 * (x * z),
                        C4 * (x * x - y * y)), dim=-1)  # fmt: skip


def sh_irradiance(normals, sh):
    """normals [..., 3], sh [9] | [9,S] -> E [...] | [..., S]"""
    return sh_basis(normals) @ sh


def sh_shade_torch(posed, topology, sh, albedo=None):
    """posed [n,V,3] (or [V,3]), sh [9] | [9,S], albedo None | [C] | [V,C] -> luminosity [n,V] (no albedo; S = 1) or colors [n,V,C]"""
    e = sh_irradiance(topology.vertex_normals(posed), sh)
    if albedo is None:
        if e.dim() == posed.dim():
            if e.shape[-1] != 1:
                raise ValueError("sh_shade_torch: a luminosity needs one column of SH coefficients")
            e = e[..., 0]
        return e
    return albedo * (e[..., None] if sh.dim() == 1 else e)


def sh_from_directional(light_directional, ambient=0.0):
    """-> sh [9], the order-2 approximation of ``max(0, -N . L) + ambient``: the clamped-cosine lobe (band factors pi, 2 pi / 3, pi / 4) around
    ``-L / |L|``, scaled by ``|L|``, the ambient term in band 0.  A fit of SH lighting can start from the directional lighting it had.
    Differentiable in both arguments; a zero (or None) light gives exactly ``(ambient / c0, 0, ..., 0)``."""
    if light_directional is None:
        ambient = torch.as_tensor(ambient, dtype=torch.float64)
        light_directional = torch.zeros(3, dtype=ambient.dtype, device=ambient.device)
    light = torch.as_tensor(light_directional)
    norm = light.norm()
    towards = -light / torch.where(norm > 0, norm, torch.ones_like(norm))
    lobe = torch.tensor([LOBE[band] for band in _BAND], dtype=light.dtype, device=light.device)
    sh = lobe * sh_basis(towards) * norm
    band0 = torch.zeros_like(sh)
    band0[0] = 1 / C0
    return sh + band0 * ambient
