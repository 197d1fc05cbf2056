"""The structural data term: ``1 - SSIM`` under an 11 x 11 Gaussian window, mixed with the pixel term, for fits against photographs whose absolute
intensities the rendering cannot match (``include/deodr_hip_ssim.h`` has the definition, DESIGN.md section 4j the kernels).

    mx = G*x   my = G*y   sxx = G*x^2 - mx^2   syy = G*y^2 - my^2   sxy = G*xy - mx my          C1 = (0.01 R)^2   C2 = (0.03 R)^2
    SSIM = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sxx + syy + C2))                     per pixel and channel
    term_0 = sum w (x - y)^2      term_1 = sum w (1 - SSIM)      loss = mix[0] term_0 + mix[1] term_1

``G`` is applied per view and per channel with ZERO PADDING (``conv2d(padding=5)``): a window over the border of the frame sees zeros in both images.
The weights multiply the SSIM MAP and do not enter the windows: a window next to a hole in the weights still sees the observation inside the hole,
and the gradient is in general not 0 where ``w = 0``.  A caller who needs more dilates the mask by 5 pixels.

``ssim_l2`` is the differentiable scalar (in ``image`` only): the kernels on ROCm tensors (``fronthalf.SSIML2Func``), the formulas below as torch ops
on CPU tensors and on whatever the kernels do not take.  All arithmetic is double whatever the dtype of the frames."""

import math

import torch
import torch.nn.functional as F

from .image_terms import check_frames, device_array, uses_kernel

WINDOW = 11  # DEODR_HIP_SSIM_WINDOW of include/deodr_hip_ssim.h
SIGMA = 1.5


def gaussian_window():
    """-> the WINDOW taps of the normalised Gaussian as Python floats, evaluated in double: the digits of SSIM_TAPS in deodr_amd/csrc/dr_ssim.h"""
    e = [math.exp(-(k * k) / (2 * SIGMA * SIGMA)) for k in range(-(WINDOW // 2), WINDOW // 2 + 1)]
    total = sum(e)
    return [v / total for v in e]


def check_data_range(data_range, what="ssim_l2"):
    data_range = float(data_range)
    if not (data_range > 0 and data_range < math.inf):
        raise ValueError(f"{what}: data_range must be finite and > 0, not {data_range}")
    return data_range


_windows = {}  # device -> the taps as a float64 tensor (made once: a stream that is being captured into a graph cannot copy them from the host)


def _windowed(t):
    """[N,1,H,W] float64 -> G*t, the window along the rows and then down the columns, zero padding"""
    if t.device not in _windows:
        _windows[t.device] = torch.tensor(gaussian_window(), dtype=torch.float64, device=t.device)
    g, half = _windows[t.device], WINDOW // 2
    return F.conv2d(F.conv2d(t, g.view(1, 1, 1, WINDOW), padding=(0, half)), g.view(1, 1, WINDOW, 1), padding=(half, 0))


def ssim_map_torch(image, obs, data_range=1.0):
    """-> SSIM [n,H,W,C] float64 of the formulas above as torch ops, differentiable in ``image``"""
    R = check_data_range(data_range, "ssim_map")
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    n, H, W, C = image.shape
    planes = lambda t: t.to(torch.float64).permute(0, 3, 1, 2).reshape(n * C, 1, H, W)
    x, y = planes(image), planes(obs.detach())
    mx, my = _windowed(x), _windowed(y)
    sxx, syy, sxy = _windowed(x * x) - mx * mx, _windowed(y * y) - my * my, _windowed(x * y) - mx * my
    ssim = (2 * mx * my + C1) * (2 * sxy + C2) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    return ssim.reshape(n, C, H, W).permute(0, 2, 3, 1)


def ssim_terms_torch(image, obs, weights=None, data_range=1.0):
    """-> [2] float64: (sum w (image - obs)^2, sum w (1 - SSIM)) as torch ops, differentiable in ``image``.  ``image``, ``obs`` [n,H,W,C], ``weights``
    [n,H,W] (>= 0) or None"""
    check_frames("ssim_terms", image, obs, weights)
    w = torch.ones(image.shape[:3], dtype=torch.float64, device=image.device) if weights is None else weights.detach().to(torch.float64)
    d = image.to(torch.float64) - obs.detach().to(torch.float64)
    return torch.stack(((w[..., None] * d * d).sum(), (w[..., None] * (1 - ssim_map_torch(image, obs, data_range))).sum()))


def _mix(mix, device, what="ssim_l2"):
    """``mix`` as a float64 tensor [2] on ``device``: None is (0, 1); a tensor that already is one passes through (a mix that is updated in place
    stays the caller's tensor)"""
    if mix is None:
        return torch.tensor([0.0, 1.0], dtype=torch.float64, device=device)
    return device_array(mix, 2, device, f"{what}: mix must have 2 entries (alpha, beta)")


def ssim_l2_torch(image, obs, weights=None, mix=None, data_range=1.0):
    """-> the loss (a float64 scalar tensor) as torch ops, differentiable in ``image``"""
    return (_mix(mix, image.device) * ssim_terms_torch(image, obs, weights, data_range)).sum()


def ssim_terms(image, obs, weights=None, data_range=1.0):
    """-> [2] float64, the unweighted (term_0, term_1), for display (no gradient)"""
    check_frames("ssim_terms", image, obs, weights)
    data_range = check_data_range(data_range, "ssim_terms")
    m = _mix(None, image.device, "ssim_terms")
    if uses_kernel(image, obs, weights, m):
        from . import hip_renderer as hr

        return hr.ssim_l2(image.detach(), obs, weights, m, data_range, want_gradient=False)[0]
    with torch.no_grad():
        return ssim_terms_torch(image, obs, weights, data_range)


def ssim_l2(image, obs, weights=None, mix=None, data_range=1.0):
    """-> ``mix[0] term_0 + mix[1] term_1`` as a float64 scalar tensor, differentiable in ``image`` only (``obs``, ``weights``, ``mix`` are constants).
    ``mix`` None: (0, 1); a float64 tensor [2] on the device of ``image`` passes through untouched and is read by the kernels when they run, so a
    captured graph sees what was copied into it since.  The weights multiply the SSIM map and do not enter the windows (the module's docstring)."""
    check_frames("ssim_l2", image, obs, weights)
    data_range = check_data_range(data_range)
    m = _mix(mix, image.device)
    if uses_kernel(image, obs, weights, m):
        from . import fronthalf

        return fronthalf.SSIML2Func.apply(image, obs, weights, m, data_range)
    return ssim_l2_torch(image, obs, weights, m, data_range)
