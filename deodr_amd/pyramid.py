"""The multi-scale (pyramid) L2 data term: residuals compared at full resolution and again after summing over 2 x 2, 4 x 4, ... cells, so that a
displacement of 2^l pixels still gives a smooth pull (``include/deodr_hip_pyramid.h`` has the definition, DESIGN.md section 4i the kernels).

    q_0 = w (image - obs)       q_{l+1}(cell) = sum of its children's q_l       w_0 = w, w_{l+1} likewise
    term_l = sum over cells and channels of q_l^2 / w_l   (0 where w_l = 0)      loss = sum_l level_weights[l] term_l

``pyramid_l2`` is the differentiable scalar (in ``image`` only): the kernels on ROCm tensors (``fronthalf.PyramidL2Func``), the formulas below as
torch ops on CPU tensors and on whatever the kernels do not take.  All arithmetic is double whatever the dtype of the frames."""

import torch

from .image_terms import check_frames, device_array, uses_kernel

MAX_LEVELS = 8  # DEODR_HIP_PYRAMID_MAX_LEVELS of include/deodr_hip_pyramid.h


def check_levels(levels, what="pyramid_l2"):
    if int(levels) != levels or not 1 <= int(levels) <= MAX_LEVELS:
        raise ValueError(f"{what}: levels must be an integer in 1 .. {MAX_LEVELS}, not {levels}")
    return int(levels)


def _children_sum(x):
    """[n,H,W,...] -> [n,ceil(H/2),ceil(W/2),...]: every cell the sum of its up to four children"""
    n, H, W = x.shape[:3]
    if H % 2 or W % 2:
        padded = x.new_zeros((n, H + H % 2, W + W % 2) + tuple(x.shape[3:]))
        padded[:, :H, :W] = x
        x = padded
    return x.reshape((n, x.shape[1] // 2, 2, x.shape[2] // 2, 2) + tuple(x.shape[3:])).sum(dim=(2, 4))


def pyramid_terms_torch(image, obs, weights, levels):
    """-> [levels+1] float64: term_l of the formulas above as torch ops, differentiable in ``image``.  ``image``, ``obs`` [n,H,W,C], ``weights``
    [n,H,W] (>= 0) or None"""
    levels = check_levels(levels, "pyramid_terms")
    check_frames("pyramid_terms", image, obs, weights)
    w = torch.ones(image.shape[:3], dtype=torch.float64, device=image.device) if weights is None else weights.detach().to(torch.float64)
    q = w[..., None] * (image.to(torch.float64) - obs.detach().to(torch.float64))
    terms = []
    for level in range(levels + 1):
        if level:
            q, w = _children_sum(q), _children_sum(w)
        positive = (w > 0)[..., None]
        terms.append(torch.where(positive, q * q / torch.where(w > 0, w, torch.ones_like(w))[..., None], torch.zeros_like(q)).sum())
    return torch.stack(terms)


def _level_weights(level_weights, levels, device, what="pyramid_l2"):
    """``level_weights`` as a float64 tensor [levels+1] on ``device``: None is all ones; a tensor that already is one passes through (a schedule that is
    updated in place stays the caller's tensor)"""
    if level_weights is None:
        return torch.ones(levels + 1, dtype=torch.float64, device=device)
    return device_array(level_weights, levels + 1, device, f"{what}: level_weights must have {levels + 1} entries (levels + 1)")


def pyramid_l2_torch(image, obs, weights, levels, level_weights):
    """-> the loss (a float64 scalar tensor) as torch ops, differentiable in ``image``"""
    levels = check_levels(levels)
    return (_level_weights(level_weights, levels, image.device) * pyramid_terms_torch(image, obs, weights, levels)).sum()


def pyramid_terms(image, obs, weights=None, levels=3):
    """-> [levels+1] float64, the unweighted term_l, for display (no gradient)"""
    levels = check_levels(levels, "pyramid_terms")
    lw = _level_weights(None, levels, image.device, "pyramid_terms")
    if uses_kernel(image, obs, weights, lw):
        from . import hip_renderer as hr

        return hr.pyramid_l2(image.detach(), obs, weights, levels, lw, want_gradient=False)[0]
    with torch.no_grad():
        return pyramid_terms_torch(image, obs, weights, levels)


def pyramid_l2(image, obs, weights=None, levels=3, level_weights=None):
    """-> ``sum_l level_weights[l] term_l`` as a float64 scalar tensor, differentiable in ``image`` only (``obs``, ``weights``, ``level_weights`` are
    constants).  ``level_weights`` None: all ones; a float64 tensor on the device of ``image`` is read by the kernels when they run, so a captured
    graph sees what was copied into it since."""
    levels = check_levels(levels)
    check_frames("pyramid_l2", image, obs, weights)
    lw = _level_weights(level_weights, levels, image.device)
    if uses_kernel(image, obs, weights, lw):
        from . import fronthalf

        return fronthalf.PyramidL2Func.apply(image, obs, weights, lw, levels)
    return pyramid_l2_torch(image, obs, weights, levels, lw)
