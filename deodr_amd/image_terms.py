"""What the image data terms (``pyramid.py``, ``ssim.py``) ask of their arguments alike."""

import torch


def check_frames(what, image, obs, weights):
    if image.dim() != 4 or image.shape != obs.shape or (weights is not None and tuple(weights.shape) != tuple(image.shape[:3])):
        raise ValueError(f"{what}: expected image and obs [n,H,W,C] and weights [n,H,W], not {list(image.shape)}, {list(obs.shape)}"
                         + (f" and {list(weights.shape)}" if weights is not None else ""))  # fmt: skip


def device_array(values, length, device, refusal):
    """a term's small parameter array as a float64 tensor [length] on ``device``: a tensor that already is one passes through (an array that is updated
    in place stays the caller's tensor); anything of another length: ValueError(``refusal``, then its shape)"""
    t = values if torch.is_tensor(values) else torch.as_tensor(values, dtype=torch.float64)
    if t.dim() != 1 or t.numel() != length:
        raise ValueError(f"{refusal}, not shape {list(t.shape)}")
    return t.detach().to(device=device, dtype=torch.float64)


def uses_kernel(image, obs, weights, array):
    """whether a term runs the kernels on these tensors: contiguous ROCm tensors of one float32 / float64 dtype on one device, ``array`` float64"""
    frames = [image, obs] + ([] if weights is None else [weights])
    return (all(torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and t.device == image.device for t in frames + [array])
            and image.dtype in (torch.float32, torch.float64) and all(t.dtype == image.dtype for t in frames) and array.dtype == torch.float64
            and image.dim() == 4 and image.numel() > 0)  # fmt: skip
