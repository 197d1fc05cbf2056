"""A linear basis as a differentiable map on the device: ``coefficients [K] -> mean + coefficients . components`` -- the morphable models a
differentiable renderer is most often fitted with (a PCA / blend-shape model of a hand or a face, an eigen-texture: the reference's
deodr/examples/eigen_faces.py).

``components`` is [K, *shape] (the layout of a PCA's ``components_``), ``mean`` [*shape].  The tables are kept on the device once, in float32 or
float64.  On ROCm tensors the map is ``deodr_hip_basis_apply`` and its backward ``deodr_hip_basis_apply_b`` (include/deodr_hip_basis.h, kernels in
csrc/dr_basis.h): double arithmetic whatever the storage, one rounding per stored value, every sum in a fixed order -- bit-identical from run
to run, which ``torch.matmul`` does not promise.  On anything else (CPU tensors: the CPU suite) the same map as torch ops.
"""

import numpy as np
import torch


class LinearBasis:
    """``apply(coeffs)``: [K] -> [*shape], [batch, K] -> [batch, *shape]; float64 coefficients, the result in ``out_dtype`` (default float64)."""

    def __init__(self, components, mean=None, device="cuda", dtype=torch.float32):
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("LinearBasis: dtype must be torch.float32 or torch.float64")
        components = components if torch.is_tensor(components) else torch.as_tensor(np.asarray(components))
        if components.dim() < 2 or components.shape[0] < 1 or components[0].numel() < 1:
            raise ValueError(f"LinearBasis: components must be [K >= 1, *shape], not {list(components.shape)}")
        self.device, self.dtype = torch.device(device), dtype
        self.K, self.shape = int(components.shape[0]), tuple(int(v) for v in components.shape[1:])
        self.N = int(np.prod(self.shape))
        self.components = components.detach().to(device=self.device, dtype=dtype).reshape(self.K, self.N).contiguous()
        self.mean = None
        if mean is not None:
            mean = mean if torch.is_tensor(mean) else torch.as_tensor(np.asarray(mean))
            if tuple(mean.shape) != self.shape:
                raise ValueError(f"LinearBasis: mean must have shape {list(self.shape)}, not {list(mean.shape)}")
            self.mean = mean.detach().to(device=self.device, dtype=dtype).reshape(self.N).contiguous()
        self._scratch = None

    def with_mean(self, mean):
        """-> a LinearBasis of the same components (shared, not copied) with ``mean`` [*shape] in place of this one's"""
        import copy

        mean = mean if torch.is_tensor(mean) else torch.as_tensor(np.asarray(mean))
        if tuple(mean.shape) != self.shape:
            raise ValueError(f"LinearBasis: mean must have shape {list(self.shape)}, not {list(mean.shape)}")
        other = copy.copy(self)
        other.mean, other._scratch = mean.detach().to(device=self.device, dtype=self.dtype).reshape(self.N).contiguous(), None
        return other

    def scratch(self, batch=1):
        """the zero-filled scratch of the adjoint kernel this basis keeps for ``batch`` gradient vectors (made or grown at the call; used by one
        stream at a time, like the basis itself -- a captured step replays on its address)"""
        from . import hip_renderer as hr

        need = int(hr.lib().deodr_hip_basis_scratch_bytes(self.K, self.N, int(batch)))
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = hr.basis_scratch(self.K, self.N, batch, self.components.device)
        return self._scratch

    def uses_kernel(self, x):
        """whether a call on ``x`` (coefficients, or a gradient of the values) runs the library's kernel"""
        from . import hip_renderer as hr

        return (x.is_cuda and self.components.is_cuda and x.device == self.components.device and x.dtype in (torch.float32, torch.float64)
                and self.K <= hr.BASIS_MAX_K and self.N <= hr.BASIS_MAX_N and self.K * self.N <= 2**31 - 1)  # fmt: skip

    def run(self, coeffs, mean=True, out=None, out_dtype=torch.float64):
        """``mean + coeffs . components`` for ``coeffs`` [batch, K] -> [batch, N]; no autograd.  ``out``: written in place (kernel path)"""
        m = self.mean if mean else None
        if coeffs.shape[0] and self.uses_kernel(coeffs):
            from . import hip_renderer as hr

            c, step = coeffs.to(torch.float64).contiguous(), hr.BASIS_MAX_BATCH
            if c.shape[0] <= step:
                return hr.basis_apply(self.components, m, c, out=out, out_dtype=out_dtype)
            if out is None:
                out = torch.empty((c.shape[0], self.N), dtype=out_dtype, device=c.device)
            for b in range(0, c.shape[0], step):  # (the library takes 64 coefficient vectors per call)
                hr.basis_apply(self.components, m, c[b : b + step], out=out[b : b + step])
            return out
        y = coeffs.to(torch.float64) @ self.components.to(device=coeffs.device, dtype=torch.float64)
        if m is not None:
            y = y + m.to(device=coeffs.device, dtype=torch.float64)
        y = y.to(out_dtype if out is None else out.dtype)
        return y if out is None else out.copy_(y)

    def run_b(self, g, out=None, accumulate=False, scratch=None):
        """``g . components^T`` for ``g`` [batch, N] -> [batch, K] float64; no autograd.  ``out`` / ``accumulate`` / ``scratch``: as basis_apply_b"""
        if g.shape[0] and self.uses_kernel(g):
            from . import hip_renderer as hr

            g, step = g.contiguous(), hr.BASIS_MAX_BATCH
            if g.shape[0] <= step:
                return hr.basis_apply_b(self.components, g, out=out, accumulate=accumulate, scratch=self.scratch(g.shape[0]) if scratch is None else scratch)
            if out is None:
                out = torch.empty((g.shape[0], self.K), dtype=torch.float64, device=g.device)
            for b in range(0, g.shape[0], step):
                hr.basis_apply_b(self.components, g[b : b + step], out=out[b : b + step], accumulate=accumulate,
                                 scratch=self.scratch(step) if scratch is None else scratch)  # fmt: skip
            return out
        c = g.to(torch.float64) @ self.components.to(device=g.device, dtype=torch.float64).T
        if out is None:
            return c
        return out.add_(c) if accumulate else out.copy_(c)

    def apply(self, coeffs, out_dtype=torch.float64):
        """[K] or [batch, K] float64 coefficients -> [*shape] or [batch, *shape] in ``out_dtype``; differentiable any number of times"""
        if coeffs.dim() not in (1, 2) or int(coeffs.shape[-1]) != self.K:
            raise ValueError(f"LinearBasis: expected coefficients [{self.K}] or [batch, {self.K}], got {list(coeffs.shape)}")
        y = _BasisApply.apply(coeffs.reshape(-1, self.K), self, True, out_dtype)
        return y.reshape(*coeffs.shape[:-1], *self.shape)

    def apply_b(self, g):
        """the adjoint as a differentiable map: [*shape] or [batch, *shape] -> [K] or [batch, K] float64"""
        lead = g.shape[: g.dim() - len(self.shape)]
        if tuple(g.shape[len(lead) :]) != self.shape or len(lead) > 1:
            raise ValueError(f"LinearBasis: expected values {list(self.shape)} or [batch, ...], got {list(g.shape)}")
        return _BasisApplyB.apply(g.reshape(-1, self.N), self).reshape(*lead, self.K)


class _BasisApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coeffs, basis, mean, out_dtype):
        ctx.basis, ctx.dtype = basis, coeffs.dtype
        return basis.run(coeffs, mean=mean, out_dtype=out_dtype)

    @staticmethod
    def backward(ctx, y_b):
        return _BasisApplyB.apply(y_b, ctx.basis).to(ctx.dtype), None, None, None


class _BasisApplyB(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, basis):
        ctx.basis, ctx.dtype = basis, g.dtype
        return basis.run_b(g)

    @staticmethod
    def backward(ctx, c_b):  # (linear: the backward of the backward is apply again, without the mean)
        return _BasisApply.apply(c_b, ctx.basis, False, ctx.dtype), None
