"""Host side of the HIP rasterizer: ctypes binding of ``libdeodr_hip.so`` (C ABI in ``include/deodr_hip.h``).

Two levels, both without any CPU fallback (a missing library or a missing GPU raises):

* :class:`DeviceScene` + :class:`HipRasterizer` -- the device-resident path: PyTorch-ROCm tensors in, PyTorch-ROCm tensors
  out, nothing crosses PCIe, calls are asynchronous on the current torch stream, ``n_views`` views per launch.
* :func:`renderSceneCpp` / :func:`renderSceneBCpp` -- drop-in replacements of the reference's Cython entry points
  (deodr/differentiable_renderer_cython.pyx:50-57 and :206-215): duck-typed ``scene`` with NumPy (or CPU torch) arrays,
  caller-owned float64 output buffers written in place, ``scene.*_b`` rebound to ``old + new`` (pyx:406-410).  They copy to
  the GPU, run the same kernels with float64 storage and copy back; the call is complete on return.

torch is used for device memory and streams only.
"""

import ctypes as C
import os
from collections import namedtuple

import numpy as np
import torch

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libdeodr_hip.so")
_H = _abi.HEADER  # the structs, the constants and (in lib()) the signatures are read from include/deodr_hip.h: deodr_amd/_abi.py
_SceneC, _FitOptionsC, ABI_VERSION = _H.structs["DeodrHipScene"], _H.structs["DeodrHipFitOptions"], _H.defines["DEODR_HIP_ABI_VERSION"]
ERR_FACES, ERR_FACES_UV, ERR_NO_TEXTURE, ERR_INTERNAL, ERR_DET_RANGE = (_H.defines["DEODR_HIP_ERR_" + n] for n in "FACES FACES_UV NO_TEXTURE INTERNAL DET_RANGE".split())
MAX_COLORS, _F32, _F64 = (_H.defines["DEODR_HIP_" + n] for n in ("MAX_COLORS", "F32", "F64"))
for _c in _abi.COMPANIONS + _abi.STAGED:  # TEXTURE_ABI_VERSION, SUBDIV_ABI_VERSION, ...: of the companion headers, each versioned on its own
    globals()[_c.key.upper() + "_ABI_VERSION"] = _abi.companion(_c)[1]
# words of the 64-byte status block at the start of the workspace
_STATUS_NEEDED, _STATUS_ERRORS = _H.defines["DEODR_HIP_STATUS_WORD_NEEDED_PAIRS"], _H.defines["DEODR_HIP_STATUS_WORD_SCENE_ERRORS"]

_lib = None


def lib():
    """The HIP library, every function of the header bound; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). deodr_amd has no CPU fallback."
            )
        L = C.CDLL(LIB_PATH)
        if L.deodr_hip_abi_version() != ABI_VERSION:
            raise ImportError("libdeodr_hip.so ABI version mismatch; rebuild it")
        for c in _abi.COMPANIONS + _abi.STAGED:  # bound onto the same library
            header, version = _abi.companion(c)
            _abi.bind(L, header)  # (a library that lacks one of its symbols is refused by name)
            if getattr(L, f"deodr_hip_{c.key}_abi_version")() != version:
                raise ImportError(f"libdeodr_hip.so {c.words} ABI version mismatch ({header.name}); rebuild it")
        _lib = _abi.bind(L)
    return _lib


def set_deterministic(on):
    """``deodr_hip_set_deterministic``: integer accumulation on the un-staged kernels -- gradients bit-identical from run to run (slow;
    for tests and for debugging an optimiser).  Process-wide; ``DeviceScene(deterministic=True)`` asks for it per scene."""
    lib().deodr_hip_set_deterministic(int(bool(on)))


def wait_flag(flag, value, status=None, timeout=1.0, stream=None):
    """``deodr_hip_wait_flag``: the current stream of ``flag``'s device (or ``stream``) waits until ``flag`` (a 4-byte integer tensor a fit step
    was given as ``done_flag``) has reached ``value``.  The step must have been queued before this call.  ``status``: a 4-byte tensor set to 1 by a
    wait that gave up after ``timeout`` seconds (check it where you synchronise)."""
    dev = flag.device
    with torch.cuda.device(dev):
        _check(lib().deodr_hip_wait_flag(_ptr(flag), int(value) & 0xFFFFFFFF, _ptr(status), float(timeout),
                                         C.c_void_p(stream.cuda_stream) if stream is not None else _stream(dev)))  # fmt: skip


def force_generic(on):
    """Test hook (``deodr_hip_force_generic``): route every call through the un-staged kernels.  Process-wide."""
    lib().deodr_hip_force_generic(int(bool(on)))


def tile_census(rasterizer, ds):
    """(tiles with a primitive, tiles with silhouette edges) of the last forward on `rasterizer`, over all views (synchronises)."""
    a, b = C.c_ulonglong(0), C.c_ulonglong(0)
    with torch.cuda.device(rasterizer.device):
        _check(lib().deodr_hip_workspace_census(C.byref(ds.c_struct()), _ptr(rasterizer.workspace), rasterizer.nbytes, _stream(rasterizer.device),
                                                C.byref(a), C.byref(b)))  # fmt: skip
    return int(a.value), int(b.value)


def scene_error_message(bits):
    what = []
    if bits & ERR_FACES:
        what.append("an entry of scene.faces is >= the number of vertices")
    if bits & ERR_FACES_UV:
        what.append("an entry of scene.faces_uv is >= the number of uv vertices")
    if bits & ERR_NO_TEXTURE:
        what.append("a triangle is textured and shaded but the scene has no texture")
    if bits & ERR_INTERNAL:
        what.append("internal: a finalize workgroup of a fit step gave up waiting for the tile walkers (gradients incomplete)")
    det = ("deterministic mode: a gradient contribution or running sum of the last deterministic adjoint left the fixed-point range +- 2^31 "
           "(the gradients of that call are wrong; the bit is cleared when the next deterministic adjoint starts)")
    if bits & ERR_DET_RANGE and not what:
        return det  # (not a statement about the scene)
    if bits & ERR_DET_RANGE:
        what.append(det)
    return "invalid scene (checkSceneValid): " + "; ".join(what)


def _check(rc):
    if rc:
        raise RuntimeError("deodr_hip: " + lib().deodr_hip_last_error().decode())


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _launch(function, device, *args):
    """one call of the library on the current stream of `device` (every function that launches takes the stream last)"""
    with torch.cuda.device(device):
        _check(function(*args, _stream(device)))


def _dtype_tag(t):
    """the dtype tag of include/deodr_hip.h for a float32 / float64 tensor"""
    return _F64 if t.dtype == torch.float64 else _F32


def _resolve_device(device):
    """the ROCm device a scene or a workspace lives on (there is no CPU path: anything else is refused)"""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("deodr_amd needs a ROCm device; there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _count(a):
    """number of elements of an array OR a tensor (np.size of a tensor is its bound `size` method, not a number)"""
    return 0 if a is None else int(a.numel()) if torch.is_tensor(a) else int(np.size(a))


def _as_tensor(a):
    return a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))


def _tensor(a, device, dtype):
    """an array or a tensor as a contiguous tensor of `dtype` on `device` (the tensor itself when it already is one)"""
    return _as_tensor(a).to(device=device, dtype=dtype).contiguous()


def _on(t, device, dtype, shape, what):
    """`t` as a contiguous tensor of `dtype` on `device` with `shape` (no copy when it already is one)."""
    t = _tensor(t, device, dtype)
    if tuple(t.shape) != tuple(shape):
        if t.numel() != int(np.prod(shape)):
            raise ValueError(f"{what}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        t = t.reshape(shape)
    return t


def _pixels(t, ds):
    """an observation or residual target as [n,H,W,C] in the pixel dtype on the scene's device; a tensor that already is that passes
    through untouched (the loss-table cache keys on its identity)"""
    shape = (ds.n_views, ds.height, ds.width, ds.nb_colors)
    t = _tensor(t, ds.device, ds.pixel_dtype)
    return t if tuple(t.shape) == shape else t.expand(shape).contiguous()  # pass [n,H,W,C] to avoid this copy


# ---- what the operator wrappers below share: one checker of tensor arguments, one cache of scratch buffers --------------------------------

_FLOATS = (torch.float32, torch.float64)
_NO_CPU = "(deodr_amd has no CPU path)"


def _rocm_tensor(what, name, t):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{what}: {name} must be a ROCm tensor {_NO_CPU}")


def _check_tensors(what, anchor, device, rows):
    """checks before the library is called.  ``rows`` [(name, tensor, dtypes, shape[, says])]: each a ROCm tensor on ``device`` (that of the argument
    called ``anchor``), of one of ``dtypes``, of ``shape`` (None: any shape; an entry None: any size, printed as "batch"), contiguous -- checked in
    this order, row by row.  ``says``: the one sentence a row gives for everything but contiguity, where the wrapper has always had one."""
    for name, t, dtypes, shape, *says in rows:
        said = f"{what}: {says[0]}" if says else None
        if not torch.is_tensor(t) or not t.is_cuda or t.device != device:
            raise ValueError(said or f"{what}: {name} must be a ROCm tensor on the device of {anchor} {_NO_CPU}")
        if t.dtype not in dtypes:
            raise ValueError(said or f"{what}: {name} must be {' or '.join(str(d).replace('torch.', '') for d in dtypes)}, not {t.dtype}")
        if shape is not None and (t.dim() != len(shape) or any(want is not None and int(have) != want for have, want in zip(t.shape, shape))):
            raise ValueError(said or f"{what}: {name} must have shape [{', '.join('batch' if v is None else str(v) for v in shape)}], not {list(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous")


_scratch_cache = {}  # (whose, device, stream) -> a zero-filled scratch of the library, grown to the largest request


def _own_or_cached_scratch(what, scratch, whose, device, need, make, *dims):
    """``scratch`` where the caller of ``what`` gave one.  None: the scratch the kernels of the family ``whose`` use on the current stream of
    ``device``, at least ``need`` bytes (a number, or the library's ``*_scratch_bytes`` to ask for ``dims``): made (``make(*dims, device)``) or
    grown at the call, which a stream that is being captured into a graph cannot do -- RuntimeError"""
    if scratch is not None:
        return scratch
    need = int(need(*dims)) if callable(need) else need
    key = (whose, device, torch.cuda.current_stream(device).cuda_stream)
    scratch = _scratch_cache.get(key)
    if scratch is None or scratch.numel() < need:
        if torch.cuda.is_current_stream_capturing():
            sized = " of this size" if dims else ""  # (a scratch without dimensions has one size)
            raise RuntimeError(f"{what}: pass scratch= ({make.__name__}) when capturing a graph: none{sized} exists for this stream yet")
        scratch = _scratch_cache[key] = make(*dims, device)
    return scratch


def _include(header):
    """the path in the repository of a header of the C ABI, for error texts: a staged companion is in include_staged/"""
    return ("include_staged/" if any(header == f"deodr_hip_{c.key}.h" for c in _abi.STAGED) else "include/") + header


def _byte_scratch(what, dims, need, header, device, zeroed=False):
    """``need`` bytes (what the library's ``*_scratch_bytes`` gave for ``dims``; 0: refused) of scratch on ``device``, uninitialised or ``zeroed``"""
    if need == 0:
        raise ValueError(f"{what}: {dims} is outside the limits of {_include(header)}")
    with torch.cuda.device(device):
        return (torch.zeros if zeroed else torch.empty)(int(need), dtype=torch.uint8, device=device)


# ---- texture estimation (include/deodr_hip_texture.h) ---------------------------------------------------------------------------------


def _texture_args(what, texture, others):
    """checks before the library is called: a [Ht,Wt,C] float32 / float64 contiguous ROCm tensor, `others` {name: tensor} of its shape, dtype and device;
    -> (Ht, Wt, C, dtype tag)"""
    _rocm_tensor(what, "texture", texture)
    if texture.dim() != 3 or texture.shape[0] < 2 or texture.shape[1] < 2 or not 1 <= texture.shape[2] <= MAX_COLORS:
        raise ValueError(f"{what}: texture must have shape [Ht >= 2, Wt >= 2, 1 <= C <= {MAX_COLORS}], not {list(texture.shape)}")
    shape = tuple(int(v) for v in texture.shape)
    rows = [("texture", texture, _FLOATS, None)]
    rows += [(name, t, (texture.dtype,), shape, f"{name} must be a tensor of the texture's shape, dtype and device") for name, t in others.items()]
    _check_tensors(what, "texture", texture.device, rows)
    return (*shape, _dtype_tag(texture))


def texture_scratch(device):
    """the scratch of :func:`texture_smoothness`, zero-filled as the library wants it once; for a caller that keeps its own (one per stream in use)"""
    need = lib().deodr_hip_texture_scratch_bytes(2, 2, 1)  # (the size does not depend on the texture)
    return _byte_scratch("texture_scratch", "", need, "deodr_hip_texture.h", device, zeroed=True)


def texture_smoothness(texture, gradient, weight, energy_out=None, scratch=None):
    """``deodr_hip_texture_smoothness``: ``E = 0.5 weight (sum of the squared differences of x- and y-neighbours)`` of ``texture`` [Ht,Wt,C], free
    boundary; ``dE/dtexture`` is ACCUMULATED into ``gradient`` (same shape and dtype -- typically the rasterizer's ``texture_b``); -> ``energy_out``
    (a float64 device tensor of one element, allocated when None) holding E.  Deterministic; asynchronous on the current stream.  ``scratch``: a
    :func:`texture_scratch` of the caller's (a fitter whose step is captured in a graph keeps one); None: one per device and stream, made at the first call."""
    what = "texture_smoothness"
    dims = _texture_args(what, texture, {"gradient": gradient})
    dev = texture.device
    with torch.cuda.device(dev):
        if energy_out is None:
            energy_out = torch.empty(1, dtype=torch.float64, device=dev)
        if energy_out.dtype != torch.float64 or energy_out.device != dev or energy_out.numel() != 1:
            raise ValueError(f"{what}: energy_out must be a float64 tensor of one element on the texture's device")
        if scratch is not None and (scratch.device != dev or scratch.dtype != torch.uint8 or not scratch.is_contiguous()):
            raise ValueError(f"{what}: scratch must be a texture_scratch() of the texture's device")
        scratch = _own_or_cached_scratch(what, scratch, "texture", dev, 0, texture_scratch)
    _launch(lib().deodr_hip_texture_smoothness, dev, _ptr(texture), *dims, float(weight), _ptr(gradient), _ptr(energy_out), _ptr(scratch), scratch.numel())
    return energy_out


def _touched(t):
    """a kernel of the library has written `t` in place: tell torch (version counters are how conversions of `t` are recognised as stale)"""
    bump = getattr(torch.autograd.graph, "increment_version", None)
    if bump is not None:
        bump(t)


def texture_step(texture, speed, gradient, factor, step_max=None, inertia=0.0, damping=0.0, clamp=None):
    """``deodr_hip_texture_step``: ``speed = (1 - damping) (inertia speed + (1 - inertia) clip(-factor gradient, +-step_max))``, ``texture += speed``,
    IN PLACE on ``texture`` and ``speed`` (``_Momentum.update`` for a pixel-typed array); ``clamp`` = (lo, hi): the texture is clipped to it and the
    speed set to 0 where it clipped.  ``gradient`` is only read.  Asynchronous on the current stream."""
    dims = _texture_args("texture_step", texture, {"speed": speed, "gradient": gradient})
    lo, hi = (0.0, 0.0) if clamp is None else (float(clamp[0]), float(clamp[1]))
    _launch(lib().deodr_hip_texture_step, texture.device, _ptr(texture), _ptr(speed), _ptr(gradient), *dims, float(factor),
            0.0 if step_max is None else float(step_max), float(inertia), float(damping), int(clamp is not None), lo, hi)  # fmt: skip
    _touched(texture), _touched(speed)


# ---- Loop subdivision (include/deodr_hip_subdiv.h) ------------------------------------------------------------------------------------

_INDICES = (torch.int32, torch.uint32)


def sparse_rows_lanes(n_rows, nnz):
    """``deodr_hip_subdiv_lanes``: the kernel instance :func:`sparse_rows_apply` runs for a matrix of ``n_rows`` rows and ``nnz`` entries -- 8 adjacent
    lanes per row, or 64 (a wavefront per row)"""
    return int(lib().deodr_hip_subdiv_lanes(int(n_rows), int(nnz)))


def sparse_rows_apply(offsets, cols, vals, x, out=None, accumulate=False):
    """``deodr_hip_subdiv_apply``: ``out[b, r, :] (= | +=) sum_k vals[k] x[b, cols[k], :]`` over the entries ``k`` of row ``r`` of a matrix in compressed
    rows -- ``offsets`` [rows + 1] and ``cols`` [nnz] as 4-byte integer tensors (uint32 bit patterns), ``vals`` [nnz] float64.  ``x`` [batch, n_cols, D]
    float32 / float64 -> ``out`` [batch, rows, D] of the same dtype (allocated when None).  Deterministic; asynchronous on the current stream.
    The tables are trusted (``offsets`` non-decreasing from 0 to nnz, ``cols`` < n_cols): :class:`deodr_amd.subdivision.LoopSubdivision` checks its
    own on the host when it builds them."""
    what = "sparse_rows_apply"
    for name, t in (("offsets", offsets), ("cols", cols), ("vals", vals), ("x", x)):  # (all four are tensors before anything is asked of one of them)
        _rocm_tensor(what, name, t)
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous")
        if t.device != x.device:
            raise ValueError(f"{what}: {name} must be on the device of x")
    tables = "offsets and cols must be one-dimensional 4-byte integer tensors"
    _check_tensors(what, "x", x.device, [
        ("offsets", offsets, _INDICES, (None,), tables), ("cols", cols, _INDICES, (None,), tables),
        ("vals", vals, (torch.float64,), tuple(cols.shape), "vals must be a float64 tensor of the shape of cols"), ("x", x, _FLOATS, None),
    ])  # fmt: skip
    if x.dim() != 3 or not 1 <= x.shape[2] <= MAX_COLORS or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{what}: x must have shape [batch >= 1, n_cols >= 1, 1 <= D <= {MAX_COLORS}], not {list(x.shape)}")
    n_rows, nnz = int(offsets.numel()) - 1, int(cols.numel())
    if n_rows < 1 or nnz < 1:
        raise ValueError(f"{what}: the matrix has no rows or no entries")
    batch, n_cols, D = (int(v) for v in x.shape)
    dev = x.device
    if out is None:
        if accumulate:
            raise ValueError(f"{what}: accumulate needs out")
        with torch.cuda.device(dev):
            out = torch.empty((batch, n_rows, D), dtype=x.dtype, device=dev)
    elif not torch.is_tensor(out) or out.device != dev or out.dtype != x.dtype or tuple(out.shape) != (batch, n_rows, D) or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous {x.dtype} tensor of shape {[batch, n_rows, D]} on the device of x")
    _launch(lib().deodr_hip_subdiv_apply, dev, _ptr(offsets), _ptr(cols), _ptr(vals), n_rows, n_cols, nnz, _ptr(x), _ptr(out), batch, D, _dtype_tag(x),
            int(bool(accumulate)))  # fmt: skip
    if accumulate:
        _touched(out)
    return out


# ---- linear bases (include/deodr_hip_basis.h) -----------------------------------------------------------------------------------------

BASIS_MAX_K, BASIS_MAX_BATCH, BASIS_MAX_N = 1024, 64, 2**30  # the limits include/deodr_hip_basis.h states


def _basis_args(what, basis, tensors):
    """checks before the library is called: ``basis`` a contiguous [K, N] float32 / float64 ROCm tensor within the header's limits; ``tensors``: rows
    of :func:`_check_tensors`, tensors on its device; -> (K, N)"""
    _rocm_tensor(what, "basis", basis)
    if basis.dtype not in _FLOATS:
        raise ValueError(f"{what}: basis must be float32 or float64, not {basis.dtype}")
    if basis.dim() != 2 or not 1 <= basis.shape[0] <= BASIS_MAX_K or not 1 <= basis.shape[1] <= BASIS_MAX_N or basis.numel() > 2**31 - 1:
        raise ValueError(f"{what}: basis must have shape [1 <= K <= {BASIS_MAX_K}, 1 <= N <= 2^30] with K N <= 2^31 - 1, not {list(basis.shape)}")
    if not basis.is_contiguous():
        raise ValueError(f"{what}: basis must be contiguous")
    _check_tensors(what, "basis", basis.device, tensors)
    return int(basis.shape[0]), int(basis.shape[1])


def _basis_batch(what, t):
    if not 1 <= int(t.shape[0]) <= BASIS_MAX_BATCH:
        raise ValueError(f"{what}: batch must be in 1 .. {BASIS_MAX_BATCH}, not {int(t.shape[0])}")
    return int(t.shape[0])


def basis_segments(K, N):
    """``deodr_hip_basis_segments``: the number of pieces into which :func:`basis_apply_b` cuts a row of a [K, N] basis (0: outside the limits)"""
    return int(lib().deodr_hip_basis_segments(int(K), int(N)))


def basis_scratch(K, N, batch, device):
    """the scratch of :func:`basis_apply_b` for a [K, N] basis and ``batch`` gradient vectors, zero-filled as the library wants it once; for a
    caller that keeps its own (one per stream in use; a fitter whose step is captured in a graph)"""
    need = lib().deodr_hip_basis_scratch_bytes(int(K), int(N), int(batch))
    return _byte_scratch("basis_scratch", f"K = {K}, N = {N}, batch = {batch}", need, "deodr_hip_basis.h", device, zeroed=True)


def basis_apply(basis, mean, coeffs, out=None, out_dtype=None):
    """``deodr_hip_basis_apply``: ``out[b, j] = mean[j] + sum_k coeffs[b, k] basis[k, j]``.  ``basis`` [K, N] float32 / float64, ``mean`` [N] of its
    dtype or None (zero), ``coeffs`` [batch, K] float64 -> ``out`` [batch, N] float32 / float64 (allocated in ``out_dtype``, default float64, when
    None).  Double arithmetic, one rounding per stored value; deterministic; asynchronous on the current stream."""
    what = "basis_apply"
    if torch.is_tensor(basis) and basis.dim() == 2:
        K, N = int(basis.shape[0]), int(basis.shape[1])
    else:
        K = N = None
    tensors = [("coeffs", coeffs, (torch.float64,), (None, K))]
    if mean is not None:
        tensors.append(("mean", mean, (getattr(basis, "dtype", None),), (N,)))
    if out is not None:
        tensors.append(("out", out, _FLOATS, (None, N)))
    K, N = _basis_args(what, basis, tensors)
    batch = _basis_batch(what, coeffs)
    if out is not None and int(out.shape[0]) != batch:
        raise ValueError(f"{what}: out must have shape {[batch, N]}, not {list(out.shape)}")
    if out is None and (out_dtype or torch.float64) not in _FLOATS:
        raise ValueError(f"{what}: out_dtype must be float32 or float64, not {out_dtype}")
    dev = basis.device
    if out is None:
        with torch.cuda.device(dev):
            out = torch.empty((batch, N), dtype=out_dtype or torch.float64, device=dev)
    _launch(lib().deodr_hip_basis_apply, dev, _ptr(basis), _ptr(mean), _ptr(coeffs), K, N, batch, _dtype_tag(basis), _ptr(out), _dtype_tag(out))
    _touched(out)
    return out


def basis_apply_b(basis, g, out=None, accumulate=False, scratch=None):
    """``deodr_hip_basis_apply_b``: ``out[b, k] (= | +=) sum_j basis[k, j] g[b, j]``.  ``basis`` [K, N] float32 / float64, ``g`` [batch, N] float32 /
    float64 -> ``out`` [batch, K] float64 (allocated when None).  Deterministic (no atomics on values); asynchronous on the current stream.
    ``scratch``: a :func:`basis_scratch` of the caller's, at least as large as this problem needs; None: one per device and stream, made or
    grown at the call (not while a graph is being captured)."""
    what = "basis_apply_b"
    if torch.is_tensor(basis) and basis.dim() == 2:
        K, N = int(basis.shape[0]), int(basis.shape[1])
    else:
        K = N = None
    tensors = [("g", g, _FLOATS, (None, N))]
    if out is not None:
        tensors.append(("out", out, (torch.float64,), (None, K)))
    if scratch is not None:
        tensors.append(("scratch", scratch, (torch.uint8,), (None,)))
    K, N = _basis_args(what, basis, tensors)
    batch = _basis_batch(what, g)
    if out is None and accumulate:
        raise ValueError(f"{what}: accumulate needs out")
    if out is not None and int(out.shape[0]) != batch:
        raise ValueError(f"{what}: out must have shape {[batch, K]}, not {list(out.shape)}")
    dev = basis.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((batch, K), dtype=torch.float64, device=dev)
        scratch = _own_or_cached_scratch(what, scratch, "basis", dev, lib().deodr_hip_basis_scratch_bytes, basis_scratch, K, N, batch)
    _launch(lib().deodr_hip_basis_apply_b, dev, _ptr(basis), _ptr(g), _dtype_tag(g), K, N, batch, _dtype_tag(basis), _ptr(out), int(bool(accumulate)),
            _ptr(scratch), scratch.numel())  # fmt: skip
    _touched(out)
    return out


# ---- camera calibration (include/deodr_hip_camera.h) ----------------------------------------------------------------------------------

CAMERA_MAX_VIEWS, CAMERA_MAX_VERTICES = 64, 2**24  # the limits include/deodr_hip_camera.h states
_F64_ONLY = (torch.float64,)


def _camera_views(what, anchor_name, anchor, tail):
    """checks before the library is called: ``anchor`` a float64 ROCm tensor [n, *tail] with n within the header's limit; -> n"""
    _rocm_tensor(what, anchor_name, anchor)
    if anchor.dim() != 1 + len(tail) or not 1 <= int(anchor.shape[0]) <= CAMERA_MAX_VIEWS:
        raise ValueError(f"{what}: {anchor_name} must have shape [1 <= n <= {CAMERA_MAX_VIEWS}, {', '.join(map(str, tail))}], not {list(anchor.shape)}")
    return int(anchor.shape[0])


def camera_blocks(V, n):
    """``deodr_hip_camera_blocks``: the workgroups per view :func:`camera_project_b` launches for V vertices and n views (0: outside the limits)"""
    return int(lib().deodr_hip_camera_blocks(int(V), int(n)))


def camera_scratch(V, n, device):
    """the scratch of :func:`camera_project_b` for V vertices and n views, zero-filled as the library wants it once (one per stream in use)"""
    need = lib().deodr_hip_camera_scratch_bytes(int(V), int(n))
    return _byte_scratch("camera_scratch", f"V = {V}, n = {n}", need, "deodr_hip_camera.h", device, zeroed=True)


def camera_project_b(points, extrinsic, intrinsic, distortion, ij_b, depths_b=None, points_b=None, extrinsic_b=None, intrinsic_b=None,
                     distortion_b=None, accumulate=False, scratch=None, want_points_b=True):
    """``deodr_hip_camera_project_b``: the full adjoint of the camera projection in one launch.  ``points`` [n,V,3], ``extrinsic`` [n,3,4],
    ``intrinsic`` [n,3,3], ``distortion`` [n,5] | None, ``ij_b`` [n,V,2], ``depths_b`` [n,V] | None, all contiguous float64 ROCm tensors ->
    (points_b [n,V,3] | None, extrinsic_b [n,3,4], intrinsic_b [n,3,3], distortion_b [n,5] | None), allocated where not given (``points_b`` only
    with ``want_points_b``).  ``accumulate``: added to the three camera adjoints, which must then be given.  Deterministic; asynchronous on the
    current stream.  ``scratch``: a :func:`camera_scratch` of the caller's; None: one per device and stream, made or grown at the call."""
    what = "camera_project_b"
    n = _camera_views(what, "extrinsic", extrinsic, (3, 4))
    if not torch.is_tensor(points) or points.dim() != 3 or int(points.shape[0]) != n or int(points.shape[2]) != 3 or not 1 <= int(points.shape[1]) <= CAMERA_MAX_VERTICES:
        raise ValueError(f"{what}: points must have shape [{n}, 1 <= V <= 2^24, 3], not {list(getattr(points, 'shape', ()))}")
    V = int(points.shape[1])
    rows = [("extrinsic", extrinsic, _F64_ONLY, (n, 3, 4)), ("points", points, _F64_ONLY, (n, V, 3)), ("intrinsic", intrinsic, _F64_ONLY, (n, 3, 3)),
            ("ij_b", ij_b, _F64_ONLY, (n, V, 2))]  # fmt: skip
    optional = [("distortion", distortion, (n, 5)), ("depths_b", depths_b, (n, V)), ("points_b", points_b, (n, V, 3)), ("extrinsic_b", extrinsic_b, (n, 3, 4)),
                ("intrinsic_b", intrinsic_b, (n, 3, 3)), ("distortion_b", distortion_b, (n, 5))]  # fmt: skip
    rows += [(name, t, _F64_ONLY, shape) for name, t, shape in optional if t is not None]
    if scratch is not None:
        rows.append(("scratch", scratch, (torch.uint8,), (None,)))
    _check_tensors(what, "extrinsic", extrinsic.device, rows)
    if distortion is None and distortion_b is not None:
        raise ValueError(f"{what}: distortion_b without distortion")
    if accumulate and (extrinsic_b is None or intrinsic_b is None or (distortion is not None and distortion_b is None)):
        raise ValueError(f"{what}: accumulate needs extrinsic_b, intrinsic_b and (with distortion) distortion_b")
    dev = extrinsic.device
    with torch.cuda.device(dev):
        if points_b is None and want_points_b:
            points_b = torch.empty_like(points)
        if extrinsic_b is None:
            extrinsic_b = torch.empty((n, 3, 4), dtype=torch.float64, device=dev)
        if intrinsic_b is None:
            intrinsic_b = torch.empty((n, 3, 3), dtype=torch.float64, device=dev)
        if distortion is not None and distortion_b is None:
            distortion_b = torch.empty((n, 5), dtype=torch.float64, device=dev)
        scratch = _own_or_cached_scratch(what, scratch, "camera", dev, lib().deodr_hip_camera_scratch_bytes, camera_scratch, V, n)
    _launch(lib().deodr_hip_camera_project_b, dev, _ptr(points), _ptr(extrinsic), _ptr(intrinsic), _ptr(distortion), _ptr(ij_b), _ptr(depths_b),
            _ptr(points_b), _ptr(extrinsic_b), _ptr(intrinsic_b), _ptr(distortion_b), V, n, int(bool(accumulate)), _ptr(scratch), scratch.numel())  # fmt: skip
    for t in (points_b, extrinsic_b, intrinsic_b, distortion_b):
        if t is not None:
            _touched(t)
    return points_b, extrinsic_b, intrinsic_b, distortion_b


def _camera_parameters(what, n, shared, rows):
    """rows of :func:`_check_tensors` for focal / center / distortion-like tensors [(name, tensor | None, width)]: [width] when shared, else [n, width]"""
    return [(name, t, _F64_ONLY, (width,) if shared else (n, width)) for name, t, width in rows if t is not None]


def camera_assemble(quaternions, translations, focal, center, distortion=None, shared=True, out=None):
    """``deodr_hip_camera_assemble``: quaternions [n,4] = (x, y, z, w) (normalised inside), translations [n,3], focal and center [2] (``shared``) or
    [n,2], distortion [5] / [n,5] | None -> (extrinsic [n,3,4] = [R(q) | t], intrinsic [n,3,3], distortion [n,5] | None): the per-view matrices the
    projection kernels index.  ``out``: that triple, to be written in place.  Contiguous float64 ROCm tensors; asynchronous on the current stream."""
    what = "camera_assemble"
    n = _camera_views(what, "quaternions", quaternions, (4,))
    rows = [("quaternions", quaternions, _F64_ONLY, (n, 4)), ("translations", translations, _F64_ONLY, (n, 3))]
    rows += _camera_parameters(what, n, shared, [("focal", focal, 2), ("center", center, 2), ("distortion", distortion, 5)])
    if focal is None or center is None:
        raise ValueError(f"{what}: focal and center are required")
    e, k, d = out if out is not None else (None, None, None)
    rows += [(name, t, _F64_ONLY, shape) for name, t, shape in (("extrinsic", e, (n, 3, 4)), ("intrinsic", k, (n, 3, 3)), ("distortion out", d, (n, 5))) if t is not None]
    _check_tensors(what, "quaternions", quaternions.device, rows)
    dev = quaternions.device
    with torch.cuda.device(dev):
        e = torch.empty((n, 3, 4), dtype=torch.float64, device=dev) if e is None else e
        k = torch.empty((n, 3, 3), dtype=torch.float64, device=dev) if k is None else k
        if distortion is not None and d is None:
            d = torch.empty((n, 5), dtype=torch.float64, device=dev)
    if distortion is None:
        d = None
    _launch(lib().deodr_hip_camera_assemble, dev, _ptr(quaternions), _ptr(translations), _ptr(focal), _ptr(center), _ptr(distortion), int(bool(shared)),
            _ptr(e), _ptr(k), _ptr(d), n)  # fmt: skip
    for t in (e, k, d):
        if t is not None:
            _touched(t)
    return e, k, d


def camera_assemble_b(quaternions, extrinsic_b, intrinsic_b, distortion_b=None, shared=True, out=None):
    """``deodr_hip_camera_assemble_b``: the adjoint of :func:`camera_assemble` -> (quaternions_b [n,4] with respect to the raw quaternions,
    translations_b [n,3], focal_b, center_b, distortion_b of the parameters' shapes ([2], [2], [5] summed over the views when ``shared``) | None).
    ``out``: that quintuple, to be written in place."""
    what = "camera_assemble_b"
    n = _camera_views(what, "quaternions", quaternions, (4,))
    rows = [("quaternions", quaternions, _F64_ONLY, (n, 4)), ("extrinsic_b", extrinsic_b, _F64_ONLY, (n, 3, 4)), ("intrinsic_b", intrinsic_b, _F64_ONLY, (n, 3, 3))]
    if distortion_b is not None:
        rows.append(("distortion_b", distortion_b, _F64_ONLY, (n, 5)))
    q_b, t_b, f_b, c_b, d_b = out if out is not None else (None,) * 5
    rows += [(name, t, _F64_ONLY, shape) for name, t, shape in (("quaternions_b", q_b, (n, 4)), ("translations_b", t_b, (n, 3))) if t is not None]
    rows += _camera_parameters(what, n, shared, [("focal_b", f_b, 2), ("center_b", c_b, 2), ("distortion_in_b", d_b, 5)])
    _check_tensors(what, "quaternions", quaternions.device, rows)
    dev = quaternions.device
    width = lambda w: (w,) if shared else (n, w)
    with torch.cuda.device(dev):
        q_b = torch.empty((n, 4), dtype=torch.float64, device=dev) if q_b is None else q_b
        t_b = torch.empty((n, 3), dtype=torch.float64, device=dev) if t_b is None else t_b
        f_b = torch.empty(width(2), dtype=torch.float64, device=dev) if f_b is None else f_b
        c_b = torch.empty(width(2), dtype=torch.float64, device=dev) if c_b is None else c_b
        if distortion_b is not None and d_b is None:
            d_b = torch.empty(width(5), dtype=torch.float64, device=dev)
    if distortion_b is None:
        d_b = None
    _launch(lib().deodr_hip_camera_assemble_b, dev, _ptr(quaternions), _ptr(extrinsic_b), _ptr(intrinsic_b), _ptr(distortion_b), int(bool(shared)),
            _ptr(q_b), _ptr(t_b), _ptr(f_b), _ptr(c_b), _ptr(d_b), n)  # fmt: skip
    for t in (q_b, t_b, f_b, c_b, d_b):
        if t is not None:
            _touched(t)
    return q_b, t_b, f_b, c_b, d_b


class DeviceScene:
    """The arrays of ``struct Scene`` (reference H.h:56-90) as contiguous ROCm tensors, for ``n_views`` views of one mesh.

    Shapes: faces / faces_uv ``[T,3] int32|uint32``; textured / shaded ``[T] uint8|bool``; uv ``[Vuv,2]``;
    per view (leading dim ``n_views``, optional for one view): ij ``[n,V,2]``, depths ``[n,V]``, colors ``[n,V,C]``,
    shade ``[n,V]``, edgeflags ``[n,T,3]``; texture ``[Ht,Wt,C]`` or None; background_color ``[C]`` or
    background_image ``[n,H,W,C]``.  Vertex arrays share one float dtype, pixel arrays another."""

    def __init__(self, faces, faces_uv, textured, shaded, uv, ij, depths, colors, shade, edgeflags, height, width, texture=None,
                 background_color=None, background_image=None, clockwise=False, backface_culling=True, strict_edge=True,
                 perspective_correct=False, integer_pixel_centers=True, vertex_dtype=torch.float64, pixel_dtype=torch.float32,
                 device="cuda", validate=True, deterministic=False):  # fmt: skip
        dev = _resolve_device(device)
        self.device, self.vertex_dtype, self.pixel_dtype = dev, vertex_dtype, pixel_dtype
        # integer accumulation for the calls on THIS scene (DeodrHipScene::deterministic): gradients bit-identical from run to run, several times
        # slower; may be switched at any time (it is read when a call is made).  set_deterministic() is the process-wide switch.
        self.deterministic = bool(deterministic)
        self.faces = _tensor(np.asarray(faces).astype(np.int64) if not torch.is_tensor(faces) else faces, dev, torch.int32)
        self.faces_uv = _tensor(np.asarray(faces_uv).astype(np.int64) if not torch.is_tensor(faces_uv) else faces_uv, dev, torch.int32)
        self.textured = _tensor(textured, dev, torch.uint8)
        self.shaded = _tensor(shaded, dev, torch.uint8)
        self.height, self.width = int(height), int(width)
        self.flags = dict(clockwise=bool(clockwise), backface_culling=bool(backface_culling), strict_edge=bool(strict_edge),
                          perspective_correct=bool(perspective_correct), integer_pixel_centers=bool(integer_pixel_centers))  # fmt: skip
        self._texture_given = self._uv_given = None  # (tensor last handed to set_texture / set_uv, its version): see there
        self._texture_buffer = self._uv_buffer = None
        self.set_views(ij, depths, colors, shade, edgeflags)
        for name, a in (("uv", uv), ("texture", texture), ("background_color", background_color), ("background_image", background_image)):
            self.upload(name, a)
        if validate:
            self.validate()

    def upload(self, name, a):
        """Replace ``uv`` [Vuv,2] (vertex dtype), ``texture`` [Ht,Wt,C], ``background_color`` [C] or ``background_image`` [n,H,W,C] (pixel dtype) by the
        array or tensor ``a``, converted as the constructor converts them: an empty texture (or None) and a background that is None leave the scene
        without one.  Unlike :meth:`set_texture` / :meth:`set_uv` the shape may change, and nothing is remembered about ``a``."""
        dev, pd = self.device, self.pixel_dtype
        if name == "uv":
            t = _tensor(a, dev, self.vertex_dtype).reshape(-1, 2).detach()
        elif name == "texture":
            t = _tensor(a, dev, pd).detach() if _count(a) > 0 else None
        elif name == "background_color":
            t = None if a is None else _tensor(a, dev, pd).reshape(-1)
        else:
            assert name == "background_image"
            t = None if a is None else _tensor(a, dev, pd).reshape(self.n_views, self.height, self.width, self.nb_colors).contiguous()
        setattr(self, name, t)

    def validate(self):
        """checkSceneValid's index checks (reference H.h:2700-2712), once per topology (synchronises).  The set-up kernel
        makes the same checks on every forward and raises the workspace's sticky error word; this one fails early."""
        V, Vuv = int(self.depths.shape[1]), int(self.uv.shape[0])
        if self.nb_triangles:
            # int32 storage of uint32 indices: a negative value is an index >= 2^31
            if int(self.faces.min()) < 0 or int(self.faces.max()) >= V:
                raise ValueError(scene_error_message(ERR_FACES))
            if int(self.faces_uv.min()) < 0 or int(self.faces_uv.max()) >= Vuv:
                raise ValueError(scene_error_message(ERR_FACES_UV))
            if self.texture is None and bool((self.textured.bool() & self.shaded.bool()).any()):
                raise ValueError(scene_error_message(ERR_NO_TEXTURE))

    def set_views(self, ij=None, depths=None, colors=None, shade=None, edgeflags=None):
        """Replace per-view arrays (tensors are used as they are when already contiguous on the device)."""
        dev, vd = self.device, self.vertex_dtype
        if depths is not None:
            d = _tensor(depths, dev, vd)
            self.depths = d.reshape(1, -1) if d.dim() == 1 else d
        n, V = self.depths.shape
        self.n_views = n
        if ij is not None:
            self.ij = _tensor(ij, dev, vd).reshape(n, V, 2)
        if colors is not None:
            self.colors = _tensor(colors, dev, vd).reshape(n, V, -1)
        if shade is not None:
            self.shade = _tensor(shade, dev, vd).reshape(n, V)
        if edgeflags is not None:
            self.edgeflags = _tensor(edgeflags, dev, torch.uint8).reshape(n, -1, 3)
        self.nb_colors = int(self.colors.shape[2])

    def _set_shared(self, name, t, dtype, shape):
        given = getattr(self, f"_{name}_given")
        if torch.is_tensor(t) and given is not None and given[0] is t and given[1] == t._version:
            return  # the same tensor, unchanged since: what the scene holds is its value
        source, t = t, _as_tensor(t).detach()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"set_{name}: expected shape {list(shape)}, got {list(t.shape)} (a new shape needs a new DeviceScene)")
        if t.device == self.device and t.dtype == dtype and t.is_contiguous():
            setattr(self, name, t)
        else:
            if getattr(self, f"_{name}_buffer") is None:
                setattr(self, f"_{name}_buffer", torch.empty(shape, dtype=dtype, device=self.device))
            getattr(self, f"_{name}_buffer").copy_(t)
            setattr(self, name, getattr(self, f"_{name}_buffer"))
        setattr(self, f"_{name}_given", (source, t._version))

    def set_texture(self, t):
        """The next calls read the value ``t`` [Ht,Wt,C] has NOW: the tensor itself when it is contiguous, on the scene's device and in the pixel dtype
        (later in-place updates -- an optimiser's, :func:`texture_step`'s -- are then seen without another call); anything else is converted, once per
        call, into a buffer the scene keeps for that purpose (the same tensor again, unchanged by torch's count, is not converted again).  The shape
        cannot change, and a scene built without a texture cannot get one."""
        if self.texture is None:
            raise ValueError("set_texture: the scene was built without a texture")
        self._set_shared("texture", t, self.pixel_dtype, self.texture.shape)

    def set_uv(self, uv):
        """The same for the texture coordinates [Vuv,2] (vertex dtype)."""
        self._set_shared("uv", uv, self.vertex_dtype, self.uv.shape)

    def shared_sources(self):
        """-> (texture, uv): the tensors last handed to :meth:`set_texture` / :meth:`set_uv` (what the scene reads them from), None for one never set"""
        return tuple(None if given is None else given[0] for given in (self._texture_given, self._uv_given))

    @property
    def nb_triangles(self):
        return int(self.faces.shape[0])

    def zero_grads(self):
        return dict(
            ij_b=torch.zeros_like(self.ij), colors_b=torch.zeros_like(self.colors), shade_b=torch.zeros_like(self.shade),
            uv_b=torch.zeros_like(self.uv), texture_b=None if self.texture is None else torch.zeros_like(self.texture),
        )  # fmt: skip

    def c_struct(self, grads=None):
        s = _SceneC()
        for name in ("faces", "faces_uv", "textured", "shaded", "depths", "ij", "shade", "colors", "edgeflags", "uv", "texture",
                     "background_image", "background_color"):  # fmt: skip
            setattr(s, name, _ptr(getattr(self, name)))
        if grads is not None:
            for name in ("uv_b", "ij_b", "shade_b", "colors_b", "texture_b"):
                setattr(s, name, _ptr(grads[name]))
        s.nb_triangles, s.nb_vertices, s.nb_uv = self.nb_triangles, int(self.depths.shape[1]), int(self.uv.shape[0])
        s.height, s.width, s.nb_colors = self.height, self.width, self.nb_colors
        if self.texture is not None:
            s.texture_height, s.texture_width = int(self.texture.shape[0]), int(self.texture.shape[1])
        for k, v in self.flags.items():
            setattr(s, k, int(v))
        s.n_views = self.n_views
        s.vertex_dtype = 1 if self.vertex_dtype == torch.float64 else 0
        s.pixel_dtype = 1 if self.pixel_dtype == torch.float64 else 0
        s.deterministic = 1 if self.deterministic else 0
        return s


# What the workspace of a HipRasterizer holds the forward state of; the tensors are kept alive with it (the launches that read them may
# still be queued).  fused: a fit step -- its forward raster has already back-propagated through the tiles without edges and kept no owner ids.
_Forward = namedtuple("_Forward", "scene sigma antialiase_error obs image err_buffer generation fused weights z")


class HipRasterizer:
    """Owns the device workspace of one scene shape and runs renderScene / renderScene_B on it.

    The workspace keeps the forward state (per-primitive records, tile lists, per-pixel owner ids) between
    :meth:`render` and :meth:`render_backward`, like ``Scene2D.store_backward`` does in the reference (dr.py:618-627).
    Every forward is stamped with a generation number (``self.generation``); :meth:`render_backward` reuses the state only
    when the caller's stamp is still the current one and recomputes it otherwise.

    Spill-pool overflow and invalid scene indices are detected WITHOUT synchronising: after a forward the 64-byte status block
    of the workspace is copied asynchronously to pinned memory (every ``poll_every`` forwards, and after each of the first
    two) and inspected at the next call.  An overflow found that way means that frames rendered since the poll were
    incomplete: the workspace is regrown and a RuntimeError says so.  ``check_overflow=True`` on a call checks synchronously
    (and regrows / repeats transparently).

    ``retain_frames`` (default True; an attribute, may be switched at any time): a fit loop renders into the same ``out=(image, z)`` at every
    iteration, and two tiles out of three of a typical frame are background before and after.  :meth:`render_fit` then tells the library that
    the buffers still hold the previous frame (``deodr_hip_render_scene_fit_retained``), and the step writes the background only into the
    tiles that have just become empty -- same image, depth buffer and gradients, half of the bytes.  It says so only when it can see that
    it is true: the previous forward of this very workspace allocation, on the same stream and not captured into a graph, wrote the same two
    tensor objects; torch has counted no in-place operation on them since (``_version``); the scene's background tensor and its version are
    the same.  Anything else -- a new ``out``, ``image.fill_()``, a regrown workspace, another background -- is a full fill, and the library
    checks the buffer addresses again on the device.  THE ONE ASSUMPTION LEFT: torch counts what torch does.  Code that writes ``image`` / ``z``
    or the background through raw pointers (a kernel of its own, another HipRasterizer rendering into the same tensors) must bump their
    version (``torch.autograd.graph.increment_version``) or set ``retain_frames = False``."""

    def __init__(self, nb_triangles, height, width, nb_colors, n_views=1, device="cuda", pool_pairs=0, poll_every=8, retain_frames=True):
        self.dims = (int(nb_triangles), int(height), int(width), int(nb_colors), int(n_views))
        self.retain_frames = bool(retain_frames)
        self.device = _resolve_device(device)
        self.poll_every = int(poll_every)
        self.generation = 0
        self.alloc_count = 0  # a captured HIP graph holds the OLD workspace address: see GraphedStep
        self._polls = 0  # calls of poll_status
        self._weights_cache = None  # (source tensor, its version, converted): the same tensor again, unchanged, is not converted again
        self._alloc(pool_pairs)

    def _alloc(self, pool_pairs):
        self.pool_pairs = int(pool_pairs)
        nbytes = lib().deodr_hip_workspace_bytes(*self.dims, self.pool_pairs)
        if nbytes == 0:
            raise ValueError("invalid scene dimensions")
        with torch.cuda.device(self.device):
            self.workspace = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)  # must start zero-filled
        self.nbytes = nbytes
        self._status_words = self.workspace[:64].view(torch.int32)
        self._status_host = torch.zeros(16, dtype=torch.int32).pin_memory()
        self._status_event = None  # recorded after the last asynchronous copy of the status block
        self._forwards = 0
        self._checked = False
        self._pool_cap = None
        self._last = None  # the _Forward whose state the workspace holds
        self._kept = None  # _frame_state() right after that forward, when it wrote a frame and a depth buffer (retain_frames)
        self._entry_of = self._entry = None  # the library whose retained entry was looked up, and the entry (_retained_entry)
        self._loss_cache = None  # (the background-loss table belongs to one (observation, background, clamp) of one workspace)
        self.alloc_count += 1

    @classmethod
    def for_scene(cls, ds, pool_pairs=0, retain_frames=True):
        return cls(ds.nb_triangles, ds.height, ds.width, ds.nb_colors, ds.n_views, ds.device, pool_pairs, retain_frames=retain_frames)

    # ---- status ------------------------------------------------------------------------------------------------------

    def _inspect_poll(self, sc):
        """Look at the last completed asynchronous copy of the status block (never waits)."""
        ev = self._status_event
        if ev is None or torch.cuda.is_current_stream_capturing() or not ev.query():
            return
        self._status_event = None
        needed, errors = int(self._status_host[_STATUS_NEEDED]) & 0xFFFFFFFF, int(self._status_host[_STATUS_ERRORS])
        if errors:
            raise RuntimeError("deodr_hip: " + scene_error_message(errors))
        if self._pool_cap is None:
            cap = C.c_ulonglong(0)
            _check(lib().deodr_hip_workspace_pool_pairs(C.byref(sc), self.nbytes, C.byref(cap)))
            self._pool_cap = int(cap.value)
        if needed > self._pool_cap:
            self._alloc(max(2 * needed, 1024))
            raise RuntimeError(
                f"deodr_hip: the spill pool of the workspace overflowed ({needed} pairs needed): frames rendered since the last "
                "check were incomplete; the workspace has been regrown, render again"
            )

    def _copy_status(self, due):
        """Queue an asynchronous copy of the status block, and the event that tells when it has landed, behind what was just launched --
        when one is `due`, none is in flight and the stream is not being captured.  -> whether a copy was queued"""
        if not due or self._status_event is not None or torch.cuda.is_current_stream_capturing():
            return False
        self._status_host.copy_(self._status_words, non_blocking=True)
        self._status_event = torch.cuda.Event()
        self._status_event.record()
        return True

    def _poll(self):
        """A forward was just launched: copy the status block after each of the first two, then after every ``poll_every``-th."""
        self._forwards += 1
        self._copy_status(self._forwards <= 2 or self._forwards % self.poll_every == 0)

    def poll_status(self):
        """For callers that launch this workspace's kernels without going through :meth:`render` & co (a captured HIP graph being
        replayed): look at the last asynchronous copy of the status block, then queue the next one.  Never waits; raises when a
        forward since the previous look overflowed the spill pool (the workspace is regrown: capture again) or met invalid indices."""
        if self._last is None:
            return
        self._inspect_poll(self._last.scene.c_struct())
        self._polls += 1
        if self._copy_status((self._polls - 1) % max(self.poll_every, 1) == 0):  # (a copy + event per replay is ~13 us of a ~200 us iteration)
            self._forwards = max(self._forwards, 2)  # (the forwards of a replayed graph: past "each of the first two")

    def status(self, ds):
        """Synchronous check: -> (overflowed, needed_pairs, scene_error_bits)."""
        over, need, errs = C.c_int(0), C.c_ulonglong(0), C.c_int(0)
        with torch.cuda.device(self.device):
            _check(lib().deodr_hip_workspace_status(C.byref(ds.c_struct()), _ptr(self.workspace), self.nbytes, _stream(self.device), C.byref(over),
                                                    C.byref(need), C.byref(errs)))  # fmt: skip
        return bool(over.value), int(need.value), int(errs.value)

    def _check_scene(self, ds):
        if (ds.nb_triangles, ds.height, ds.width, ds.nb_colors, ds.n_views) != self.dims:
            raise ValueError("scene shape differs from the workspace shape")
        if ds.device != self.device:
            raise ValueError(f"scene lives on {ds.device}, the workspace on {self.device}")

    def _frame(self, ds, out):
        n, H, W, Cc = ds.n_views, ds.height, ds.width, ds.nb_colors
        pd = ds.pixel_dtype
        if out is None:
            return torch.empty((n, H, W, Cc), dtype=pd, device=ds.device), torch.empty((n, H, W), dtype=pd, device=ds.device)
        image, z = out
        for t, shape in ((image, (n, H, W, Cc)), (z, (n, H, W))):
            if t.device != ds.device or t.dtype != pd or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("out= buffers must be contiguous pixel-dtype tensors [n,H,W,C] / [n,H,W] on the scene's device")
        return image, z

    def _until_it_fits(self, ds, launch):
        """`launch()` something that runs a forward, check synchronously, regrow the workspace and repeat until nothing spills;
        -> what the last `launch()` returned"""
        for _attempt in range(16):
            result = launch()
            over, need, errs = self.status(ds)
            self._checked = True
            if errs:
                raise RuntimeError("deodr_hip: " + scene_error_message(errs))
            if not over:
                return result
            self._alloc(max(2 * need, 1024))  # regrow (zero-filled) and launch again
        # the pool doubles every time: this is not a scene that needs more room, something is wrong
        raise RuntimeError("deodr_hip: the spill pool still overflows after 16 regrows")

    def _frame_state(self, ds, image, z):
        """what must not have changed between two forwards for the second to claim that (image, z) still hold the first one's frame: the
        allocation, the stream, torch's count of in-place operations on the two buffers, the background (tensor and count; the tensors are part
        of the state, so they stay alive and no new one can land on a kept address), the shape of the launch"""
        return (self.alloc_count, torch.cuda.current_stream(self.device).cuda_stream, image._version, z._version, ds.background_color,
                None if ds.background_color is None else ds.background_color._version, ds.background_image,
                None if ds.background_image is None else ds.background_image._version, ds.n_views, self.dims)  # fmt: skip

    @staticmethod
    def _same_state(a, b):
        return a is not None and b is not None and len(a) == len(b) and all(x is y if torch.is_tensor(x) or torch.is_tensor(y) else x == y for x, y in zip(a, b))

    def _retained_entry(self):
        """``deodr_hip_render_scene_fit_retained`` of the loaded library, looked up once per library object; None: it has none (the test harness's)"""
        L = lib()
        if self._entry_of is not L:
            self._entry_of, self._entry = L, getattr(L, "deodr_hip_render_scene_fit_retained", None)
        return self._entry

    def _retained_claim(self, ds, image, z):
        """-> (claim, state): 1 when this fit step may tell the library that (image, z) still hold the frame of the previous forward on this
        workspace (see the class), and the :meth:`_frame_state` to keep once the step has been launched (None: a captured launch runs when the
        graph is replayed, any number of times and whatever happens in between -- nothing is known afterwards).  What was kept is forgotten
        here: a step that fails after its scan has left a bitmap of a frame that was never written, and the next one must fill everything."""
        last, kept, self._kept = self._last, self._kept, None
        state = None if torch.cuda.is_current_stream_capturing() else self._frame_state(ds, image, z)
        return int(last is not None and last.image is image and last.z is z and self._same_state(kept, state)), state

    _COMPUTE = object()

    def _stamp(self, ds, sigma, antialiase_error, obs, image, err_buffer=None, fused=False, weights=None, z=None, state=_COMPUTE):
        """The workspace now holds the forward state of these: a new generation.  ``z``: the depth buffer that forward wrote, when it wrote one
        next to ``image`` (None: a forward that rendered no frame -- the next fit step claims nothing); ``state``: their :meth:`_frame_state`
        when the caller has formed it already"""
        self.generation += 1
        self._last = _Forward(ds, float(sigma), bool(antialiase_error), obs, image, err_buffer, self.generation, fused, weights, z)
        if z is None or image is None:
            self._kept = None
        elif state is not HipRasterizer._COMPUTE:
            self._kept = state
        else:  # (a captured launch: see _retained_claim)
            self._kept = None if torch.cuda.is_current_stream_capturing() else self._frame_state(ds, image, z)

    # ---- calls -------------------------------------------------------------------------------------------------------

    def render(self, ds, sigma=1.0, antialiase_error=False, obs=None, out=None, check_overflow=None):
        """-> (image [n,H,W,C], z_buffer [n,H,W][, err_buffer [n,H,W]]) as pixel-dtype device tensors.

        ``check_overflow``: True = synchronise and make sure no tile list spilled past the pool (regrow + repeat if one did);
        None (default) = do that on the first call only, afterwards poll asynchronously; False = only poll."""
        self._check_scene(ds)
        n, H, W, Cc = ds.n_views, ds.height, ds.width, ds.nb_colors
        pd = ds.pixel_dtype
        with torch.cuda.device(self.device):
            sc = ds.c_struct()
            self._inspect_poll(sc)
            image, z = self._frame(ds, out)
            err = obs_t = None
            if antialiase_error:
                obs_t = _on(obs, ds.device, pd, (n, H, W, Cc), "obs")
                err = torch.empty((n, H, W), dtype=pd, device=ds.device)

            self._kept = None  # (until this forward has been launched: see _retained_claim)

            def launch():
                _check(lib().deodr_hip_render_scene(C.byref(sc), _ptr(image), _ptr(z), float(sigma), int(antialiase_error), _ptr(obs_t),
                                                    _ptr(err), _ptr(self.workspace), self.nbytes, _stream(self.device)))  # fmt: skip

            if check_overflow is True or (check_overflow is None and not self._checked):
                self._until_it_fits(ds, launch)
                self._forwards += 1
            else:
                launch()
                self._poll()
        self._stamp(ds, sigma, antialiase_error, obs_t, image, err, z=z)
        return (image, z, err) if antialiase_error else (image, z)

    def _loss_table(self, ds, sc, obs_t, options, weights_t=None):
        """the background-loss table of (obs, background, clamp, weights) for the loss of a fit step, computed once (deodr_hip_background_loss)"""
        key = (obs_t.data_ptr(), obs_t._version, tuple(obs_t.shape), None if ds.background_color is None else (ds.background_color.data_ptr(), ds.background_color._version),
               None if ds.background_image is None else (ds.background_image.data_ptr(), ds.background_image._version),
               (options.clamp, options.clamp_lo, options.clamp_hi), None if weights_t is None else (weights_t.data_ptr(), weights_t._version))  # fmt: skip
        cache = self._loss_cache
        if cache is None or cache[0] != key:
            L = lib()
            n = int(L.deodr_hip_fit_loss_bytes(ds.height, ds.width, ds.n_views)) // 8
            table, scratch = torch.empty(n, dtype=torch.float64, device=self.device), torch.empty(n, dtype=torch.float64, device=self.device)
            _check(L.deodr_hip_background_loss(C.byref(sc), _ptr(obs_t), C.byref(options), _ptr(table), _ptr(self.workspace), self.nbytes,
                                               _stream(self.device)))  # fmt: skip
            # (every tensor whose address is part of the key is kept alive by the cache: a new tensor cannot land on a keyed address)
            self._loss_cache = cache = (key, table, scratch, (obs_t, ds.background_color, ds.background_image, weights_t))
        return cache[1], cache[2]

    def _fit_weights(self, ds, weights):
        """per-pixel weights of a fit step as the library wants them: [n_views, H, W], the scene's device and pixel dtype, contiguous (a tensor
        that already is all that is passed through untouched, so that the loss-table cache recognises it); [H, W] is expanded over the views"""
        n, H, W = ds.n_views, ds.height, ds.width
        w = _as_tensor(weights)
        if tuple(w.shape) not in ((n, H, W), (H, W)):
            raise ValueError(f"weights must have shape [{n}, {H}, {W}] (one value per view and pixel) or [{H}, {W}], not {list(w.shape)}")
        if w.dim() == 3 and w.device == ds.device and w.dtype == ds.pixel_dtype and w.is_contiguous():
            return w
        cached = self._weights_cache
        if torch.is_tensor(weights) and cached is not None and cached[0] is weights and cached[1] == weights._version:
            return cached[2]
        w_t = w.to(device=ds.device, dtype=ds.pixel_dtype).expand(n, H, W).contiguous()
        if torch.is_tensor(weights):  # (an array can change without a trace: converted at every call)
            self._weights_cache = (weights, weights._version, w_t)
        return w_t

    def render_fit(self, ds, obs, sigma=1.0, grads=None, out=None, check_overflow=None, clear_grads=False, loss_out=None, clamp=None, done_flag=None,
                   weights=None):  # fmt: skip
        """One fit step in one call: render ``ds`` and back-propagate ``sum((image - obs)**2)``; -> (image, z_buffer, grads).

        Same results as :meth:`render` followed by ``render_backward(residual_obs=obs)`` (what the reference's
        ``Scene2D.render_compare_and_backward`` does with ``antialiase_error=False``), but the forward raster already
        back-propagates through every tile without silhouette edges, so the frame is traversed once.  ``clear_grads``: zero
        ``grads`` first, inside the same kernel launches (otherwise they are accumulated into).  ``loss_out``: a float64 device
        tensor of one element that receives ``sum((image - obs)**2)`` -- from the same launches, without a pass over the frame
        (``deodr_hip_render_scene_fit_ex``; the table it needs is computed at the first call with this observation).  ``clamp`` =
        (lo, hi): the loss is ``sum((image.clamp(lo, hi) - obs)**2)``, the depth fitter's data term (deodr/mesh_fitter.py:108-123);
        the returned image is the un-clamped rendering.  ``done_flag`` = (int32 / uint32 device tensor of one element, value): the step
        stores ``value`` there when its gradients are complete -- what a consumer on another stream waits for with :func:`wait_flag`
        instead of an event (``DeodrHipFitOptions::done_flag``).  ``weights``: one value per view and pixel, ``[n_views, H, W]`` (or
        ``[H, W]`` for all views): the loss is ``sum(weights[..., None] * (image - obs)**2)`` (of the clamped image with ``clamp``) and
        the residual is scaled alike -- masks, sensor holes, per-camera confidence.  Meant to be ``>= 0`` and not checked; pixels of weight
        0 are still rendered, only their residual vanishes.  Pass a contiguous tensor in the scene's pixel dtype on its device to avoid a
        conversion.  Any other shape raises ``ValueError``."""
        self._check_scene(ds)
        weights_t = None if weights is None else self._fit_weights(ds, weights)
        with torch.cuda.device(self.device):
            image, z = self._frame(ds, out)
            obs_t = _pixels(obs, ds)
            if check_overflow or (check_overflow is None and not self._checked):
                self.render(ds, sigma, out=(image, z), check_overflow=True)  # sizes the spill pool once (synchronises)
            if grads is None:
                grads = ds.zero_grads()
            sc = ds.c_struct(grads)
            self._inspect_poll(sc)
            if done_flag is not None and (done_flag[0].element_size() != 4 or done_flag[0].numel() != 1 or done_flag[0].device != ds.device):
                raise ValueError("done_flag must be (a 4-byte integer tensor of one element on the scene's device, value)")
            # (a library without the entry -- the test harness's -- is called as ever)
            retained_entry = self._retained_entry() if self.retain_frames else None
            claim, state = self._retained_claim(ds, image, z) if retained_entry is not None else (0, HipRasterizer._COMPUTE)
            self._kept = None  # (until this step has been launched: a step that fails is followed by a full fill)
            plain = loss_out is None and clamp is None and done_flag is None and weights_t is None
            if plain and retained_entry is not None:
                _check(retained_entry(C.byref(sc), _ptr(image), _ptr(z), float(sigma), _ptr(obs_t), int(bool(clear_grads)), None, claim,
                                      _ptr(self.workspace), self.nbytes, _stream(self.device)))  # fmt: skip
            elif plain:
                _check(lib().deodr_hip_render_scene_fit(C.byref(sc), _ptr(image), _ptr(z), float(sigma), _ptr(obs_t), int(bool(clear_grads)),
                                                        _ptr(self.workspace), self.nbytes, _stream(self.device)))  # fmt: skip
            else:
                options = _FitOptionsC()
                if weights_t is not None:
                    options.weights = weights_t.data_ptr()
                if done_flag is not None:
                    options.done_flag, options.done_value = done_flag[0].data_ptr(), int(done_flag[1]) & 0xFFFFFFFF
                if clamp is not None:
                    options.clamp, options.clamp_lo, options.clamp_hi = 1, float(clamp[0]), float(clamp[1])
                if loss_out is not None:
                    if loss_out.dtype != torch.float64 or loss_out.device != ds.device or loss_out.numel() != 1:
                        raise ValueError("loss_out must be a float64 tensor of one element on the scene's device")
                    table, scratch = self._loss_table(ds, sc, obs_t, options, weights_t)
                    options.tile_loss, options.loss, options.loss_scratch = table.data_ptr(), loss_out.data_ptr(), scratch.data_ptr()
                if retained_entry is not None:
                    _check(retained_entry(C.byref(sc), _ptr(image), _ptr(z), float(sigma), _ptr(obs_t), int(bool(clear_grads)), C.byref(options), claim,
                                          _ptr(self.workspace), self.nbytes, _stream(self.device)))  # fmt: skip
                else:
                    _check(lib().deodr_hip_render_scene_fit_ex(C.byref(sc), _ptr(image), _ptr(z), float(sigma), _ptr(obs_t), int(bool(clear_grads)),
                                                               C.byref(options), _ptr(self.workspace), self.nbytes, _stream(self.device)))  # fmt: skip
            self._poll()
        self._stamp(ds, sigma, False, obs_t, image, fused=True, weights=weights_t, z=z, state=state)
        return image, z, grads

    def render_backward(self, ds, image_b=None, err_buffer_b=None, grads=None, have_forward_state=True, residual_obs=None,
                        generation=None, sigma=None):  # fmt: skip
        """Adjoint of the last :meth:`render` of ``ds``; returns the dict of gradient tensors (accumulated into ``grads``
        when given, fresh zeros otherwise).  Nothing passed in is mutated.

        ``residual_obs`` (instead of ``image_b``): propagate the gradient of ``sum((image - residual_obs)**2)`` where
        ``image`` is the output of the last render; ``2 (image - obs)`` is formed inside the kernel.
        ``generation``: the value of ``self.generation`` right after the forward this adjoint belongs to; when another forward
        has run on the workspace since (two renders in one autograd graph), the forward state is recomputed from ``ds``
        instead of being trusted (pass that forward's ``sigma`` too)."""
        self._check_scene(ds)
        if self._last is None:
            raise RuntimeError("deodr_hip: render_backward called before any render on this workspace")
        last = self._last
        aa, obs_t, image = last.antialiase_error, last.obs, last.image
        sigma = last.sigma if sigma is None else float(sigma)
        n, H, W, Cc = ds.n_views, ds.height, ds.width, ds.nb_colors
        pd = ds.pixel_dtype
        with torch.cuda.device(self.device):
            if grads is None:
                grads = ds.zero_grads()
            sc = ds.c_struct(grads)
            ib = eb = None
            if aa:
                eb = _on(err_buffer_b, ds.device, pd, (n, H, W), "err_buffer_b")
            elif residual_obs is not None:
                obs_t = _pixels(residual_obs, ds)
            else:
                ib = _on(image_b, ds.device, pd, (n, H, W, Cc), "image_b")
            state = have_forward_state and last.scene is ds and not last.fused and (generation is None or generation == last.generation)
            if not state and not aa and residual_obs is not None:
                # residual mode forms 2 (image - obs) inside the kernels from the frame of THIS forward; the frame at hand belongs to
                # another one (a later forward used the workspace, or the last call was a fit step): render again, then the state --
                # and the frame -- are this scene's
                image, _z = self.render(ds, sigma, check_overflow=False)
                state = True
            if not state:
                self._kept = None  # (a forward runs inside the call)
            _check(lib().deodr_hip_render_scene_b(C.byref(sc), _ptr(image), None, _ptr(ib), sigma, int(aa), _ptr(obs_t), None, _ptr(eb),
                                                  _ptr(self.workspace), self.nbytes, int(state), _stream(self.device)))  # fmt: skip
            if not state:
                # a forward ran inside the call: the workspace now holds the state of THIS (ds, sigma), stamped anew so that
                # any other pending adjoint sees that its own forward state is gone
                self._poll()
                self._stamp(ds, sigma, aa, obs_t, image, last.err_buffer)
        return grads

    def render_backward_of(self, ds, sigma, image, antialiase_error=False, obs=None, image_b=None, err_buffer_b=None):
        """Adjoint of a frame the CALLER hands in (``image`` [n,H,W,C], of ``ds`` at ``sigma``; ``obs`` with ``antialiase_error``) without
        a forward on this workspace before: the forward state is recomputed inside the call, which synchronises and makes sure that
        nothing spilled (regrow + repeat otherwise).  -> fresh gradient tensors."""

        def launch():
            self._stamp(ds, sigma, antialiase_error, obs, image)
            return self.render_backward(ds, image_b=image_b, err_buffer_b=err_buffer_b, have_forward_state=False)

        return self._until_it_fits(ds, launch)


# ---- spherical-harmonic lighting and per-vertex albedo (include/deodr_hip_lighting.h) ---------------------------------------------------

SH_MAX_VIEWS, SH_MAX_VERTICES, SH_COEFFS = 64, 2**24, 9  # the limits include/deodr_hip_lighting.h states
_I32_ONLY = (torch.int32,)  # (uint32 index arrays travel as int32 tensors, as MeshTopology keeps them)


def sh_blocks(V, n):
    """``deodr_hip_sh_blocks``: the workgroups of the per-(view, vertex) kernel of :func:`sh_shade_b` (0: outside the limits)"""
    return int(lib().deodr_hip_sh_blocks(int(V), int(n)))


def sh_scratch(V, n, C, device):
    """the scratch of :func:`sh_shade_b` for V vertices, n views and C channels, zero-filled as the library wants it once (one per stream in use)"""
    need = lib().deodr_hip_sh_scratch_bytes(int(V), int(n), int(C))
    return _byte_scratch("sh_scratch", f"V = {V}, n = {n}, C = {C}", need, "deodr_hip_lighting.h", device, zeroed=True)


def sh_products(scratch, V, n, C):
    """the view [n,V,C] of a :func:`sh_scratch` that :func:`sh_shade_b` leaves the products ``colors_b * E`` in when the albedo is per vertex and n > 1
    (include/deodr_hip_lighting.h, "the scratch after the call"): their sum over the views is ``albedo_b``"""
    at = 64 + 8 * 3 * n * V
    return scratch[at : at + 8 * n * V * C].view(torch.float64).view(n, V, C)


def _sh_args(what, posed, faces, vf_offsets, vf_corners, sh, albedo):
    """checks before the library is called -> (n, V, S, C, per_vertex, rows of :func:`_check_tensors` for the inputs)"""
    _rocm_tensor(what, "posed", posed)
    if posed.dim() != 3 or int(posed.shape[2]) != 3 or not 1 <= int(posed.shape[0]) <= SH_MAX_VIEWS or not 1 <= int(posed.shape[1]) <= SH_MAX_VERTICES:
        raise ValueError(f"{what}: posed must have shape [1 <= n <= {SH_MAX_VIEWS}, 1 <= V <= 2^24, 3], not {list(posed.shape)}")
    n, V = int(posed.shape[0]), int(posed.shape[1])
    if not torch.is_tensor(sh) or sh.dim() not in (1, 2) or int(sh.shape[0]) != SH_COEFFS:
        raise ValueError(f"{what}: sh must have shape [9] or [9, S], not {list(getattr(sh, 'shape', ()))}")
    S = 1 if sh.dim() == 1 else int(sh.shape[1])
    C, per_vertex = 1, False
    rows = [("posed", posed, _F64_ONLY, (n, V, 3)), ("sh", sh, _F64_ONLY, None), ("faces", faces, _I32_ONLY, (None, 3)),
            ("vf_offsets", vf_offsets, _I32_ONLY, (V + 1,))]  # fmt: skip
    if not torch.is_tensor(faces) or faces.dim() != 2 or int(faces.shape[0]) < 1:
        raise ValueError(f"{what}: faces must have shape [T >= 1, 3]")
    rows.append(("vf_corners", vf_corners, _I32_ONLY, (3 * int(faces.shape[0]),)))
    if albedo is not None:
        if not torch.is_tensor(albedo) or albedo.dim() not in (1, 2) or not 1 <= int(albedo.shape[-1]) <= 3 or (albedo.dim() == 2 and int(albedo.shape[0]) != V):
            raise ValueError(f"{what}: albedo must have shape [1 <= C <= 3] or [{V}, C], not {list(getattr(albedo, 'shape', ()))}")
        C, per_vertex = int(albedo.shape[-1]), albedo.dim() == 2
        rows.append(("albedo", albedo, _F64_ONLY, None))
    if S != 1 and S != C:
        raise ValueError(f"{what}: sh must have 1 column or one per channel ({C}), not {S}")
    return n, V, S, C, per_vertex, rows


def sh_shade(posed, faces, vf_offsets, vf_corners, sh, albedo=None, luminosity=None, colors=None, clockwise=False, want_luminosity=None):
    """``deodr_hip_sh_shade``: order-2 spherical-harmonic lighting of the vertex normals in one launch.  ``posed`` [n,V,3], ``sh`` [9] | [9,S], ``albedo``
    None | [C] | [V,C], float64 ROCm tensors; ``faces`` [T,3], ``vf_offsets`` [V+1], ``vf_corners`` [3T] the int32 tensors of a ``MeshTopology``
    -> (luminosity [n,V] | None, colors [n,V,C] | None): colours with an albedo, the luminosity without one (or with ``want_luminosity``, S = 1)."""
    what = "sh_shade"
    n, V, S, C, per_vertex, rows = _sh_args(what, posed, faces, vf_offsets, vf_corners, sh, albedo)
    if want_luminosity is None:
        want_luminosity = albedo is None or luminosity is not None
    rows += [(name, t, _F64_ONLY, shape) for name, t, shape in (("luminosity", luminosity, (n, V)), ("colors", colors, (n, V, C))) if t is not None]
    _check_tensors(what, "posed", posed.device, rows)
    if colors is not None and albedo is None:
        raise ValueError(f"{what}: colors without albedo")
    dev = posed.device
    with torch.cuda.device(dev):
        if luminosity is None and want_luminosity:
            luminosity = torch.empty((n, V), dtype=torch.float64, device=dev)
        if colors is None and albedo is not None:
            colors = torch.empty((n, V, C), dtype=torch.float64, device=dev)
    _launch(lib().deodr_hip_sh_shade, dev, _ptr(posed), _ptr(faces), _ptr(vf_offsets), _ptr(vf_corners), _ptr(sh), S, _ptr(albedo), int(per_vertex), C,
            _ptr(luminosity), _ptr(colors), V, n, int(bool(clockwise)))  # fmt: skip
    for t in (luminosity, colors):
        if t is not None:
            _touched(t)
    return luminosity, colors


def sh_shade_b(posed, faces, vf_offsets, vf_corners, sh, albedo=None, luminosity_b=None, colors_b=None, posed_b=None, sh_b=None, albedo_b=None,
               accumulate=False, scratch=None, clockwise=False, want=(True, True, True)):
    """``deodr_hip_sh_shade_b``: the adjoint of :func:`sh_shade` -> (posed_b [n,V,3] | None, sh_b of ``sh``'s shape | None, albedo_b of ``albedo``'s shape |
    None), allocated where not given and ``want`` = (posed_b, sh_b, albedo_b) asks for them.  ``accumulate``: added to sh_b and albedo_b, which must then
    be given.  Deterministic; asynchronous on the current stream.  ``scratch``: a :func:`sh_scratch` of the caller's; None: one per device and stream."""
    what = "sh_shade_b"
    n, V, S, C, per_vertex, rows = _sh_args(what, posed, faces, vf_offsets, vf_corners, sh, albedo)
    optional = [("luminosity_b", luminosity_b, (n, V)), ("colors_b", colors_b, (n, V, C)), ("posed_b", posed_b, (n, V, 3)), ("sh_b", sh_b, tuple(sh.shape)),
                ("albedo_b", albedo_b, None if albedo is None else tuple(albedo.shape))]  # fmt: skip
    rows += [(name, t, _F64_ONLY, shape) for name, t, shape in optional if t is not None]
    if scratch is not None:
        rows.append(("scratch", scratch, (torch.uint8,), (None,)))
    _check_tensors(what, "posed", posed.device, rows)
    if albedo is None and albedo_b is not None:
        raise ValueError(f"{what}: albedo_b without albedo")
    want_posed, want_sh, want_albedo = want
    if accumulate and ((want_sh and sh_b is None) or (want_albedo and albedo is not None and albedo_b is None)):
        raise ValueError(f"{what}: accumulate needs sh_b and (with an albedo) albedo_b")
    dev = posed.device
    with torch.cuda.device(dev):
        if posed_b is None and want_posed:
            posed_b = torch.empty_like(posed)
        if sh_b is None and want_sh:
            sh_b = torch.empty_like(sh)
        if albedo_b is None and want_albedo and albedo is not None:
            albedo_b = torch.empty_like(albedo)
        scratch = _own_or_cached_scratch(what, scratch, "sh", dev, lib().deodr_hip_sh_scratch_bytes, sh_scratch, V, n, C)
    _launch(lib().deodr_hip_sh_shade_b, dev, _ptr(posed), _ptr(faces), _ptr(vf_offsets), _ptr(vf_corners), _ptr(sh), S, _ptr(albedo), int(per_vertex), C,
            _ptr(luminosity_b), _ptr(colors_b), _ptr(posed_b), _ptr(sh_b), _ptr(albedo_b), int(bool(accumulate)), _ptr(scratch), scratch.numel(), V, n,
            int(bool(clockwise)))  # fmt: skip
    for t in (posed_b, sh_b, albedo_b):
        if t is not None:
            _touched(t)
    return posed_b, sh_b, albedo_b


# ---- linear blend skinning (include/deodr_hip_skinning.h) ---------------------------------------------------------------------------------

SKIN_MAX_VIEWS, SKIN_MAX_JOINTS, SKIN_MAX_INFLUENCES, SKIN_MAX_VERTICES = 64, 256, 8, 2**24  # the limits include/deodr_hip_skinning.h states


def skin_scratch(V, J, K, n, device):
    """the scratch of :func:`skin_apply_b` for V vertices, J joints, K influences per vertex and n poses (one per stream in use)"""
    need = lib().deodr_hip_skin_scratch_bytes(int(V), int(J), int(K), int(n))
    return _byte_scratch("skin_scratch", f"V = {V}, J = {J}, K = {K}, n = {n}", need, "deodr_hip_skinning.h", device, zeroed=True)


def _skin_args(what, vertices, joints, parents, quaternions, indices, weights):
    """checks before the library is called -> (V, J, K, n, rows of :func:`_check_tensors` for the inputs)"""
    _rocm_tensor(what, "vertices", vertices)
    if vertices.dim() != 2 or int(vertices.shape[1]) != 3 or not 1 <= int(vertices.shape[0]) <= SKIN_MAX_VERTICES:
        raise ValueError(f"{what}: vertices must have shape [1 <= V <= 2^24, 3], not {list(vertices.shape)}")
    V = int(vertices.shape[0])
    if not torch.is_tensor(quaternions) or quaternions.dim() != 3 or int(quaternions.shape[2]) != 4 or not 1 <= int(quaternions.shape[0]) <= SKIN_MAX_VIEWS \
            or not 1 <= int(quaternions.shape[1]) <= SKIN_MAX_JOINTS:  # fmt: skip
        raise ValueError(f"{what}: quaternions must have shape [1 <= n <= {SKIN_MAX_VIEWS}, 1 <= J <= {SKIN_MAX_JOINTS}, 4], not "
                         f"{list(getattr(quaternions, 'shape', ()))}")  # fmt: skip
    n, J = int(quaternions.shape[0]), int(quaternions.shape[1])
    if not torch.is_tensor(indices) or indices.dim() != 2 or int(indices.shape[0]) != V or not 1 <= int(indices.shape[1]) <= SKIN_MAX_INFLUENCES:
        raise ValueError(f"{what}: indices must have shape [{V}, 1 <= K <= {SKIN_MAX_INFLUENCES}], not {list(getattr(indices, 'shape', ()))}")
    K = int(indices.shape[1])
    rows = [("vertices", vertices, _F64_ONLY, (V, 3)), ("joints", joints, _F64_ONLY, (J, 3)), ("parents", parents, _I32_ONLY, (J,)),
            ("quaternions", quaternions, _F64_ONLY, (n, J, 4)), ("indices", indices, _I32_ONLY, (V, K)), ("weights", weights, _F64_ONLY, (V, K))]  # fmt: skip
    return V, J, K, n, rows


def skin_apply(vertices, joints, parents, quaternions, indices, weights, world=None, posed=None):
    """``deodr_hip_skin_apply``: linear blend skinning in two launches.  ``vertices`` [V,3], ``joints`` [J,3], ``quaternions`` [n,J,4] (raw), ``weights``
    [V,K] float64 ROCm tensors; ``parents`` [J], ``indices`` [V,K] int32 (the uint32 tables of the header) -> (world [n,J,7], posed [n,V,3]).
    The tables are NOT checked here (:class:`deodr_amd.skinning.Skin` does that on the host); the kernels skip what is out of range."""
    what = "skin_apply"
    V, J, K, n, rows = _skin_args(what, vertices, joints, parents, quaternions, indices, weights)
    rows += [(name, t, _F64_ONLY, shape) for name, t, shape in (("world", world, (n, J, 7)), ("posed", posed, (n, V, 3))) if t is not None]
    _check_tensors(what, "vertices", vertices.device, rows)
    dev = vertices.device
    with torch.cuda.device(dev):
        world = torch.empty((n, J, 7), dtype=torch.float64, device=dev) if world is None else world
        posed = torch.empty((n, V, 3), dtype=torch.float64, device=dev) if posed is None else posed
    _launch(lib().deodr_hip_skin_apply, dev, _ptr(vertices), _ptr(joints), _ptr(parents), _ptr(quaternions), _ptr(indices), _ptr(weights), _ptr(world),
            _ptr(posed), V, J, K, n)  # fmt: skip
    _touched(world), _touched(posed)
    return world, posed


def skin_apply_b(vertices, joints, parents, quaternions, indices, weights, world, posed_b, joint_offsets, joint_slots, vertices_b=None,
                 quaternions_b=None, joints_b=None, scratch=None, want=(True, True, True)):
    """``deodr_hip_skin_apply_b``: the adjoint of :func:`skin_apply` -> (vertices_b [V,3] | None, quaternions_b [n,J,4] | None, joints_b [J,3] | None),
    allocated where not given and ``want`` asks for them.  ``world`` [n,J,7] from the forward call; ``joint_offsets`` [J+1], ``joint_slots`` [nnz] the
    transposed table (int32).  Deterministic; asynchronous on the current stream.  ``scratch``: a :func:`skin_scratch` of the caller's; None: one per
    device and stream."""
    what = "skin_apply_b"
    V, J, K, n, rows = _skin_args(what, vertices, joints, parents, quaternions, indices, weights)
    rows += [("world", world, _F64_ONLY, (n, J, 7)), ("posed_b", posed_b, _F64_ONLY, (n, V, 3)), ("joint_offsets", joint_offsets, _I32_ONLY, (J + 1,)),
             ("joint_slots", joint_slots, _I32_ONLY, (None,))]  # fmt: skip
    optional = (("vertices_b", vertices_b, (V, 3)), ("quaternions_b", quaternions_b, (n, J, 4)), ("joints_b", joints_b, (J, 3)))
    rows += [(name, t, _F64_ONLY, shape) for name, t, shape in optional if t is not None]
    if scratch is not None:
        rows.append(("scratch", scratch, (torch.uint8,), (None,)))
    _check_tensors(what, "vertices", vertices.device, rows)
    nnz = int(joint_slots.shape[0])
    if nnz > V * K:
        raise ValueError(f"{what}: joint_slots must have at most V K = {V * K} entries, not {nnz}")
    if not any(w or t is not None for w, t in zip(want, (vertices_b, quaternions_b, joints_b))):
        raise ValueError(f"{what}: no output requested")
    dev = vertices.device
    with torch.cuda.device(dev):
        vertices_b, quaternions_b, joints_b = (torch.empty(shape, dtype=torch.float64, device=dev) if t is None and w else t
                                               for w, (_, t, shape) in zip(want, optional))  # fmt: skip
        scratch = _own_or_cached_scratch(what, scratch, "skin", dev, lib().deodr_hip_skin_scratch_bytes, skin_scratch, V, J, K, n)
    # (a table without entries: torch gives an empty tensor no address, the library wants one it never reads)
    slots = joint_slots if nnz else joint_offsets
    _launch(lib().deodr_hip_skin_apply_b, dev, _ptr(vertices), _ptr(joints), _ptr(parents), _ptr(quaternions), _ptr(indices), _ptr(weights), _ptr(world),
            _ptr(posed_b), _ptr(joint_offsets), _ptr(slots), nnz, _ptr(vertices_b), _ptr(quaternions_b), _ptr(joints_b), _ptr(scratch), scratch.numel(),
            V, J, K, n)  # fmt: skip
    for t in (vertices_b, quaternions_b, joints_b):
        if t is not None:
            _touched(t)
    return vertices_b, quaternions_b, joints_b


# ---- the image data terms: multi-scale L2 (include/deodr_hip_pyramid.h) and structural (include/deodr_hip_ssim.h) ------------------------------


def _image_term(what, header, make_scratch, image, obs, weights, array_name, array, scalar, terms, loss, image_b, scratch, want_gradient):
    """What :func:`pyramid_l2` and :func:`ssim_l2` share: the checks of their tensors, the results and the scratch where none were given, the call
    ``deodr_hip_<what>``.  ``array``: the term's float64 parameters on the device, called ``array_name``; ``scalar(what)`` checks the term's number
    -> (the number as the library takes it, the length of ``array`` and of ``terms``, what it adds to (n, H, W, C) for the scratch).  -> (terms,
    loss, image_b)"""
    _rocm_tensor(what, "image", image)
    if image.dim() != 4 or min(image.shape) < 1:
        raise ValueError(f"{what}: image must have shape [n >= 1, H >= 1, W >= 1, C >= 1], not {list(image.shape)}")
    n, H, W, Cn = (int(v) for v in image.shape)
    number, length, extra = scalar(what)
    pix = (image.dtype,)
    rows = [("image", image, _FLOATS, None), ("obs", obs, pix, (n, H, W, Cn)), (array_name, array, _F64_ONLY, (length,))]
    optional = (("weights", weights, pix, (n, H, W)), ("terms", terms, _F64_ONLY, (length,)), ("loss", loss, _F64_ONLY, (1,)),
                ("image_b", image_b, pix, (n, H, W, Cn)), ("scratch", scratch, (torch.uint8,), (None,)))  # fmt: skip
    rows += [row for row in optional if row[1] is not None]
    _check_tensors(what, "image", image.device, rows)
    dev, family = image.device, make_scratch.__name__[: -len("_scratch")]
    need = int(getattr(lib(), f"deodr_hip_{family}_scratch_bytes")(n, H, W, Cn, *extra))
    if need == 0:
        raise ValueError(f"{what}: image of shape {list(image.shape)} is outside the limits of include/{header}")
    with torch.cuda.device(dev):
        terms = torch.empty(length, dtype=torch.float64, device=dev) if terms is None else terms
        loss = torch.empty(1, dtype=torch.float64, device=dev) if loss is None else loss
        if image_b is None and want_gradient:
            image_b = torch.empty_like(image)
        scratch = _own_or_cached_scratch(what, scratch, family, dev, need, make_scratch, n, H, W, Cn, *extra)
    _launch(getattr(lib(), f"deodr_hip_{what}"), dev, _ptr(image), _ptr(obs), _ptr(weights), n, H, W, Cn, _dtype_tag(image), number, _ptr(array),
            _ptr(terms), _ptr(loss), _ptr(image_b), _ptr(scratch), scratch.numel())  # fmt: skip
    for t in (terms, loss, image_b):
        if t is not None:
            _touched(t)
    return terms, loss, image_b


# ---- the multi-scale L2 data term (include/deodr_hip_pyramid.h) ---------------------------------------------------------------------------

PYRAMID_MAX_LEVELS = _abi.PYRAMID_HEADER.defines["DEODR_HIP_PYRAMID_MAX_LEVELS"]


def pyramid_scratch(n, H, W, C, levels, device):
    """the scratch of :func:`pyramid_l2` for n frames of H x W x C and ``levels`` coarse levels (one per stream in use; it need not be zeroed)"""
    need = lib().deodr_hip_pyramid_scratch_bytes(int(n), int(H), int(W), int(C), int(levels))
    return _byte_scratch("pyramid_scratch", f"n = {n}, H = {H}, W = {W}, C = {C}, levels = {levels}", need, "deodr_hip_pyramid.h", device)


def pyramid_l2(image, obs, weights, levels, level_weights, terms=None, loss=None, image_b=None, scratch=None, want_gradient=True):
    """``deodr_hip_pyramid_l2``: ``loss = sum_l level_weights[l] term_l`` of the residual ``image - obs`` summed over 2^l x 2^l cells (the header has
    the formulas) -> (terms [levels+1] float64: the unweighted ``term_l``; loss [1] float64; image_b = d loss / d image, or None).  ``image``, ``obs``
    [n,H,W,C] float32 / float64 contiguous ROCm tensors, ``weights`` [n,H,W] of the same dtype or None, ``level_weights`` [levels+1] float64 ON THE
    DEVICE (read when the kernels run).  ``image_b`` is allocated when None and ``want_gradient``.  Deterministic; asynchronous on the current
    stream.  ``scratch``: a :func:`pyramid_scratch` of the caller's; None: one per device and stream."""
    def checked_levels(what):
        count = int(levels)
        if not 1 <= count <= PYRAMID_MAX_LEVELS:
            raise ValueError(f"{what}: levels must be in 1 .. {PYRAMID_MAX_LEVELS}, not {count}")
        return count, count + 1, (count,)

    return _image_term("pyramid_l2", "deodr_hip_pyramid.h", pyramid_scratch, image, obs, weights, "level_weights", level_weights, checked_levels, terms, loss,
                       image_b, scratch, want_gradient)  # fmt: skip


# ---- the structural (SSIM) data term (include/deodr_hip_ssim.h) ----------------------------------------------------------------------------

SSIM_WINDOW = _abi.SSIM_HEADER.defines["DEODR_HIP_SSIM_WINDOW"]


def ssim_scratch(n, H, W, C, device):
    """the scratch of :func:`ssim_l2` for n frames of H x W x C (one per stream in use; it need not be zeroed)"""
    need = lib().deodr_hip_ssim_scratch_bytes(int(n), int(H), int(W), int(C))
    return _byte_scratch("ssim_scratch", f"n = {n}, H = {H}, W = {W}, C = {C}", need, "deodr_hip_ssim.h", device)


def ssim_l2(image, obs, weights, mix, data_range=1.0, terms=None, loss=None, image_b=None, scratch=None, want_gradient=True):
    """``deodr_hip_ssim_l2``: ``loss = mix[0] sum w (image - obs)^2 + mix[1] sum w (1 - SSIM)`` under the 11 x 11 Gaussian window with zero padding
    (the header has the formulas) -> (terms [2] float64: the two unweighted sums; loss [1] float64; image_b = d loss / d image, or None).  ``image``,
    ``obs`` [n,H,W,C] float32 / float64 contiguous ROCm tensors, ``weights`` [n,H,W] of the same dtype or None -- they multiply the SSIM map and do
    not enter the windows, so ``image_b`` is in general not 0 where a weight is --, ``mix`` [2] float64 ON THE DEVICE (read when the kernels run).
    ``image_b`` is allocated when None and ``want_gradient``.  Deterministic; asynchronous on the current stream.  ``scratch``: a
    :func:`ssim_scratch` of the caller's; None: one per device and stream."""
    def checked_range(what):
        span = float(data_range)
        if not (span > 0 and span < float("inf")):
            raise ValueError(f"{what}: data_range must be finite and > 0, not {span}")
        return span, 2, ()

    return _image_term("ssim_l2", "deodr_hip_ssim.h", ssim_scratch, image, obs, weights, "mix", mix, checked_range, terms, loss, image_b, scratch, want_gradient)


# ---- sparse symmetric positive definite solve (include/deodr_hip_solve.h) -----------------------------------------------------------------

SOLVE_N_SMALL = _abi.SOLVE_HEADER.defines["DEODR_HIP_SOLVE_N_SMALL"]
SOLVE_MAX_D = 4  # (the limit include/deodr_hip_solve.h states)


def spd_launches(n, nnz, D, iterations):
    """``deodr_hip_spd_solve_launches``: the kernel launches of a :func:`spd_solve` call -- 1 up to ``SOLVE_N_SMALL`` rows, ``2 + 2 iterations`` above"""
    return int(lib().deodr_hip_spd_solve_launches(int(n), int(nnz), int(D), int(iterations)))


def spd_scratch(n, D, device):
    """the scratch of :func:`spd_solve` for a system of n rows and D columns (one per stream in use; it need not be zeroed)"""
    need = lib().deodr_hip_spd_solve_scratch_bytes(int(n), int(D))
    return _byte_scratch("spd_scratch", f"n = {n}, D = {D}", need, "deodr_hip_solve.h", device)


def spd_solve(offsets, cols, vals, b, iterations, rel_tol=0.0, x=None, residual=None, scratch=None):
    """``deodr_hip_spd_solve``: ``iterations`` steps of conjugate gradients from ``x = 0`` on ``A x = b``, the columns of ``b`` [n, D <= 4] (float64)
    independently -> (x [n, D], residual [D]: the squared relative residual of the recurrence); the header has the recurrence.  ``A`` in compressed
    rows: ``offsets`` [n + 1] and ``cols`` [nnz] as 4-byte integer tensors (uint32 bit patterns), ``vals`` [nnz] float64, read when the kernels run.
    The tables are trusted (symmetric positive definite, ``offsets`` non-decreasing from 0 to nnz, ``cols`` < n): :mod:`deodr_amd.smoothing` checks
    its own on the host.  Deterministic; asynchronous on the current stream.  ``scratch``: a :func:`spd_scratch` of the caller's; None: one per
    device and stream."""
    what = "spd_solve"
    _rocm_tensor(what, "b", b)
    if b.dim() != 2 or b.shape[0] < 1 or not 1 <= b.shape[1] <= SOLVE_MAX_D:
        raise ValueError(f"{what}: b must have shape [n >= 1, 1 <= D <= {SOLVE_MAX_D}], not {list(b.shape)}")
    n, D = (int(v) for v in b.shape)
    iterations, rel_tol = int(iterations), float(rel_tol)
    if iterations < 1:
        raise ValueError(f"{what}: iterations must be >= 1, not {iterations}")
    if not rel_tol >= 0:
        raise ValueError(f"{what}: rel_tol must be >= 0, not {rel_tol}")
    tables = "offsets and cols must be one-dimensional 4-byte integer tensors"
    rows = [("b", b, _F64_ONLY, None), ("offsets", offsets, _INDICES, (n + 1,), f"offsets must be a 4-byte integer tensor of n + 1 = {n + 1} entries"),
            ("cols", cols, _INDICES, (None,), tables)]  # fmt: skip
    _check_tensors(what, "b", b.device, rows)
    rows = [("vals", vals, _F64_ONLY, tuple(cols.shape), "vals must be a float64 tensor of the shape of cols")]
    optional = (("x", x, _F64_ONLY, (n, D)), ("residual", residual, _F64_ONLY, (D,)), ("scratch", scratch, (torch.uint8,), (None,)))
    rows += [row for row in optional if row[1] is not None]
    _check_tensors(what, "b", b.device, rows)
    nnz, dev = int(cols.numel()), b.device
    if nnz < n:
        raise ValueError(f"{what}: the matrix has {nnz} entries for {n} rows (the diagonal is stored)")
    with torch.cuda.device(dev):
        x = torch.empty_like(b) if x is None else x
        residual = torch.empty(D, dtype=torch.float64, device=dev) if residual is None else residual
        scratch = _own_or_cached_scratch(what, scratch, "solve", dev, lib().deodr_hip_spd_solve_scratch_bytes, spd_scratch, n, D)
    _launch(lib().deodr_hip_spd_solve, dev, _ptr(offsets), _ptr(cols), _ptr(vals), n, nnz, _ptr(b), _ptr(x), D, iterations, rel_tol, _ptr(residual),
            _ptr(scratch), scratch.numel())  # fmt: skip
    _touched(x), _touched(residual)
    return x, residual


# ---- as-rigid-as-possible energy (include/deodr_hip_arap.h) --------------------------------------------------------------------------------

ARAP_SWEEPS, ARAP_BLOCK, ARAP_MAX_BLOCKS = (_abi.ARAP_HEADER.defines["DEODR_HIP_ARAP_" + n] for n in ("SWEEPS", "BLOCK", "MAX_BLOCKS"))


def arap_launches(V, nnz, n):
    """``deodr_hip_arap_launches``: the kernel launches of an :func:`arap_energy` call, 2 (0 for shapes the call refuses)"""
    return int(lib().deodr_hip_arap_launches(int(V), int(nnz), int(n)))


def arap_blocks(V):
    """``deodr_hip_arap_blocks``: the workgroups per pose of both launches, ``min(ceil(V / ARAP_BLOCK), ARAP_MAX_BLOCKS)``; the grid is (blocks, n)"""
    return int(lib().deodr_hip_arap_blocks(int(V)))


def arap_scratch(V, n, device):
    """the scratch of :func:`arap_energy` for n poses of V vertices (one per stream in use; it need not be zeroed)"""
    need = lib().deodr_hip_arap_scratch_bytes(int(V), int(n))
    return _byte_scratch("arap_scratch", f"V = {V}, n = {n}", need, "deodr_hip_arap.h", device)


def arap_energy(offsets, cols, weights, vertices_ref, vertices, cregu, energy=None, gradient=None, rotations=None, scratch=None, want_rotations=False):
    """``deodr_hip_arap_energy``: the as-rigid-as-possible energy of ``vertices`` [n,V,3] against ``vertices_ref`` [V,3] (float64) over the vertex
    adjacency in compressed rows -- ``offsets`` [V + 1] and ``cols`` [nnz] as 4-byte integer tensors (uint32 bit patterns), ``weights`` [nnz]
    float64, read when the kernels run -> (energy [n], gradient [n,V,3], rotations [n,V,4] as (x, y, z, w) quaternions or None); the header has
    the operation.  ``rotations`` is written when a tensor is given or ``want_rotations``.  The tables are trusted (:mod:`deodr_amd.arap` checks
    its own on the host).  Deterministic; asynchronous on the current stream.  ``scratch``: an :func:`arap_scratch` of the caller's; None: one per
    device and stream."""
    what = "arap_energy"
    _rocm_tensor(what, "vertices", vertices)
    if vertices.dim() != 3 or vertices.shape[0] < 1 or vertices.shape[1] < 1 or vertices.shape[2] != 3:
        raise ValueError(f"{what}: vertices must have shape [n >= 1, V >= 1, 3], not {list(vertices.shape)}")
    n, V = int(vertices.shape[0]), int(vertices.shape[1])
    cregu = float(cregu)
    if not cregu >= 0:
        raise ValueError(f"{what}: cregu must be >= 0, not {cregu}")
    tables = "offsets and cols must be one-dimensional 4-byte integer tensors"
    rows = [("vertices", vertices, _F64_ONLY, None), ("vertices_ref", vertices_ref, _F64_ONLY, (V, 3)),
            ("offsets", offsets, _INDICES, (V + 1,), f"offsets must be a 4-byte integer tensor of V + 1 = {V + 1} entries"),
            ("cols", cols, _INDICES, (None,), tables)]  # fmt: skip
    _check_tensors(what, "vertices", vertices.device, rows)
    rows = [("weights", weights, _F64_ONLY, tuple(cols.shape), "weights must be a float64 tensor of the shape of cols")]
    optional = (("energy", energy, _F64_ONLY, (n,)), ("gradient", gradient, _F64_ONLY, (n, V, 3)), ("rotations", rotations, _F64_ONLY, (n, V, 4)),
                ("scratch", scratch, (torch.uint8,), (None,)))  # fmt: skip
    rows += [row for row in optional if row[1] is not None]
    _check_tensors(what, "vertices", vertices.device, rows)
    nnz, dev = int(cols.numel()), vertices.device
    with torch.cuda.device(dev):
        energy = torch.empty(n, dtype=torch.float64, device=dev) if energy is None else energy
        gradient = torch.empty_like(vertices) if gradient is None else gradient
        if rotations is None and want_rotations:
            rotations = torch.empty((n, V, 4), dtype=torch.float64, device=dev)
        scratch = _own_or_cached_scratch(what, scratch, "arap", dev, lib().deodr_hip_arap_scratch_bytes, arap_scratch, V, n)
    _launch(lib().deodr_hip_arap_energy, dev, _ptr(offsets), _ptr(cols), _ptr(weights), V, nnz, _ptr(vertices_ref), _ptr(vertices), n, cregu,
            _ptr(energy), _ptr(gradient), _ptr(rotations), _ptr(scratch), scratch.numel())  # fmt: skip
    _touched(energy), _touched(gradient)
    if rotations is not None:
        _touched(rotations)
    return energy, gradient, rotations


# ---- closest-point (Chamfer) energy (include/deodr_hip_chamfer.h) ---------------------------------------------------------------------------

CHAMFER_POINTS_TO_MESH, CHAMFER_MESH_TO_POINTS, CHAMFER_BLOCK, CHAMFER_TILE, CHAMFER_MAX_BLOCKS, CHAMFER_TARGET_BLOCKS, CHAMFER_MAX_SEGMENTS, CHAMFER_MAX_PAIRS = (
    _abi.CHAMFER_HEADER.defines["DEODR_HIP_CHAMFER_" + n] for n in ("POINTS_TO_MESH", "MESH_TO_POINTS", "BLOCK", "TILE", "MAX_BLOCKS", "TARGET_BLOCKS", "MAX_SEGMENTS", "MAX_PAIRS")
)


def chamfer_launches(V, P, n, directions=3):
    """``deodr_hip_chamfer_launches``: the kernel launches of a :func:`chamfer` call -- 4 with points -> mesh, 2 with mesh -> points alone (0 for
    arguments the call refuses)"""
    return int(lib().deodr_hip_chamfer_launches(int(V), int(P), int(n), int(directions)))


def chamfer_segments(queries, references):
    """``deodr_hip_chamfer_segments``: into how many contiguous parts the references of a search are cut (the second dimension of its grid)"""
    return int(lib().deodr_hip_chamfer_segments(int(queries), int(references)))


def chamfer_scratch(V, P, n, device):
    """the scratch of :func:`chamfer` for n poses of V vertices against P points (one per stream in use; it need not be zeroed)"""
    need = lib().deodr_hip_chamfer_scratch_bytes(int(V), int(P), int(n))
    return _byte_scratch("chamfer_scratch", f"V = {V}, P = {P}, n = {n}", need, "deodr_hip_chamfer.h", device)


def _closest_point(what, header, limits, make_scratch, vertices, points, params, point_weights, vertex_weights, directions, terms, loss, vertices_b, found,
                   nearest_point, scratch, want_nearest, mesh=None, cell_size=()):  # fmt: skip
    """What :func:`chamfer`, :func:`chamfer_grid` and :func:`surface_distance` share: the checks of their tensors, the results and the scratch where
    none were given, the call ``deodr_hip_<what>``.  ``found``: the results per point of points -> mesh as (name, tensor | None, dtypes, trailing
    shape); ``mesh``: (faces, corner_offsets, corners) of the surface operator; ``cell_size``: (the cell size,) of the grid.  -> (terms, loss,
    vertices_b, *found, nearest_point)"""
    _rocm_tensor(what, "vertices", vertices)
    if vertices.dim() != 3 or vertices.shape[0] < 1 or vertices.shape[1] < 1 or vertices.shape[2] != 3:
        raise ValueError(f"{what}: vertices must have shape [n >= 1, V >= 1, 3], not {list(vertices.shape)}")
    n, V = int(vertices.shape[0]), int(vertices.shape[1])
    if mesh is not None and (not torch.is_tensor(mesh[0]) or mesh[0].dim() != 2 or mesh[0].shape[0] < 1 or mesh[0].shape[1] != 3):
        raise ValueError(f"{what}: faces must have shape [F >= 1, 3], not {list(getattr(mesh[0], 'shape', ()))}")
    if not torch.is_tensor(points) or points.dim() != 3 or int(points.shape[0]) != n or points.shape[1] < 1 or points.shape[2] != 3:
        raise ValueError(f"{what}: points must have shape [{n}, P >= 1, 3], not {list(getattr(points, 'shape', ()))}")
    P, directions, cell_size = int(points.shape[1]), int(directions), tuple(float(c) for c in cell_size)
    if not 1 <= directions <= 3:
        raise ValueError(f"{what}: directions must be in 1 .. 3, not {directions}")
    if not all(c > 0 and c < float("inf") for c in cell_size):
        raise ValueError(f"{what}: cell_size must be finite and > 0, not {cell_size[0]}")
    rows, dims, said = [("vertices", vertices, _F64_ONLY, None)], (V, P, n), f"V = {V}, P = {P}, n = {n}"
    if mesh is not None:
        F = int(mesh[0].shape[0])
        rows += [("faces", mesh[0], (torch.int32,), (F, 3)), ("corner_offsets", mesh[1], (torch.int32,), (V + 1,)), ("corners", mesh[2], (torch.int32,), (3 * F,))]
        dims, said = (V, F, P, n), f"V = {V}, F = {F}, P = {P}, n = {n}"
    rows += [("points", points, _F64_ONLY, (n, P, 3)), ("params", params, _F64_ONLY, (3,))]
    optional = [("point_weights", point_weights, _F64_ONLY, (n, P)), ("vertex_weights", vertex_weights, _F64_ONLY, (V,)),
                ("terms", terms, _F64_ONLY, (n, 2)), ("loss", loss, _F64_ONLY, (n,)), ("vertices_b", vertices_b, _F64_ONLY, (n, V, 3))]  # fmt: skip
    optional += [(name, t, dtypes, (n, P) + tail) for name, t, dtypes, tail in found]
    optional += [("nearest_point", nearest_point, _INDICES, (n, V)), ("scratch", scratch, (torch.uint8,), (None,))]
    rows += [row for row in optional if row[1] is not None]
    _check_tensors(what, "vertices", vertices.device, rows)
    dev = vertices.device
    need = int(getattr(lib(), f"deodr_hip_{what}_scratch_bytes")(*dims))
    if need == 0 or not getattr(lib(), f"deodr_hip_{what}_launches")(*dims, directions):  # (the launches: a limit that depends on the directions)
        raise ValueError(f"{what}: {said} is outside the limits of {_include(header)} ({limits})")
    results = [t for _, t, _, _ in found]
    with torch.cuda.device(dev):
        terms = torch.empty((n, 2), dtype=torch.float64, device=dev) if terms is None else terms
        loss = torch.empty(n, dtype=torch.float64, device=dev) if loss is None else loss
        vertices_b = torch.empty_like(vertices) if vertices_b is None else vertices_b
        if want_nearest and directions & CHAMFER_POINTS_TO_MESH:
            results = [torch.empty((n, P) + tail, dtype=torch.int32 if dtypes is _INDICES else torch.float64, device=dev) if t is None else t
                       for _, t, dtypes, tail in found]  # fmt: skip
        if want_nearest and nearest_point is None and directions & CHAMFER_MESH_TO_POINTS:
            nearest_point = torch.empty((n, V), dtype=torch.int32, device=dev)
        scratch = _own_or_cached_scratch(what, scratch, make_scratch.__name__[: -len("_scratch")], dev, need, make_scratch, *dims)
    out = (terms, loss, vertices_b, *results, nearest_point)
    of_mesh = () if mesh is None else (_ptr(mesh[0]), dims[1], _ptr(mesh[1]), _ptr(mesh[2]))
    _launch(getattr(lib(), f"deodr_hip_{what}"), dev, _ptr(vertices), V, *of_mesh, _ptr(points), P, _ptr(point_weights), _ptr(vertex_weights), _ptr(params),
            *cell_size, n, directions, *(_ptr(t) for t in out), _ptr(scratch), scratch.numel())  # fmt: skip
    for t in out:
        if t is not None:
            _touched(t)
    return out


def chamfer(vertices, points, params, point_weights=None, vertex_weights=None, directions=3, terms=None, loss=None, vertices_b=None,
            nearest_vertex=None, nearest_point=None, scratch=None, want_nearest=False):  # fmt: skip
    """``deodr_hip_chamfer``: the closest-point energy of ``vertices`` [n,V,3] against ``points`` [n,P,3] (float64) -> (terms [n,2], loss [n],
    vertices_b [n,V,3], nearest_vertex [n,P] | None, nearest_point [n,V] | None as int32 tensors holding uint32 bit patterns); the header has the
    operation.  ``params`` [3] float64 ON THE DEVICE = (mix_0, mix_1, max_distance), read when the kernels run; ``point_weights`` [n,P] and
    ``vertex_weights`` [V] float64 or None (ones); ``directions``: bit 1 points -> mesh, bit 2 mesh -> points.  The nearest_* arrays are written when
    a tensor is given or ``want_nearest``, for the directions that are on.  The values are trusted (:mod:`deodr_amd.chamfer` checks its own on the
    host).  Deterministic; asynchronous on the current stream.  ``scratch``: a :func:`chamfer_scratch` of the caller's; None: one per device and
    stream."""
    return _closest_point("chamfer", "deodr_hip_chamfer.h", f"V * P <= {CHAMFER_MAX_PAIRS}, n <= 65535", chamfer_scratch, vertices, points, params, point_weights,
                          vertex_weights, directions, terms, loss, vertices_b, [("nearest_vertex", nearest_vertex, _INDICES, ())], nearest_point, scratch, want_nearest)  # fmt: skip


# ---- stable sort by key, closest-point energy over a uniform grid (include/deodr_hip_chamfer_grid.h) ----------------------------------------

_G = _abi.CHAMFER_GRID_HEADER.defines
SORT_DIGIT_BITS, SORT_BLOCK, SORT_ITEMS, SORT_MAX_ITEMS = (_G["DEODR_HIP_SORT_" + n] for n in ("DIGIT_BITS", "BLOCK", "ITEMS", "MAX_ITEMS"))
CHAMFER_GRID_NONE, CHAMFER_GRID_RINGS, CHAMFER_GRID_CELL_LIMIT, CHAMFER_GRID_MAX_ITEMS, CHAMFER_GRID_MIN_TABLE_BITS, CHAMFER_GRID_MAX_TABLE_BITS = (
    _G["DEODR_HIP_CHAMFER_GRID_" + n] for n in ("NONE", "RINGS", "CELL_LIMIT", "MAX_ITEMS", "MIN_TABLE_BITS", "MAX_TABLE_BITS")
)


def sort_keys_launches(N, n, bits):
    """``deodr_hip_sort_keys_launches``: three per pass of ``SORT_DIGIT_BITS`` bits (0 for arguments the call refuses)"""
    return int(lib().deodr_hip_sort_keys_launches(int(N), int(n), int(bits)))


def sort_keys_scratch(N, n, bits, device):
    """the scratch of :func:`sort_keys` for n rows of N keys (it need not be zeroed)"""
    need = lib().deodr_hip_sort_keys_scratch_bytes(int(N), int(n), int(bits))
    return _byte_scratch("sort_keys_scratch", f"N = {N}, n = {n}, bits = {bits}", need, "deodr_hip_chamfer_grid.h", device)


def sort_keys(keys, bits=32, sorted_keys=None, order=None, scratch=None, want_sorted=True):
    """``deodr_hip_sort_keys``: ``keys`` [n,N] (int32 or uint32 tensors holding uint32 bit patterns) -> (sorted_keys [n,N] | None, order [n,N] int32):
    per row the stable permutation that sorts the low ``bits`` bits of the keys, and ``keys[order]``.  Deterministic; asynchronous on the current
    stream; nothing is read back.  ``scratch``: a :func:`sort_keys_scratch` of the caller's; None: one per device and stream."""
    what = "sort_keys"
    _rocm_tensor(what, "keys", keys)
    if keys.dim() != 2 or keys.shape[0] < 1 or keys.shape[1] < 1:
        raise ValueError(f"{what}: keys must have shape [n >= 1, N >= 1], not {list(keys.shape)}")
    n, N, bits = int(keys.shape[0]), int(keys.shape[1]), int(bits)
    if not 1 <= bits <= 32:
        raise ValueError(f"{what}: bits must be in 1 .. 32, not {bits}")
    rows = [("keys", keys, _INDICES, None)]
    rows += [row for row in (("sorted_keys", sorted_keys, _INDICES, (n, N)), ("order", order, _INDICES, (n, N)), ("scratch", scratch, (torch.uint8,), (None,)))
             if row[1] is not None]  # fmt: skip
    _check_tensors(what, "keys", keys.device, rows)
    dev = keys.device
    need = int(lib().deodr_hip_sort_keys_scratch_bytes(N, n, bits))
    if need == 0:
        raise ValueError(f"{what}: N = {N}, n = {n} is outside the limits of include/deodr_hip_chamfer_grid.h (N <= {SORT_MAX_ITEMS}, n <= 65535)")
    with torch.cuda.device(dev):
        if want_sorted and sorted_keys is None:
            sorted_keys = torch.empty_like(keys)
        order = torch.empty((n, N), dtype=torch.int32, device=dev) if order is None else order
        scratch = _own_or_cached_scratch(what, scratch, "sort_keys", dev, need, sort_keys_scratch, N, n, bits)
    _launch(lib().deodr_hip_sort_keys, dev, _ptr(keys), N, n, bits, _ptr(sorted_keys), _ptr(order), _ptr(scratch), scratch.numel())
    for t in (sorted_keys, order):
        if t is not None:
            _touched(t)
    return sorted_keys, order


def chamfer_grid_table_bits(references):
    """``deodr_hip_chamfer_grid_table_bits``: log2 of the buckets of the hash table of a grid over ``references`` references (0: outside the limits)"""
    return int(lib().deodr_hip_chamfer_grid_table_bits(int(references)))


def chamfer_grid_launches(V, P, n, directions=3):
    """``deodr_hip_chamfer_grid_launches``: the kernel launches of a :func:`chamfer_grid` call (0 for arguments the call refuses)"""
    return int(lib().deodr_hip_chamfer_grid_launches(int(V), int(P), int(n), int(directions)))


def chamfer_grid_scratch(V, P, n, device):
    """the scratch of :func:`chamfer_grid` for n poses of V vertices against P points (one per stream in use; it need not be zeroed)"""
    need = lib().deodr_hip_chamfer_grid_scratch_bytes(int(V), int(P), int(n))
    return _byte_scratch("chamfer_grid_scratch", f"V = {V}, P = {P}, n = {n}", need, "deodr_hip_chamfer_grid.h", device)


def chamfer_grid(vertices, points, params, cell_size, point_weights=None, vertex_weights=None, directions=3, terms=None, loss=None, vertices_b=None,
                 nearest_vertex=None, nearest_point=None, scratch=None, want_nearest=False):  # fmt: skip
    """``deodr_hip_chamfer_grid``: :func:`chamfer` with the nearest neighbours found over a uniform grid of cells of size ``max(cell_size,
    max_distance / CHAMFER_GRID_RINGS)`` -- the same arguments and results, the same indices; a query with no neighbour within ``max_distance``
    (``params[2]``, which must be FINITE: trusted here, :mod:`deodr_amd.chamfer` checks its own) reports ``CHAMFER_GRID_NONE``.  No cap on V * P.
    ``scratch``: a :func:`chamfer_grid_scratch` of the caller's; None: one per device and stream."""
    return _closest_point("chamfer_grid", "deodr_hip_chamfer_grid.h", f"V, P <= {CHAMFER_GRID_MAX_ITEMS}, n <= 65535", chamfer_grid_scratch, vertices, points, params,
                          point_weights, vertex_weights, directions, terms, loss, vertices_b, [("nearest_vertex", nearest_vertex, _INDICES, ())], nearest_point, scratch,
                          want_nearest, cell_size=(cell_size,))  # fmt: skip


# ---- point-to-surface distance (include/deodr_hip_surface.h) --------------------------------------------------------------------------------

SURFACE_MAX_PAIRS = _abi.SURFACE_HEADER.defines["DEODR_HIP_SURFACE_MAX_PAIRS"]


def surface_launches(V, F, P, n, directions=3):
    """``deodr_hip_surface_distance_launches``: the kernel launches of a :func:`surface_distance` call -- 5 with points -> mesh alone, 6 with both
    directions, 2 with mesh -> points alone (0 for arguments the call refuses)"""
    return int(lib().deodr_hip_surface_distance_launches(int(V), int(F), int(P), int(n), int(directions)))


def surface_scratch(V, F, P, n, device):
    """the scratch of :func:`surface_distance` for n poses of V vertices and F faces against P points (one per stream in use; it need not be zeroed)"""
    need = lib().deodr_hip_surface_distance_scratch_bytes(int(V), int(F), int(P), int(n))
    return _byte_scratch("surface_scratch", f"V = {V}, F = {F}, P = {P}, n = {n}", need, "deodr_hip_surface.h", device)


def surface_distance(vertices, faces, corner_offsets, corners, points, params, point_weights=None, vertex_weights=None, directions=3, terms=None,
                     loss=None, vertices_b=None, nearest_face=None, barycentric=None, nearest_point=None, scratch=None, want_nearest=False):  # fmt: skip
    """``deodr_hip_surface_distance``: the point-to-surface distance of ``points`` [n,P,3] to the triangles ``faces`` [F,3] (int32) of ``vertices``
    [n,V,3] (float64) -> (terms [n,2], loss [n], vertices_b [n,V,3], nearest_face [n,P] | None, barycentric [n,P,3] | None, nearest_point [n,V] |
    None; the indices as int32 tensors holding uint32 bit patterns); the header has the operation.  ``corner_offsets`` [V + 1] and ``corners``
    [3 F] (int32): the transposed table of ``faces`` (:func:`deodr_amd.surface.corner_table`).  ``params`` [3] float64 ON THE DEVICE = (mix_0,
    mix_1, max_distance), read when the kernels run; ``point_weights`` [n,P] and ``vertex_weights`` [V] float64 or None (ones); ``directions``: bit
    1 points -> mesh, bit 2 mesh -> points.  The nearest_* and barycentric arrays are written when a tensor is given or ``want_nearest``, for the
    directions that are on.  The values and the tables are trusted (:mod:`deodr_amd.surface` checks its own on the host).  Deterministic;
    asynchronous on the current stream.  ``scratch``: a :func:`surface_scratch` of the caller's; None: one per device and stream."""
    found = [("nearest_face", nearest_face, _INDICES, ()), ("barycentric", barycentric, _F64_ONLY, (3,))]
    return _closest_point("surface_distance", "deodr_hip_surface.h", f"F * P <= {SURFACE_MAX_PAIRS}, V * P <= {CHAMFER_MAX_PAIRS} with mesh -> points, n <= 65535",
                          surface_scratch, vertices, points, params, point_weights, vertex_weights, directions, terms, loss, vertices_b, found, nearest_point, scratch,
                          want_nearest, mesh=(faces, corner_offsets, corners))  # fmt: skip


# ---- point-to-surface distance over a uniform grid of triangles (include_staged/deodr_hip_surface_grid.h) -----------------------------------

SURFACE_GRID_NONE, SURFACE_GRID_GATHER_FACES = (_abi.SURFACE_GRID_HEADER.defines["DEODR_HIP_SURFACE_GRID_" + n] for n in ("NONE", "GATHER_FACES"))


def surface_grid_launches(V, F, P, n, directions=3):
    """``deodr_hip_surface_grid_launches``: the kernel launches of a :func:`surface_grid` call (0 for arguments the call refuses)"""
    return int(lib().deodr_hip_surface_grid_launches(int(V), int(F), int(P), int(n), int(directions)))


def surface_grid_scratch(V, F, P, n, device):
    """the scratch of :func:`surface_grid` for n poses of V vertices and F faces against P points (one per stream in use; it need not be zeroed)"""
    need = lib().deodr_hip_surface_grid_scratch_bytes(int(V), int(F), int(P), int(n))
    return _byte_scratch("surface_grid_scratch", f"V = {V}, F = {F}, P = {P}, n = {n}", need, "deodr_hip_surface_grid.h", device)


def surface_grid(vertices, faces, corner_offsets, corners, points, params, cell_size, point_weights=None, vertex_weights=None, directions=3, terms=None,
                 loss=None, vertices_b=None, nearest_face=None, barycentric=None, nearest_point=None, scratch=None, want_nearest=False):  # fmt: skip
    """``deodr_hip_surface_grid``: :func:`surface_distance` with the closest face found over a uniform grid of triangles, one record per face, the
    cell edge ``max(cell_size, max_distance / CHAMFER_GRID_RINGS, the longest side of a face's box)`` -- the same arguments and results, the same
    faces and barycentric coordinates; a point with no face (a vertex with no point) within ``max_distance`` (``params[2]``, which must be FINITE:
    trusted here, :mod:`deodr_amd.surface` checks its own) reports ``SURFACE_GRID_NONE`` and barycentric coordinates (0, 0, 0).  No cap on F * P
    or V * P.  ``scratch``: a :func:`surface_grid_scratch` of the caller's; None: one per device and stream."""
    found = [("nearest_face", nearest_face, _INDICES, ()), ("barycentric", barycentric, _F64_ONLY, (3,))]
    return _closest_point("surface_grid", "deodr_hip_surface_grid.h", f"V, F, P <= {CHAMFER_GRID_MAX_ITEMS}, n <= 65535", surface_grid_scratch, vertices, points, params,
                          point_weights, vertex_weights, directions, terms, loss, vertices_b, found, nearest_point, scratch, want_nearest,
                          mesh=(faces, corner_offsets, corners), cell_size=(cell_size,))  # fmt: skip


# ---------------------------------------------------------------------------------------------------------------------
# drop-in NumPy entry points (reference pyx:50-57, 206-215)


def _np(a, dtype=None):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def _f64(a):
    """an array of the caller as a float64 CPU tensor (None stays None)"""
    return None if a is None else torch.as_tensor(_np(a, np.float64))


_ctx_cache = {}


def _device_scene(scene, nb_colors):
    tex = _np(scene.texture, np.float64)
    bgi = getattr(scene, "background_image", None)
    bgc = getattr(scene, "background_color", None)
    return DeviceScene(
        faces=_np(scene.faces), faces_uv=_np(scene.faces_uv), textured=_np(scene.textured, np.uint8), shaded=_np(scene.shaded, np.uint8),
        uv=_np(scene.uv, np.float64), ij=_np(scene.ij, np.float64)[None], depths=_np(scene.depths, np.float64)[None],
        colors=_np(scene.colors, np.float64).reshape(1, -1, nb_colors), shade=_np(scene.shade, np.float64)[None],
        edgeflags=_np(scene.edgeflags, np.uint8)[None], height=scene.height, width=scene.width,
        texture=tex if tex.size else None, background_color=None if bgc is None else _np(bgc, np.float64),
        background_image=None if bgi is None else _np(bgi, np.float64)[None], clockwise=scene.clockwise,
        backface_culling=scene.backface_culling, strict_edge=scene.strict_edge, perspective_correct=scene.perspective_correct,
        integer_pixel_centers=scene.integer_pixel_centers, vertex_dtype=torch.float64, pixel_dtype=torch.float64,
    )  # fmt: skip


def _rasterizer_for(ds):
    key = (ds.nb_triangles, ds.height, ds.width, ds.nb_colors, str(ds.device))
    if key not in _ctx_cache:
        if len(_ctx_cache) > 8:
            _ctx_cache.clear()
        _ctx_cache[key] = HipRasterizer.for_scene(ds)
    return _ctx_cache[key]


def renderSceneCpp(scene, sigma, image, z_buffer, antialiase_error=False, obs=None, err_buffer=None, check_valid=True):
    """Same contract as the reference's Cython ``renderSceneCpp``: fills ``image`` / ``z_buffer`` (/ ``err_buffer``) in place."""
    if check_valid:
        from .differentiable_renderer import check_scene

        check_scene(scene, image, z_buffer, False, None, antialiase_error, obs, err_buffer)
    ds = _device_scene(scene, image.shape[2])
    r = _rasterizer_for(ds)
    out = r.render(ds, sigma, bool(antialiase_error), _f64(obs), check_overflow=True)
    for buffer, rendered in zip((image, z_buffer, err_buffer), out):  # (out has the error buffer with antialiase_error only)
        buffer[...] = rendered[0].cpu().numpy()


def renderSceneBCpp(scene, sigma, image, z_buffer, image_b=None, antialiase_error=False, obs=None, err_buffer=None, err_buffer_b=None,
                    check_valid=True):  # fmt: skip
    """Same contract as the reference's Cython ``renderSceneBCpp``: ``scene.{uv,ij,shade,colors,texture}_b`` are rebound to
    ``old + new`` (pyx:406-410).  Stateless like the reference: the forward state is recomputed on the device.  The
    reference's in-place side effects on ``image`` / ``image_b`` / ``err_buffer`` are NOT reproduced."""
    if check_valid:
        from .differentiable_renderer import check_scene

        check_scene(scene, image, z_buffer, True, image_b, antialiase_error, obs, err_buffer)
    if scene.perspective_correct:
        raise RuntimeError("backward gradient propagation not supported yet with perspective_correct=True")
    ds = _device_scene(scene, image.shape[2])
    obs_t = None if obs is None else _f64(obs).to(ds.device)[None].contiguous()
    # stateless: the forward state is recomputed inside (the seed that does not belong to the mode is ignored); synchronous anyway
    g = _rasterizer_for(ds).render_backward_of(ds, sigma, _f64(image).to(ds.device)[None], bool(antialiase_error), obs_t, _f64(image_b), _f64(err_buffer_b))
    for name in ("uv_b", "ij_b", "shade_b", "colors_b", "texture_b"):
        new, old = g[name], getattr(scene, name, None)
        if new is not None and old is not None and _count(old):
            setattr(scene, name, _np(old, np.float64) + new.cpu().numpy().reshape(np.shape(old)))
