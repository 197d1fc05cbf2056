"""GPU checks of ``texture_smoothness_kernel`` and ``texture_step_kernel`` (deodr_amd/csrc/dr_texfit.h) over the cases of tests/texture_kernel_cases.py:
rows shorter than a 16-byte vector on the vector path, one interior row, every tail, C = 2, 5 and 64, textures that start 1, 2 and 3 elements behind
a 16-byte boundary, piece counts at and above the caps of both grids, and the step's parameters at their edges -- against the long-double
restatement, within the tolerances of ``test_texture_fit.close_in_storage`` (1e-14 of the largest entry in float64, one float32 ulp of the rounded
long-double value in float32) and 1e-12 for the energy.  Texture, gradient, speed and the energy are carved out of NaN-filled buffers; the scratch
is the caller's own ``texture_scratch`` bytes followed by a guard, its counter word zero after every call; what the header calls read-only is
bit-unchanged; two calls give the same bits, the energy included; the gradient is accumulated onto a non-zero g0."""

import numpy as np
import pytest
import torch

import texture_kernel_cases as tk
from fititer_reference import longdouble_is_extended
from test_basis_gpu import GUARD_BYTE, GUARD_BYTES, PAD, Arena, host
from test_texture_fit import close_in_storage

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not longdouble_is_extended(), reason="np.longdouble is not wider than float64 here: no reference")]

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
DTYPES = pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])


class OffsetArena(Arena):
    """``Arena`` whose tensors start ``behind`` elements behind a 16-byte boundary"""

    def __init__(self, behind=0):
        super().__init__()
        self.behind = behind

    def carve(self, values=None, shape=None, dtype=F64):
        shape = tuple(values.shape) if values is not None else tuple(shape)
        numel, start = int(np.prod(shape)), PAD + self.behind
        buffer = torch.full((2 * PAD + numel + 4,), float("nan"), dtype=dtype, device=DEV)
        t = buffer[start : start + numel].view(*shape)
        assert t.data_ptr() % 16 == (self.behind * t.element_size()) % 16 and t.is_contiguous()
        if values is not None:
            t.copy_(torch.as_tensor(np.ascontiguousarray(values)).to(dtype))
        self.made.append((buffer, start, numel, shape, values is None))
        return t


class Scratch:
    """exactly deodr_hip_texture_scratch_bytes bytes, zero-filled once, followed in the same allocation by a guard pattern"""

    def __init__(self):
        from deodr_amd.hip_renderer import lib

        self.nbytes = int(lib().deodr_hip_texture_scratch_bytes(2, 2, 1))
        assert self.nbytes >= 8 + 8 * tk.kernel_constants()["TEX_SMOOTH_BLOCKS"]  # the counter word and a partial per workgroup
        self.buffer = torch.zeros(self.nbytes + GUARD_BYTES, dtype=torch.uint8, device=DEV)
        self.buffer[self.nbytes :] = GUARD_BYTE
        self.front = self.buffer[: self.nbytes]

    def check(self):
        assert bool((self.buffer[self.nbytes :] == GUARD_BYTE).all()), "the scratch was written beyond deodr_hip_texture_scratch_bytes"
        assert int(self.front[:4].view(torch.int32)) == 0, "the counter word did not come back to zero"


def np_dtype(dtype):
    return np.float32 if dtype == F32 else np.float64


def check_smoothness(shape, dtype, behind=0):
    from deodr_amd import hip_renderer as hr

    t0, _s0, g0 = tk.arrays(shape, dtype == F32)
    energy, gradient = tk.smoothness(t0, tk.WEIGHT)
    what = f"{shape} {dtype} behind {behind}"
    scratch, runs = Scratch(), []
    for _ in range(2):  # (the second call on the scratch the first one left)
        arena = OffsetArena(behind)
        texture, g, e = arena.carve(t0, dtype=dtype), arena.carve(g0, dtype=dtype), arena.carve(shape=(1,), dtype=F64)
        out = hr.texture_smoothness(texture, g, tk.WEIGHT, energy_out=e, scratch=scratch.front)
        torch.cuda.synchronize()
        assert out is e
        arena.check(), scratch.check()
        assert np.array_equal(host(texture).astype(np.float64), t0), "the texture was written"
        runs.append((g, e))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), what  # bit-identical, the energy included
    close_in_storage(runs[0][0], g0.astype(tk.LD) + gradient, dtype, f"smoothness gradient {what}")
    e_err = abs(float(tk.LD(float(runs[0][1])) - energy) / float(energy))
    print(f"smoothness energy {what}: relative error {e_err:.3e}")
    assert e_err <= 1e-12, what


def check_step(shape, dtype, kwargs, behind=0, infinite=False):
    from deodr_amd import hip_renderer as hr

    t0, s0, g0 = tk.arrays(shape, dtype == F32)
    if infinite:  # (clipped to -+step_max: nothing infinite comes out)
        assert kwargs["step_max"] > 0
        g0.reshape(-1)[[3, g0.size - 1]] = np.inf, -np.inf
    t_ref, s_ref = tk.step(t0, s0, g0, tk.FACTOR, **kwargs)
    what = f"{shape} {dtype} behind {behind} {kwargs}{' infinite gradient' if infinite else ''}"
    runs = []
    for _ in range(2):
        arena = OffsetArena(behind)
        texture, speed, g = arena.carve(t0, dtype=dtype), arena.carve(s0, dtype=dtype), arena.carve(g0, dtype=dtype)
        hr.texture_step(texture, speed, g, tk.FACTOR, **kwargs)
        torch.cuda.synchronize()
        arena.check()
        assert np.array_equal(host(g).astype(np.float64), g0), "the gradient was written"
        runs.append((texture, speed))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), what
    got_t, got_s = host(runs[0][0]), host(runs[0][1])
    assert np.isfinite(got_t).all() and np.isfinite(got_s).all(), what
    close_in_storage(runs[0][0], t_ref, dtype, f"step texture {what}")
    # (a speed that is exactly 0 -- at a wall, or with damping = 1 -- has no ulp to be measured in: exactly 0 it must be)
    moving = np.asarray(s_ref.astype(np_dtype(dtype)) != 0)
    assert np.array_equal(got_s != 0, moving), what
    if moving.any():
        close_in_storage(runs[0][1][torch.as_tensor(moving, device=DEV)], s_ref[moving], dtype, f"step speed {what}")
    if kwargs.get("damping") == 1.0:
        assert not moving.any() and np.array_equal(got_t.astype(np.float64), t0)
    if "clamp" in kwargs:
        lo, hi = kwargs["clamp"]
        wall = np.asarray(s_ref == 0) & (kwargs.get("damping") != 1.0)
        assert got_t.min() >= lo and got_t.max() <= hi and np.isin(got_t[wall], (np_dtype(dtype)(lo), np_dtype(dtype)(hi))).all()
        if lo == hi:
            assert wall.all()


@DTYPES
@pytest.mark.parametrize("shape", tk.SMALL, ids=str)
def test_smoothness_small_shapes(shape, dtype):
    check_smoothness(shape, dtype)


@DTYPES
@pytest.mark.parametrize("shape", tk.SMALL, ids=str)
def test_step_small_shapes(shape, dtype):
    for kwargs in tk.STEP_PARAMETERS:
        check_step(shape, dtype, kwargs)


@DTYPES
def test_step_clips_an_infinite_gradient(dtype):
    for kwargs in tk.STEP_PARAMETERS:
        if (kwargs.get("step_max") or 0) > 0:
            for shape in ((5, 7, 3), (7, 3, 1)):
                check_step(shape, dtype, kwargs, infinite=True)


@pytest.mark.parametrize("dtype,behind", [(F32, 1), (F32, 2), (F32, 3), (F64, 1)], ids=["f32+1", "f32+2", "f32+3", "f64+1"])
def test_textures_that_start_behind_a_16_byte_boundary(dtype, behind):
    for shape in tk.MISALIGNED:
        check_smoothness(shape, dtype, behind)
        for kwargs in tk.STEP_PARAMETERS[:3]:
            check_step(shape, dtype, kwargs, behind)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["at", "one above", "above twice"])
@pytest.mark.parametrize("kernel,dtype", [("smooth", F32), ("smooth", F64), ("step", F32), ("step", F64)], ids=["smooth-f32", "smooth-f64", "step-f32", "step-f64"])
def test_piece_counts_at_and_above_the_cap_of_the_grid(kernel, dtype, which):
    shape = tk.CAPS[(kernel, 4 if dtype == F32 else 8)][which]
    g = tk.geometry(kernel, shape, 4 if dtype == F32 else 8)
    assert g["trips"] == which + 1 and g["grid"] * tk.kernel_constants()["FH_BLOCK"] == g["cap"]
    if kernel == "smooth":
        check_smoothness(shape, dtype)
    else:
        check_step(shape, dtype, tk.STEP_PARAMETERS[2])
