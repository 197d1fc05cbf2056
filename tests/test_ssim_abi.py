"""CPU checks of the structural data term at the C ABI (include/deodr_hip_ssim.h; the header itself: tests/test_companion_headers.py): the taps and
the tiling in deodr_amd/csrc/dr_ssim.h are the ones the Python side and the case table use, every bad argument of the launching entry point is
refused through its error code with a message before any launch (fake pointers, no GPU), the scratch size is 0 outside the limits, monotone inside
them and the documented formula, and the host wrapper refuses CPU tensors, wrong dtypes and wrong shapes without reaching the library."""

import os
import re

import pytest


def test_the_window_is_the_header_s():
    from deodr_amd import hip_renderer as hr
    from deodr_amd import ssim

    assert hr.SSIM_WINDOW == ssim.WINDOW == 11


def test_the_taps_and_the_tiling_of_the_kernels_are_the_python_side_s():
    import __graft_entry__ as g
    import ssim_reference as sr
    from deodr_amd import ssim

    source = open(os.path.join(g.CSRC, "dr_ssim.h")).read()
    table = re.search(r"SSIM_TAPS\[SSIM_WINDOW\]\s*=\s*\{(.*?)\}", source, re.S).group(1)
    assert [float(v) for v in table.split(",")] == ssim.gaussian_window()  # the same doubles
    constant = lambda name: int(re.search(rf"^constexpr int [^;]*\b{name} = (\d+)", source, re.M).group(1))
    assert (constant("SSIM_TH"), constant("SSIM_TW")) == sr.TILE and constant("SSIM_BLOCKS") == sr.GRID_CAP and constant("SSIM_WINDOW") == ssim.WINDOW
    (n, H, W, _), _ = sr.CASES["grid cap 1x17x16385x1"]
    tiles = n * -(-H // sr.TILE[0]) * -(-W // sr.TILE[1])
    assert sr.GRID_CAP < tiles <= 2 * sr.GRID_CAP  # the case walks a second tile, once


def test_scratch_is_zero_outside_the_limits_monotone_inside_and_the_documented_formula():
    from deodr_amd import hip_renderer as hr

    need = hr.lib().deodr_hip_ssim_scratch_bytes
    for n, H, W, Cn in ((0, 8, 8, 3), (-1, 8, 8, 3), (1, 0, 8, 3), (1, 8, 0, 3), (1, 8, -8, 3), (1, 8, 8, 0), (1, 8, 8, -1), (64, 2**15, 2**15, 16)):
        assert need(n, H, W, Cn) == 0, (n, H, W, Cn)
    # 64 bytes of counter words, 2 doubles per workgroup of at most 1024, three maps of doubles: 24 n H W C bytes
    for n, H, W, Cn in ((1, 1, 1, 1), (3, 17, 23, 5), (8, 1024, 1024, 4)):
        assert need(n, H, W, Cn) == 64 + 8 * (2 * 1024 + 3 * n * H * W * Cn), (n, H, W, Cn)
    base = (2, 100, 90, 3)
    for axis, values in ((0, (1, 2, 3, 7, 64)), (1, (1, 15, 16, 17, 100, 1000)), (2, (1, 31, 32, 33, 90, 4096)), (3, (1, 2, 3, 4, 5, 17))):
        sizes = []
        for v in values:
            args = list(base)
            args[axis] = v
            sizes.append(need(*args))
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes), (axis, sizes)


def test_bad_arguments_are_refused_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from abi_cases import entry, misaligned, nulls, overlap_placements
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    n, H, W, Cn = 2, 20, 30, 3
    base = dict(image=0x10000000, obs=0x11000000, weights=0x12000000, mix=0x13000000, terms=0x14000000, loss=0x15000000, image_b=0x16000000,
                scratch=0x17000000)  # fmt: skip

    call = entry(L, _abi.SSIM_HEADER, "deodr_hip_ssim_l2", base, n=n, H=H, W=W, C=Cn, pixel_dtype=hr._F64, data_range=1.0,
                 scratch_bytes=lambda a: L.deodr_hip_ssim_scratch_bytes(a["n"], a["H"], a["W"], a["C"]))  # fmt: skip
    what = "ssim_l2"
    for bad in nulls(("image", "obs", "mix", "terms", "scratch")):  # a NULL that is not allowed
        rc, msg = call(**bad)
        assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (bad, msg)
    for bad in (dict(n=0), dict(H=0), dict(W=-1), dict(C=0), dict(C=-3)):
        assert call(**bad) == (1, what + ": n, H, W and C must be >= 1"), bad
    assert call(n=64, H=2**15, W=2**15, C=16) == (1, what + ": n H W C must be below 2^40")
    for bad in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert call(data_range=bad) == (1, what + ": data_range must be finite and > 0"), bad
    for bad in (2, -1, 7):
        assert call(pixel_dtype=bad) == (1, what + ": pixel_dtype must be DEODR_HIP_F32 or DEODR_HIP_F64"), bad
    for p in ("image", "obs", "weights", "image_b"):  # aligned to their element
        assert call(**{p: base[p] + 4}) == (1, what + ": misaligned pointer"), p
        assert call(pixel_dtype=hr._F32, **{p: base[p] + 2}) == (1, what + ": misaligned pointer"), p
    for bad in misaligned(base, ("mix", "terms", "loss", "scratch"), 4):
        assert call(**bad) == (1, what + ": misaligned pointer"), bad
    need = L.deodr_hip_ssim_scratch_bytes(n, H, W, Cn)
    for short in (0, 64, need - 1):
        assert call(scratch_bytes=short) == (1, what + ": scratch too small (deodr_hip_ssim_scratch_bytes)"), short
    frame, pixels = 8 * n * H * W * Cn, 8 * n * H * W
    sizes = dict(image=frame, obs=frame, weights=pixels, mix=16, terms=16, loss=8, image_b=frame, scratch=need)
    refusal = (1, what + ": an output must not overlap an input, the scratch or another output")
    for out in ("terms", "loss", "image_b", "scratch"):
        for other in sizes:
            if other != out:
                for at in overlap_placements(base, sizes, out, other):
                    assert call(**{out: at}) == refusal, (out, other, hex(at))
    # two things wrong at once: the checks run in the order above, and the first one speaks
    assert call(image=None, n=0) == (1, what + ": image, obs, mix, terms or scratch == NULL")
    assert call(n=0, pixel_dtype=7) == (1, what + ": n, H, W and C must be >= 1")
    assert call(data_range=0.0, pixel_dtype=7) == (1, what + ": data_range must be finite and > 0")
    assert call(pixel_dtype=7, image=base["image"] + 4) == (1, what + ": pixel_dtype must be DEODR_HIP_F32 or DEODR_HIP_F64")
    assert call(image=base["image"] + 4, scratch_bytes=need - 1) == (1, what + ": misaligned pointer")
    assert call(scratch_bytes=need - 1, terms=base["image"]) == (1, what + ": scratch too small (deodr_hip_ssim_scratch_bytes)")


def test_host_wrapper_checks_its_tensors_before_the_library(monkeypatch):
    import torch

    from abi_cases import no_library
    from abi_cases import on_device as dev
    from deodr_amd import hip_renderer as hr

    monkeypatch.setattr(hr, "lib", no_library)
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    image, mix = f64(2, 5, 6, 3), f64(2)
    with pytest.raises(ValueError, match="image must be a ROCm tensor"):
        hr.ssim_l2(image, image, None, mix)

    I, O, M = dev(image), dev(f64(2, 5, 6, 3)), dev(mix)
    with pytest.raises(ValueError, match=r"image must have shape \[n >= 1, H >= 1, W >= 1, C >= 1\]"):
        hr.ssim_l2(dev(f64(5, 6, 3)), O, None, M)
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="data_range must be finite and > 0"):
            hr.ssim_l2(I, O, None, M, data_range=bad)
    with pytest.raises(ValueError, match=r"obs must have shape \[2, 5, 6, 3\]"):
        hr.ssim_l2(I, dev(f64(2, 5, 6, 4)), None, M)
    with pytest.raises(ValueError, match="obs must be float64"):
        hr.ssim_l2(I, dev(image.float()), None, M)
    with pytest.raises(ValueError, match="image must be float32 or float64"):
        hr.ssim_l2(dev(image.half()), O, None, M)
    with pytest.raises(ValueError, match=r"mix must have shape \[2\]"):
        hr.ssim_l2(I, O, None, dev(f64(3)))
    with pytest.raises(ValueError, match="mix must be float64"):
        hr.ssim_l2(I, O, None, dev(mix.float()))
    with pytest.raises(ValueError, match="mix must be a ROCm tensor"):
        hr.ssim_l2(I, O, None, mix)
    with pytest.raises(ValueError, match=r"weights must have shape \[2, 5, 6\]"):
        hr.ssim_l2(I, O, dev(f64(5, 6)), M)
    with pytest.raises(ValueError, match="weights must be contiguous"):
        hr.ssim_l2(I, O, dev(f64(2, 6, 5).transpose(1, 2)), M)
    with pytest.raises(ValueError, match=r"terms must have shape \[2\]"):
        hr.ssim_l2(I, O, None, M, terms=dev(f64(3)))
    with pytest.raises(ValueError, match=r"image_b must have shape \[2, 5, 6, 3\]"):
        hr.ssim_l2(I, O, None, M, image_b=dev(f64(2, 5, 6)))
    with pytest.raises(ValueError, match="scratch must be uint8"):
        hr.ssim_l2(I, O, None, M, scratch=dev(torch.zeros(64)))
