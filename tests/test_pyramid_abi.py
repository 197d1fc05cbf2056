"""CPU checks of the multi-scale L2 data term at the C ABI (include/deodr_hip_pyramid.h; the header itself: tests/test_companion_headers.py):
every bad argument of the launching entry point is refused through its error code with a message before any launch (fake pointers, no GPU), the
scratch size is 0 outside the limits and monotone inside them, and the host wrapper refuses CPU tensors, wrong dtypes and wrong shapes without
reaching the library."""

import pytest


def test_the_level_limit_is_the_header_s():
    from deodr_amd import hip_renderer as hr
    from deodr_amd import pyramid

    assert hr.PYRAMID_MAX_LEVELS == pyramid.MAX_LEVELS == 8


def test_scratch_is_zero_outside_the_limits_and_monotone_inside():
    from deodr_amd import hip_renderer as hr

    need = hr.lib().deodr_hip_pyramid_scratch_bytes
    for n, H, W, Cn, levels in ((0, 8, 8, 3, 3), (-1, 8, 8, 3, 3), (1, 0, 8, 3, 3), (1, 8, 0, 3, 3), (1, 8, -8, 3, 3), (1, 8, 8, 0, 3), (1, 8, 8, -1, 3),
                                (1, 8, 8, 3, 0), (1, 8, 8, 3, 9), (1, 8, 8, 3, -1), (64, 2**15, 2**15, 16, 3)):  # fmt: skip
        assert need(n, H, W, Cn, levels) == 0, (n, H, W, Cn, levels)
    # levels <= 3: the partials of the tile kernel alone, whatever the frame
    assert need(1, 1, 1, 1, 1) == need(8, 1024, 1024, 4, 3) == 64 + 8 * 4 * 1024
    # levels > 3: + 5 doubles per region of 32 x 32 tiles and 1 + 2 C doubles per tile
    assert need(1, 16, 16, 4, 4) == 64 + 8 * (4 * 1024 + 5 + 4 * 9)
    assert need(3, 17, 23, 4, 5) == 64 + 8 * (4 * 1024 + 3 * 5 + 3 * 9 * 9)
    assert need(1, 520, 264, 2, 8) == 64 + 8 * (4 * 1024 + 3 * 2 * 5 + 65 * 33 * 5)
    base = (2, 100, 90, 3, 3)
    for axis, values in ((0, (1, 2, 3, 7, 64)), (1, (1, 8, 9, 100, 255, 256, 257, 1000)), (2, (1, 8, 9, 90, 256, 257, 4096)), (3, (1, 2, 3, 4, 5, 17)),
                         (4, (1, 2, 3, 4, 5, 6, 7, 8))):  # fmt: skip
        for levels in (3, 4, 8):
            sizes = []
            for v in values:
                args = list(base[:4]) + [levels]
                args[axis] = v
                sizes.append(need(*args))
            assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (axis, levels, sizes)


def test_bad_arguments_are_refused_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from abi_cases import entry, misaligned, nulls, overlap_placements
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    n, H, W, Cn, levels = 2, 20, 30, 3, 5
    base = dict(image=0x10000000, obs=0x11000000, weights=0x12000000, level_weights=0x13000000, terms=0x14000000, loss=0x15000000, image_b=0x16000000,
                scratch=0x17000000)  # fmt: skip

    call = entry(L, _abi.PYRAMID_HEADER, "deodr_hip_pyramid_l2", base, n=n, H=H, W=W, C=Cn, pixel_dtype=hr._F64, levels=levels,
                 scratch_bytes=lambda a: L.deodr_hip_pyramid_scratch_bytes(a["n"], a["H"], a["W"], a["C"], a["levels"]))  # fmt: skip
    what = "pyramid_l2"
    for bad in nulls(("image", "obs", "level_weights", "terms", "scratch")):  # a NULL that is not allowed
        rc, msg = call(**bad)
        assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (bad, msg)
    for bad in (0, -1, 9, 100):
        assert call(levels=bad) == (1, what + ": levels must be in 1 .. 8"), bad
    for bad in (0, -3):
        assert call(C=bad) == (1, what + ": C must be >= 1"), bad
    for bad in (dict(n=0), dict(H=0), dict(W=-1)):
        assert call(**bad) == (1, what + ": n, H and W must be >= 1"), bad
    assert call(n=64, H=2**15, W=2**15, C=16) == (1, what + ": n H W C must be below 2^40")
    for bad in (2, -1, 7):
        assert call(pixel_dtype=bad) == (1, what + ": pixel_dtype must be DEODR_HIP_F32 or DEODR_HIP_F64"), bad
    for p in ("image", "obs", "weights", "image_b"):  # aligned to their element
        assert call(**{p: base[p] + 4}) == (1, what + ": misaligned pointer"), p
        assert call(pixel_dtype=hr._F32, **{p: base[p] + 2}) == (1, what + ": misaligned pointer"), p
    for bad in misaligned(base, ("level_weights", "terms", "loss", "scratch"), 4):
        assert call(**bad) == (1, what + ": misaligned pointer"), bad
    need = L.deodr_hip_pyramid_scratch_bytes(n, H, W, Cn, levels)
    for short in (0, 64, need - 1):
        assert call(scratch_bytes=short) == (1, what + ": scratch too small (deodr_hip_pyramid_scratch_bytes)"), short
    frame, pixels = 8 * n * H * W * Cn, 8 * n * H * W
    sizes = dict(image=frame, obs=frame, weights=pixels, level_weights=8 * (levels + 1), terms=8 * (levels + 1), loss=8, image_b=frame, scratch=need)
    refusal = (1, what + ": an output must not overlap an input, the scratch or another output")
    for out in ("terms", "loss", "image_b", "scratch"):
        for other in sizes:
            if other != out:
                for at in overlap_placements(base, sizes, out, other):
                    assert call(**{out: at}) == refusal, (out, other, hex(at))
    # two things wrong at once: the checks run in the order above, and the first one speaks
    assert call(image=None, n=0) == (1, what + ": image, obs, level_weights, terms or scratch == NULL")
    assert call(n=0, pixel_dtype=7) == (1, what + ": n, H and W must be >= 1")
    assert call(pixel_dtype=7, image=base["image"] + 4) == (1, what + ": pixel_dtype must be DEODR_HIP_F32 or DEODR_HIP_F64")
    assert call(image=base["image"] + 4, scratch_bytes=need - 1) == (1, what + ": misaligned pointer")
    assert call(scratch_bytes=need - 1, terms=base["image"]) == (1, what + ": scratch too small (deodr_hip_pyramid_scratch_bytes)")


def test_host_wrapper_checks_its_tensors_before_the_library(monkeypatch):
    import torch

    from abi_cases import no_library
    from abi_cases import on_device as dev
    from deodr_amd import hip_renderer as hr

    monkeypatch.setattr(hr, "lib", no_library)
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    image, lam = f64(2, 5, 6, 3), f64(4)
    with pytest.raises(ValueError, match="image must be a ROCm tensor"):
        hr.pyramid_l2(image, image, None, 3, lam)

    I, O, Lw = dev(image), dev(f64(2, 5, 6, 3)), dev(lam)
    with pytest.raises(ValueError, match=r"image must have shape \[n >= 1, H >= 1, W >= 1, C >= 1\]"):
        hr.pyramid_l2(dev(f64(5, 6, 3)), O, None, 3, Lw)
    for levels in (0, 9):
        with pytest.raises(ValueError, match="levels must be in 1 .. 8"):
            hr.pyramid_l2(I, O, None, levels, Lw)
    with pytest.raises(ValueError, match=r"obs must have shape \[2, 5, 6, 3\]"):
        hr.pyramid_l2(I, dev(f64(2, 5, 6, 4)), None, 3, Lw)
    with pytest.raises(ValueError, match="obs must be float64"):
        hr.pyramid_l2(I, dev(image.float()), None, 3, Lw)
    with pytest.raises(ValueError, match="image must be float32 or float64"):
        hr.pyramid_l2(dev(image.half()), O, None, 3, Lw)
    with pytest.raises(ValueError, match=r"level_weights must have shape \[4\]"):
        hr.pyramid_l2(I, O, None, 3, dev(f64(3)))
    with pytest.raises(ValueError, match="level_weights must be float64"):
        hr.pyramid_l2(I, O, None, 3, dev(lam.float()))
    with pytest.raises(ValueError, match="level_weights must be a ROCm tensor"):
        hr.pyramid_l2(I, O, None, 3, lam)
    with pytest.raises(ValueError, match=r"weights must have shape \[2, 5, 6\]"):
        hr.pyramid_l2(I, O, dev(f64(5, 6)), 3, Lw)
    with pytest.raises(ValueError, match="weights must be contiguous"):
        hr.pyramid_l2(I, O, dev(f64(2, 6, 5).transpose(1, 2)), 3, Lw)
    with pytest.raises(ValueError, match=r"terms must have shape \[4\]"):
        hr.pyramid_l2(I, O, None, 3, Lw, terms=dev(f64(5)))
    with pytest.raises(ValueError, match=r"image_b must have shape \[2, 5, 6, 3\]"):
        hr.pyramid_l2(I, O, None, 3, Lw, image_b=dev(f64(2, 5, 6)))
    with pytest.raises(ValueError, match="scratch must be uint8"):
        hr.pyramid_l2(I, O, None, 3, Lw, scratch=dev(torch.zeros(64)))
