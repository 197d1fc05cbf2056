"""What the CPU tests of the C ABI's refusals share (tests/test_*_abi.py): calls of an entry point by the header's own parameter names, the three
families of bad pointers (NULL, misaligned, overlapping), and the stand-ins of the host-wrapper tests.  These produce cases; what the library must
answer to each stays in the test, with its exact message."""

import torch


def entry(L, header, name, base=(), **defaults):
    """-> call(**changed) -> (rc, last error) of the library's `name`.  Arguments go by the parameter names of the header's prototype and are laid
    out in its order: `changed` over `defaults` over `base` (the fake pointers; it may hold more than this prototype takes), `stream` None unless
    given.  A callable among `defaults` is called with the other arguments by name, on every call (a scratch size that follows the dimensions of the
    call, computed whether or not `changed` then overrides it).  A parameter nobody supplied, or a name the prototype does not have, raises here."""
    names = header.parameters[name]
    function = getattr(L, name)

    def call(**changed):
        given = {"stream": None, **dict(base), **defaults, **changed}
        missing, unknown = [p for p in names if p not in given], [p for p in {**defaults, **changed} if p not in names]
        if missing or unknown:
            raise TypeError(f"{name}: not supplied {missing}, not parameters {unknown}")
        plain = {p: given[p] for p in names if not callable(given[p])}
        computed = {p: v(plain) for p, v in defaults.items() if callable(v)}
        rc = function(*(computed[p] if callable(given[p]) else given[p] for p in names))
        return rc, L.deodr_hip_last_error().decode()

    return call


def nulls(pointers):
    """each pointer NULL in turn"""
    return ({p: None} for p in pointers)


def misaligned(base, pointers, step):
    """each pointer `step` bytes off its (aligned) fake address in turn"""
    return ({p: base[p] + step} for p in pointers)


def overlap_placements(base, sizes, out, other, unit=8):
    """where `out` overlaps `other`: at its start, over its last `unit` bytes, and ending `unit` bytes into it"""
    return (base[other], base[other] + sizes[other] - unit, base[other] - sizes[out] + unit)


def no_library():
    """stands in for hip_renderer.lib where a wrapper must refuse before it reaches the library"""
    raise AssertionError("the library was reached")


class OnDevice(torch.Tensor):
    """a CPU tensor that claims to be on the device: reaches the checks behind the device check"""

    is_cuda = property(lambda self: True)
    device = property(lambda self: torch.device("cuda", 0))


def on_device(t):
    return t.as_subclass(OnDevice)
