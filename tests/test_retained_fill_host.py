"""CPU checks of the retained background fill: what only include/deodr_hip_retained.h says at the C ABI (the header itself:
tests/test_companion_headers.py), and -- with
tests/fake_hip.py standing in for the library -- WHEN HipRasterizer.render_fit tells the library that the buffers still hold the previous frame.
The fake renders every frame in full whatever it is told: what is under test is the claim, call by call."""

import ctypes as C
import types

import pytest
import torch

import fake_hip
from deodr_amd import scenes

ENTRY = "deodr_hip_render_scene_fit_retained"


def test_the_entry_is_fit_ex_with_the_claim_and_points_to_the_main_header_s_structs():
    from deodr_amd import _abi

    h = _abi.RETAINED_HEADER
    assert _abi.HEADER.defines["DEODR_HIP_ABI_VERSION"] == 13
    # deodr_hip_render_scene_fit_ex's arguments with `retained` between the options and the workspace; the structs are the main header's
    ex = _abi.HEADER.functions["deodr_hip_render_scene_fit_ex"][1]
    assert h.functions[ENTRY][1] == ex[:7] + [C.c_int] + ex[7:]
    with pytest.raises(ImportError, match=r"include/deodr_hip_retained\.h: no ctypes type for `const DeodrHipScene \*`"):
        _abi.parse(open(_abi.RETAINED_HEADER_PATH).read(), "include/deodr_hip_retained.h")  # (without the main header's structs)


def test_the_workspace_holds_one_more_tile_bitmap_per_view():
    from deodr_amd import hip_renderer as hr

    # one more tile bitmap per view than one bitmap's worth: 64 x 64 pixels are 64 tiles, two words
    L = hr.lib()
    assert L.deodr_hip_workspace_bytes(10, 64, 64, 3, 2, 0) == 2 * L.deodr_hip_workspace_bytes(10, 64, 64, 3, 1, 0) > 0


class RetainedLib(fake_hip.FakeLib):
    """FakeLib + the retained entry: records `retained` and renders as the plain entries do"""

    def __init__(self, checker, checker_repaired):
        super().__init__(checker, checker_repaired)
        self.retained = []
        self.fail_next = False  # the next call of the retained entry returns an error without rendering

    def __getattribute__(self, name):
        if name != ENTRY:
            return super().__getattribute__(name)
        from deodr_amd import _abi

        argtypes = _abi.RETAINED_HEADER.functions[name][1]

        def checked(*args):
            assert len(args) == len(argtypes), name
            for argtype, arg in zip(argtypes, args):
                argtype.from_param(arg)
            sc, image, z, sigma, obs, clear, options, retained, ws, nbytes, stream = args
            self.retained.append(retained)
            if self.fail_next:
                self.fail_next = False
                return 1
            if options is None:
                return self.deodr_hip_render_scene_fit(sc, image, z, sigma, obs, clear, ws, nbytes, stream)
            return self.deodr_hip_render_scene_fit_ex(sc, image, z, sigma, obs, clear, options, ws, nbytes, stream)

        return checked


@pytest.fixture
def fake(oracle_api, monkeypatch):
    with fake_hip.emulate(oracle_api.ref() or oracle_api.port(), oracle_api.ref(fixed=True) or oracle_api.port(fixed=True)) as plain:
        yield plain, monkeypatch


@pytest.fixture
def retained(fake):
    from deodr_amd import hip_renderer as hr

    plain, monkeypatch = fake
    lib = RetainedLib(plain.checker, plain.repaired)
    monkeypatch.setattr(hr, "lib", lambda: lib)
    yield lib
    monkeypatch.undo()  # (before emulate() restores what IT replaced)


def two_views():
    from hip_util import device_scene

    views = [scenes.soup_scene(n_tri=8, width=24, height=16, seed=5 + v, flat=False, min_area=10.0) for v in range(2)]
    return device_scene(views, torch.float64)


def frame(ds):
    return (torch.empty(ds.n_views, ds.height, ds.width, ds.nb_colors, dtype=torch.float64), torch.empty(ds.n_views, ds.height, ds.width, dtype=torch.float64))


def test_the_claim_call_by_call(retained, monkeypatch):
    from deodr_amd.hip_renderer import HipRasterizer

    ds = two_views()
    obs = torch.rand(2, 16, 24, 3, dtype=torch.float64)
    r = HipRasterizer.for_scene(ds)
    assert r.retain_frames is True
    out, grads = frame(ds), ds.zero_grads()
    fit = lambda **kw: r.render_fit(ds, obs, 1.0, **{**dict(grads=grads, out=out, check_overflow=False, clear_grads=True), **kw})
    last = lambda: retained.retained[-1]
    image_ref, z_ref, _ = HipRasterizer.for_scene(ds, retain_frames=False).render_fit(ds, obs, 1.0, check_overflow=False)
    assert retained.retained == []  # retain_frames=False: the entries of deodr_hip.h
    calls = retained.calls["render_scene_fit"]

    fit()
    assert last() == 0, "nothing has been rendered on this workspace"
    fit()
    assert last() == 1 and torch.equal(out[0], image_ref) and torch.equal(out[1], z_ref)
    assert retained.calls["render_scene_fit"] == calls + 2
    # torch saw an in-place operation on a buffer: once refused, then kept again
    out[0].fill_(7)
    fit()
    assert last() == 0 and torch.equal(out[0], image_ref)
    fit()
    assert last() == 1
    out[1].zero_()
    fit()
    assert last() == 0
    # other buffers, then the same ones again
    out = frame(ds)
    fit()
    assert last() == 0
    fit()
    assert last() == 1
    fit(out=None)
    assert last() == 0, "buffers of the call's own"
    fit()
    assert last() == 0, "the previous forward wrote other buffers"
    # the background: changed in place, replaced
    fit()
    assert last() == 1
    ds.background_image.mul_(0.5)
    fit()
    assert last() == 0
    fit()
    assert last() == 1
    ds.upload("background_image", ds.background_image.clone())
    fit()
    assert last() == 0
    # the options entry carries the claim too
    loss = torch.zeros(1, dtype=torch.float64)
    fit(loss_out=loss)
    assert last() == 1 and float(loss) > 0
    # a regrown workspace
    r._alloc(2048)
    fit()
    assert last() == 0
    fit()
    assert last() == 1
    # a forward that rendered no frame (the adjoint of a stale state rebuilds it)
    r.render_backward(ds, image_b=torch.ones_like(out[0]))
    fit()
    assert last() == 0
    # render(out=...) is a forward like any other
    r.render(ds, 1.0, out=out, check_overflow=False)
    fit()
    assert last() == 1
    # another stream
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=99))
    fit()
    assert last() == 0
    fit()
    assert last() == 1
    # a captured launch claims nothing, and nothing is known after it
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    fit()
    assert last() == 0
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    fit()
    assert last() == 0
    fit()
    assert last() == 1
    # a step the library refused (after its scan, for all the host knows): the next one claims nothing
    retained.fail_next = True
    with pytest.raises(RuntimeError, match="deodr_hip"):
        fit()
    assert last() == 1
    fit()
    assert last() == 0
    fit()
    assert last() == 1
    # switched off: the old entries; switched on again: the forward in between counts
    seen = len(retained.retained)
    r.retain_frames = False
    fit()
    assert len(retained.retained) == seen
    r.retain_frames = True
    fit()
    assert last() == 1 and len(retained.retained) == seen + 1


def test_a_library_without_the_entry_is_called_as_ever(fake):
    from deodr_amd.hip_renderer import HipRasterizer

    plain, _ = fake
    assert getattr(plain, ENTRY, None) is None
    ds = two_views()
    obs = torch.rand(2, 16, 24, 3, dtype=torch.float64)
    r = HipRasterizer.for_scene(ds)
    out = frame(ds)
    for _ in range(3):
        r.render_fit(ds, obs, 1.0, out=out, check_overflow=False, clear_grads=True)
    assert plain.calls["render_scene_fit"] == 3
    loss = torch.zeros(1, dtype=torch.float64)
    r.render_fit(ds, obs, 1.0, out=out, check_overflow=False, loss_out=loss)
    assert plain.calls["render_scene_fit"] == 4 and float(loss) > 0
