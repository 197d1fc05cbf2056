"""CPU checks of linear blend skinning at the C ABI (include/deodr_hip_skinning.h; the header itself: tests/test_companion_headers.py): its tables
are device arrays, every bad argument of the two launching entry points is refused with a message before any launch (fake pointers, no GPU), the
scratch size is what the header says and 0 outside the limits, the host wrappers refuse CPU tensors, wrong dtypes and wrong shapes without
reaching the library, and ``Skin`` refuses every table the header's model does not allow."""

import re

import numpy as np
import pytest


def test_the_tables_are_device_arrays():
    from deodr_amd import _abi

    text = open(_abi.SKINNING_HEADER_PATH).read()
    assert not re.search(r"\bint\s*\*", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))  # the tables are device arrays: uint32_t *, never int * (host memory to _abi)


def test_scratch_follows_the_header_and_is_zero_outside_the_limits():
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    assert (hr.SKIN_MAX_VIEWS, hr.SKIN_MAX_JOINTS, hr.SKIN_MAX_INFLUENCES, hr.SKIN_MAX_VERTICES) == (64, 256, 8, 2**24)
    for V, J, K, n in ((0, 4, 2, 1), (-1, 4, 2, 1), (2**24 + 1, 4, 2, 1), (10, 0, 2, 1), (10, 257, 2, 1), (10, -4, 2, 1), (10, 4, 0, 1), (10, 4, 9, 1),
                       (10, 4, -1, 1), (10, 4, 2, 0), (10, 4, 2, 65), (10, 4, 2, -2)):  # fmt: skip
        assert L.deodr_hip_skin_scratch_bytes(V, J, K, n) == 0, (V, J, K, n)
    for V, J, K, n in ((1, 1, 1, 1), (2**24, 256, 8, 64), (526, 4, 2, 1), (33, 17, 7, 2)):
        assert L.deodr_hip_skin_scratch_bytes(V, J, K, n) == 64 + 80 * n * J, (V, J, K, n)


def test_bad_arguments_are_refused_before_any_launch():
    """every pointer below is fake and never dereferenced: a refusal happens before any HIP call"""
    from abi_cases import entry, misaligned, nulls
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    V, J, K, n, nnz = 100, 4, 2, 2, 150
    base = dict(vertices=0x10000000, joints=0x11000000, parents=0x12000000, quaternions=0x13000000, indices=0x14000000, weights=0x15000000,
                world=0x16000000, posed=0x17000000, posed_b=0x17000000, joint_offsets=0x18000000, joint_slots=0x19000000, vertices_b=0x1A000000,
                quaternions_b=0x1B000000, joints_b=0x1C000000, scratch=0x1D000000)  # fmt: skip
    apply = entry(L, _abi.SKINNING_HEADER, "deodr_hip_skin_apply", base, V=V, J=J, K=K, n=n)
    apply_b = entry(L, _abi.SKINNING_HEADER, "deodr_hip_skin_apply_b", base, V=V, J=J, K=K, n=n, nnz=nnz,
                    scratch_bytes=lambda a: L.deodr_hip_skin_scratch_bytes(a["V"], a["J"], a["K"], a["n"]))  # fmt: skip

    inputs = ("vertices", "joints", "parents", "quaternions", "indices", "weights")
    for call, what, required in ((apply, "skin_apply", inputs + ("world", "posed")),
                                 (apply_b, "skin_apply_b", inputs + ("world", "posed_b", "joint_offsets", "joint_slots", "scratch"))):  # fmt: skip
        for bad in nulls(required):  # a NULL among the required pointers
            rc, msg = call(**bad)
            assert rc == 1 and msg.startswith(what + ":") and "== NULL" in msg, (bad, msg)
        for bad in (dict(n=0), dict(n=-1), dict(n=65)):
            assert call(**bad) == (1, what + ": n must be in 1 .. 64"), bad
        for bad in (dict(J=0), dict(J=-3), dict(J=257)):
            assert call(**bad) == (1, what + ": J must be in 1 .. 256"), bad
        for bad in (dict(K=0), dict(K=-1), dict(K=9)):
            assert call(**bad) == (1, what + ": K must be in 1 .. 8"), bad
        for bad in (dict(V=0), dict(V=-7), dict(V=2**24 + 1)):
            assert call(**bad) == (1, what + ": V must be in 1 .. 2^24"), bad
        doubles = ("vertices", "joints", "quaternions", "weights", "world") + (("posed_b", "vertices_b", "quaternions_b", "joints_b", "scratch") if call is apply_b else ("posed",))
        for bad in misaligned(base, doubles, 4):
            assert call(**bad) == (1, what + ": misaligned pointer"), bad
        for bad in misaligned(base, ("parents", "indices") + (("joint_offsets", "joint_slots") if call is apply_b else ()), 2):  # 4-byte aligned
            assert call(**bad) == (1, what + ": misaligned pointer"), bad
    # bytes: vertices(_b) 2400, joints(_b) 96, parents 16, quaternions(_b) 256, indices 800, weights 1600, world 448, posed(_b) 4800, offsets 20, slots 600
    sizes = dict(vertices=2400, joints=96, parents=16, quaternions=256, indices=800, weights=1600, world=448, posed=4800, posed_b=4800, joint_offsets=20,
                 joint_slots=600, vertices_b=2400, quaternions_b=256, joints_b=96)  # fmt: skip
    refusal = (1, "skin_apply: an output must not overlap an input or the other output")
    for out in ("world", "posed"):
        for inp in inputs:
            for at in (base[inp], base[inp] + (sizes[inp] - 4) // 8 * 8, base[inp] - sizes[out] + 8):
                assert apply(**{out: at}) == refusal, (out, inp, hex(at))
    assert apply(world=base["posed"] + 4792) == refusal and apply(posed=base["world"] + 440) == refusal
    # the adjoint's own refusals
    what = "skin_apply_b"
    assert apply_b(vertices_b=None, quaternions_b=None, joints_b=None) == (1, what + ": no output requested (vertices_b, quaternions_b, joints_b)")
    for keep in ("vertices_b", "quaternions_b", "joints_b"):  # each alone is a request
        others = {k: None for k in ("vertices_b", "quaternions_b", "joints_b") if k != keep}
        assert apply_b(**others, V=0) == (1, what + ": V must be in 1 .. 2^24")  # (past the output check)
    for bad in (-1, V * K + 1):
        assert apply_b(nnz=bad) == (1, what + ": nnz must be in 0 .. V K"), bad
    need = L.deodr_hip_skin_scratch_bytes(V, J, K, n)
    for short in (0, 8, need - 1):
        assert apply_b(scratch_bytes=short) == (1, what + ": scratch too small (deodr_hip_skin_scratch_bytes)"), short
    refusal = (1, what + ": an output must not overlap an input, the scratch or another output")
    for out in ("vertices_b", "quaternions_b", "joints_b"):
        for inp in inputs + ("world", "posed_b", "joint_offsets", "joint_slots"):
            for at in (base[inp], base[inp] + (sizes[inp] - 4) // 8 * 8, base[inp] - sizes[out] + 8):
                assert apply_b(**{out: at}) == refusal, (out, inp, hex(at))
        assert apply_b(**{out: base["scratch"] + 64}) == refusal and apply_b(**{out: base["scratch"] + need - 8}) == refusal, out
    assert apply_b(quaternions_b=base["vertices_b"] + 2392) == refusal and apply_b(joints_b=base["quaternions_b"] + 248) == refusal
    assert apply_b(joints_b=base["vertices_b"] - 88) == refusal and apply_b(scratch=base["vertices"] - 64) == refusal


def test_host_wrappers_check_their_tensors_before_the_library(monkeypatch):
    import torch

    from abi_cases import no_library
    from abi_cases import on_device as dev
    from deodr_amd import hip_renderer as hr

    monkeypatch.setattr(hr, "lib", no_library)
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    V, J, K, n = 10, 4, 2, 2
    v, c, par, q, idx, w = f64(V, 3), f64(J, 3), i32(J), f64(n, J, 4), i32(V, K), f64(V, K)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.skin_apply(v, c, par, q, idx, w)
    with pytest.raises(ValueError, match="ROCm tensor"):
        hr.skin_apply_b(v, c, par, q, idx, w, f64(n, J, 7), f64(n, V, 3), i32(J + 1), i32(5))

    Vt, Ct, P, Q, I, W = (dev(t) for t in (v, c, par, q, idx, w))
    with pytest.raises(ValueError, match=r"vertices must have shape \[1 <= V <= 2\^24, 3\]"):
        hr.skin_apply(dev(f64(V, 2)), Ct, P, Q, I, W)
    with pytest.raises(ValueError, match=r"quaternions must have shape \[1 <= n <= 64, 1 <= J <= 256, 4\]"):
        hr.skin_apply(Vt, Ct, P, dev(f64(65, J, 4)), I, W)
    with pytest.raises(ValueError, match=r"quaternions must have shape"):
        hr.skin_apply(Vt, Ct, P, dev(f64(J, 4)), I, W)
    with pytest.raises(ValueError, match=r"indices must have shape \[10, 1 <= K <= 8\]"):
        hr.skin_apply(Vt, Ct, P, Q, dev(i32(V, 9)), W)
    with pytest.raises(ValueError, match=r"joints must have shape \[4, 3\]"):
        hr.skin_apply(Vt, dev(f64(J + 1, 3)), P, Q, I, W)
    with pytest.raises(ValueError, match="parents must be int32"):
        hr.skin_apply(Vt, Ct, dev(par.long()), Q, I, W)
    with pytest.raises(ValueError, match="indices must be int32"):
        hr.skin_apply(Vt, Ct, P, Q, dev(idx.long()), W)
    with pytest.raises(ValueError, match=r"weights must have shape \[10, 2\]"):
        hr.skin_apply(Vt, Ct, P, Q, I, dev(f64(V, 3)))
    with pytest.raises(ValueError, match="vertices must be float64"):
        hr.skin_apply(dev(v.float()), Ct, P, Q, I, W)
    with pytest.raises(ValueError, match="weights must be contiguous"):
        hr.skin_apply(Vt, Ct, P, Q, I, dev(f64(K, V).t()))
    with pytest.raises(ValueError, match=r"posed must have shape \[2, 10, 3\]"):
        hr.skin_apply(Vt, Ct, P, Q, I, W, posed=dev(f64(n, V, 2)))
    world, posed_b, off, slots = dev(f64(n, J, 7)), dev(f64(n, V, 3)), dev(i32(J + 1)), dev(i32(5))
    with pytest.raises(ValueError, match=r"world must have shape \[2, 4, 7\]"):
        hr.skin_apply_b(Vt, Ct, P, Q, I, W, dev(f64(n, J, 12)), posed_b, off, slots)
    with pytest.raises(ValueError, match=r"joint_offsets must have shape \[5\]"):
        hr.skin_apply_b(Vt, Ct, P, Q, I, W, world, posed_b, dev(i32(J)), slots)
    with pytest.raises(ValueError, match="joint_slots must have at most V K = 20 entries"):
        hr.skin_apply_b(Vt, Ct, P, Q, I, W, world, posed_b, off, dev(i32(21)))
    with pytest.raises(ValueError, match=r"quaternions_b must have shape \[2, 4, 4\]"):
        hr.skin_apply_b(Vt, Ct, P, Q, I, W, world, posed_b, off, slots, quaternions_b=dev(f64(J, 4)))
    with pytest.raises(ValueError, match="scratch must be uint8"):
        hr.skin_apply_b(Vt, Ct, P, Q, I, W, world, posed_b, off, slots, scratch=dev(torch.zeros(64)))
    with pytest.raises(ValueError, match="no output requested"):
        hr.skin_apply_b(Vt, Ct, P, Q, I, W, world, posed_b, off, slots, want=(False, False, False))


def test_skin_refuses_every_table_the_model_does_not_allow():
    from deodr_amd.skinning import ROOT, Skin

    joints = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]])
    indices, weights = np.array([[0, 1], [1, 2], [2, 0]]), np.array([[0.5, 0.5], [0.25, 0.75], [1.0, 0.0]])
    good = Skin(joints, [ROOT, 0, 1], (indices, weights), device="cpu")
    assert (good.V, good.J, good.K) == (3, 3, 2) and ROOT == -1
    assert good.parents.dtype == good.indices.dtype == good.joint_slots.dtype == good.joint_offsets.dtype
    assert good.parents.tolist() == [-1, 0, 1]  # 0xFFFFFFFF as int32
    assert good.joint_offsets_np.tolist() == [0, 1, 3, 5] and good.joint_slots_np.tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match=r"parents\[0\] must be the root marker"):
        Skin(joints, [0, 0, 1], (indices, weights), device="cpu")
    for parents in ([ROOT, 1, 1], [ROOT, 0, 2], [ROOT, 0, 5], [ROOT, ROOT, 0]):  # parents[j] >= j, or no parent at all
        with pytest.raises(ValueError, match=r"parents\[\d\] = -?\d must be in 0 \.\."):
            Skin(joints, parents, (indices, weights), device="cpu")
    for bad in (3, 7, -1):
        with pytest.raises(ValueError, match="an index is outside 0 .. 2"):
            Skin(joints, [ROOT, 0, 1], (np.where(indices == 2, bad, indices), weights), device="cpu")
    with pytest.raises(ValueError, match="a weight is negative"):
        Skin(joints, [ROOT, 0, 1], (indices, np.array([[1.5, -0.5], [0.25, 0.75], [1.0, 0.0]])), device="cpu")
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="a weight is not finite"):
            Skin(joints, [ROOT, 0, 1], (indices, np.array([[0.5, 0.5], [bad, 0.75], [1.0, 0.0]])), device="cpu")
    with pytest.raises(ValueError, match="the weights of row 1 do not sum to 1 within 1e-9"):
        Skin(joints, [ROOT, 0, 1], (indices, np.array([[0.5, 0.5], [0.25, 0.75 + 1e-8], [1.0, 0.0]])), device="cpu")
    Skin(joints, [ROOT, 0, 1], (indices, np.array([[0.5, 0.5], [0.25, 0.75 + 1e-10], [1.0, 0.0]])), device="cpu")  # within 1e-9
    nine = np.zeros((2, 10))
    nine[:, :9] = 1.0 / 9
    chain = [ROOT] + list(range(9))
    with pytest.raises(ValueError, match="more than 8 non-zero weights"):
        Skin(np.zeros((10, 3)), chain, nine, device="cpu")
    with pytest.raises(ValueError, match="more than 8 non-zero weights"):
        Skin(np.zeros((10, 3)), chain, (np.tile(np.arange(10), (2, 1)), nine), device="cpu")
    with pytest.raises(ValueError, match="at most 8 columns"):
        Skin(np.zeros((10, 3)), chain, (np.tile(np.arange(10), (2, 1)), np.eye(10)[:2]), device="cpu")
    eight = np.zeros((2, 10))
    eight[:, 2:] = 0.125
    assert Skin(np.zeros((10, 3)), chain, eight, device="cpu").K == 8
    with pytest.raises(ValueError, match=r"dense weights must have shape \[V, 3\]"):
        Skin(joints, [ROOT, 0, 1], np.ones((4, 2)) / 2, device="cpu")
    with pytest.raises(ValueError, match="joints must have shape"):
        Skin(np.zeros((257, 3)), [ROOT] + list(range(256)), np.ones((1, 257)), device="cpu")
