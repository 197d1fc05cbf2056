"""GPU checks of the stable sort by key (include/deodr_hip_chamfer_grid.h, deodr_amd/csrc/dr_sort.h): ``order`` and ``sorted_keys`` EQUAL to
NumPy's stable argsort.  N through 1, 2, around a wavefront, around a round of the scatter (256), around one and two workgroups' items (2 048,
4 096) and several workgroups with a ragged end -- the scan walks the workgroups of a row in one loop and the grid has no cap below
DEODR_HIP_SORT_MAX_ITEMS, so there is no further size at which the geometry changes --; ``bits`` 1, around one digit, two digits + 1, 24, 32;
n = 1 and 3; keys all equal, sorted, reversed, different in the top digit only, with high bits set above ``bits``; outputs between guards, the
scratch exactly ``deodr_hip_sort_keys_scratch_bytes`` long between guards and filled with a NaN pattern; two calls bit-identical; one graph
replayed over overwritten keys."""

import numpy as np
import pytest
import torch

import chamfer_grid_reference as gr

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD_WORDS, GUARD = 1024, 0x5A5A5A5A
ITEMS, BLOCK, DIGIT = gr.SORT_ITEMS, gr.SORT_BLOCK, gr.DIGIT_BITS
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, ITEMS - 1, ITEMS, ITEMS + 1, 2 * ITEMS - 1, 2 * ITEMS, 2 * ITEMS + 1, 5 * ITEMS + 77)
BITS = (1, DIGIT - 1, DIGIT, DIGIT + 1, 2 * DIGIT + 1, 24, 32)


def guarded(n, N):
    """[n, N] int32 between guards, pre-filled with the guard pattern"""
    buffer = torch.full((n * N + 2 * GUARD_WORDS,), GUARD, dtype=torch.int32, device=DEV)
    return buffer, buffer[GUARD_WORDS : GUARD_WORDS + n * N].view(n, N)


def intact(buffer, numel):
    return bool((buffer[:GUARD_WORDS] == GUARD).all()) and bool((buffer[GUARD_WORDS + numel :] == GUARD).all())


def keys_of(pattern, n, N, bits, seed):
    rs = np.random.RandomState(seed)
    top = 1 << bits
    if pattern == "random":
        k = rs.randint(0, 2**32, size=(n, N), dtype=np.uint64)
    elif pattern == "few":  # many equal keys: stability shows
        k = rs.randint(0, 5, size=(n, N)).astype(np.uint64) * np.uint64(max(1, top // 5))
    elif pattern == "equal":
        k = np.full((n, N), 0xDEADBEEF % top, dtype=np.uint64)
    elif pattern == "sorted":
        k = np.sort(rs.randint(0, top, size=(n, N), dtype=np.uint64), axis=1)
    elif pattern == "reversed":
        k = np.sort(rs.randint(0, top, size=(n, N), dtype=np.uint64), axis=1)[:, ::-1]
    elif pattern == "top digit":
        shift = DIGIT * ((bits - 1) // DIGIT)
        k = (rs.randint(0, 1 << (bits - shift), size=(n, N), dtype=np.uint64) << np.uint64(shift)) | np.uint64(0x2A & ((1 << shift) - 1))
    else:
        assert pattern == "high bits"  # set above `bits`: ignored by the order, kept in sorted_keys
        k = rs.randint(0, min(top, 7), size=(n, N), dtype=np.uint64) | (rs.randint(0, 2**32, size=(n, N), dtype=np.uint64) & np.uint64((0xFFFFFFFF << bits) & 0xFFFFFFFF))
    return np.ascontiguousarray(k).astype(np.uint32)


def check(keys, bits, want_sorted=True):
    from deodr_amd import hip_renderer as hr

    n, N = keys.shape
    need = int(hr.lib().deodr_hip_sort_keys_scratch_bytes(N, n, bits))
    assert need == gr.sort_scratch_bytes(N, n, bits) and need % 4 == 0
    assert hr.sort_keys_launches(N, n, bits) == gr.sort_launches(N, n, bits)
    k = torch.as_tensor(keys.view(np.int32), device=DEV)
    words = need // 4
    sbuf = torch.full((words + 2 * GUARD_WORDS,), GUARD, dtype=torch.int32, device=DEV)
    scratch = sbuf[GUARD_WORDS : GUARD_WORDS + words]
    scratch.fill_(0x7FC00000)  # a NaN pattern: the scratch need not be zeroed
    outs = []
    for _ in range(2):
        (sb, s), (ob, o) = guarded(n, N), guarded(n, N)
        got = hr.sort_keys(k, bits, sorted_keys=s if want_sorted else None, order=o, scratch=scratch.view(torch.uint8), want_sorted=want_sorted)
        assert got[1] is o and (got[0] is s if want_sorted else got[0] is None)
        outs.append((sb, s, ob, o))
    torch.cuda.synchronize()
    assert intact(sbuf, words), "written outside the scratch"
    for sb, s, ob, o in outs:
        assert intact(sb, n * N) and intact(ob, n * N), "written outside an output"
    assert torch.equal(outs[0][3], outs[1][3]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(k, torch.as_tensor(keys.view(np.int32), device=DEV))  # the keys are only read
    want_keys, want_order = gr.stable_order(keys, bits)
    assert np.array_equal(outs[0][3].cpu().numpy().view(np.uint32), want_order), (n, N, bits)
    if want_sorted:
        assert np.array_equal(outs[0][1].cpu().numpy().view(np.uint32), want_keys), (n, N, bits)
    else:
        assert bool((outs[0][1] == GUARD).all())  # not wanted: not written


@pytest.mark.parametrize("n", (1, 3))
@pytest.mark.parametrize("N", SIZES)
def test_sizes_against_numpy(N, n):
    for bits in BITS:
        check(keys_of("random", n, N, bits, seed=N + bits), bits)
    check(keys_of("few", n, N, 9, seed=N), 9)


@pytest.mark.parametrize("pattern", ("equal", "sorted", "reversed", "top digit", "high bits", "few"))
def test_key_patterns(pattern):
    for N in (257, ITEMS + 1, 2 * ITEMS + 300):
        for bits in BITS:
            check(keys_of(pattern, 3, N, bits, seed=N), bits)


def test_without_sorted_keys():
    check(keys_of("random", 3, ITEMS + 5, 17, seed=1), 17, want_sorted=False)
    check(keys_of("few", 1, 300, 8, seed=2), 8, want_sorted=False)


def test_one_graph_replayed_over_overwritten_keys():
    from deodr_amd import hip_renderer as hr

    n, N, bits = 3, 2 * ITEMS + 9, 19
    k = torch.as_tensor(keys_of("random", n, N, bits, seed=0).view(np.int32), device=DEV)
    scratch = hr.sort_keys_scratch(N, n, bits, DEV)
    s, o = hr.sort_keys(k, bits, scratch=scratch)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hr.sort_keys(k, bits, sorted_keys=s, order=o, scratch=scratch)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        hr.sort_keys(k, bits, sorted_keys=s, order=o, scratch=scratch)
    for seed, pattern in ((1, "few"), (2, "reversed"), (3, "high bits")):
        keys = keys_of(pattern, n, N, bits, seed=seed)
        k.copy_(torch.as_tensor(keys.view(np.int32), device=DEV))
        s.zero_(), o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want_keys, want_order = gr.stable_order(keys, bits)
        assert np.array_equal(o.cpu().numpy().view(np.uint32), want_order) and np.array_equal(s.cpu().numpy().view(np.uint32), want_keys), pattern
