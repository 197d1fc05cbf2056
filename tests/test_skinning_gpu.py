"""GPU tests of linear blend skinning: ``deodr_hip_skin_apply`` / ``deodr_hip_skin_apply_b`` against the long-double restatement of
tests/skinning_reference.py over its case table (the shapes at which the loops and the launch geometry of the kernels change), the autograd op
against the torch formulas on the same tensors, and the depth fit of the rigged hand -- eager, and replayed as a HIP graph.

The tolerance is derived in tests/skinning_reference.py: every element of every output lies within TOLERANCE = 16 x (the largest float64 error of the
NumPy restatement, relative to the scale) of the long-double value, relative to that element's own scale -- the sum of the absolute values of its
terms.  A term, an influence or a pose that goes missing is of the order of the scale divided by the number of terms: twelve orders above it.

Every call: the outputs are carved out of larger NaN-filled buffers and the scratch has exactly deodr_hip_skin_scratch_bytes bytes, filled with a
pattern (the header: it need not be cleared), followed by a guard; all checked after the call.  The same call into fresh outputs gives the same
bits, and asking for fewer outputs does not change the bits of the others."""

import functools

import numpy as np
import pytest
import torch

import skinning_reference as sr
from test_basis_gpu import Arena, host

pytestmark = pytest.mark.gpu

LD = np.longdouble
DEV = "cuda"
GUARD_BYTES, GUARD_BYTE, FILL_BYTE = 4096, 0xA5, 0x7F


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (case, long-double forward, long-double adjoint), computed once per case"""
    case = sr.make_case(name)
    fwd = sr.forward(case, LD)
    return case, fwd, sr.adjoint(case, case["posed_b"], LD, fwd)


def u32(a):
    """a uint32 table as the int32 tensor the wrappers take"""
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy(), device=DEV)


def f64(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


class GuardedScratch:
    """exactly deodr_hip_skin_scratch_bytes bytes filled with a pattern, followed in the same allocation by a guard"""

    def __init__(self, V, J, K, n):
        from deodr_amd.hip_renderer import lib

        self.nbytes = int(lib().deodr_hip_skin_scratch_bytes(V, J, K, n))
        assert self.nbytes == 64 + 80 * n * J
        self.buffer = torch.full((self.nbytes + GUARD_BYTES,), FILL_BYTE, dtype=torch.uint8, device=DEV)
        self.buffer[self.nbytes :] = GUARD_BYTE
        self.front = self.buffer[: self.nbytes]

    def check(self):
        assert bool((self.buffer[self.nbytes :] == GUARD_BYTE).all()), "the scratch was written beyond deodr_hip_skin_scratch_bytes"
        assert bool((self.front[:64] == FILL_BYTE).all()), "the first 64 bytes of the scratch were touched"


def within(got, ref, what):
    err = np.abs(host(got).astype(LD) - ref.v)
    assert np.all(err <= sr.TOLERANCE * ref.m), (what, float((err / np.maximum(ref.m, LD(1e-300))).max()), np.argwhere(err > sr.TOLERANCE * ref.m)[:4])
    return float((err[ref.m > 0] / ref.m[ref.m > 0]).max()) if (ref.m > 0).any() else 0.0


def run_case(case, fwd, adj, offsets=None, slots=None):
    """forward and adjoint of one case through the wrappers of hip_renderer, everything guarded -> the outputs of the full adjoint"""
    from deodr_amd import hip_renderer as hr

    V, K = case["indices"].shape
    n, J = case["quaternions"].shape[:2]
    if offsets is None:
        offsets, slots = sr.transposed_table(case["indices"], case["weights"], J)
    v, c, q, w, g = (f64(case[k]) for k in ("vertices", "joints", "quaternions", "weights", "posed_b"))
    parents, indices, offsets, slots = u32(case["parents"]), u32(case["indices"]), u32(offsets), u32(slots)
    arena = Arena()
    world, posed, world2, posed2 = (arena.carve(shape=s) for s in ((n, J, 7), (n, V, 3)) * 2)
    got = hr.skin_apply(v, c, parents, q, indices, w, world=world, posed=posed)
    assert got[0] is world and got[1] is posed
    hr.skin_apply(v, c, parents, q, indices, w, world=world2, posed=posed2)
    torch.cuda.synchronize()
    arena.check()
    assert torch.equal(world, world2) and torch.equal(posed, posed2)  # bit-identical from run to run
    worst = {"world": within(world, fwd["world"], "world"), "posed": within(posed, fwd["posed"], "posed")}
    shapes = dict(vertices_b=(V, 3), quaternions_b=(n, J, 4), joints_b=(J, 3))
    results = {}
    for want in ((True, True, True), (True, True, True), (False, True, True), (True, False, True), (True, True, False), (True, False, False),
                 (False, False, True), (False, True, False)):  # fmt: skip
        arena, scratch = Arena(), GuardedScratch(V, J, K, n)
        outs = {name: arena.carve(shape=shapes[name]) if on else None for name, on in zip(shapes, want)}
        got = hr.skin_apply_b(v, c, parents, q, indices, w, world, g, offsets, slots, scratch=scratch.front, want=want, **outs)
        torch.cuda.synchronize()
        arena.check(), scratch.check()
        assert all((a is None and b is None) or a is b for a, b in zip(got, outs.values()))  # NULL stays NULL
        for name, t in outs.items():
            if t is None:
                continue
            if name in results:  # the second full run, and every run that asks for fewer outputs: the same bits
                assert torch.equal(t, results[name]), (name, want)
            else:
                results[name] = t
                worst[name] = within(t, adj[name], name)
    print(f"{case['name']}: largest error relative to the scale " + "  ".join(f"{k} {e:.2e}" for k, e in worst.items()) + f"  (tolerance {sr.TOLERANCE:.2e})")
    return results


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_values_and_adjoints_against_long_double(name):
    case, fwd, adj = reference(name)
    results = run_case(case, fwd, adj)
    assert all(float(t.abs().max()) > 0 for t in results.values())


def test_out_of_range_tables_are_skipped():
    """straight to the wrappers of hip_renderer (``Skin`` would refuse these): an index >= J counts as weight 0, a slot >= V K of the transposed table is
    skipped -- the values are those of the tables without them, and nothing outside the outputs is written.  (A parent that does not point below
    its joint makes a root: the case "V33_K2_two_roots" of the table above.)"""
    name = "V33_K8_star9_n2"
    base = sr.make_case(name)
    V, K = base["indices"].shape
    J = len(base["parents"])
    rs = np.random.RandomState(1)
    bad = rs.rand(V, K) < 0.2
    case = dict(base, name=name + " with indices >= J", indices=np.where(bad, rs.choice([J, J + 5, 2**31, 0xFFFFFFFF], size=(V, K)), base["indices"]).astype(np.uint32))
    fwd = sr.forward(case, LD)  # (the restatement gives an index >= J weight 0)
    adj = sr.adjoint(case, case["posed_b"], LD, fwd)
    offsets, slots = sr.transposed_table(case["indices"], case["weights"], J)
    assert len(slots) < V * K - 10  # the table leaves the bad influences out ...
    results = run_case(case, fwd, adj, offsets, slots)
    # ... and a table that lists slots beyond V K between the good ones gives the same bits
    extra = {2: [V * K, 2**31], 5: [0xFFFFFFFF]}
    padded, starts = [], [0]
    for j in range(J):
        mine = list(slots[offsets[j] : offsets[j + 1]])
        for s in extra.get(j, []):
            mine.insert(len(mine) // 2, s)
        padded += mine
        starts.append(len(padded))
    again = run_case(dict(case, name=name + " with slots >= V K"), fwd, adj, np.array(starts, dtype=np.uint32), np.array(padded, dtype=np.uint32))
    # (an entry in the middle of a joint's list moves the later ones to other threads: the same terms, another order -- values, not bits)
    assert set(again) == set(results)


def test_autograd_op_against_the_torch_formulas_on_the_same_tensors():
    from deodr_amd.skinning import Skin, skin_torch

    name = "V33_K2_J4_empty_joint"  # V = 33, J = 4, K = 2, n = 2
    case, fwd, adj = reference(name)
    parents = np.where(case["parents"] == sr.ROOT_MARKER, -1, case["parents"].astype(np.int64))
    skin = Skin(case["joints"], parents, (case["indices"].astype(np.int64), case["weights"]), device=DEV)
    assert (skin.V, skin.J, skin.K) == (33, 4, 2)
    leaves = lambda: [f64(case[k]).requires_grad_(True) for k in ("vertices", "quaternions", "joints")]
    (v, q, c), (v2, q2, c2) = leaves(), leaves()
    assert skin.uses_kernel(v, q, c)
    posed = skin.apply(v, q, c)
    expected = skin_torch(v2, q2, c2, skin.parents_np, skin._indices_long, skin.weights)
    g = f64(case["posed_b"])
    grads, grads_torch = torch.autograd.grad(posed, (v, q, c), g), torch.autograd.grad(expected, (v2, q2, c2), g)
    # the kernels within TOLERANCE of the exact value, the torch formulas in float64 within MEASURED, both relative to the scale
    bound = sr.TOLERANCE + sr.MEASURED
    for what, a, b, ref in [("posed", posed, expected, fwd["posed"])] + [(k, a, b, adj[k]) for k, a, b in zip(("vertices_b", "quaternions_b", "joints_b"), grads, grads_torch)]:
        err = np.abs(host(a).astype(LD) - host(b).astype(LD))
        print(f"{what}: largest difference relative to the scale {float((err / np.maximum(ref.m, LD(1e-300))).max()):.2e}")
        assert a.shape == b.shape and np.all(err <= bound * ref.m), what
        within(a, ref, what)
    # [J,4] quaternions give [V,3]; rest joints by default; only what is asked for is computed
    one = skin.apply(v, q[0])
    assert one.shape == (33, 3) and torch.equal(one, skin.apply(v, q[:1], skin.joints)[0])
    (only_q,) = torch.autograd.grad(skin.apply(v.detach(), q, c.detach()), (q,), g)
    assert torch.equal(only_q, grads[1])


def test_depth_fit_of_the_rigged_hand_eager_and_graphed():
    from deodr_amd.mesh_fitter import GraphedStep
    from test_skinning_fit_host import SIZE, render_target, rig_fitter

    def fitter():
        f, rig, focal = rig_fitter(device=DEV)
        target = render_target(f, focal, sr.hand_target_quaternions())
        assert target.shape == (SIZE, SIZE) and (target < 1).sum() > 200
        f.step_factor_vertices = f.step_factor_quaternion = f.step_factor_translation = 0.0  # geometry and rigid pose held, as in the CPU fit
        f.step_factor_joints = 3e-4
        return f

    eager = fitter()
    assert eager._direct_iteration(1, False) is None and eager.skin.uses_kernel(eager.vertices, eager.joint_quaternions, eager.skin.joints)
    e_eager = [float(eager.step_device()[0]) for _ in range(12)]
    print("eager:", e_eager)
    assert e_eager[11] < e_eager[0] and eager.joint_quaternions.shape == (4, 4)
    assert float((eager.joint_quaternions - eager.joint_quaternions_init).abs().max()) > 0
    f = fitter()
    graphed = GraphedStep(f, warmup=3)  # 3 + 1 eager steps and 1 on the capture stream: iterations 0 .. 4
    assert f.iter == 5 and ("attr", "joint_quaternions") in graphed.state  # (its speed is updated in place by the momentum kernel: fixed storage already)
    e_graph = [float(graphed.step_device()[0]) for _ in range(7)]  # iterations 5 .. 11
    print("graphed:", e_graph)
    assert np.abs(np.array(e_graph) - np.array(e_eager[5:])).max() <= 1e-6 * e_eager[0]
