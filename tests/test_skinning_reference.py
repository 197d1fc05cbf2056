"""CPU checks of linear blend skinning (deodr_amd/skinning.py): the torch formulation -- what runs on tensors the library does not take, and what the
kernels are tested against in tests/test_skinning_gpu.py -- against the NumPy restatement of tests/skinning_reference.py, its properties, its
derivatives, the hand-written adjoint of the restatement, and the figure the GPU tolerance is made of."""

import numpy as np
import pytest
import torch

import skinning_reference as sr

EPS = float(np.finfo(np.float64).eps)


def skin_torch_of(case, requires_grad=False, quaternions=None):
    from deodr_amd.skinning import skin_torch

    leaf = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=requires_grad)
    v, q, c = leaf(case["vertices"]), leaf(case["quaternions"] if quaternions is None else quaternions), leaf(case["joints"])
    idx = case["indices"].astype(np.int64)
    valid = idx < len(case["parents"])  # (the torch formulas take checked tables: an index out of range is weight 0 on joint 0)
    posed = skin_torch(v, q, c, case["parents"].astype(np.int64), torch.as_tensor(np.where(valid, idx, 0)), torch.as_tensor(np.where(valid, case["weights"], 0.0)))
    return posed, (v, q, c)


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_skin_torch_equals_the_float64_restatement(name):
    case = sr.make_case(name)
    ref = sr.forward(case, np.float64)["posed"]
    posed, _ = skin_torch_of(case)
    assert posed.shape == ref.v.shape and posed.dtype == torch.float64
    # two float64 evaluations of the same formulas (torch rounds its norms and sums in another order, and the chain carries that on): each within
    # MEASURED of the exact value, relative to the scale
    err = np.abs(posed.numpy() - ref.v) / ref.m
    print(f"{name}: largest difference relative to the scale {float(err.max()):.2e}")
    assert np.all(err <= 2 * sr.MEASURED)


def test_float64_error_of_the_restatement_is_what_the_gpu_tolerance_is_made_of():
    table = sr.measure()
    for name, row in table.items():
        print(f"{name:34s} " + "  ".join(f"{k} {e:.2e}" for k, e in row.items()))
    largest = max(max(row.values()) for row in table.values())
    print(f"largest float64 error relative to the scale: {largest:.3e}; MEASURED {sr.MEASURED:.3e}, FACTOR {sr.FACTOR}, TOLERANCE {sr.TOLERANCE:.3e}")
    assert 0.5 * sr.MEASURED <= largest <= sr.MEASURED and sr.TOLERANCE == 16 * sr.MEASURED


def test_identity_quaternions_give_the_vertices_back():
    for name in ("V33_K8_star9_n2", "V32_K7_chain17_n2", "V300_K8_star9_n1_padded"):
        case = sr.make_case(name)
        identity = np.zeros_like(case["quaternions"])
        identity[..., 3] = 1
        posed, _ = skin_torch_of(case, quaternions=identity)
        scale = np.abs(case["vertices"]).max() + 2 * np.abs(case["joints"]).sum()  # (v - c_j) + t_j, t_j a sum of differences of joints down the chain
        assert np.abs(posed.numpy() - case["vertices"][None]).max() <= 4 * EPS * scale


def test_a_root_rotation_alone_is_the_rigid_rotation_about_the_root():
    from scipy.spatial.transform import Rotation

    case = sr.make_case("V32_K7_chain17_n2")
    n, J = case["quaternions"].shape[:2]
    q = np.zeros((n, J, 4))
    q[..., 3] = 1
    rotations = Rotation.from_rotvec([[0.3, -0.5, 0.2], [-1.0, 0.4, 0.8]])
    q[:, 0] = rotations.as_quat() * np.array([[2.5], [0.7]])  # (not normalised)
    posed, _ = skin_torch_of(case, quaternions=q)
    c0 = case["joints"][0]
    expected = np.stack([r.apply(case["vertices"] - c0) + c0 for r in rotations])
    assert np.abs(posed.numpy() - expected).max() <= 64 * EPS * (np.abs(case["vertices"]).max() + np.abs(case["joints"]).sum())


def test_two_joints_worked_out_by_hand():
    """root at the origin turned by 90 degrees about z, its child at (1, 0, 0) turned by 90 degrees about z again.  The child's world rotation is 180
    degrees about z and it sits at R_0 (1, 0, 0) = (0, 1, 0).  The vertex (2, 0, 0): with the root (0, 2, 0), with the child R_1 (1, 0, 0) + t_1 =
    (-1, 0, 0) + (0, 1, 0); blended 1/4 : 3/4 -> (-3/4, 5/4, 0)"""
    from deodr_amd.skinning import Skin

    h = np.sqrt(0.5)
    skin = Skin(np.array([[0.0, 0, 0], [1.0, 0, 0]]), [-1, 0], (np.array([[0, 1], [1, 0]]), np.array([[0.25, 0.75], [1.0, 0.0]])), device="cpu")
    assert (skin.V, skin.K, skin.J) == (2, 2, 2)
    assert skin.joint_offsets_np.tolist() == [0, 1, 3] and skin.joint_slots_np.tolist() == [0, 1, 2]  # joint 0: slot 0; joint 1: slots 1 and 2 (3 has weight 0)
    posed = skin.apply(torch.tensor([[2.0, 0, 0], [1.0, 1.0, 0]]), torch.tensor([[0.0, 0, h, h], [0.0, 0, h, h]]))
    assert posed.shape == (2, 3)
    # the second vertex follows the child alone: R_1 ((1, 1, 0) - (1, 0, 0)) + t_1 = (0, -1, 0) + (0, 1, 0)
    assert np.abs(posed.numpy() - np.array([[-0.75, 1.25, 0.0], [0.0, 0.0, 0.0]])).max() <= 8 * EPS
    batch = skin.apply(torch.tensor([[2.0, 0, 0], [1.0, 1.0, 0]]), torch.tensor([[[0.0, 0, h, h], [0.0, 0, h, h]], [[0.0, 0, 0, 3.0], [0.0, 0, 0, 0.5]]]))
    assert batch.shape == (2, 2, 3) and torch.equal(batch[0], posed) and np.abs(batch[1].numpy() - np.array([[2.0, 0, 0], [1.0, 1.0, 0]])).max() <= 8 * EPS
    dense = Skin(np.array([[0.0, 0, 0], [1.0, 0, 0]]), [-1, 0], np.array([[0.25, 0.75], [0.0, 1.0]]), device="cpu")
    assert torch.equal(dense.apply(torch.tensor([[2.0, 0, 0], [1.0, 1.0, 0]]), torch.tensor([[0.0, 0, h, h], [0.0, 0, h, h]])), posed)


def test_gradcheck_of_the_torch_formulas_in_all_three_inputs():
    from deodr_amd.skinning import skin_torch

    rs = np.random.RandomState(5)
    J, V, K, n = 3, 5, 2, 2
    indices, weights = torch.as_tensor(rs.randint(0, J, size=(V, K))), rs.rand(V, K) + 0.1
    weights = torch.as_tensor(weights / weights.sum(axis=1, keepdims=True))
    leaf = lambda *shape: torch.tensor(rs.randn(*shape), requires_grad=True)
    v, c = leaf(V, 3), leaf(J, 3)
    q = torch.tensor(rs.randn(n, J, 4) * rs.uniform(0.5, 2.0, size=(n, J, 1)), requires_grad=True)  # not normalised
    for parents in ([-1, 0, 1], [-1, 0, 0]):
        assert torch.autograd.gradcheck(lambda v, q, c: skin_torch(v, q, c, parents, indices, weights), (v, q, c))
    assert torch.autograd.gradcheck(lambda v, q, c: skin_torch(v, q, c, [-1, 0, 1], indices, weights), (v, q[0], c))  # [J,4] -> [V,3]


@pytest.mark.parametrize("name", ["V33_K8_star9_n2", "V32_K7_chain17_n2", "V33_K2_J4_empty_joint", "V300_K8_star9_n1_padded", "V33_K2_two_roots"])
def test_hand_written_adjoint_agrees_with_autograd_of_the_torch_formulas(name):
    case = sr.make_case(name)
    posed, leaves = skin_torch_of(case, requires_grad=True)
    grads = torch.autograd.grad(posed, leaves, torch.as_tensor(case["posed_b"]))
    mine = sr.adjoint(case, case["posed_b"], np.float64)
    for key, g in zip(("vertices_b", "quaternions_b", "joints_b"), grads):
        err = np.abs(g.numpy() - mine[key].v)
        print(f"{name} {key}: largest error relative to the scale {float((err / np.maximum(mine[key].m, 1e-300)).max()):.2e}")
        # two float64 evaluations of one function in different orders: each within MEASURED of the exact value, relative to the scale
        assert np.all(err <= 2 * sr.MEASURED * mine[key].m), key
        assert np.abs(mine[key].v).max() > 0


def test_the_hand_rig():
    from deodr_amd.skinning import Skin

    v, faces, joints, parents, w = sr.hand_rig(measured_from="far")
    assert v.shape == (526, 3) and np.abs(v.mean(axis=0)).max() < 1e-12 and parents.tolist() == [-1, 0, 1, 2]
    assert not joints[0].any() and (np.count_nonzero(joints, axis=1) <= 1).all() and np.count_nonzero(w, axis=1).max() == 2
    skin = Skin(joints, parents, w, device="cpu")
    assert (skin.V, skin.J, skin.K) == (526, 4, 2) and len(skin.joint_slots_np) == np.count_nonzero(w)
    assert all(np.count_nonzero(w[:, j]) > 10 for j in range(4))  # every joint moves a part of the hand
    bent = skin.apply(torch.as_tensor(v), torch.as_tensor(sr.hand_target_quaternions())).numpy()
    assert 0.01 * np.ptp(v) < np.abs(bent - v).max() < 0.5 * np.ptp(v)
