"""Linear blend skinning: a skeleton with skin weights between the shape parameters of a mesh and its pose (MANO, SMPL, any rigged mesh).

The model (``include/deodr_hip_skinning.h``): ``J`` joints with rest positions ``joints`` [J,3] and ``parents`` [J] (joint 0 is the root, ``parents[j] < j``
for ``j > 0``), one quaternion ``(x, y, z, w)`` per pose and joint, normalised inside.  World transforms ``R_0 = R(q_0)``, ``t_0 = joints_0`` and
``R_j = R_p R(q_j)``, ``t_j = t_p + R_p (joints_j - joints_p)``; skinned vertices ``posed[b,i] = sum_k weights[i,k] (R_j (vertices[i] - joints_j) + t_j)``
with ``j = indices[i,k]``.  With every quaternion at identity the vertices come back as they are.

:class:`Skin` checks the tables on the host, keeps them on a device and applies them: on float64 ROCm tensors through the kernels of
``deodr_amd/csrc/dr_skinning.h`` (:class:`deodr_amd.fronthalf.SkinFunc`), elsewhere through :func:`skin_torch`, the same formulas as torch ops."""

import numpy as np
import torch

ROOT = -1  # the marker of a joint without a parent in ``parents`` (0xFFFFFFFF in the uint32 table of the header): what ``parents[0]`` must be
MAX_INFLUENCES = 8


def _qmul(a, b):
    """the Hamilton product of quaternions [..., 4] = (x, y, z, w): R(a b) = R(a) R(b)"""
    au, aw, bu, bw = a[..., :3], a[..., 3:], b[..., :3], b[..., 3:]
    return torch.cat((aw * bu + bw * au + torch.cross(au, bu, dim=-1), aw * bw - (au * bu).sum(dim=-1, keepdim=True)), dim=-1)


def _qrot(q, p):
    """the points p [..., 3] rotated by the unit quaternions q [..., 4] (broadcast against each other)"""
    u, p = torch.broadcast_tensors(q[..., :3], p)
    a = torch.cross(u, p, dim=-1)
    return p + 2 * (q[..., 3:] * a + torch.cross(u, a, dim=-1))


def skin_torch(vertices, quaternions, joints, parents, indices, weights):
    """The formulas of ``deodr_hip_skin_apply`` as torch ops (differentiable by autograd): what runs on CPU tensors and on anything the kernels do not
    take.  ``vertices`` [V,3], ``quaternions`` [n,J,4] or [J,4] (raw), ``joints`` [J,3], ``parents`` a sequence of J integers (:data:`ROOT` or any value
    ``>= j`` for a root), ``indices`` [V,K] integer tensor, ``weights`` [V,K] -> posed [n,V,3] ([V,3] for [J,4] quaternions)."""
    single = quaternions.dim() == 2
    q = quaternions[None] if single else quaternions
    q = q / q.norm(dim=-1, keepdim=True)
    J = q.shape[1]
    Q, t = [None] * J, [None] * J
    for j in range(J):
        p = int(parents[j])
        if j == 0 or p < 0 or p >= j:
            Q[j], t[j] = q[:, j], joints[j][None].expand(q.shape[0], 3)
        else:
            Q[j], t[j] = _qmul(Q[p], q[:, j]), t[p] + _qrot(Q[p], (joints[j] - joints[p])[None])
    Q, t = torch.stack(Q, dim=1), torch.stack(t, dim=1)  # [n,J,4], [n,J,3]
    idx = indices.long()
    local = vertices[:, None, :] - joints[idx]  # [V,K,3]
    terms = _qrot(Q[:, idx], local[None]) + t[:, idx]  # [n,V,K,3]
    posed = (weights[None, :, :, None] * terms).sum(dim=2)
    return posed[0] if single else posed


class Skin:
    """A skeleton and the skin weights of a mesh of V vertices, checked once and kept on ``device``.

    ``joints`` [J,3] rest positions (in the frame of the vertices); ``parents`` [J] integers, ``parents[0] == ROOT`` (-1) and ``0 <= parents[j] < j``
    for ``j > 0``; ``weights``: a dense [V,J] array, or a pair ``(indices [V,K], weights [V,K])`` with ``K <= 8`` (rows with fewer influences padded with
    weight 0).  Raises ``ValueError`` for a ``parents[0]`` that is not the root marker, a ``parents[j] >= j`` (or negative), an index ``>= J``, a negative
    or non-finite weight, more than 8 non-zero weights in a row, a row whose weights do not sum to 1 within 1e-9.

    Builds the [V,K] tables and the transposed table of the adjoint (the slots ``i K + k`` of every joint's influences, in increasing order) once."""

    def __init__(self, joints, parents, weights, device="cuda"):
        joints = np.array(joints, dtype=np.float64)
        if joints.ndim != 2 or joints.shape[1] != 3 or not 1 <= joints.shape[0] <= 256:
            raise ValueError(f"Skin: joints must have shape [1 <= J <= 256, 3], not {list(joints.shape)}")
        J = joints.shape[0]
        if not np.all(np.isfinite(joints)):
            raise ValueError("Skin: a joint position is not finite")
        parents = np.asarray(parents)
        if parents.shape != (J,) or not np.issubdtype(parents.dtype, np.integer):
            raise ValueError(f"Skin: parents must be {J} integers")
        parents = parents.astype(np.int64)
        if parents[0] != ROOT:
            raise ValueError(f"Skin: parents[0] must be the root marker {ROOT} (joint 0 is the root), not {parents[0]}")
        for j in range(1, J):
            if not 0 <= parents[j] < j:
                raise ValueError(f"Skin: parents[{j}] = {parents[j]} must be in 0 .. {j - 1} (a parent comes before its children)")
        if isinstance(weights, (tuple, list)) and len(weights) == 2:
            indices, w = np.asarray(weights[0]), np.array(weights[1], dtype=np.float64)
            if indices.ndim != 2 or w.shape != indices.shape or not np.issubdtype(indices.dtype, np.integer) or indices.shape[1] < 1:
                raise ValueError(f"Skin: (indices, weights) must be an integer and a float array of one shape [V, K], not {list(indices.shape)} and {list(w.shape)}")
            indices = indices.astype(np.int64)
            if np.any(indices < 0) or np.any(indices >= J):
                raise ValueError(f"Skin: an index is outside 0 .. {J - 1}")
            self._check_weights(w)
            if np.count_nonzero(w, axis=1).max(initial=0) > MAX_INFLUENCES:
                raise ValueError(f"Skin: a row has more than {MAX_INFLUENCES} non-zero weights")
            if w.shape[1] > MAX_INFLUENCES:
                raise ValueError(f"Skin: (indices, weights) must have at most {MAX_INFLUENCES} columns, not {w.shape[1]} (dense [V, J] weights may be wider)")
        else:
            dense = np.array(weights, dtype=np.float64)
            if dense.ndim != 2 or dense.shape[1] != J:
                raise ValueError(f"Skin: dense weights must have shape [V, {J}], not {list(dense.shape)}")
            self._check_weights(dense)
            K = int(np.count_nonzero(dense, axis=1).max(initial=1))
            if K > MAX_INFLUENCES:
                raise ValueError(f"Skin: a row has more than {MAX_INFLUENCES} non-zero weights")
            order = np.argsort(dense == 0, axis=1, kind="stable")[:, : max(K, 1)]  # the non-zero columns of a row first, in joint order
            w = np.take_along_axis(dense, order, axis=1)
            indices = np.where(w != 0, order, 0)
        if w.shape[0] < 1 or w.shape[0] > 2**24:
            raise ValueError(f"Skin: the number of vertices must be in 1 .. 2^24, not {w.shape[0]}")
        if np.abs(w.sum(axis=1) - 1).max() > 1e-9:
            raise ValueError(f"Skin: the weights of row {int(np.abs(w.sum(axis=1) - 1).argmax())} do not sum to 1 within 1e-9")
        self.V, self.K, self.J = int(w.shape[0]), int(w.shape[1]), J
        self.joints_np, self.parents_np, self.indices_np, self.weights_np = joints, parents, np.ascontiguousarray(indices), np.ascontiguousarray(w)
        # the transposed table: the slots i K + k with a non-zero weight, grouped by joint, increasing within a joint
        slots = np.flatnonzero(self.weights_np.reshape(-1) != 0)
        joint_of = self.indices_np.reshape(-1)[slots]
        order = np.argsort(joint_of, kind="stable")
        self.joint_slots_np = slots[order].astype(np.int64)
        self.joint_offsets_np = np.concatenate(([0], np.cumsum(np.bincount(joint_of, minlength=J)))).astype(np.int64)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:  # (the device tensors report: uses_kernel compares with it)
            self.device = torch.device("cuda", torch.cuda.current_device())
        i32 = lambda a: torch.as_tensor(a.astype(np.uint32).view(np.int32).copy(), device=self.device)  # (uint32 tables travel as int32 tensors)
        self.joints = torch.as_tensor(joints, device=self.device)
        self.weights = torch.as_tensor(self.weights_np, device=self.device)
        self.parents = i32(np.where(parents < 0, 0xFFFFFFFF, parents))
        self.indices, self.joint_offsets, self.joint_slots = i32(self.indices_np), i32(self.joint_offsets_np), i32(self.joint_slots_np)
        self._indices_long = torch.as_tensor(self.indices_np, device=self.device)

    @staticmethod
    def _check_weights(w):
        if not np.all(np.isfinite(w)):
            raise ValueError("Skin: a weight is not finite")
        if np.any(w < 0):
            raise ValueError("Skin: a weight is negative")

    def uses_kernel(self, vertices, quaternions, joints):
        """whether :meth:`apply` runs the kernels on these tensors: float64 ROCm tensors on this skin's device, at most 64 poses"""
        from . import fronthalf

        n = 1 if quaternions.dim() == 2 else int(quaternions.shape[0])
        return fronthalf.usable(vertices, quaternions, joints) and all(t.device == self.device for t in (vertices, quaternions, joints)) and 1 <= n <= 64

    def apply(self, vertices, quaternions, joints=None):
        """-> the skinned vertices, differentiable in all three inputs.  ``vertices`` [V,3]; ``quaternions`` [J,4] -> [V,3], or [n,J,4] -> [n,V,3];
        ``joints`` None (the rest positions given at construction) or a [J,3] tensor: joints that depend on the shape, as the output of a joint
        regressor does."""
        joints = self.joints if joints is None else joints
        if tuple(vertices.shape) != (self.V, 3) or tuple(quaternions.shape[-2:]) != (self.J, 4) or quaternions.dim() not in (2, 3) or tuple(joints.shape) != (self.J, 3):
            raise ValueError(f"Skin.apply: expected vertices [{self.V}, 3], quaternions [{self.J}, 4] or [n, {self.J}, 4] and joints [{self.J}, 3], not "
                             f"{list(vertices.shape)}, {list(quaternions.shape)} and {list(joints.shape)}")  # fmt: skip
        if self.uses_kernel(vertices, quaternions, joints):
            from . import fronthalf

            posed = fronthalf.SkinFunc.apply(vertices, quaternions if quaternions.dim() == 3 else quaternions[None], joints, self)
            return posed if quaternions.dim() == 3 else posed[0]
        to = lambda t: t.to(vertices.device)
        return skin_torch(vertices, quaternions, to(joints), self.parents_np, to(self._indices_long), to(self.weights))
