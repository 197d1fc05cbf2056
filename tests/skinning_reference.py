"""What the skinning tests share: the model of include/deodr_hip_skinning.h restated in NumPy -- the forward and the hand-written adjoint, in float64
or in long double --, the cases the CPU and the GPU tests run, the synthetic four-joint rig of the hand, and the tolerance of the GPU tests.

Every number of the restatement is a :class:`T`: a value together with the sum of the absolute values of the terms it was made of (a product of sums
is the product of their magnitudes).  That magnitude, computed in long double, is the SCALE an output's error is measured against.  A world transform
enters the next level of the chain, the blend and the adjoint as a fresh value (magnitude = absolute value), as it enters the kernels that read
``world``.

THE TOLERANCE OF THE GPU TESTS.  ``python tests/skinning_reference.py`` runs the float64 restatement against the long-double one over all CASES and
prints the largest ``|float64 - long double| / scale`` over every element of every output: MEASURED below is that figure.  The kernels compute the
same formulas in float64 but add in another order (butterflies over the lanes of a vertex, strided lists per joint) and go through ``world`` once
more, hence FACTOR = 16 on top of it."""

import os

import numpy as np

LD = np.longdouble
MEASURED = 3.5e-15  # python tests/skinning_reference.py: "largest float64 error relative to the scale" 3.418e-15 (posed of the chain of depth 17, n = 64)
FACTOR = 16
TOLERANCE = FACTOR * MEASURED
ROOT_MARKER = 0xFFFFFFFF


class T:
    """a value and the sum of the absolute values of its terms (arrays of one shape)"""

    __slots__ = ("v", "m")

    def __init__(self, v, m=None):
        self.v = np.asarray(v)
        self.m = np.abs(self.v) if m is None else m

    def __add__(self, o):
        o = _lift(o)
        return T(self.v + o.v, self.m + o.m)

    __radd__ = __add__

    def __sub__(self, o):
        o = _lift(o)
        return T(self.v - o.v, self.m + o.m)

    def __neg__(self):
        return T(-self.v, self.m)

    def __mul__(self, o):
        o = _lift(o)
        return T(self.v * o.v, self.m * o.m)

    __rmul__ = __mul__

    def __truediv__(self, o):  # (by a length)
        o = _lift(o)
        return T(self.v / o.v, self.m / np.abs(o.v))

    def __getitem__(self, k):
        return T(self.v[k], self.m[k])

    def sum(self, axis):
        return T(self.v.sum(axis=axis), self.m.sum(axis=axis))

    def fresh(self):
        return T(self.v)


def _lift(o):
    return o if isinstance(o, T) else T(o)


def comps(x):
    return tuple(x[..., i] for i in range(x.v.shape[-1]))


def stack(cs):
    vs = np.broadcast_arrays(*[c.v for c in cs])
    ms = np.broadcast_arrays(*[c.m for c in cs])
    return T(np.stack(vs, axis=-1), np.stack(ms, axis=-1))


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot(a, b):
    s = a[0] * b[0]
    for x, y in zip(a[1:], b[1:]):
        s = s + x * y
    return s


def qrot(u, w, p):
    a = cross(u, p)
    bb = cross(u, a)
    return tuple(p[i] + 2 * (w * a[i] + bb[i]) for i in range(3))


def qrot_b(u, w, p, g):
    """the adjoint of qrot for r_b = g -> (p_b, u_b, w_b)"""
    a = cross(u, p)
    w_b = 2 * dot(g, a)
    bb_b = tuple(2 * x for x in g)
    cr = cross(bb_b, u)
    a_b = tuple(2 * w * g[i] + cr[i] for i in range(3))
    c1, c2 = cross(a, bb_b), cross(p, a_b)
    c3 = cross(a_b, u)
    return tuple(g[i] + c3[i] for i in range(3)), tuple(c1[i] + c2[i] for i in range(3)), w_b


def qmul(a, b):
    """Hamilton product of (x, y, z, w) quaternions given as 4-tuples"""
    c = cross(a[:3], b[:3])
    return tuple(a[3] * b[i] + b[3] * a[i] + c[i] for i in range(3)) + (a[3] * b[3] - dot(a[:3], b[:3]),)


def conj(a):
    return (-a[0], -a[1], -a[2], a[3])


def is_root(parents, j):
    return j == 0 or int(parents[j]) >= j


def forward(case, dtype=np.float64):
    """-> dict(world T [n,J,7], posed T [n,V,3]) and what the adjoint reuses"""
    v, q, c, w = (np.asarray(case[k], dtype=dtype) for k in ("vertices", "quaternions", "joints", "weights"))
    parents, idx = case["parents"], case["indices"].astype(np.int64)
    n, J = q.shape[:2]
    qc = comps(T(q))
    length = T(np.sqrt(dot(qc, qc).v))  # [n,J]
    qn = tuple(x / length for x in qc)
    cj = comps(T(c))
    Q, t = [None] * J, [None] * J
    for j in range(J):
        qj = tuple(x[:, j] for x in qn)
        if is_root(parents, j):
            Q[j], t[j] = qj, tuple(T(np.broadcast_to(x[j].v, (n,))) for x in cj)
        else:
            p = int(parents[j])
            P = tuple(x.fresh() for x in Q[p])
            Q[j] = qmul(P, qj)
            r = qrot(P[:3], P[3], tuple(x[j] - x[p] for x in cj))
            t[j] = tuple(a.fresh() + b for a, b in zip(t[p], r))
    world = stack([stack([Q[j][i] for j in range(J)]) for i in range(4)] + [stack([t[j][i] for j in range(J)]) for i in range(3)])  # [n,J,7]
    valid = idx < J
    idx_c, weff = np.where(valid, idx, 0), T(np.where(valid, w, 0))
    W = comps(T(world.v[:, idx_c]))  # seven of [n,V,K]
    local = tuple(T(v)[:, None, i] - T(c[idx_c])[..., i] for i in range(3))  # [V,K]
    rot = qrot(W[:3], W[3], local)
    posed = stack([(weff * (rot[i] + W[4 + i])).sum(axis=2) for i in range(3)])
    return dict(world=world, posed=posed, qn=qn, length=length, W=W, local=local, weff=weff, valid=valid, idx=idx, n=n, J=J)


def adjoint(case, g, dtype=np.float64, fwd=None):
    """the hand-written adjoint for posed_b = g [n,V,3] -> dict(vertices_b T [V,3], quaternions_b T [n,J,4], joints_b T [J,3])"""
    f = forward(case, dtype) if fwd is None else fwd
    c = np.asarray(case["joints"], dtype=dtype)
    parents, n, J = case["parents"], f["n"], f["J"]
    W, weff = f["W"], f["weff"]
    gT = T(np.asarray(g, dtype=dtype))
    gw = tuple(weff * gT[:, :, None, i] for i in range(3))  # [n,V,K]
    p_b, u_b, w_b = qrot_b(W[:3], W[3], f["local"], gw)
    vertices_b = stack([x.sum(axis=2).sum(axis=0) for x in p_b])
    zero = T(np.zeros(n, dtype=dtype))
    A = []  # per joint: adjoints of Q (4), of t (3), this pose's share of joints_b (3), each [n]
    for j in range(J):
        mask = f["valid"] & (f["idx"] == j) & (weff.v != 0)
        pick = lambda x: x[:, mask].sum(axis=1) if mask.any() else zero
        A.append([pick(x) for x in u_b] + [pick(w_b)] + [pick(x) for x in gw] + [-pick(x) for x in p_b])
    world = f["world"]
    cj = comps(T(c))
    q_b = [None] * J
    for j in range(J - 1, -1, -1):
        Q_b, t_b = tuple(A[j][:4]), tuple(A[j][4:7])
        qj = tuple(x[:, j] for x in f["qn"])
        if is_root(parents, j):
            qn_b = Q_b
            for i in range(3):
                A[j][7 + i] = A[j][7 + i] + t_b[i]
        else:
            p = int(parents[j])
            P = comps(T(world.v[:, p, :4]))
            qn_b = qmul(conj(P), Q_b)
            P_b = qmul(Q_b, conj(qj))
            r_p, r_u, r_w = qrot_b(P[:3], P[3], tuple(x[j] - x[p] for x in cj), t_b)
            for i in range(3):
                A[p][i] = A[p][i] + (P_b[i] + r_u[i])
                A[p][4 + i] = A[p][4 + i] + t_b[i]
                A[j][7 + i] = A[j][7 + i] + r_p[i]
                A[p][7 + i] = A[p][7 + i] - r_p[i]
            A[p][3] = A[p][3] + (P_b[3] + r_w)
        along = dot(qj, qn_b)
        length = f["length"][:, j]
        q_b[j] = stack([(qn_b[i] - qj[i] * along) / length for i in range(4)])  # [n,4]
    quaternions_b = T(np.stack([x.v for x in q_b], axis=1), np.stack([x.m for x in q_b], axis=1))
    joints_b = stack([stack([A[j][7 + i] for j in range(J)]).sum(axis=0) for i in range(3)])
    return dict(vertices_b=vertices_b, quaternions_b=quaternions_b, joints_b=joints_b)


def transposed_table(indices, weights, J):
    """-> (joint_offsets [J+1], joint_slots [nnz]): the slots i K + k of the influences with a joint < J and a non-zero weight, grouped by joint,
    increasing within a joint -- what ``deodr_amd.skinning.Skin`` builds"""
    flat_i, flat_w = np.asarray(indices).reshape(-1).astype(np.int64), np.asarray(weights).reshape(-1)
    slots = np.flatnonzero((flat_w != 0) & (flat_i < J))
    order = np.argsort(flat_i[slots], kind="stable")
    offsets = np.concatenate(([0], np.cumsum(np.bincount(flat_i[slots], minlength=J))))
    return offsets.astype(np.uint32), slots[order].astype(np.uint32)


# ---- the cases.  V: 1, 31, 32, 33 (the last lane group of a workgroup of 256 threads = 32 vertices, and one past it), 300.  K: 1, 2, 7, 8.  J: 1, 2, a
# chain of depth 17, a star of 9.  n: 1, 2, 64.  A joint without vertices; one joint holding every influence with V K = 300 (two strided trips of
# skin_joint_b_kernel's 256 threads) and 600 (three); rows padded with weight 0; quaternions that are not normalised (all but "unit_quaternions").

_CHAIN17 = [ROOT_MARKER] + list(range(16))
_STAR9 = [ROOT_MARKER] + [0] * 8
CASES = {
    #  name:                 (V,   K, parents,                 n,  what is special)
    "V1_K1_J1_n1":           (1,   1, [ROOT_MARKER],           1,  ""),
    "V31_K2_J2_n1":          (31,  2, [ROOT_MARKER, 0],        1,  ""),
    "V32_K7_chain17_n2":     (32,  7, _CHAIN17,                2,  ""),
    "V33_K8_star9_n2":       (33,  8, _STAR9,                  2,  ""),
    "V300_K2_chain17_n64":   (300, 2, _CHAIN17,                64, ""),
    "V300_K8_star9_n1_padded": (300, 8, _STAR9,                1,  "padded"),
    "V33_K2_J4_empty_joint": (33,  2, [ROOT_MARKER, 0, 1, 2],  2,  "empty"),
    "V300_K1_one_joint_300": (300, 1, [ROOT_MARKER, 0],        2,  "one"),
    "V300_K2_one_joint_600": (300, 2, [ROOT_MARKER, 0],        1,  "one"),
    "V33_K2_J4_n2_unit_quaternions": (33, 2, [ROOT_MARKER, 0, 0, 2], 2, "unit"),
    "V33_K2_two_roots":      (33,  2, [ROOT_MARKER, 0, ROOT_MARKER, 2], 2, ""),
}  # fmt: skip


def make_case(name):
    V, K, parents, n, special = CASES[name]
    J = len(parents)
    rs = np.random.RandomState(sorted(CASES).index(name))
    indices = rs.randint(0, J, size=(V, K))
    weights = rs.rand(V, K) + 0.05
    if special == "padded":  # two or three influences, the rest of the row weight 0 on joint 0
        keep = 2 + rs.randint(0, 2, size=V)
        weights[np.arange(K)[None, :] >= keep[:, None]] = 0
        indices[weights == 0] = 0
    if special == "empty":  # joint 2 influences nothing (its child 3 does)
        indices[indices == 2] = 3
    if special == "one":  # every influence on joint 1
        indices[:] = 1
    weights /= weights.sum(axis=1, keepdims=True)
    q = rs.randn(n, J, 4)
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    if special != "unit":
        q *= rs.uniform(0.5, 2.0, size=(n, J, 1))
    return dict(name=name, vertices=rs.randn(V, 3), joints=0.5 * rs.randn(J, 3), parents=np.array(parents, dtype=np.uint32),
                quaternions=q, indices=indices.astype(np.uint32), weights=weights, posed_b=rs.randn(n, V, 3))  # fmt: skip


def relative_errors(got, reference):
    """{name: largest |got - reference value| / reference magnitude} over the elements whose magnitude is not zero (the others must be equal)"""
    out = {}
    for name, ref in reference.items():
        have = got[name].v if isinstance(got[name], T) else np.asarray(got[name])
        err = np.abs(have.astype(LD) - ref.v)
        zero = ref.m == 0
        assert np.all(err[zero] == 0), name
        out[name] = float((err[~zero] / ref.m[~zero]).max()) if (~zero).any() else 0.0
    return out


def measure():
    """-> {case: {output: float64 error of the restatement relative to the long-double scale}}"""
    assert np.finfo(LD).eps < 2e-19, "np.longdouble is not wider than float64 here: no reference"
    table = {}
    for name in CASES:
        case = make_case(name)
        f64, ld = forward(case, np.float64), forward(case, LD)
        b64, bld = adjoint(case, case["posed_b"], np.float64, f64), adjoint(case, case["posed_b"], LD, ld)
        table[name] = relative_errors(dict(world=f64["world"], posed=f64["posed"], **b64), dict(world=ld["world"], posed=ld["posed"], **bld))
    return table


# ---- the synthetic rig of the hand


def hand():
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hand_mesh.npz"))
    return d["vertices"], d["faces"].astype(np.int64)


def hand_rig(fractions=(0.0, 0.35, 0.6, 0.8), width=0.06, keep=2, measured_from="near"):
    """-> (centred vertices [526,3], faces, joints [4,3], parents, dense weights [526,4]): a chain of joints on the longest axis of the centred hand, at the
    given fractions of its extent, the root moved to the origin; soft weights from logistic steps of ``width`` x the extent at each cut, the ``keep``
    largest of a row kept and renormalised.  Which end of the axis the fractions are measured from is a choice: "near" is the end nearer to the origin
    (the finger tips: the root then sits at 0.23 and the chain runs from it towards the forearm in one direction; the last two joints move the 25 and
    8 vertices of the forearm's stub), "far" the other one (the cuts at 0.35, 0.6 and 0.8 from the forearm run through palm and fingers: every joint
    moves a large part of the hand, and an articulated pose changes the image -- and the energy -- about fifteen times as much)."""
    vertices, faces = hand()
    v = vertices - vertices.mean(axis=0)
    axis = int(np.argmax(v.max(axis=0) - v.min(axis=0)))
    lo, hi = v[:, axis].min(), v[:, axis].max()
    extent, along = hi - lo, (1.0 if -lo < hi else -1.0)  # `along`: from the end the fractions are measured from to the other one
    along = along if measured_from == "near" else -along
    near = lo if along > 0 else hi
    J = len(fractions)
    joints = np.zeros((J, 3))
    joints[:, axis] = near + along * np.array(fractions) * extent
    joints[0] = 0
    steps = [np.ones(len(v))] + [1 / (1 + np.exp(-along * (v[:, axis] - joints[j, axis]) / (width * extent))) for j in range(1, J)] + [np.zeros(len(v))]
    w = np.stack([steps[j] * (1 - steps[j + 1]) for j in range(J)], axis=1)  # past cut j and not yet past cut j + 1
    w[np.arange(len(v))[:, None], np.argsort(w, axis=1)[:, : J - keep]] = 0
    w /= w.sum(axis=1, keepdims=True)
    return v, faces, joints, np.array([-1] + list(range(J - 1))), w


def axis_quaternion(axis, angle):
    q = np.zeros(4)
    q[axis], q[3] = np.sin(angle / 2), np.cos(angle / 2)
    return q


def hand_target_quaternions():
    """the articulated pose the fit tests look for: 0.35 and -0.30 rad about the second axis (joints 1, 2), 0.40 rad about the third (joint 3)"""
    return np.stack([axis_quaternion(0, 0.0), axis_quaternion(1, 0.35), axis_quaternion(1, -0.30), axis_quaternion(2, 0.40)])


if __name__ == "__main__":
    table = measure()
    for name, row in table.items():
        print(f"{name:34s} " + "  ".join(f"{k} {e:.2e}" for k, e in row.items()))
    print(f"largest float64 error relative to the scale: {max(max(r.values()) for r in table.values()):.3e}")
