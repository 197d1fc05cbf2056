"""The keyword combinations of the three pose fitters on the device, in lock-step with the CPU path (tests/fitter_matrix_cases.py has the table and the
driver; tests/test_fitter_matrix_host.py shows that the CPU path -- torch formulas of every op, the checker in the rasterizer's place -- equals a
long-double restatement of the composition).

Every case: three steps of the ``cuda`` fitter, each from the parameters and momentum speeds the CPU fitter had before the same step, compared where the
gradients enter the momentum rule.  Tolerances: DESIGN.md section 6 -- float64 frames: image within 1e-9, every gradient and second gradient within
1e-8 of the largest reference entry of its group, energy within 1e-9 relative; float32 frames: image within 1e-5, gradients within 1e-4, energy within
what the image bound allows, ``data weight * (2 |r| |d| + |d|^2)`` for ``|d| <= 1e-5 sqrt(n H W C)`` and r the reference's weighted residual (plus
1e-9 of the energy for the float64 terms).  The worst ratio of every case is printed.

The comparison is not torch against torch: the library's entry points are counted per step (as tests/test_lighting_gpu.py counts launches), and
every op of the case must have gone through its kernel, forward and adjoint.  An op that fell back to its torch formulas because of what the op
before it returned (dtype, contiguity, requires_grad) fails here.

``GraphedStep`` on the six richest cases: seven replays against eager steps of a twin within 1e-6 of the first energy -- the bound of the keyword
tests of tests/test_basis_gpu.py, test_skinning_gpu.py and test_subdivision_gpu.py, which give its reason: the rasterizer's float64 atomics."""

import numpy as np
import pytest
import torch

import fitter_matrix_cases as fm
from fitter_matrix_cases import CASES

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOLERANCES = {torch.float64: dict(image=1e-9, gradient=1e-8, energy=1e-9), torch.float32: dict(image=1e-5, gradient=1e-4, energy=1e-9)}
PRIOR = 1e-8  # second gradients (rigid, priors, albedo smoothness) are float64 arithmetic whatever the frames are


def required_launches(case, f):
    """{entry point of the library: predicate on its arguments | None} one step of the case must go through"""
    need = {"deodr_hip_rigid_transform": None, "deodr_hip_rigid_transform_b": None}
    if "skin" in case.shape:
        need.update(deodr_hip_skin_apply=None, deodr_hip_skin_apply_b=None)
    if "basis3" in case.shape:
        need.update(deodr_hip_basis_apply=None, deodr_hip_basis_apply_b=None)
    if case.light in ("sh", "sh3-albedo"):
        need.update(deodr_hip_sh_shade=None, deodr_hip_sh_shade_b=None)
    return need


def run_counted(f, follow):
    """fitter_matrix_cases.run in lock-step, with the calls of the library's entry points of every step in ``row["launches"]``: [(name, arguments)]"""
    from deodr_amd import fronthalf
    from deodr_amd import hip_renderer as hr

    original, rows = hr._launch, []
    assert fronthalf._launch is original
    for k in range(len(follow)):
        calls = []

        def spy(function, device, *args):
            calls.append((function.__name__, args))
            return original(function, device, *args)

        fm.load(f, follow[k]["params"], follow[k]["speed"])
        hr._launch = fronthalf._launch = spy
        try:
            row = fm.step_recorded(f)
        finally:
            hr._launch = fronthalf._launch = original
        row["launches"] = calls
        rows.append(row)
    return rows


def check_launches(case, f, row):
    names = [name for name, _ in row["launches"]]
    for name in required_launches(case, f):
        assert name in names, f"{case.name}: {name} was not called in a step (the op ran its torch formulas); called: {sorted(set(names))}"
    if "sub1" in case.shape:  # the subdivision: the rows of S forward, the rows of S^T (the transposed table) in the adjoint
        Vf, Vc = f.subdivision.matrix.shape
        shapes = [(args[3], args[4]) for name, args in row["launches"] if name == "deodr_hip_subdiv_apply"]
        assert (Vf, Vc) in shapes and (Vc, Vf) in shapes, f"{case.name}: deodr_hip_subdiv_apply ran with (rows, columns) {shapes}, not with S and its transposed table"


def largest(a):
    return float(np.abs(a).max())


def within(what, error, bound, worst, key):
    """assert ``error <= bound`` (False for a NaN on either side: a non-finite result cannot pass) and keep the worst ratio for the report"""
    assert np.isfinite(error) and np.isfinite(bound) and bound > 0 and error <= bound, f"{what}: error {error!r} against the bound {bound!r}"
    if error / bound >= worst[key][0]:
        worst[key] = (error / bound, what)


@pytest.mark.parametrize("name", list(CASES))
def test_lock_step_with_the_cpu_path(name, oracle_api):
    case = CASES[name]
    tol = TOLERANCES[case.pixel_dtype]
    reference, ref_rows = fm.reference_recording(case, oracle_api)
    f = fm.build(case, DEV)
    assert f._direct_iteration(1, False) is None and f.vertices.is_cuda
    rows = run_counted(f, ref_rows)
    worst = dict(image=(0.0, None), energy=(0.0, None), gradient=(0.0, None))
    for step, (ref, got) in enumerate(zip(ref_rows, rows)):
        check_launches(case, f, got)
        assert set(got["entries"]) == set(ref["entries"]) == set(case.groups)
        # nothing the device hands back may be NaN or infinite (the parameters of the next step are loaded from the recording: it would not show later)
        assert np.all(np.isfinite(got["image"])) and np.isfinite(got["energy"]) and got["image"].shape == ref["image"].shape, f"step {step}"
        for group, (g, g2) in got["entries"].items():
            assert np.all(np.isfinite(g)) and (g2 is None or np.all(np.isfinite(g2))), f"{group}, step {step}: a gradient is not finite"
        within(f"image, step {step}", largest(got["image"] - ref["image"]), tol["image"], worst, "image")
        bound = tol["energy"] * abs(ref["energy"])
        if case.pixel_dtype == torch.float32:
            r, data_weight, w_max = fm.weighted_residual_norm(case, reference, ref["image"])
            d = 1e-5 * np.sqrt(ref["image"].size * w_max)
            bound += data_weight * (2 * r * d + d * d)
        within(f"energy, step {step}", abs(got["energy"] - ref["energy"]), bound, worst, "energy")
        # the gradients, where they enter the momentum rule
        for group, (g_ref, g2_ref) in ref["entries"].items():
            g, g2 = got["entries"][group]
            assert g.shape == g_ref.shape and (g2 is None) == (g2_ref is None), group
            within(f"{group}, step {step}", largest(g - g_ref), tol["gradient"] * largest(g_ref), worst, "gradient")
            if g2 is not None:
                within(f"second gradient of {group}, step {step}", largest(g2 - g2_ref), PRIOR * largest(g2_ref), worst, "gradient")
    print(f"{name}: worst error in units of its tolerance -- image {worst['image'][0]:.2e} (of {tol['image']:.0e}), energy {worst['energy'][0]:.2e}, "
          f"gradient {worst['gradient'][0]:.2e} ({worst['gradient'][1]}; of {tol['gradient']:.0e} of the largest entry)")  # fmt: skip


# ---- GraphedStep on the richest cases -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", fm.GRAPHED)
def test_a_graph_replay_equals_eager_steps(name, oracle_api):
    """3 + 1 eager steps and 1 on the capture stream, then seven replays: the energies of a twin fitter's iterations 5 .. 11 within 1e-6 of the first
    energy; the final parameters AND momentum speeds within 1e-6 of their largest entry, each parameter having moved over the seven replays by more than
    that bound (a parameter the replay left where it was would otherwise pass).  ``graphed.state`` lists every parameter group of the case.  A momentum
    speed is listed exactly when a step rebinds it: on float64 ROCm tensors the momentum kernel updates the speeds in place (the twin's speed tensors
    are the same objects after an eager step), which is the fixed storage a replay needs, and then none of them is listed."""
    from deodr_amd.mesh_fitter import GraphedStep

    case = CASES[name]
    fm.reference_recording(case, oracle_api)  # (a depth case: the CPU fitter renders the target both twins are given)
    eager, f = fm.build_free_running(case, DEV), fm.build_free_running(case, DEV)
    assert eager._direct_iteration(1, False) is None
    e_eager = [float(eager.step_device()[0].detach()) for _ in range(5)]
    speeds = dict(eager.momentum.speed)
    e_eager += [float(eager.step_device()[0].detach()) for _ in range(7)]
    rebound = {group: eager.momentum.speed[group] is not speeds[group] for group in case.groups}
    graphed = GraphedStep(f, warmup=3)
    assert f.iter == 5 and set(f.momentum.speed) == set(case.groups)
    attributes = [fm.ATTRIBUTE_OF.get(group, group) for group in case.groups]
    for attribute in attributes:
        assert ("attr", attribute) in graphed.state, (attribute, graphed.state)
    for group in case.groups:
        assert (("speed", group) in graphed.state) == rebound[group], (group, rebound, graphed.state)
    before = {attribute: fm.host(getattr(f, attribute)) for attribute in attributes}
    e_graph = [float(graphed.step_device()[0]) for _ in range(7)]
    torch.cuda.synchronize()
    print(f"{name}: eager {e_eager[5:]}\n{name}: graph {e_graph}\nstate: {graphed.state}")
    assert np.all(np.isfinite(e_graph)) and len(set(e_graph)) == 7 and np.abs(np.array(e_graph) - np.array(e_eager[5:])).max() <= 1e-6 * e_eager[0]
    for attribute in attributes:
        a, b = fm.host(getattr(f, attribute)), fm.host(getattr(eager, attribute))
        moved = largest(a - before[attribute])
        print(f"  {attribute}: {largest(a - b) / largest(b):.2e} of the largest entry from the eager twin, moved by {moved / largest(b):.2e} of it")
        assert np.all(np.isfinite(a)) and largest(a - b) <= 1e-6 * largest(b) < moved, attribute
    for group in case.groups:
        a, b = fm.host(f.momentum.speed[group]), fm.host(eager.momentum.speed[group])
        assert np.all(np.isfinite(a)) and largest(b) > 0 and largest(a - b) <= 1e-6 * largest(b), group
