"""CPU checks of the binding deodr_amd/_abi.py derives from include/deodr_hip.h: every prototype bound, with the return type and the number
of parameters written out here; the long signatures type by type; tests/fake_hip.py::FakeLib in step with the header; and a header the
derivation does not understand, or a library that lacks a symbol, refused by name."""

import ctypes as C
import inspect

import pytest

VP, INT, DOUBLE, SIZE = C.c_void_p, C.c_int, C.c_double, C.c_size_t

# name: (restype, number of parameters), read off include/deodr_hip.h
PROTOTYPES = {
    "deodr_hip_workspace_bytes": (SIZE, 6), "deodr_hip_render_scene": (INT, 10), "deodr_hip_render_scene_b": (INT, 13),
    "deodr_hip_render_scene_fit": (INT, 9), "deodr_hip_fit_loss_bytes": (SIZE, 3), "deodr_hip_background_loss": (INT, 7),
    "deodr_hip_render_scene_fit_ex": (INT, 10), "deodr_hip_rigid_transform": (INT, 7), "deodr_hip_rigid_transform_b": (INT, 8),
    "deodr_hip_project_points": (INT, 9), "deodr_hip_project_points_b": (INT, 10), "deodr_hip_silhouette_flags": (INT, 9),
    "deodr_hip_momentum_update": (INT, 20), "deodr_hip_fit_scratch_bytes": (SIZE, 2), "deodr_hip_fit_front": (INT, 28),
    "deodr_hip_fit_pose_project": (INT, 15), "deodr_hip_fit_pose_project_b": (INT, 20), "deodr_hip_vertex_shade": (INT, 14),
    "deodr_hip_vertex_shade_b": (INT, 18), "deodr_hip_rigid_energy": (INT, 14), "deodr_hip_l2_loss": (INT, 8),
    "deodr_hip_depth_residual": (INT, 12), "deodr_hip_workspace_status": (INT, 7), "deodr_hip_workspace_pool_pairs": (INT, 3),
    "deodr_hip_profile_enable": (INT, 1), "deodr_hip_profile_read": (INT, 2), "deodr_hip_profile_stamps": (INT, 2),
    "deodr_hip_workspace_census": (INT, 6), "deodr_hip_copy_probe": (INT, 6), "deodr_hip_force_generic": (INT, 1),
    "deodr_hip_set_deterministic": (INT, 1), "deodr_hip_views_gradient_sum": (INT, 14), "deodr_hip_wait_flag": (INT, 5),
    "deodr_hip_last_error": (C.c_char_p, 0), "deodr_hip_abi_version": (INT, 0),
}  # fmt: skip


def long_signatures(scene_pointer):
    """the argtypes of the signatures nobody counts right by hand, parameter by parameter as the header lists them"""
    return {
        # scene, image, z_buffer, image_b, sigma, antialiase_error, obs, err_buffer, err_buffer_b, workspace, workspace_bytes, have_forward_state, stream
        "deodr_hip_render_scene_b": [scene_pointer, VP, VP, VP, DOUBLE, INT, VP, VP, VP, VP, SIZE, INT, VP],
        # n_tensors, x, speed, grad, grad2, factor, step_max, count, normalize_rows, inertia, damping, grad_scale, grad_mean, mean_out, energy,
        # data_energy, data_weight, scratch, scratch_bytes, stream
        "deodr_hip_momentum_update": [INT, VP, VP, VP, VP, VP, VP, C.POINTER(INT), C.POINTER(INT), DOUBLE, DOUBLE, VP, VP, VP, VP, VP, DOUBLE, VP, SIZE, VP],
        # vertices, quaternions, posed, extrinsic, intrinsic, distortion, posed_b, ij_b, depths_b, depths_b_scale, vertices_b, out, scratch,
        # scratch_bytes, V, n, colors_b, nb_colors, colors_sum, stream
        "deodr_hip_fit_pose_project_b": [VP, VP, VP, VP, VP, VP, VP, VP, VP, DOUBLE, VP, VP, VP, SIZE, INT, INT, VP, INT, VP, VP],
        # ij, faces, edge_faces, flags, T, posed, vf_offsets, vf_corners, light, ambient, color, C, luminosity, colors, vertices, vertices_ref,
        # m_offsets, m_cols, m_vals, cregu, gradient, energy, scratch, scratch_bytes, V, n, clockwise, stream
        "deodr_hip_fit_front": [VP, VP, VP, VP, INT, VP, VP, VP, VP, VP, VP, INT, VP, VP, VP, VP, VP, VP, VP, DOUBLE, VP, VP, VP, SIZE, INT, INT, INT, VP],
        # scene, workspace, workspace_bytes, stream, overflowed, needed_pairs, scene_errors: the host out-parameters are typed
        "deodr_hip_workspace_status": [scene_pointer, VP, SIZE, VP, C.POINTER(INT), C.POINTER(C.c_ulonglong), C.POINTER(INT)],
    }  # fmt: skip


def check_signatures(functions, scene_pointer):
    """`functions`: {name: (restype, argtypes)} -- of a parsed header, or read back from a bound library"""
    assert sorted(functions) == sorted(PROTOTYPES) and len(PROTOTYPES) == 35
    for name, (restype, count) in PROTOTYPES.items():
        assert functions[name][0] is restype, name
        assert len(functions[name][1]) == count, name
    for name, argtypes in long_signatures(scene_pointer).items():
        assert list(functions[name][1]) == argtypes, name


def test_every_prototype_of_the_header_is_bound_as_declared():
    from deodr_amd import _abi
    from deodr_amd import hip_renderer as hr
    from sim_util import declared_symbols

    assert declared_symbols() == sorted(PROTOTYPES)  # (an independent list of what the header declares: one regular expression)
    L = hr.lib()
    check_signatures({name: (getattr(L, name).restype, getattr(L, name).argtypes) for name in PROTOTYPES}, C.POINTER(hr._SceneC))
    check_signatures(_abi.HEADER.functions, C.POINTER(hr._SceneC))
    options = C.POINTER(hr._FitOptionsC)
    assert L.deodr_hip_render_scene_fit_ex.argtypes[6] is options and L.deodr_hip_background_loss.argtypes[2] is options


def test_bound_functions_take_what_callers_pass():
    """None, bare addresses, c_void_p, byref and ctypes arrays all convert (nothing is called: from_param is the conversion of a call)"""
    from deodr_amd import hip_renderer as hr

    L = hr.lib()
    for value in (None, 0x1000, C.c_void_p(0x1000), (C.c_double * 4)(), (C.c_void_p * 3)(), C.byref(C.c_int(0))):
        L.deodr_hip_copy_probe.argtypes[0].from_param(value)
    read = L.deodr_hip_profile_read.argtypes
    read[0].from_param((C.c_double * 4)()), read[1].from_param((C.c_ulonglong * 4)()), read[1].from_param(C.byref(C.c_ulonglong(0)))
    L.deodr_hip_momentum_update.argtypes[7].from_param((C.c_int * 3)())
    with pytest.raises(C.ArgumentError):
        L.deodr_hip_workspace_pool_pairs(C.byref(hr._SceneC()), 0, C.byref(C.c_int(0)))  # (an out-parameter of the wrong width)
    assert L.deodr_hip_profile_stamps(None, 0) == 0 and L.deodr_hip_profile_enable(0) == 0  # (two of the six that used to be unbound)


def test_fake_library_follows_the_header():
    """every entry point tests/fake_hip.py::FakeLib restates is one the header declares, with as many parameters"""
    from fake_hip import FakeLib

    entry_points = {name: f for name, f in inspect.getmembers(FakeLib, inspect.isfunction) if name.startswith("deodr_hip_")}
    assert len(entry_points) >= 15
    for name, f in entry_points.items():
        assert name in PROTOTYPES, name
        assert len(inspect.signature(f).parameters) - 1 == PROTOTYPES[name][1], name  # (- self)


def test_what_the_derivation_does_not_understand_is_refused_by_name():
    import __graft_entry__ as g
    from deodr_amd import _abi

    text = open(_abi.HEADER_PATH).read()
    one = "int deodr_hip_force_generic(int on);"
    assert one in text
    for replacement, quoted in (("int deodr_hip_force_generic(float on);", "float"), ("int deodr_hip_force_generic(int (*on)(int));", "(*on)"),
                                ("static int deodr_hip_counter = 3;", "deodr_hip_counter = 3"), ("int deodr_hip_force_generic(int);", "(int)")):  # fmt: skip
        with pytest.raises(ImportError, match="deodr_hip.h") as refused:
            _abi.parse(text.replace(one, replacement))
        assert quoted in str(refused.value), replacement
    with pytest.raises(ImportError, match="int clamp, \\*clamp_p"):
        _abi.parse(text.replace("int clamp;", "int clamp, *clamp_p;"))
    # a parameter swapped in the header shows in the signatures written out above
    swapped = _abi.parse(text.replace("double cregu, double *gradient, double *energy, void *scratch, size_t scratch_bytes, int V, int n, int clockwise",
                                      "double *gradient, double cregu, double *energy, void *scratch, size_t scratch_bytes, int V, int n, int clockwise"))  # fmt: skip
    with pytest.raises(AssertionError, match="deodr_hip_fit_front"):
        check_signatures(swapped.functions, C.POINTER(swapped.structs["DeodrHipScene"]))
    # a declared symbol the library lacks
    more = _abi.parse(text.replace(one, one + "\nint deodr_hip_not_there(int on);"))
    with pytest.raises(ImportError, match="deodr_hip_not_there"):
        _abi.bind(C.CDLL(g.build_hip()), more)
