"""ctypes binding of the C ABI in `include/trs_solver.h`, `include/trs_modes.h`, `include/trs_effects.h`, `include/trs_loss.h`, `include/trs_influence.h`, `include/trs_sets.h`, `include/trs_dynamics.h`, `include/trs_nonlinear.h`, `include/trs_buckling.h`, `include/trs_modegrad.h`, `include/trs_spectrum.h`, `include/trs_harmonic.h`, `include/trs_sizing.h`, `include/trs_compliance.h`, `include/trs_minweight.h`, `include/trs_minweight_stress.h`, `include/trs_unilateral.h` and `include/trs_plastic.h` (library: `libtrs_hip.so`, in-tree).

There is no fallback: if the library is missing, `load()` raises `HipExtensionError`.
"""
import ctypes
import os

from .utils import HipExtensionError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtrs_hip.so")
CSRC_DIR = os.path.join(_HERE, "csrc")

_P = ctypes.c_void_p
_I = ctypes.c_int
_D = ctypes.c_double

#: every symbol `include/trs_solver.h` declares -> (restype, argtypes)
SIGNATURES = {
    "trs_abi_version": (_I, []),
    "trs_slab_ld": (_I, [_I]),
    "trs_slab_rows": (_I, [_I]),
    "trs_dofmap": (_I, [_I, _I, _P, _P, _P, _P, _P]),
    "trs_env_ints": (_I, [_I]),
    "trs_assemble_work_bytes": (ctypes.c_size_t, [_I, _I, _I]),
    "trs_assemble": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _I, _P, _P, _P, _I, _P]),
    "trs_potrf_batched": (_I, [_I, _P, _I, _I, _P, _P, _P, _P, _P, _I, _I, _P]),
    "trs_potrs_batched": (_I, [_I, _P, _I, _I, _P, _P, _I, _P, _I, _P]),
    "trs_recover": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _I, _P]),
    "trs_ga_sections": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "trs_fitness": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _D, _D, _P, _P, _P, _P]),
    "trs_solve_small_fits": (_I, [_I, _I, _I]),
    "trs_solve_small": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                             _D, _D, _P, _P, _P, _P]),
    "trs_graph_features_dev": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _D, _D, _D, _D,
                                    _I, _P, _P, _P, _P, _P, _P]),
    "trs_graph_features_packed": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _D, _D, _D, _D,
                                       _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "trs_joint_order_fits": (_I, [_I, _I]),
    "trs_joint_order": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "trs_joint_order_rows": (_I, [_I, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                  _P, _P, _I, _P]),
    "trs_recover_rows": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _P, _P, _P, _P,
                              _I, _P]),
    "trs_cubegen_dev": (_I, [_I, ctypes.c_uint64, _I, _I, _I, _P, _I, _I, _I, _D, _D, _P, _I, _I, _P, _I, _I, _I,
                             _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_int64, _P]),
    "trs_copy_rows": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _P]),
    "trs_stream_create_masked": (_I, [_P, _I, _P]),
    "trs_stream_destroy": (_I, [_P]),
    "trs_solve_rows": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _I,
                            _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _I, _P]),
    "trs_solve": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _I,
                       _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    # table member form (ABI 10): (conn16, type_idx, types) in place of (conn, E, A)
    "trs_assemble_tab": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _I, _P, _P, _P, _I, _P]),
    "trs_recover_tab": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _I, _P]),
    "trs_recover_rows_tab": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _P, _P, _P, _P,
                                  _I, _P]),
    "trs_solve_small_tab": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                 _D, _D, _P, _P, _P, _P]),
    "trs_joint_order_tab": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "trs_joint_order_rows_tab": (_I, [_I, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                      _P, _P, _I, _P]),
    "trs_solve_tab": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _I,
                           _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "trs_solve_rows_tab": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _I,
                                _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _I, _P]),
    # load cases (several right-hand sides per factorisation)
    "trs_gather_cases": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P]),
    "trs_potrs_cases": (_I, [_I, _I, _P, _I, _I, _P, _P, _I, _P, _P]),
    "trs_recover_cases_fits": (_I, [_I, _I]),
    "trs_recover_cases": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "trs_recover_tab_cases": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    # adjoint gradients (one more substitution against the factor; csrc/adjoint.hip)
    "trs_adjoint_fits": (_I, [_I, _I]),
    "trs_adjoint_rhs": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "trs_adjoint_tab_rhs": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "trs_adjoint_grad": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
    "trs_adjoint_tab_grad": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
}

#: every symbol `include/trs_modes.h` declares (natural frequencies; csrc/modes.hip, the same library)
MODES_SIGNATURES = {
    "trs_modes_abi_version": (_I, []),
    "trs_modes_fits": (_I, [_I, _I]),
    "trs_modes_mass": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _D, _P, _P, _P, _P, _P, _I, _P, _P]),
    "trs_modes_tab_mass": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _D, _P, _P, _P, _P, _P, _I, _P, _P]),
    "trs_modes_step": (_I, [_I, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _D, _P]),
    "trs_modes_shapes": (_I, [_I, _I, _I, _P, _I, _P, _P, _P, _P, _P]),
}

#: every symbol `include/trs_effects.h` declares (settlements, pre-strain, self-weight; csrc/effects.hip, the same library)
EFFECTS_SIGNATURES = {
    "trs_effects_abi_version": (_I, []),
    "trs_effects_fits": (_I, [_I, _I]),
    "trs_effects_rhs": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "trs_effects_tab_rhs": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "trs_effects_recover": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P,
                                 _P, _P]),
    "trs_effects_tab_recover": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P,
                                     _P, _P]),
}

#: every symbol `include/trs_loss.h` declares (member-loss analysis; csrc/loss.hip, the same library)
LOSS_SIGNATURES = {
    "trs_loss_abi_version": (_I, []),
    "trs_loss_fits": (_I, [_I, _I, _I]),
    "trs_loss_rhs": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "trs_loss_tab_rhs": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "trs_loss_apply": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _D, _P, _P, _P, _P, _P, _P,
                            _P, _P, _P]),
    "trs_loss_tab_apply": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _D, _P, _P, _P, _P, _P,
                                _P, _P, _P, _P]),
}

#: every symbol `include/trs_influence.h` declares (influence lines and moving-load envelopes; csrc/influence.hip, the
#: same library)
INFLUENCE_SIGNATURES = {
    "trs_influence_abi_version": (_I, []),
    "trs_influence_fits": (_I, [_I, _I, _I]),
    "trs_influence_apply": (_I, [_I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P,
                                 _P, _P, _P, _P, _P, _P, _P, _P]),
    "trs_influence_tab_apply": (_I, [_I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I,
                                     _P, _P, _P, _P, _P, _P, _P, _P, _P]),
}

#: every symbol `include/trs_sets.h` declares (member-set scenarios: up to eight members removed or resized at once;
#: csrc/sets.hip, the same library)
SETS_SIGNATURES = {
    "trs_sets_abi_version": (_I, []),
    "trs_sets_fits": (_I, [_I, _I, _I]),
    "trs_sets_rhs": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "trs_sets_tab_rhs": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "trs_sets_apply": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _D, _P, _P,
                            _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "trs_sets_tab_apply": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _D, _P,
                                _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
}

#: every symbol `include/trs_dynamics.h` declares (transient response: Newmark time stepping on a factor of K + sigma M;
#: csrc/dynamics.hip, the same library)
DYN_SIGNATURES = {
    "trs_dyn_abi_version": (_I, []),
    "trs_dyn_fits": (_I, [_I, _I, _I]),
    "trs_dyn_shift": (_I, [_I, _P, _I, _I, _P, _P, _I, _D, _P]),
    "trs_dyn_step": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _D, _D, _D, _D, _D,
                          _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P]),
    "trs_dyn_tab_step": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _D, _D, _D, _D,
                              _D, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P]),
    "trs_dyn_collect": (_I, [_I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
}

#: every symbol `include/trs_nonlinear.h` declares (geometrically nonlinear statics: Newton on the tangent factor;
#: csrc/nonlinear.hip, the same library)
NL_SIGNATURES = {
    "trs_nl_abi_version": (_I, []),
    "trs_nl_fits": (_I, [_I, _I]),
    "trs_nl_state": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _D, _D, _I, _I, _I, _I, _P, _P, _P, _P, _P,
                          _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "trs_nl_state_tab": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _D, _D, _I, _I, _I, _I, _P, _P, _P, _P,
                              _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "trs_nl_tangent": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _I, _P, _P]),
    "trs_nl_tangent_tab": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _I, _P, _P]),
    "trs_nl_update": (_I, [_I, _I, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P]),
}

#: every symbol `include/trs_buckling.h` declares (linear buckling: critical load factors from shifted factors of
#: K + theta Kg; csrc/buckling.hip, the same library)
BK_SIGNATURES = {
    "trs_bk_abi_version": (_I, []),
    "trs_bk_fits": (_I, [_I, _I]),
    "trs_bk_members": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
    "trs_bk_members_tab": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
    "trs_bk_product": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "trs_bk_step": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _D, _P]),
    "trs_bk_shapes": (_I, [_I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
}

#: every symbol `include/trs_modegrad.h` declares (gradients of the natural frequencies from the converged mode block;
#: csrc/modegrad.hip, the same library)
MG_SIGNATURES = {
    "trs_mg_abi_version": (_I, []),
    "trs_mg_fits": (_I, [_I, _I, _I]),
    "trs_mg_grad": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _D, _P, _P, _P, _P, _P, _P,
                         _P]),
    "trs_mg_tab_grad": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _D, _P, _P, _P, _P, _P, _P,
                             _P]),
}

#: every symbol `include/trs_spectrum.h` declares (response spectrum analysis from the converged mode block;
#: csrc/spectrum.hip, the same library)
RS_SIGNATURES = {
    "trs_rs_abi_version": (_I, []),
    "trs_rs_fits": (_I, [_I, _I, _I]),
    "trs_rs_modal": (_I, [_I, _I, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _P, _I, _P, _P, _P, _D, _I, _I, _P, _P, _P, _P, _P,
                          _P, _P, _P, _P]),
    "trs_rs_combine": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _P, _P, _I, _I, _P, _P, _P,
                            _P, _P, _P, _P, _P]),
    "trs_rs_combine_tab": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _P, _P, _I, _I, _P, _P,
                                _P, _P, _P, _P, _P, _P]),
}

#: every symbol `include/trs_harmonic.h` declares (harmonic response over a frequency sweep from the converged mode
#: block; csrc/harmonic.hip, the same library)
HR_SIGNATURES = {
    "trs_hr_abi_version": (_I, []),
    "trs_hr_fits": (_I, [_I, _I, _I]),
    "trs_hr_modal": (_I, [_I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _P, _I, _P, _P, _P]),
    "trs_hr_sweep": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P, _I, _P, _D, _D, _D,
                          _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P]),
    "trs_hr_sweep_tab": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P, _I, _P, _D, _D,
                              _D, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P]),
}

#: every symbol `include/trs_sizing.h` declares (member sizing: fully stressed design iterated on the device;
#: csrc/sizing.hip, the same library).  General member form only: the step writes areas, which a type table cannot hold
SZ_SIGNATURES = {
    "trs_sz_abi_version": (_I, []),
    "trs_sz_fits": (_I, [_I, _I]),
    "trs_sz_step": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _D, _D, _D, _P, _D, _D, _D, _P, _D,
                         _P, _D, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "trs_sz_snap": (_I, [_I, _I, _P, _P, _P, _I, _P, _P, _P]),
}

#: every symbol `include/trs_compliance.h` declares (compliance sizing: the stiffest design at a given weight, iterated on
#: the device; csrc/compliance.hip, the same library).  General member form only, as the member sizing
CM_SIGNATURES = {
    "trs_cm_abi_version": (_I, []),
    "trs_cm_fits": (_I, [_I, _I]),
    "trs_cm_step": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _D, _D, _D, _P, _D, _P,
                         _D, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P]),
}

#: every symbol `include/trs_minweight.h` declares (minimum weight under displacement limits: the optimality-criteria
#: method with one multiplier per limit, iterated on the device; csrc/minweight.hip, the same library).  General member
#: form only, as the member sizing
MW_SIGNATURES = {
    "trs_mw_abi_version": (_I, []),
    "trs_mw_fits": (_I, [_I, _I, _I]),
    "trs_mw_step": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _I, _D, _D, _D,
                         _I, _P, _D, _P, _D, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
}

#: every symbol `include/trs_minweight_stress.h` declares (minimum weight under stress and displacement limits in one run:
#: the stress-ratio area as the lower bound of the optimality-criteria subproblem; csrc/minweight.hip, the same library,
#: a second instantiation of the same kernel).  A header and a version of its own: `trs_minweight.h` is as it was
MWS_SIGNATURES = {
    "trs_mws_abi_version": (_I, []),
    "trs_mw_fits_stress": (_I, [_I, _I, _I]),
    "trs_mw_step_stress": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _I, _D, _D,
                                _D, _I, _P, _D, _P, _D, _D, _D, _P, _D, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P,
                                _P, _P, _P, _P, _P]),
}

#: every symbol `include/trs_unilateral.h` declares (tension-only and compression-only members: the active-set iteration
#: on the device; csrc/unilateral.hip, the same library).  General member form only, as the member sizing
UN_SIGNATURES = {
    "trs_un_abi_version": (_I, []),
    "trs_un_fits": (_I, [_I, _I]),
    "trs_un_step": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _D, _P, _I, _I, _P, _P, _P, _P, _P,
                         _P, _I, _P]),
}

#: every symbol `include/trs_plastic.h` declares (collapse load: the event-to-event elastic-plastic analysis on the device;
#: csrc/plastic.hip, the same library).  General member form only, as the member sizing
PL_SIGNATURES = {
    "trs_pl_abi_version": (_I, []),
    "trs_pl_fits": (_I, [_I, _I]),
    "trs_pl_step": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _D, _D, _D, _D, _D, _I, _I, _P,
                         _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "trs_pl_finish": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
}

#: must equal TRS_ABI_VERSION of include/trs_solver.h
ABI_VERSION = 10
#: must equal TRS_MODES_ABI_VERSION of include/trs_modes.h
MODES_ABI_VERSION = 1
#: must equal TRS_EFFECTS_ABI_VERSION of include/trs_effects.h
EFFECTS_ABI_VERSION = 1
#: must equal TRS_LOSS_ABI_VERSION of include/trs_loss.h
LOSS_ABI_VERSION = 1
#: must equal TRS_INFLUENCE_ABI_VERSION of include/trs_influence.h
INFLUENCE_ABI_VERSION = 1
#: must equal TRS_SETS_ABI_VERSION of include/trs_sets.h
SETS_ABI_VERSION = 1
#: must equal TRS_DYN_ABI_VERSION of include/trs_dynamics.h
DYN_ABI_VERSION = 1
#: must equal TRS_NL_ABI_VERSION of include/trs_nonlinear.h
NL_ABI_VERSION = 1
#: must equal TRS_BK_ABI_VERSION of include/trs_buckling.h
BK_ABI_VERSION = 1
#: must equal TRS_MG_ABI_VERSION of include/trs_modegrad.h
MG_ABI_VERSION = 1
#: must equal TRS_RS_ABI_VERSION of include/trs_spectrum.h
RS_ABI_VERSION = 1
#: must equal TRS_HR_ABI_VERSION of include/trs_harmonic.h
HR_ABI_VERSION = 1
#: must equal TRS_SZ_ABI_VERSION of include/trs_sizing.h
SZ_ABI_VERSION = 1
#: must equal TRS_CM_ABI_VERSION of include/trs_compliance.h
CM_ABI_VERSION = 1
#: must equal TRS_MW_ABI_VERSION of include/trs_minweight.h
MW_ABI_VERSION = 1
#: must equal TRS_MWS_ABI_VERSION of include/trs_minweight_stress.h
MWS_ABI_VERSION = 1
#: must equal TRS_UN_ABI_VERSION of include/trs_unilateral.h
UN_ABI_VERSION = 1
#: must equal TRS_PL_ABI_VERSION of include/trs_plastic.h
PL_ABI_VERSION = 1
#: TRS_RS_SRSS, TRS_RS_CQC, TRS_RS_ABS of include/trs_spectrum.h: the modal combination rules
RS_RULES = {"srss": 0, "cqc": 1, "abs": 2}
#: TRS_NL_* of include/trs_nonlinear.h: the status of a truss in a load step of the nonlinear analysis
NL_ACTIVE, NL_CONVERGED, NL_ITER_LIMIT, NL_NOT_PD, NL_NOT_ATTEMPTED = -1, 0, 1, 2, 3
#: TRS_SZ_* of include/trs_sizing.h: the status of a truss in a sizing run, and the catalogue's size limit
SZ_ACTIVE, SZ_CONVERGED, SZ_ITER_LIMIT, SZ_NOT_PD = -1, 0, 1, 2
SZ_MAX_CATALOG = 256
#: TRS_CM_* of include/trs_compliance.h: the status of a truss in a compliance sizing run, and the measures
CM_ACTIVE, CM_CONVERGED, CM_ITER_LIMIT, CM_NOT_PD = -1, 0, 1, 2
CM_MEASURES = {"weight": 0, "volume": 1}
#: TRS_MW_* of include/trs_minweight.h: the status of a truss in a minimum-weight run, the measures and the most limits
MW_ACTIVE, MW_CONVERGED, MW_ITER_LIMIT, MW_NOT_PD, MW_INFEASIBLE = -1, 0, 1, 2, 3
MW_MEASURES = {"weight": 0, "volume": 1}
MW_MAX_LIMITS = 8
#: TRS_UN_* of include/trs_unilateral.h: the status of a truss in a run of the active-set iteration
UN_ACTIVE, UN_CONVERGED, UN_ITER_LIMIT, UN_NOT_PD = -1, 0, 1, 2
#: TRS_PL_* of include/trs_plastic.h: the status of a truss in a run of the event-to-event analysis
PL_ACTIVE, PL_LAMBDA_MAX, PL_EVENT_LIMIT, PL_MECHANISM, PL_DISP_LIMIT = -1, 0, 1, 2, 3
#: TRS_SETS_MAX of include/trs_sets.h: members per scenario at most
SETS_MAX = 8
#: TRS_MODES_BLOCK of include/trs_modes.h: vectors per truss of the block iteration (one case group)
MODES_BLOCK = 16

# The flag words of the ABI (tests/test_capi_symbols.py compares every one with its define).
# TRS_ASM_* of include/trs_solver.h: `flags` of trs_assemble
ASM_FULL_SYMMETRIC, ASM_COMPACT, ASM_ALL_NARROW, ASM_ALL_TILES, ASM_ALL_WIDE = 1, 2, 4, 8, 16
# TRS_HINT_* of include/trs_solver.h: `hints` of the factorisation, substitution, recovery and whole-pipeline calls
HINT_NO_WIDE, HINT_SUBSTITUTED, HINT_COMPACT, HINT_SEPARATE_STAGES, HINT_NO_SMALL, HINT_RECOVER_UNSTAGED = 1, 2, 4, 8, 16, 32
HINT_ALL_TILES, HINT_RECOVER_SCAN, HINT_ALL_WIDE = 64, 128, 256
NARROW_MAX_BELOW = 24   # csrc/trs_common.h TRS_NARROW_MAX_BELOW: reach up to which a matrix goes to a wave of its own
ORDER_RCM_BELOW = 128   # csrc/reorder.c TRS_ORDER_RCM_BELOW, csrc/order.hip RCM_BELOW: effort 3 prices Cuthill-McKee
#                         below this many free joints

_lib = None


def build(verbose=False):
    """Compile the HIP sources for gfx950 into `libtrs_hip.so` (hipcc cross-compiles without a GPU)."""
    import subprocess
    cmd = ["make", "-C", CSRC_DIR, "-j4"]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or proc.returncode != 0:
        print(proc.stdout + proc.stderr)
    if proc.returncode != 0:
        raise HipExtensionError("building libtrs_hip.so failed:\n" + proc.stderr[-2000:])
    return LIB_PATH


def load():
    """Load the library once and attach the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: it brings a HIP runtime of its own, and in a process that loads the system's runtime (through this
    # library) before torch's, every later call finds no device (hipError 100) - `solve_influence` asks
    # trs_influence_fits before it touches torch
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise HipExtensionError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C python_stable_3d_truss_analysis_amd/csrc`). There is no CPU fallback.")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as exc:
        raise HipExtensionError(f"cannot load {LIB_PATH}: {exc}") from exc
    for table, version, expected in (   # per header: its signature table, its version symbol, the version bound here
            (SIGNATURES, "trs_abi_version", ABI_VERSION), (MODES_SIGNATURES, "trs_modes_abi_version", MODES_ABI_VERSION),
            (EFFECTS_SIGNATURES, "trs_effects_abi_version", EFFECTS_ABI_VERSION),
            (INFLUENCE_SIGNATURES, "trs_influence_abi_version", INFLUENCE_ABI_VERSION),
            (LOSS_SIGNATURES, "trs_loss_abi_version", LOSS_ABI_VERSION), (SETS_SIGNATURES, "trs_sets_abi_version", SETS_ABI_VERSION),
            (DYN_SIGNATURES, "trs_dyn_abi_version", DYN_ABI_VERSION), (NL_SIGNATURES, "trs_nl_abi_version", NL_ABI_VERSION),
            (BK_SIGNATURES, "trs_bk_abi_version", BK_ABI_VERSION), (MG_SIGNATURES, "trs_mg_abi_version", MG_ABI_VERSION),
            (RS_SIGNATURES, "trs_rs_abi_version", RS_ABI_VERSION), (HR_SIGNATURES, "trs_hr_abi_version", HR_ABI_VERSION),
            (SZ_SIGNATURES, "trs_sz_abi_version", SZ_ABI_VERSION), (CM_SIGNATURES, "trs_cm_abi_version", CM_ABI_VERSION),
            (MW_SIGNATURES, "trs_mw_abi_version", MW_ABI_VERSION),
            (MWS_SIGNATURES, "trs_mws_abi_version", MWS_ABI_VERSION),
            (UN_SIGNATURES, "trs_un_abi_version", UN_ABI_VERSION), (PL_SIGNATURES, "trs_pl_abi_version", PL_ABI_VERSION)):
        for name, (restype, argtypes) in table.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        if getattr(lib, version)() != expected:
            raise HipExtensionError("libtrs_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise HipExtensionError(f"{what} failed with hipError_t {rc}")
