"""Transient response, the parts that need no GPU: the numpy yardstick (`tests/dynamics_reference.py`) against physics -
so that parity with it means something -, the refusals of `_check_transient_args`, and the C interface of
include/trs_dynamics.h against its ctypes table and the library."""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import truss_oracle as orc
from python_stable_3d_truss_analysis_amd import _capi, batch
from tests import dynamics_reference as dref
from tests import modes_reference as mref
from tests.helpers import GOLDEN, ROOT, load_json
from tests.test_capi_symbols import declared_prototypes, declared_symbols


def _modes(data):
    K, m, mask = mref.matrices(data)
    s = 1.0 / np.sqrt(m)
    lam, y = np.linalg.eigh(K * s[:, None] * s[None, :])
    return K, m, mask, lam, s[:, None] * y


def _own_pattern(data):
    p = orc.prepare(data)
    return orc.force_vector(p).reshape(1, len(p.pos), p.dim)


# bar-72_input_1, not _input_0: the load of _input_0 is orthogonal to the (double) first mode of the tower, so its
# projection is rounding noise and has no order
@pytest.mark.parametrize("name", ["bar-10_input_0", "bar-25_input_0", "bar-47_input_0", "bar-72_input_1", "cube-7_case_3"])
def test_step_load_converges_at_second_order_on_the_first_mode(name):
    """q_1(t) = phi_1^T M u(t) under a step load against (phi_1^T f / lambda_1)(1 - cos omega_1 t), the first term of
    sum_i phi_i (phi_i^T f / lambda_i)(1 - cos omega_i t): over one fundamental period with 64, 128 and 256 steps the
    largest error falls by 4 per halving (measured: 3.997 and 3.999 on all five)."""
    data = load_json(name)
    K, m, mask, lam, phi = _modes(data)
    f = orc.force_vector(data)[mask]
    omega = np.sqrt(lam[0])
    errs = []
    for steps in (64, 128, 256):
        dt = 2.0 * np.pi / omega / steps
        u = dref.newmark(data, _own_pattern(data), dt, steps)["u"][0].reshape(steps + 1, -1)[:, mask]
        exact = (phi[:, 0] @ f / lam[0]) * (1.0 - np.cos(omega * dt * np.arange(steps + 1)))
        errs.append(np.abs(u @ (m * phi[:, 0]) - exact).max())
    for ratio in (errs[0] / errs[1], errs[1] / errs[2]):
        assert 3.8 <= ratio <= 4.2, (name, errs)


@pytest.mark.parametrize("name", ["bar-25_input_0", "bar-47_input_0"])
def test_average_acceleration_conserves_energy_once_the_load_is_gone(name):
    data = load_json(name)
    K, m, mask, lam, _ = _modes(data)
    steps, loaded = 96, 24
    dt = 2.0 * np.pi / np.sqrt(lam[0]) / 24
    scale = np.zeros([1, steps + 1])
    scale[0, :loaded] = 1.0
    r = dref.newmark(data, _own_pattern(data), dt, steps, scale=scale)
    u = r["u"][0].reshape(steps + 1, -1)[:, mask]
    v = r["v"][0].reshape(steps + 1, -1)[:, mask]
    energy = 0.5 * (v * v * m).sum(1) + 0.5 * np.einsum("ti,ij,tj->t", u, K, u)
    free = energy[loaded:]      # f_n = f_(n+1) = 0 from point `loaded` on
    assert free.min() > 0 and np.ptp(free) <= 1e-10 * free.max(), (free.min(), free.max())
    assert np.ptp(energy[:loaded]) > 1e-3 * free.max()      # (while the load works the energy does change)


@pytest.mark.parametrize("name", ["bar-10_input_0", "bar-25_input_0"])
def test_strong_mass_damping_under_a_step_load_tends_to_the_static_solution(name):
    """alpha = 2 omega_1: the first mode is critically damped, (1 + omega_1 t) exp(-omega_1 t), and every other mode decays
    like exp(-omega_1 t).  The scheme's own decay rate is off by O((omega_1 dt)^2) = 4 % at 32 steps per period, so even at
    half the exact rate what is left at t = 80 / omega_1 is below 81 exp(-40) = 3e-16 of the static response; the bound
    1e-9 leaves room for the rounding of the oracle's own solve."""
    data = load_json(name)
    K, m, mask, lam, _ = _modes(data)
    omega = np.sqrt(lam[0])
    dt = 2.0 * np.pi / omega / 32
    steps = int(np.ceil(80.0 / omega / dt))
    r = dref.newmark(data, _own_pattern(data), dt, steps, damp_mass=2.0 * omega)
    static = orc.solve(data)["u"]
    assert np.abs(r["u"][0, -1] - static).max() <= 1e-9 * np.abs(static).max()
    assert np.abs(r["v"][0, -1]).max() <= 1e-9 * omega * np.abs(static).max()


def test_the_excitations_of_the_parity_tests_show_no_tie_in_the_yardstick_itself():
    """The peak steps of the float64 and the longdouble yardstick agree entry for entry on the default batch (both
    settings), so a device step that differs is the device's doing; their relative difference is the measured 1e-14 ..
    1e-13 from which the GPU tests take their tolerance."""
    datas = [load_json(n) for n in dref.BATCH]
    for damped in (False, True):
        r64, rld = dref.reference(datas, 3, 32, damped), dref.reference(datas, 3, 32, damped, np.longdouble)
        for b in range(len(datas)):
            for key in ("u_step", "N_max_step", "N_min_step"):
                np.testing.assert_array_equal(r64[b][key], rld[b][key], err_msg=f"{dref.BATCH[b]} {key}")
            assert dref.relative_difference(r64[b], rld[b]) <= 1e-11


def test_stored_tolerance_of_the_large_truss_names_its_inputs():
    """tests/golden/dynamics_tol.json: the float64 - longdouble difference of the yardstick on bar-942 (computed once, it
    takes seconds) with the seed and the shape of the excitation it was measured on."""
    with open(os.path.join(GOLDEN, "dynamics_tol.json")) as fh:
        tol = json.load(fh)
    assert tol["truss"] == dref.BIG and tol["seed"] == dref.SEED and tol["L"] == 3 and tol["steps"] == 32
    for key in ("undamped", "damped"):
        assert 1e-13 < tol["relative_difference"][key] < 1e-9


# ---- the pure host pieces ---------------------------------------------------------------------------------------------
def _packed():
    return batch.pack_json([load_json("bar-10_input_0"), load_json("bar-25_input_0")])


def _good(packed, L=2, steps=4):
    return dict(pattern=np.zeros([packed.B, L, packed.nJ_max, 3]), dt=0.01, steps=steps)


def test_check_transient_args_accepts_and_normalises():
    packed = _packed()
    T1 = 5
    given = batch._check_transient_args(packed, np.ones([2, 2, packed.nJ_max, 2]), 0.01, 4, scale=np.ones([2, 2, T1]),
                                        accel=np.ones([2, 2, T1, 2]), monitor_joints=[[0, -1], [3, 9]],
                                        monitor_members=np.array([[0], [24]]), joint_mass=np.ones([2, packed.nJ_max]))
    assert given["pattern"].shape == (2, 2, packed.nJ_max, 3) and not given["pattern"][..., 2].any()
    assert given["accel"].shape == (2, 2, T1, 3) and given["monitor_joints"].dtype == np.int32
    assert given["monitor_members"].shape == (2, 1) and given["scale"].flags.c_contiguous
    none = batch._check_transient_args(packed, **_good(packed))
    assert none["scale"] is None and none["accel"] is None and none["monitor_joints"].shape == (2, 0)


@pytest.mark.parametrize("change, word", [
    (dict(dt=0.0), "dt"), (dict(dt=-1.0), "dt"), (dict(dt=float("nan")), "dt"), (dict(beta=0.0), "beta"),
    (dict(gamma=0.49), "gamma"), (dict(damp_mass=-1e-3), "damp"), (dict(damp_stiff=float("inf")), "damp_stiff"),
    (dict(damp_stiff=-1.0), "damp"), (dict(steps=0), "steps"), (dict(steps=2.5), "steps"), (dict(steps=True), "steps"),
    (dict(sections=[(1.0, 1.0, 1.0)]), "sections"), (dict(max_result_bytes=100), "max_result_bytes"),
    (dict(mass_scale=-1.0), "mass_scale"),
])
def test_check_transient_args_refuses_bad_scalars(change, word):
    packed = _packed()
    with pytest.raises(ValueError, match=word):
        batch._check_transient_args(packed, **dict(_good(packed), **change))


def test_check_transient_args_refuses_bad_arrays():
    packed = _packed()
    nJ = packed.nJ_max
    good = _good(packed)

    def refuse(match, **change):
        with pytest.raises(ValueError, match=match):
            batch._check_transient_args(packed, **dict(good, **change))

    refuse("pattern", pattern=np.zeros([2, 0, nJ, 3]))                  # L = 0
    refuse("pattern", pattern=np.zeros([2, 2, nJ + 1, 3]))
    refuse("pattern", pattern=np.zeros([3, 2, nJ, 3]))
    refuse("pattern", pattern=np.zeros([2, 2, nJ, 4]))
    refuse("pattern", pattern=np.zeros([2, nJ, 3]))
    nan = np.zeros([2, 2, nJ, 3])
    nan[1, 0, 2, 1] = np.nan
    refuse("non-finite", pattern=nan)
    z = np.zeros([2, 2, nJ, 3])
    z[0, 1, 0, 2] = 1.0                                                    # truss 0 (bar-10) is 2D
    refuse("2D", pattern=z)
    z3 = np.zeros([2, 2, nJ, 3])
    z3[1, 1, 0, 2] = 1.0                                                   # truss 1 (bar-25) is 3D: fine
    batch._check_transient_args(packed, **dict(good, pattern=z3))
    refuse("scale", scale=np.ones([2, 2, 4]))
    refuse("scale", scale=np.full([2, 2, 5], np.inf))
    refuse("accel", accel=np.ones([2, 2, 4, 3]))
    refuse("accel", accel=np.ones([2, 2, 5]))
    za = np.zeros([2, 2, 5, 3])
    za[0, 0, 3, 2] = 1.0
    refuse("2D", accel=za)
    refuse("non-finite", accel=np.full([2, 2, 5, 3], np.nan))
    refuse("monitor_joints", monitor_joints=[[0], [int(packed.nJ[1])]])
    refuse("monitor_joints", monitor_joints=[[int(packed.nJ[0])], [0]])   # inside the padding, outside the truss
    refuse("monitor_joints", monitor_joints=[[-2], [0]])
    refuse("monitor_joints", monitor_joints=[0, 1])
    refuse("monitor_joints", monitor_joints=[[0.5], [1.0]])
    refuse("monitor_members", monitor_members=[[int(packed.nM[0])], [0]])
    refuse("joint_mass", joint_mass=np.ones([2, nJ + 1]))
    refuse("joint_mass", joint_mass=-np.ones([2, nJ]))


def test_newmark_constants_are_the_headers_formulas():
    c = batch.newmark_constants(0.02, 0.3, 0.6, 0.5, 0.001)
    r = dref.constants(0.02, 0.3, 0.6, 0.5, 0.001)
    for key in ("a0", "a1", "a2", "a3", "a4", "a5", "s", "sigma"):
        assert c[key] == float(r[key]), key
    assert batch.newmark_constants(0.5)["sigma"] == 16.0 and batch.newmark_constants(0.5)["s"] == 1.0


def test_header_table_and_library_agree():
    names = declared_symbols("trs_dynamics.h")
    assert names == ["trs_dyn_abi_version", "trs_dyn_collect", "trs_dyn_fits", "trs_dyn_shift", "trs_dyn_step",
                     "trs_dyn_tab_step"]
    assert sorted(_capi.DYN_SIGNATURES) == names
    protos = declared_prototypes("trs_dynamics.h")
    assert sorted(protos) == names
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name, (is_void, n_params) in protos.items():
        restype, argtypes = _capi.DYN_SIGNATURES[name]
        assert hasattr(lib, name), name
        assert len(argtypes) == n_params and not is_void and restype is ctypes.c_int, name
    header = open(os.path.join(ROOT, "include", "trs_dynamics.h")).read()
    assert "#define TRS_DYN_ABI_VERSION %d\n" % _capi.DYN_ABI_VERSION in header
    assert _capi.load().trs_dyn_abi_version() == _capi.DYN_ABI_VERSION == 1
    # nothing was added to trs_solver.h
    assert not any(name.startswith("trs_dyn") for name in _capi.SIGNATURES)


def test_tab_twin_mirrors_the_general_step():
    sig = _capi.DYN_SIGNATURES
    assert [name for name in sig if "_tab_" in name] == ["trs_dyn_tab_step"]
    assert sig["trs_dyn_tab_step"] == sig["trs_dyn_step"]      # (conn16, type_idx, types) for (conn, E, A): pointers all


def test_fits_rule_in_bytes():
    """One DOF vector; with beta_R > 0 one double per member and the end lists - the rule of trs_effects_fits - within
    160 KB, rounded up to 16 bytes."""
    lib = _capi.load()
    budget = 160 * 1024
    undamped = lambda nJ: (24 * nJ + 15) // 16 * 16
    damped = lambda nJ, nM: (32 * nJ + 16 * nM + 4 + 15) // 16 * 16
    assert lib.trs_dyn_fits(244, 942, 0) and lib.trs_dyn_fits(244, 942, 1)
    assert undamped(6826) <= budget < undamped(6827)
    assert lib.trs_dyn_fits(6826, 10 ** 6, 0) == 1 and lib.trs_dyn_fits(6827, 0, 0) == 0
    for nJ, nM in ((100, 10233), (100, 10234), (5119, 0), (5120, 0), (2000, 6239), (2000, 6240), (2000, 6241)):
        assert lib.trs_dyn_fits(nJ, nM, 1) == int(damped(nJ, nM) <= budget), (nJ, nM)
        assert lib.trs_dyn_fits(nJ, nM, 1) == lib.trs_effects_fits(nJ, nM), (nJ, nM)
    assert damped(2000, 6239) <= budget < damped(2000, 6240)
    assert lib.trs_dyn_fits(-1, 0, 0) == 0 and lib.trs_dyn_fits(0, -1, 1) == 0
    # argument errors come back before any launch
    assert lib.trs_dyn_shift(1, None, 100, 128, None, None, 128, 1.0, None) != 0        # ld < slab_rows
    assert lib.trs_dyn_shift(0, None, 144, 128, None, None, 128, 1.0, None) == 0         # an empty batch: nothing to do
