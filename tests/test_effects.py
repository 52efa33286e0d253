"""Load cases with support settlements, member pre-strain and self-weight, the part that needs no device: the numpy
yardstick of the GPU tests (`tests/effects_reference.py`) against physics, the header `include/trs_effects.h` against
its ctypes table and the library's exports, the argument errors of `solve_effect_cases`, and `LoadCase` packing."""
import ctypes
import os

import numpy as np
import pytest

from oracle import truss_oracle as orc
from python_stable_3d_truss_analysis_amd import _capi
from tests import effects_reference as R
from tests import helpers as H
from tests.test_capi_symbols import declared_prototypes, declared_symbols

TOL = 1e-9      # the project's tolerance for load cases (tests/test_gpu_load_cases.py)
NAMES = ["bar-25_input_0", "bar-72_input_0", "bar-942_input_0", "bar-10_input_0"]   # bar-10 is the 2D one


def geometry(data):
    dim = orc.truss_dim(data)
    X = np.array([p for p, _s in data["joint"]], dtype=float).reshape(-1, dim)
    members = R.members_of(data)
    return dim, X, max(k for _j0, _j1, _EA, k, _c, _h in members), max(EA for _j0, _j1, EA, _k, _c, _h in members)


def check_common_translation(data, solve):
    """(a) every constrained DOF settled by the same vector t: u = t at every joint, no member force, no support force."""
    dim, X, k_max, _ = geometry(data)
    t = np.array([0.013, -0.007, 0.021])[:dim]
    res = solve(data, settlement=np.tile(t, (len(X), 1)) * ~res_mask(data))
    assert H.max_scaled_err(res["u"], np.tile(t, (len(X), 1))) <= TOL
    scale = k_max * np.linalg.norm(t)
    assert np.abs(res["N"]).max() <= TOL * scale
    assert np.abs(res["f_ext"]).max() <= TOL * scale


def check_uniform_strain(data, solve):
    """(b) eps0 = e on every member, settlements e (x - x0) at the constrained DOFs: u = e (x - x0), N = 0."""
    dim, X, _, EA_max = geometry(data)
    e = 3.5e-4
    want = e * (X - X[0])
    res = solve(data, prestrain=np.full([len(data["member"])], e), settlement=want * ~res_mask(data))
    assert H.max_scaled_err(res["u"], want) <= TOL
    assert np.abs(res["N"]).max() <= TOL * EA_max * abs(e)
    assert np.abs(res["f_ext"]).max() <= TOL * EA_max * abs(e)


def check_unit_gravity(data, solve):
    """(c) unit downward accel: the supports carry the weight, and f_ext + body sums to zero per component."""
    from python_stable_3d_truss_analysis_amd import Truss
    dim = orc.truss_dim(data)
    weight = Truss(dim).LoadFromJSON(data=data).weight
    g = np.zeros([dim])
    g[dim - 1] = -1.0
    res = solve(data, accel=g)
    up = np.zeros([dim])
    up[dim - 1] = weight
    assert np.abs(res["f_ext"].sum(axis=0) - up).max() <= TOL * weight
    assert np.abs((res["f_ext"] + res["body"]).sum(axis=0)).max() <= TOL * weight
    assert np.abs(res["body"].sum(axis=0) + up).max() <= TOL * weight


def res_mask(data):
    """[nJ, dim] True at the FREE DOFs."""
    return orc.free_mask(data).reshape(len(data["joint"]), orc.truss_dim(data))


@pytest.mark.parametrize("name", NAMES)
def test_reference_common_translation(name):
    check_common_translation(H.load_json(name), R.solve)


@pytest.mark.parametrize("name", NAMES)
def test_reference_uniform_strain(name):
    check_uniform_strain(H.load_json(name), R.solve)


@pytest.mark.parametrize("name", NAMES)
def test_reference_unit_gravity(name):
    check_unit_gravity(H.load_json(name), R.solve)


@pytest.mark.parametrize("name", NAMES)
def test_reference_prestrain_is_its_equivalent_joint_loads(name):
    """(d) a prestrain-only case = the oracle under the equivalent joint loads, E A eps0 then taken off N (and the
    equivalent loads off the support forces)."""
    data = H.load_json(name)
    dim = orc.truss_dim(data)
    rng = np.random.default_rng(7)
    eps0 = rng.uniform(-5e-4, 5e-4, size=len(data["member"]))
    res = R.solve(data, prestrain=eps0)
    P0 = R.equivalent_loads(data, eps0)
    ref = orc.solve(dict(data, force=[[j, [float(x) for x in P0[j]]] for j in range(len(P0))]))
    EA = np.array([m[2] for m in R.members_of(data)])
    free = res_mask(data)
    assert H.max_scaled_err(res["u"], ref["u"]) <= TOL
    assert H.max_scaled_err(res["N"], ref["N"] - EA * eps0) <= TOL
    assert H.max_scaled_err(res["f_ext"], np.where(free, 0.0, ref["f_ext"] - P0)) <= TOL
    assert not res["body"].any() and res["u"].shape == (len(P0), dim)


def test_effects_header_table_and_exports_agree():
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    names = declared_symbols("trs_effects.h")
    protos = declared_prototypes("trs_effects.h")
    assert sorted(protos) == names == sorted(_capi.EFFECTS_SIGNATURES)
    assert names == ["trs_effects_abi_version", "trs_effects_fits", "trs_effects_recover", "trs_effects_rhs",
                     "trs_effects_tab_recover", "trs_effects_tab_rhs"]
    for name in names:
        assert hasattr(lib, name), f"{name} declared in trs_effects.h but not exported"
        restype, argtypes = _capi.EFFECTS_SIGNATURES[name]
        is_void, n_params = protos[name]
        assert len(argtypes) == n_params and not is_void and restype is ctypes.c_int, name
        assert not name.endswith("_tab")
    # the table form takes (conn16, type_idx, types) where the general form takes (conn, E, A, rho)
    for stage in ("rhs", "recover"):
        assert len(_capi.EFFECTS_SIGNATURES[f"trs_effects_tab_{stage}"][1]) == \
            len(_capi.EFFECTS_SIGNATURES[f"trs_effects_{stage}"][1]) - 1
    # the other tables are disjoint from this one and are what they were
    assert not set(_capi.EFFECTS_SIGNATURES) & (set(_capi.SIGNATURES) | set(_capi.MODES_SIGNATURES))
    assert sorted(_capi.SIGNATURES) == declared_symbols() and len(_capi.SIGNATURES) == 44
    loaded = _capi.load()
    assert loaded.trs_effects_abi_version() == _capi.EFFECTS_ABI_VERSION == 1 and loaded.trs_abi_version() == 10
    header = open(os.path.join(H.ROOT, "include", "trs_effects.h")).read()
    assert "#define TRS_EFFECTS_ABI_VERSION 1\n" in header
    # host-side answers: every truss of the tests fits, a shape beyond a CU's LDS does not and is refused before a launch
    assert loaded.trs_effects_fits(244, 942) == 1 and loaded.trs_effects_fits(10, 1 << 20) == 0
    assert loaded.trs_effects_rhs(1, 1, 10, 1 << 20, *[None] * 14, None, 64, None) != 0
    assert loaded.trs_effects_recover(1, 1, 10, 1 << 20, *[None] * 13, 64, *[None] * 6) != 0
    assert loaded.trs_effects_rhs(0, 1, 10, 20, *[None] * 14, None, 64, None) == 0


def test_solve_effect_cases_argument_errors_need_no_gpu():
    import python_stable_3d_truss_analysis_amd as pkg
    from python_stable_3d_truss_analysis_amd import batch
    assert {"solve_effect_cases", "EffectCaseResult", "LoadCase"} <= set(pkg.__all__)
    assert pkg.solve_effect_cases is batch.solve_effect_cases and pkg.EffectCaseResult is batch.EffectCaseResult
    assert hasattr(pkg.Truss, "SolveEffectCases") and hasattr(batch.DeviceBatch, "solve_effect_cases")
    data3, data2 = H.load_json("bar-25_input_0"), H.load_json("bar-10_input_0")
    packed = batch.pack_json([data3, data2])
    B, nJ, nM, L = 2, packed.nJ_max, packed.nM_max, 3
    held = ~np.stack([np.pad(res_mask(data3), ((0, nJ - len(data3["joint"])), (0, 0))),
                      np.pad(res_mask(data2), ((0, nJ - len(data2["joint"])), (0, 1)))])     # [B, nJ, 3]
    free3 = np.argwhere(res_mask(data3))[0]
    held3, held2 = np.argwhere(held[0])[0], np.argwhere(held[1, :, :2])[0]

    def settle(b, j, a, value=0.01):
        x = np.zeros([B, L, nJ, 3])
        x[b, 1, j, a] = value
        return x

    def accel(b, a, value=-1.0):
        x = np.zeros([B, L, 3])
        x[b, 2, a] = value
        return x

    bad = [dict(),                                                                     # nothing given
           dict(settlement=settle(0, *free3)),                                         # non-zero at a free DOF
           dict(settlement=settle(1, len(data2["joint"]), 0)),                         # ... at a padding joint
           dict(settlement=settle(1, held2[0], 2)),                                    # z settlement on the 2D truss
           dict(accel=accel(1, 2)),                                                    # z gravity on the 2D truss
           dict(accel=accel(0, 2, np.nan)), dict(prestrain=np.full([B, L, nM], np.inf)),
           dict(loads=settle(0, 0, 0, np.nan)), dict(settlement=settle(0, *held3, -np.inf)),
           dict(accel=accel(0, 2), sections=[None]),
           dict(loads=np.zeros([B, L, nJ, 3]), prestrain=np.zeros([B, L + 1, nM])),   # L differs
           dict(prestrain=np.zeros([B, L, nM + 1])), dict(accel=np.zeros([B, L])), dict(accel=np.zeros([B, L, 4])),
           dict(settlement=np.zeros([B + 1, L, nJ, 3])), dict(loads=np.zeros([B, L, nJ]))]
    for kw in bad:
        with pytest.raises(ValueError):
            batch.solve_effect_cases(packed, **kw)
    # what IS allowed gets past the checks (and then needs the device or not, which is not this test's business)
    L_ok, arrays = batch._check_effect_args(packed, None, np.zeros([B, L, nM]), settle(0, *held3) + settle(1, *held2),
                                            accel(0, 2) + accel(1, 1), None)
    assert L_ok == L and sorted(arrays) == ["accel", "prestrain", "settlement"]
    _, arrays = batch._check_effect_args(packed.take([1]), np.ones([1, L, nJ, 2]), None, None, np.ones([1, L, 2]), None)
    assert arrays["loads"].shape == (1, L, nJ, 3) and not arrays["loads"][..., 2].any() and arrays["accel"].shape == (1, L, 3)


def test_constrained_mask():
    """`PackedBatch.constrained()`: the bits of `cbits`, per axis, and nothing on padding joints."""
    from python_stable_3d_truss_analysis_amd import batch
    packed = batch.pack_json([H.load_json("bar-25_input_0"), H.load_json("bar-10_input_0")])
    held = packed.constrained()
    assert held.shape == (2, packed.nJ_max, 3) and held.dtype == bool
    for b in range(2):
        nJ = int(packed.nJ[b])
        for a in range(3):
            np.testing.assert_array_equal(held[b, :nJ, a], (packed.cbits[b, :nJ] >> a) & 1 == 1)
        assert not held[b, nJ:].any()
    assert held[1, :int(packed.nJ[1]), 2].all()          # a 2D truss never moves in z
    assert 3 * int(packed.nJ[0]) - int(held[0].sum()) == int(packed.n_free[0])


def test_load_case_packing():
    from python_stable_3d_truss_analysis_amd import LoadCase, Truss
    from python_stable_3d_truss_analysis_amd.truss import pack_load_cases
    from python_stable_3d_truss_analysis_amd.utils import DimensionError, InvaildJointError
    cases = [LoadCase(forces={3: (1.0, 2.0, 3.0)}),
             LoadCase(settlements={0: (0.0, 0.0, -0.01)}, prestrains={5: 1e-4, 0: -2e-4}),
             LoadCase(gravity=(0, 0, -1), forces={1: (0.0, -5.0, 0.0), 3: (4.0, 0.0, 0.0)})]
    d = pack_load_cases(cases, 6, 8, 3)
    assert d["loads"].shape == d["settlement"].shape == (1, 3, 6, 3) and d["prestrain"].shape == (1, 3, 8)
    assert d["accel"].shape == (1, 3, 3)
    want = np.zeros([1, 3, 6, 3])
    want[0, 0, 3], want[0, 2, 1], want[0, 2, 3] = (1, 2, 3), (0, -5, 0), (4, 0, 0)
    np.testing.assert_array_equal(d["loads"], want)
    assert d["settlement"][0, 1, 0, 2] == -0.01 and np.count_nonzero(d["settlement"]) == 1
    assert d["prestrain"][0, 1, 5] == 1e-4 and d["prestrain"][0, 1, 0] == -2e-4 and np.count_nonzero(d["prestrain"]) == 2
    np.testing.assert_array_equal(d["accel"][0], [[0, 0, 0], [0, 0, 0], [0, 0, -1]])
    # an effect that no case carries is absent; 2D vectors get z = 0
    d2 = pack_load_cases([LoadCase(gravity=(0, -1)), LoadCase(forces={0: (1.0, 2.0)})], 4, 5, 2)
    assert d2["settlement"] is None and d2["prestrain"] is None
    np.testing.assert_array_equal(d2["accel"][0], [[0, -1, 0], [0, 0, 0]])
    np.testing.assert_array_equal(d2["loads"][0, 1, 0], [1, 2, 0])
    assert all(v is None for v in pack_load_cases([LoadCase()], 4, 5, 2).values())
    with pytest.raises(InvaildJointError):
        pack_load_cases([LoadCase(settlements={6: (0, 0, 1)})], 6, 8, 3)
    with pytest.raises(KeyError):
        pack_load_cases([LoadCase(prestrains={8: 1e-4})], 6, 8, 3)
    with pytest.raises(DimensionError):
        pack_load_cases([LoadCase(gravity=(0, -1))], 6, 8, 3)
    # a LoadCase is a value: it copies what it is given
    forces = {0: (1.0, 0.0, 0.0)}
    case = LoadCase(forces=forces)
    forces[1] = (2.0, 0.0, 0.0)
    assert list(case.forces) == [0] and case.gravity is None and "LoadCase(" in repr(case)
    # the unstable-truss refusal of SolveEffectCases comes before any arithmetic, and no cases need no device
    from python_stable_3d_truss_analysis_amd.utils import TrussNotStableError
    loose = Truss(3)
    loose.AddNewJoint((0.0, 0.0, 0.0))
    with pytest.raises(TrussNotStableError):
        loose.SolveEffectCases([LoadCase(gravity=(0, 0, -1))])
    assert Truss(3).LoadFromJSON(data=H.load_json("bar-25_input_0")).SolveEffectCases([]) == []
