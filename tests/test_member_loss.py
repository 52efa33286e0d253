"""Member-loss analysis, the part that needs no device: the numpy yardstick of the GPU tests
(`tests/member_loss_reference.py`) against itself and the exact invariant, the header `include/trs_loss.h` against its
ctypes table and the library's exports, `trs_loss_fits` against its documented rule, and the argument errors of
`solve_member_loss`."""
import ctypes
import os

import numpy as np
import pytest

from oracle import truss_oracle as orc
from python_stable_3d_truss_analysis_amd import _capi
from tests import helpers as H
from tests import member_loss_reference as M
from tests.test_capi_symbols import declared_prototypes, declared_symbols

#: fixture -> the number of members whose loss leaves a mechanism
CRITICAL = {"bar-10_input_0": 0, "bar-6_input_0": 0, "bar-25_input_0": 0, "bar-47_input_0": 12, "bar-72_input_0": 0,
            "bar-120_input_0": 0, "bar-942_input_0": 1, "cube-7_case_3": 9, "cube-7_case_10": 3}


@pytest.mark.parametrize("name", sorted(CRITICAL))
def test_the_two_routes_of_the_yardstick_agree(name):
    data, _loads, solved, closed, d = M.fixture(name)
    nM = len(data["member"])
    # the same members are critical either way, as many as known, with eleven orders of magnitude between the classes
    np.testing.assert_array_equal(solved["critical"], closed["critical"])
    assert int(solved["critical"].sum()) == CRITICAL[name]
    crit = solved["critical"]
    assert np.abs(closed["r"][crit]).max(initial=0.0) <= 1e-13 and closed["r"][~crit].min() >= 1e-4
    assert solved["eig_ratio"][crit].max(initial=0.0) <= 1e-15 and solved["eig_ratio"][~crit].min() >= 1e-8
    assert (closed["r"][~crit] <= 1.0 + 1e-12).all()
    # the exact invariant: the redundancies sum to the degree of statical indeterminacy
    assert abs(closed["r"].sum() - (nM - closed["n_free"])) <= 1e-9
    # rank-one update against deleting the member and solving again
    print(f"{name}: d = {d:.3e}")
    assert d <= (2e-10 if name == "bar-942_input_0" else 1e-12)
    for key in ("peak_stress", "peak_displace"):
        assert H.max_scaled_err(closed[key][:, ~crit], solved[key][:, ~crit]) <= 10 * max(d, 1e-15)
        assert np.isinf(solved[key][:, crit]).all() and np.isinf(closed[key][:, crit]).all()
    for key, gap, peak in (("peak_member", "stress_gap", "peak_stress"), ("peak_joint", "displace_gap", "peak_displace")):
        clear = (solved[gap] > 1e-6 * solved[peak][:, ~crit].max()) & ~crit[None, :]
        np.testing.assert_array_equal(closed[key][clear], solved[key][clear])
    assert (solved["N_after"][0, ~crit][:, ~crit].diagonal() == 0).all()


def test_stiffness_without_is_the_oracles_matrix_of_the_shortened_data():
    data = H.load_json("bar-72_input_0")
    p, dim = orc.prepare(data), 3
    blocks = [(j0 * dim, j1 * dim, orc.member_matK(p.pos[j0], p.pos[j1], a, e, length))
              for (j0, j1, a, e, _rho), length in zip(p.members, p.lengths)]
    for e in (0, 17, 71):
        less = dict(data, member=[m for i, m in enumerate(data["member"]) if i != e])
        np.testing.assert_array_equal(orc.global_K(less), M.stiffness_without(blocks, e, len(data["joint"]) * dim, dim))


def test_loss_header_table_and_exports_agree():
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    names = declared_symbols("trs_loss.h")
    protos = declared_prototypes("trs_loss.h")
    assert sorted(protos) == names == sorted(_capi.LOSS_SIGNATURES)
    assert names == ["trs_loss_abi_version", "trs_loss_apply", "trs_loss_fits", "trs_loss_rhs", "trs_loss_tab_apply",
                     "trs_loss_tab_rhs"]
    for name in names:
        assert hasattr(lib, name), f"{name} declared in trs_loss.h but not exported"
        restype, argtypes = _capi.LOSS_SIGNATURES[name]
        is_void, n_params = protos[name]
        assert len(argtypes) == n_params and not is_void and restype is ctypes.c_int, name
        assert not name.endswith("_tab")
    # the table form takes (conn16, type_idx, types) where the general form takes (conn, E, A)
    for stage in ("rhs", "apply"):
        assert _capi.LOSS_SIGNATURES[f"trs_loss_tab_{stage}"][1] == _capi.LOSS_SIGNATURES[f"trs_loss_{stage}"][1]
    # the other tables are disjoint from this one and are what they were
    others = set(_capi.SIGNATURES) | set(_capi.MODES_SIGNATURES) | set(_capi.EFFECTS_SIGNATURES)
    assert not set(_capi.LOSS_SIGNATURES) & others
    assert sorted(_capi.SIGNATURES) == declared_symbols() and len(_capi.SIGNATURES) == 44
    loaded = _capi.load()
    assert loaded.trs_loss_abi_version() == _capi.LOSS_ABI_VERSION == 1 and loaded.trs_abi_version() == 10
    header = open(os.path.join(H.ROOT, "include", "trs_loss.h")).read()
    assert "#define TRS_LOSS_ABI_VERSION 1\n" in header
    makefile = open(os.path.join(_capi.CSRC_DIR, "Makefile")).read()
    assert " loss.hip " in makefile and "../../include/trs_loss.h" in makefile


def loss_lds_rule(nJ_max, nM_max, cases=1):
    """The LDS rule as include/trs_loss.h states it, in bytes (rounded up to 16)."""
    doubles = 5 * nM_max + 4 * 3 * nJ_max + cases * (3 * nJ_max + nM_max)
    ints = 2 * nM_max + 4 * nJ_max
    return (8 * doubles + 4 * ints + 15) // 16 * 16


def test_loss_fits_is_its_documented_rule():
    lib = _capi.load()
    shapes = [(244, 942), (6, 10), (0, 0), (10, 1 << 20), (3000, 100), (1200, 1500), (1100, 1500), (500, 2400),
              (500, 2500), (2273, 0), (2274, 0), (-1, 5), (5, -1)]
    for nJ_max, nM_max in shapes:
        want = nJ_max >= 0 and nM_max >= 0 and loss_lds_rule(nJ_max, nM_max) <= 160 * 1024
        for L in (0, 1, 8, 100):
            assert lib.trs_loss_fits(nJ_max, nM_max, L) == int(want), (nJ_max, nM_max, L)
        assert lib.trs_loss_fits(nJ_max, nM_max, -1) == 0
    # both sides of the limit are in the list
    assert {bool(lib.trs_loss_fits(j, m, 1)) for j, m in shapes} == {True, False}
    assert lib.trs_loss_fits(244, 942, 8) == 1 and loss_lds_rule(244, 942, 8) > 160 * 1024   # eight cases: two passes
    # refused before any launch; an empty call is no error
    assert lib.trs_loss_apply(1, 1, 0, 16, 10, 1 << 20, *[None] * 9, 64, 1e-8, *[None] * 9) != 0
    assert lib.trs_loss_tab_apply(1, 1, 0, 16, 10, 20, *[None] * 9, 64, 1e-8, *[None] * 9) != 0   # no member table
    assert lib.trs_loss_apply(0, 1, 0, 16, 10, 20, *[None] * 9, 64, 1e-8, *[None] * 9) == 0
    assert lib.trs_loss_rhs(0, 0, 16, 10, 20, *[None] * 8, 64, None) == 0
    assert lib.trs_loss_rhs(1, -1, 16, 10, 20, *[None] * 8, 64, None) != 0


def test_solve_member_loss_argument_errors_need_no_gpu():
    import python_stable_3d_truss_analysis_amd as pkg
    from python_stable_3d_truss_analysis_amd import batch
    assert {"solve_member_loss", "MemberLossResult"} <= set(pkg.__all__)
    assert pkg.solve_member_loss is batch.solve_member_loss and pkg.MemberLossResult is batch.MemberLossResult
    assert hasattr(pkg.Truss, "MemberLoss") and hasattr(batch.DeviceBatch, "member_loss")
    assert 0.0 < batch.MEMBER_LOSS_R_TOL < 1.0
    packed = batch.pack_json([H.load_json("bar-25_input_0"), H.load_json("bar-10_input_0")])
    B, nJ, nM, L = 2, packed.nJ_max, packed.nM_max, 3
    ok = np.zeros([B, L, nJ, 3])
    nan = ok.copy()
    nan[1, 2, 0, 1] = np.nan
    bad = [dict(loads=np.zeros([B, L, nJ])), dict(loads=np.zeros([B + 1, L, nJ, 3])), dict(loads=np.zeros([B, L, nJ + 1, 3])),
           dict(loads=np.zeros([B, L, nJ, 4])), dict(loads=nan), dict(loads=np.full([B, L, nJ, 2], np.inf)),
           dict(loads=ok, sections=[None]), dict(sections=[(1.0, 1.0, 1.0)]),
           dict(loads=ok, r_tol=0.0), dict(loads=ok, r_tol=1.0), dict(loads=ok, r_tol=-1e-8), dict(r_tol=float("nan")),
           dict(r_tol=None), dict(r_tol=True), dict(chunk=0), dict(loads=ok, chunk=-16), dict(chunk=1.5),
           dict(loads=ok, want_forces=True, max_result_bytes=B * L * nM * nM * 8 - 1)]
    for kw in bad:
        with pytest.raises(ValueError):
            batch.solve_member_loss(packed, **kw)
    with pytest.raises(ValueError, match=str(B * L * nM * nM * 8)):   # the refusal names the byte count
        batch.solve_member_loss(packed, ok, want_forces=True, max_result_bytes=1000)
    # what IS allowed gets past the checks: the batch's own loads as one case, two-component loads padded
    own = batch._check_member_loss_args(packed, None, 1e-8, None)
    assert own.shape == (B, 1, nJ, 3) and np.array_equal(own[:, 0], packed.loads)
    two = batch._check_member_loss_args(packed, np.ones([B, L, nJ, 2]), 1e-6, None, True, B * L * nM * nM * 8)
    assert two.shape == (B, L, nJ, 3) and not two[..., 2].any() and two[..., :2].all()
    # the unstable-truss refusal of MemberLoss comes before any arithmetic, and no cases need no device
    from python_stable_3d_truss_analysis_amd.utils import TrussNotStableError
    loose = pkg.Truss(3)
    loose.AddNewJoint((0.0, 0.0, 0.0))
    with pytest.raises(TrussNotStableError):
        loose.MemberLoss()
    assert pkg.Truss(3).LoadFromJSON(data=H.load_json("bar-25_input_0")).MemberLoss([]) == []
