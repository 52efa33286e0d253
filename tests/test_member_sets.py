"""Member-set scenarios, the part that needs no device: the numpy yardstick of the GPU tests
(`tests/member_sets_reference.py`) against itself and against the member-loss yardstick, the planner of
`DeviceBatch.member_sets`, the header `include/trs_sets.h` against its ctypes table, the library's exports and the
documented `trs_sets_fits` rule, and the argument errors of `solve_member_sets`."""
import ctypes
import os

import numpy as np
import pytest

from python_stable_3d_truss_analysis_amd import _capi
from tests import helpers as H
from tests import member_loss_reference as M
from tests import member_sets_reference as R
from tests.test_capi_symbols import declared_prototypes, declared_symbols

FIXTURES = ["bar-6_input_0", "bar-10_input_0", "bar-25_input_0", "bar-47_input_0", "bar-72_input_0", "bar-120_input_0",
            "cube-7_case_3"]
BOTH_KINDS = {"bar-6_input_0", "bar-10_input_0", "bar-25_input_0", "bar-47_input_0", "cube-7_case_3"}
R_TOL = 1e-8


@pytest.mark.parametrize("name", FIXTURES)
def test_the_two_routes_of_the_yardstick_agree(name):
    data, scen, _loads, solved, closed, d = R.fixture(name)
    nM = len(data["member"])
    assert scen[40] == ([], []) and len(scen) == 41 + nM
    # the two routes agree on stability and on where it is lost, for every scenario
    np.testing.assert_array_equal(solved["unstable"], closed["unstable"])
    np.testing.assert_array_equal(solved["first_unstable"], closed["first_unstable"])
    bad = solved["unstable"]
    # a condition on the inputs (change the seed if it fails): no scenario sits between the two classes
    assert not ((solved["eig_ratio"] >= 1e-12) & (solved["eig_ratio"] < 1e-7)).any()
    # the default r_tol lies a factor 100 from either class
    sizes = np.array([len(members) for members, _f in scen])
    for s in range(len(scen)):
        p = closed["pivot"][s]
        if bad[s]:
            j = closed["first_unstable"][s]
            assert abs(p[j]) <= R_TOL / 100 and np.isnan(p[j + 1:]).all() and (p[:j] >= 100 * R_TOL).all()
        else:
            assert (p[:sizes[s]] >= 100 * R_TOL).all() and np.isnan(p[sizes[s]:]).all()
    print(f"{name}: {int(bad.sum())} of {len(scen)} unstable, d = {d:.3e}, smallest stable pivot "
          f"{np.nanmin(closed['pivot'][~bad]):.2e}")
    if name in BOTH_KINDS:
        assert bad[:40].any() and not bad[:40].all()
    assert d <= 1e-11
    ok = ~bad
    for key in ("peak_stress", "peak_displace"):
        assert H.max_scaled_err(closed[key][:, ok], solved[key][:, ok]) <= 10 * max(d, 1e-15)
        assert np.isinf(solved[key][:, bad]).all() and np.isinf(closed[key][:, bad]).all()
    for key, gap, peak in (("peak_member", "stress_gap", "peak_stress"), ("peak_joint", "displace_gap", "peak_displace")):
        clear = (solved[gap] > 1e-6 * solved[peak][:, ok].max()) & ok[None, :]
        np.testing.assert_array_equal(closed[key][clear], solved[key][clear])
    # the empty set is the intact state
    np.testing.assert_array_equal(closed["N_after"][:, 40], closed["N"])
    np.testing.assert_array_equal(closed["U_after"][:, 40], closed["u"])
    # the singleton removals are the member-loss yardstick's closed form
    loss = M.closed_form(data)
    np.testing.assert_array_equal(closed["unstable"][41:], loss["critical"])
    assert np.abs(closed["pivot"][41:, 0] - loss["r"]).max() <= 1e-13
    keep = ~loss["critical"]
    for key in ("N_after", "U_after", "peak_stress", "peak_displace"):
        assert H.max_scaled_err(closed[key][:, 41:][:, keep], loss[key][:, keep]) <= 1e-12, key


def test_reordering_a_set_changes_the_pivots_but_not_their_product_or_the_state():
    data = H.load_json("bar-25_input_0")
    members, factors = [3, 11, 20, 7], [0.0, 0.5, 2.0, 0.0]
    a = R.closed_form(data, [(members, factors)])
    b = R.closed_form(data, [(members[::-1], factors[::-1])])
    assert not a["unstable"][0] and not b["unstable"][0]
    assert np.abs(a["pivot"][0, :4] - b["pivot"][0, 3::-1]).max() > 1e-3
    assert abs(np.prod(a["pivot"][0, :4]) / np.prod(b["pivot"][0, :4]) - 1.0) <= 1e-12
    assert H.max_scaled_err(a["U_after"], b["U_after"]) <= 1e-12 and H.max_scaled_err(a["N_after"], b["N_after"]) <= 1e-12


# ---- the planner --------------------------------------------------------------------------------------------------------
def random_sets(rng, B, S, nM, share=None):
    sets = np.full([B, S, 8], -1, dtype=np.int64)
    for b in range(B):
        for s in range(S):
            k = int(rng.integers(0, 9))
            sets[b, s, :k] = rng.choice(nM if share is None else share, size=k, replace=False)
    return sets


@pytest.mark.parametrize("chunk, nM, share", [(16, 200, None), (64, 200, None), (17, 942, None), (64, 942, 40),
                                               (1, 30, None), (1024, 30, None)])
def test_the_planner_cuts_the_scenarios_into_ranges_that_fit(chunk, nM, share):
    from python_stable_3d_truss_analysis_amd import batch
    B, S = 5, 37
    sets = random_sets(np.random.default_rng(chunk + nM), B, S, nM, share)
    plan = batch.plan_member_sets(sets, chunk, nM)
    C = max(16, min(-(-chunk // 16) * 16, -(-nM // 16) * 16))
    at, columns = 0, 0
    for s0, s1, cols, slot in plan:
        assert s0 == at and s1 > s0                     # consecutive, never empty: a scenario is never split
        at = s1
        assert cols.shape == (B, C) and cols.dtype == np.int32 and slot.shape == (B, s1 - s0, 8) and slot.dtype == np.int32
        for b in range(B):
            named = cols[b][cols[b] >= 0]
            want = np.unique(sets[b, s0:s1][sets[b, s0:s1] >= 0])
            assert len(named) == len(set(named)) <= C and sorted(named) == want.tolist()      # one column per DISTINCT member
            assert (cols[b][len(named):] == -1).all()
            columns += len(named)
            back = np.where(slot[b] >= 0, cols[b][np.maximum(slot[b], 0)], -1)
            np.testing.assert_array_equal(back, sets[b, s0:s1])                               # cols[slot] gives back every id
        # greedy: the next scenario would not have fitted
        if s1 < S:
            assert max(len(np.unique(sets[b, s0:s1 + 1][sets[b, s0:s1 + 1] >= 0])) for b in range(B)) > C
    assert at == S
    if share is not None:
        assert columns < (sets >= 0).sum() / 2          # shared members cost one column each
    assert batch.plan_member_sets(np.zeros([B, 0, 8], dtype=np.int64), chunk, nM) == []
    # all sets empty: one range, no column used
    (s0, s1, cols, slot), = batch.plan_member_sets(np.full([B, 4, 8], -1), chunk, nM)
    assert (s0, s1) == (0, 4) and (cols == -1).all() and (slot == -1).all()


# ---- header, table, exports, the fits rule, refusals before launch -------------------------------------------------------
def sets_lds_rule(nJ_max, nM_max, cases=1):
    """The LDS rule as include/trs_sets.h states it, in bytes (rounded up to 16)."""
    doubles = 5 * nM_max + 4 * 3 * nJ_max + 4 * 128 + cases * (3 * nJ_max + nM_max)
    ints = 2 * nM_max + 4 * nJ_max
    return (8 * doubles + 4 * ints + 15) // 16 * 16


def test_header_table_exports_and_the_fits_rule_agree():
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    names = declared_symbols("trs_sets.h")
    protos = declared_prototypes("trs_sets.h")
    assert sorted(protos) == names == sorted(_capi.SETS_SIGNATURES)
    assert names == ["trs_sets_abi_version", "trs_sets_apply", "trs_sets_fits", "trs_sets_rhs", "trs_sets_tab_apply",
                     "trs_sets_tab_rhs"]
    for name in names:
        assert hasattr(lib, name), f"{name} declared in trs_sets.h but not exported"
        restype, argtypes = _capi.SETS_SIGNATURES[name]
        is_void, n_params = protos[name]
        assert len(argtypes) == n_params and not is_void and restype is ctypes.c_int, name
    for stage in ("rhs", "apply"):
        assert _capi.SETS_SIGNATURES[f"trs_sets_tab_{stage}"][1] == _capi.SETS_SIGNATURES[f"trs_sets_{stage}"][1]
    others = set(_capi.SIGNATURES) | set(_capi.MODES_SIGNATURES) | set(_capi.EFFECTS_SIGNATURES) \
        | set(_capi.LOSS_SIGNATURES) | set(_capi.INFLUENCE_SIGNATURES)
    assert not set(_capi.SETS_SIGNATURES) & others
    header = open(os.path.join(H.ROOT, "include", "trs_sets.h")).read()
    assert "#define TRS_SETS_ABI_VERSION 1\n" in header and "#define TRS_SETS_MAX 8 " in header
    loaded = _capi.load()
    assert loaded.trs_sets_abi_version() == _capi.SETS_ABI_VERSION == 1 and _capi.SETS_MAX == 8
    makefile = open(os.path.join(_capi.CSRC_DIR, "Makefile")).read()
    assert " sets.hip " in makefile and " influence.hip " in makefile and "../../include/trs_sets.h" in makefile
    assert " trs_columns.h " in makefile
    # the row of the right-hand side exists once: the shared header forms it, the ONE rhs kernel (loss.hip) calls it,
    # and trs_sets_rhs goes through that kernel's launcher
    texts = {src: open(os.path.join(_capi.CSRC_DIR, src)).read() for src in ("loss.hip", "sets.hip", "trs_columns.h")}
    for src in ("loss.hip", "sets.hip"):
        assert '#include "trs_columns.h"' in texts[src] and "int at[6]" not in texts[src]
    assert texts["trs_columns.h"].count("int at[6]") == 1
    assert texts["loss.hip"].count("write_row(") == 1 and "write_row(" not in texts["sets.hip"]
    assert "rhs_kernel" not in texts["sets.hip"] and texts["sets.hip"].count("return rhs_launch(") == 1
    # trs_sets_fits is its documented rule, on both sides of the limit
    shapes = [(244, 942), (6, 10), (0, 0), (10, 1 << 20), (3000, 100), (1200, 1500), (1100, 1500), (500, 2400),
              (500, 2500), (2200, 0), (2300, 0), (-1, 5), (5, -1)]
    for nJ_max, nM_max in shapes:
        want = nJ_max >= 0 and nM_max >= 0 and sets_lds_rule(nJ_max, nM_max) <= 160 * 1024
        for L in (0, 1, 8, 100):
            assert loaded.trs_sets_fits(nJ_max, nM_max, L) == int(want), (nJ_max, nM_max, L)
        assert loaded.trs_sets_fits(nJ_max, nM_max, -1) == 0
    assert {bool(loaded.trs_sets_fits(j, m, 1)) for j, m in shapes} == {True, False}
    assert loaded.trs_sets_fits(244, 942, 8) == 1 and sets_lds_rule(244, 942, 8) > 160 * 1024   # eight cases: two passes
    # refused before any launch; an empty call is no error
    def apply(fn, B=1, L=1, S=4, s0=0, Sc=4, C=16, nJ_max=10, nM_max=20):
        return fn(B, L, S, s0, Sc, C, nJ_max, nM_max, *[None] * 12, 64, 1e-8, *[None] * 11)
    assert apply(loaded.trs_sets_apply, nM_max=1 << 20) != 0            # does not fit
    assert apply(loaded.trs_sets_apply, L=-1) != 0
    assert apply(loaded.trs_sets_apply, s0=2) != 0                       # s0 + Sc > S
    assert apply(loaded.trs_sets_apply) != 0                             # null arrays
    assert apply(loaded.trs_sets_tab_apply) != 0                         # no member table
    assert apply(loaded.trs_sets_apply, B=0) == 0 and apply(loaded.trs_sets_apply, Sc=0, S=0) == 0
    assert loaded.trs_sets_rhs(0, 16, 10, 20, *[None] * 9, 64, None) == 0
    assert loaded.trs_sets_rhs(1, 0, 10, 20, *[None] * 9, 64, None) == 0
    assert loaded.trs_sets_rhs(1, -1, 10, 20, *[None] * 9, 64, None) != 0
    assert loaded.trs_sets_rhs(1, 16, 10, 20, *[None] * 9, 64, None) != 0
    assert loaded.trs_sets_tab_rhs(1, 16, 10, 20, *[None] * 9, 64, None) != 0


# ---- the argument errors need no device -----------------------------------------------------------------------------------
def test_solve_member_sets_argument_errors_need_no_gpu():
    import python_stable_3d_truss_analysis_amd as pkg
    from python_stable_3d_truss_analysis_amd import batch
    assert {"solve_member_sets", "MemberSetResult"} <= set(pkg.__all__)
    assert pkg.solve_member_sets is batch.solve_member_sets and pkg.MemberSetResult is batch.MemberSetResult
    assert hasattr(pkg.Truss, "MemberSets") and hasattr(batch.DeviceBatch, "member_sets") and batch.MEMBER_SETS_MAX == 8
    packed = batch.pack_json([H.load_json("bar-25_input_0"), H.load_json("bar-10_input_0")])     # 25 and 10 members
    B, nJ, nM, L = 2, packed.nJ_max, packed.nM_max, 3
    ok_loads = np.zeros([B, L, nJ, 3])
    nan_loads = ok_loads.copy()
    nan_loads[1, 2, 0, 1] = np.nan
    good = [[[0, 3], [24]], [[9, 1, 2]]]
    arr = np.full([B, 2, 3], -1)
    arr[0, 0, :2], arr[0, 1, 0], arr[1, 0] = [0, 3], 24, [9, 1, 2]
    bad = [dict(sets=[[[0, 25]], []]),                                   # an id outside [0, nM[b])
           dict(sets=[[], [[10]]]),                                      # ... judged per truss: bar-10 has members 0 .. 9
           dict(sets=[[[-1]], []]), dict(sets=np.full([B, 1, 2], -2)),
           dict(sets=[[[4, 7, 4]], []]),                                 # a repeated id
           dict(sets=[[list(range(9))], []]), dict(sets=np.zeros([B, 1, 9], dtype=int)),   # more than 8 members
           dict(sets=np.array([[[-1, 3]], [[1, 2]]])),                   # padding inside a set
           dict(sets=[[[0]]]), dict(sets=np.zeros([B + 1, 1, 2], dtype=int)), dict(sets=np.zeros([B, 2])),
           dict(sets=np.zeros([B, 1, 2])),                               # ids must be integers
           dict(sets=good, factors=[[[0.5, -0.1], [1.0]], [[1, 1, 1]]]),          # a negative factor
           dict(sets=good, factors=[[[0.5, np.inf], [1.0]], [[1, 1, 1]]]),
           dict(sets=good, factors=[[[0.5, np.nan], [1.0]], [[1, 1, 1]]]),
           dict(sets=good, factors=[[[0.5], [1.0]], [[1, 1, 1]]]),                # not entry for entry
           dict(sets=arr, factors=np.ones([B, 2, 2])), dict(sets=arr, factors=np.ones([B, 3, 3])),
           dict(sets=good, sections=[None]), dict(sets=good, loads=nan_loads),
           dict(sets=good, loads=np.zeros([B, L, nJ + 1, 3])),
           dict(sets=good, r_tol=0.0), dict(sets=good, r_tol=1.0), dict(sets=good, r_tol=float("nan")),
           dict(sets=good, r_tol=True), dict(sets=good, chunk=0), dict(sets=good, chunk=1.5),
           dict(sets=good, loads=ok_loads, want_forces=True, max_result_bytes=B * L * 2 * nM * 8 - 1),
           dict(sets=good, loads=ok_loads, want_displace=True, max_result_bytes=B * L * 2 * nJ * 3 * 8 - 1)]
    for kw in bad:
        with pytest.raises(ValueError):
            batch.solve_member_sets(packed, **kw)
    with pytest.raises(ValueError, match=str(B * L * 2 * (nM + 3 * nJ) * 8)):   # the refusal names the byte count
        batch.solve_member_sets(packed, good, loads=ok_loads, want_forces=True, want_displace=True, max_result_bytes=1000)
    # what IS allowed gets past the checks: nested lists and the padded array give the same arrays
    sets, factors, loads = batch._check_member_sets_args(packed, good, None, None, 1e-8, None)
    assert sets.shape == (B, 2, 8) and sets.dtype == np.int32 and factors is None and loads.shape == (B, 1, nJ, 3)
    np.testing.assert_array_equal(sets[:, :, :3], arr)
    assert (sets[:, :, 3:] == -1).all() and (sets[1, 1] == -1).all()            # the shorter list is padded with an empty set
    again, g, _ = batch._check_member_sets_args(packed, arr, np.full([B, 2, 3], 0.5), ok_loads, 1e-6, None, True, True,
                                                B * L * 2 * (nM + 3 * nJ) * 8)
    np.testing.assert_array_equal(again, sets)
    assert g.shape == (B, 2, 8) and ((g == 0.5) == (sets >= 0)).all() and not g[sets < 0].any()
    _, g2, _ = batch._check_member_sets_args(packed, good, [[[0.5, 2.0], [0.0]], [[1, 1, 1]]], None, 1e-8, None)
    assert g2[0, 0, :2].tolist() == [0.5, 2.0] and g2[0, 1, 0] == 0.0 and g2[1, 0, :3].tolist() == [1, 1, 1]
    # the unstable-truss refusal of MemberSets comes before any arithmetic, and no cases need no device
    from python_stable_3d_truss_analysis_amd.utils import TrussNotStableError
    loose = pkg.Truss(3)
    loose.AddNewJoint((0.0, 0.0, 0.0))
    with pytest.raises(TrussNotStableError):
        loose.MemberSets([[0]])
    assert pkg.Truss(3).LoadFromJSON(data=H.load_json("bar-25_input_0")).MemberSets([[0, 1]], cases=[]) == []
