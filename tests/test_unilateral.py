"""Tension-only and compression-only members, the parts that need no GPU: the numpy yardstick
(`tests/unilateral_reference.py`) against a closed form, the admissibility of every parity case of the GPU tests and the
recorded float64-against-longdouble floors, the refusals of `_check_unilateral_args` and `Truss.SolveUnilateral`, the LDS
rule of `trs_un_fits` to the byte, and the C interface of include/trs_unilateral.h against its ctypes table and the
library."""
import ctypes
import json
import os

import numpy as np
import pytest

from python_stable_3d_truss_analysis_amd import _capi, batch
from tests import unilateral_reference as uref
from tests.helpers import GOLDEN, ROOT, load_json
from tests.test_capi_symbols import declared_prototypes, declared_symbols
from tests.test_sizing import largest

H = 1000.0
ROOT2 = np.sqrt(2.0)


def panel_run(kinds, pretension=0.0, **kw):
    data, kind, pre = uref.panel(H, kinds, pretension)
    return uref.unilateral(data, uref.cases(data)[0], kind, pre, **kw)


def test_panel_with_two_tension_only_diagonals():
    """The square panel under the lateral load H: the diagonal that would shorten goes slack, the other carries sqrt 2 H,
    the leeward column H in compression, the beam half of H, the windward column nothing - statics alone, because the
    panel without one diagonal is determinate.  With both diagonals bilateral each carries half the shear."""
    r = panel_run((1, 1))
    assert (r["status"], r["iterations"], r["violations"]) == (uref.CONVERGED, 1, 0)
    assert list(r["state"]) == [1, 1, 1, 1, 0] and list(r["flips_history"][:3]) == [1, 0, 0]
    assert np.abs(r["N"] - np.array([0.0, -H, -0.5 * H, ROOT2 * H, 0.0])).max() <= 1e-12 * H
    assert r["areas_effective"][4] == 0.0 and (r["areas_effective"][:4] == 1.5).all()
    # the supports: joint 0 holds the diagonal's pull, joint 1 the column's push
    assert np.abs(r["f_ext"] - np.array([[-H, -H], [0.0, H], [0.5 * H, 0.0], [0.5 * H, 0.0]])).max() <= 1e-12 * H
    both = panel_run((0, 0))
    assert (both["status"], both["iterations"]) == (uref.CONVERGED, 0) and both["margin"] == np.inf
    assert np.abs(both["N"] - np.array([0.5 * H, -0.5 * H, 0.0, H / ROOT2, -H / ROOT2])).max() <= 1e-12 * H
    # compression-only diagonals: the mirror image
    struts = panel_run((-1, -1))
    assert list(struts["state"]) == [1, 1, 1, 0, 1]
    assert np.abs(struts["N"] - np.array([H, 0.0, 0.5 * H, 0.0, -ROOT2 * H])).max() <= 1e-12 * H
    # a slack member keeps slack_factor of its area: a thousandth of the force its shortening would give it
    soft = panel_run((1, 1), slack_factor=1e-3)
    data, _, _ = uref.panel(H)
    geo = uref.Geometry(data, np.float64)
    shortening = ((soft["u"][geo.j1[4]] - soft["u"][geo.j0[4]]) * geo.c[4]).sum()
    assert list(soft["state"]) == [1, 1, 1, 1, 0] and shortening < 0
    assert abs(soft["N"][4] - 1e-3 * geo.E[4] * geo.A0[4] * shortening / geo.L0[4]) <= 1e-12 * H
    assert abs(soft["N"][3] - ROOT2 * H) <= 1e-2 * H
    # the iteration limit, and an initial state that is the converged one
    cut = panel_run((1, 1), max_iters=0)
    assert (cut["status"], cut["iterations"], cut["violations"]) == (uref.ITER_LIMIT, 0, 1) and cut["state"].all()
    again = panel_run((1, 1), state=r["state"])
    assert (again["status"], again["iterations"]) == (uref.CONVERGED, 0) and np.array_equal(again["N"], r["N"])


def test_panel_with_pretension_keeps_both_diagonals():
    """A pretension of 2 H: neither diagonal goes slack, no flip.  The forces are the bilateral answer plus the panel's
    one self-stress state (x in both diagonals, -x / sqrt 2 in the four sides, the base being the supports)."""
    r = panel_run((1, 1), pretension=2.0 * H)
    assert (r["status"], r["iterations"], r["violations"]) == (uref.CONVERGED, 0, 0) and r["state"].all()
    N = r["N"]
    assert N[3] > 0 and N[4] > 0
    assert abs((N[3] - N[4]) - ROOT2 * H) <= 1e-12 * H                  # the shear, by statics
    x = 0.5 * (N[3] + N[4])
    assert 0 < x < 2.0 * H                                              # the frame gives: less than the pull put in
    want = np.array([0.5 * H - x / ROOT2, -0.5 * H - x / ROOT2, -x / ROOT2, H / ROOT2 + x, -H / ROOT2 + x])
    assert np.abs(N - want).max() <= 1e-12 * H
    # too little pretension: the windward diagonal still goes slack, and the other keeps its own pull on top
    weak = panel_run((1, 1), pretension=0.1 * H)
    assert list(weak["state"]) == [1, 1, 1, 1, 0] and weak["iterations"] == 1


def _runs():
    for name in uref.RUNS:
        if name == "big":
            continue
        rows, slack = uref.run_inputs(name)
        for b, (data, load, kind, pre) in enumerate(rows):
            yield name, b, slack, data, load, kind, pre


def test_parity_cases_are_admissible_and_cover_the_method():
    """Every case of the GPU parity tests: float64 and longdouble agree in state, status and iterations, and the sign
    of every unilateral e is clear in every analysis - margin >= 1000 x the float64-against-longdouble difference of e on
    the same scale.  The results are those of uref.TABLE.  Over the six fixtures at slack 0 at least four trusses
    converge and one takes two rounds; the status-2 trusses are there too."""
    with open(os.path.join(GOLDEN, "unilateral_tol.json")) as fh:
        rec = json.load(fh)
    assert rec["trusses"] == list(uref.BATCH) and rec["big_truss"] == uref.BIG and rec["max_iters"] == uref.MAX_ITERS
    assert sorted(rec["runs"]) == sorted(n for n in uref.RUNS if n != "big")
    worst = {}
    for name, b, slack, data, load, kind, pre in _runs():
        f64 = uref.unilateral(data, load, kind, pre, slack, uref.MAX_ITERS)
        f80 = uref.unilateral(data, load, kind, pre, slack, uref.MAX_ITERS, dtype=np.longdouble)
        what = (name, uref.RUNS[name][1][b])
        assert (f64["status"], f64["iterations"]) == (f80["status"], f80["iterations"]), what
        assert np.array_equal(f64["state"], f80["state"]) and np.array_equal(f64["flips_history"], f80["flips_history"]), what
        diff = uref.elongation_difference(f64, f80)
        print(what, "margin %.3g" % f64["margin"], "e difference %.3g" % diff, "status", f64["status"], f64["iterations"])
        assert f64["margin"] >= uref.ADMISSIBLE * diff, (what, f64["margin"], diff)
        status, iterations, flips = uref.TABLE[name][b]
        assert (f64["status"], f64["iterations"]) == (status, iterations), what
        assert tuple(f64["flips_history"][:len(flips)]) == flips and not f64["flips_history"][len(flips):].any(), what
        worst[name] = max(worst.get(name, 0.0), uref.relative_difference(f64, f80))
    for name, rel in worst.items():
        entry = rec["runs"][name]
        assert entry["slack_factor"] == uref.RUNS[name][0]
        assert [tuple(c) for c in entry["configs"]] == list(uref.RUNS[name][1])
        assert 0.5 * entry["relative_difference"] <= rel <= 2.0 * entry["relative_difference"], (name, rel)
    # coverage at slack 0, over the six fixtures
    table = dict(zip([c[0] for c in uref.RUNS["slack0"][1]][:6], uref.TABLE["slack0"][:6]))
    assert sorted(table) == sorted(uref.BATCH)
    assert sum(status == 0 for status, _, _ in table.values()) >= 4
    assert max(iterations for status, iterations, _ in table.values() if status == 0) >= 2
    assert sum(status == 2 for status, _, _ in table.values()) == 2
    # bar-942 takes a minute in longdouble: its record is only read
    big = rec["big"]
    assert [tuple(c) for c in big["configs"]] == list(uref.RUNS["big"][1]) and big["slack_factor"] == uref.RUNS["big"][0]
    assert 0 < big["relative_difference"] < 1e-9
    assert big["per_truss"][0]["margin"] >= uref.ADMISSIBLE * big["per_truss"][0]["elongation_difference"]


def _refused(word, packed, kind, **kwargs):
    with pytest.raises(ValueError, match=word):
        batch._check_unilateral_args(packed, kind, **kwargs)


def test_check_unilateral_args():
    packed = batch.pack_json([load_json("bar-10_input_0"), load_json("bar-25_input_0")])
    B, nJ, nM = packed.B, packed.nJ_max, packed.nM_max
    kind = np.zeros([B, nM])
    kind[0, 1], kind[1, 3] = 1, -1
    val = batch._check_unilateral_args(packed, kind)
    assert val["kind"].dtype == np.int8 and val["kind"][0, 1] == 1 and val["kind"][1, 3] == -1 and val["L"] == 1
    assert (val["slack_factor"], val["max_iters"], val["check_every"]) == (0.0, 20, 1)
    assert val["loads"] is None and val["prestrain"] is None and val["state"] is None
    val = batch._check_unilateral_args(packed, kind, np.zeros([B, 2, nJ, 2]), np.zeros([B, 2, nM]), slack_factor=1e-3,
                                       max_iters=0, state=np.ones([B, nM]))
    assert val["loads"].shape == (B, 2, nJ, 3) and val["prestrain"].shape == (B, 2, nM) and val["L"] == 2
    assert val["state"].dtype == np.int8 and val["max_iters"] == 0
    # the padding members are not looked at
    ragged = np.where(np.arange(nM)[None, :] < packed.nM[:, None], kind, 7.0)
    assert not batch._check_unilateral_args(packed, ragged)["kind"][0, packed.nM[0]:].any()
    for bad in (None, np.zeros([B, nM + 1]), np.zeros([B]), np.full([B, nM], 2.0), np.full([B, nM], 0.5),
                np.full([B, nM], float("nan")), "abc"):
        _refused("kind", packed, bad)
    for bad in (-1e-9, float("nan"), float("inf"), True, "0", None):
        _refused("slack_factor", packed, kind, slack_factor=bad)
    for bad in (-1, 2.5, True, None):
        _refused("max_iters", packed, kind, max_iters=bad)
    for bad in (0, -1, 2.5, True):
        _refused("check_every", packed, kind, check_every=bad)
    for bad in (np.zeros([B, 2, nJ]), np.zeros([B + 1, 1, nJ, 3]), np.zeros([B, 0, nJ, 3]), np.zeros([B, 1, nJ, 4]),
                np.full([B, 1, nJ, 3], float("nan"))):
        _refused("loads", packed, kind, loads=bad)
    for bad in (np.zeros([B, nM]), np.zeros([B, 1, nM + 1]), np.full([B, 1, nM], float("inf"))):
        _refused("prestrain", packed, kind, prestrain=bad)
    _refused("prestrain has L", packed, kind, loads=np.zeros([B, 2, nJ, 3]), prestrain=np.zeros([B, 3, nM]))
    for bad in (np.zeros([B, nM + 1]), np.full([B, nM], float("nan"))):
        _refused("state", packed, kind, state=bad)
    _refused("compact", packed, kind, options={"compact": True})
    _refused("sections", packed, kind, sections=[(1.0, 1.0, 1.0)])
    _refused("max_result_bytes", packed, kind, max_result_bytes=100)


def test_truss_solve_unilateral_refusals():
    """What `Truss.SolveUnilateral` refuses before any device work."""
    from python_stable_3d_truss_analysis_amd import LoadCase, Truss
    data, _, _ = uref.panel(H)
    truss = Truss(2).LoadFromJSON(data=data)
    with pytest.raises(ValueError, match="no such member"):
        truss.SolveUnilateral({7: "tension"})
    with pytest.raises(ValueError, match="'tension' or 'compression'"):
        truss.SolveUnilateral({3: "cable"})
    with pytest.raises(ValueError, match="one value per member"):
        truss.SolveUnilateral([0, 0, 1])
    with pytest.raises(ValueError, match="kind must hold"):
        truss.SolveUnilateral([0, 0, 0, 2, 0])
    with pytest.raises(ValueError, match="slack_factor"):
        truss.SolveUnilateral({3: "tension"}, slackFactor=-1.0)
    with pytest.raises(ValueError, match="forces and prestrains only"):
        truss.SolveUnilateral({3: "tension"}, [LoadCase(forces={3: (1.0, 0.0)}, gravity=(0.0, -1.0))])
    assert truss.SolveUnilateral({3: "tension"}, []) == []


def test_header_table_and_library_agree():
    names = declared_symbols("trs_unilateral.h")
    assert names == ["trs_un_abi_version", "trs_un_fits", "trs_un_step"]
    assert sorted(_capi.UN_SIGNATURES) == names
    protos = declared_prototypes("trs_unilateral.h")
    assert sorted(protos) == names
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name, (is_void, n_params) in protos.items():
        restype, argtypes = _capi.UN_SIGNATURES[name]
        assert hasattr(lib, name), name
        assert len(argtypes) == n_params and not is_void and restype is ctypes.c_int, name
    assert protos["trs_un_step"][1] == 28
    header = open(os.path.join(ROOT, "include", "trs_unilateral.h")).read()
    assert "#define TRS_UN_ABI_VERSION %d\n" % _capi.UN_ABI_VERSION in header
    assert _capi.load().trs_un_abi_version() == _capi.UN_ABI_VERSION == 1
    for word, value in (("ACTIVE", "(-1)"), ("CONVERGED", "0"), ("ITER_LIMIT", "1"), ("NOT_PD", "2")):
        assert "#define TRS_UN_%s %s\n" % (word, value) in header
        assert getattr(_capi, "UN_" + word) == getattr(uref, word) == int(value.strip("()"))
    assert "trs_unilateral.h" in _capi.__doc__
    # general member form only, and nothing was added to the other headers' tables
    assert not any(name.endswith("_tab") for name in _capi.UN_SIGNATURES)
    assert not any(name.startswith("trs_un") for table in (_capi.SIGNATURES, _capi.SZ_SIGNATURES, _capi.EFFECTS_SIGNATURES)
                   for name in table)
    makefile = open(os.path.join(_capi.CSRC_DIR, "Makefile")).read()
    assert " unilateral.hip " in makefile and makefile.count("include/trs_unilateral.h") == 2
    import python_stable_3d_truss_analysis_amd as pkg
    assert {"solve_unilateral", "UnilateralResult"} <= set(pkg.__all__)
    assert pkg.solve_unilateral is batch.solve_unilateral and pkg.UnilateralResult is batch.UnilateralResult
    assert set(batch.UnilateralResult.FIELDS) == set(batch.UnilateralResult.CASE_FIELDS)
    assert all(shape[0] == "L" for *_, shape in batch.UnilateralResult.FIELDS.values())


def test_fits_rule_in_bytes():
    """The step kernel: one displacement vector (3 nJ doubles), four ints for the wave counts, one byte per member:
    24 nJ + 16 + nM bytes, rounded up to 16, within the 160 KB of a CU - on shapes on both sides of the limit."""
    lib = _capi.load()
    budget = 160 * 1024
    rule = lambda nJ, nM: (8 * 3 * nJ + 4 * 4 + nM + 15) // 16 * 16
    assert rule(244, 942) == (24 * 244 + 16 + 942 + 15) // 16 * 16 <= budget and lib.trs_un_fits(244, 942) == 1
    assert lib.trs_un_fits(-1, 4) == 0 and lib.trs_un_fits(4, -1) == 0 and lib.trs_un_fits(65536, 0) == 0
    seen = set()
    for nJ in (0, 1, 7, 100, 244, 1000, 4000, 6825, 6826, 6827, 7000):
        if rule(nJ, 0) > budget:
            assert lib.trs_un_fits(nJ, 0) == 0
            continue
        top = largest(lambda nM: rule(nJ, nM) <= budget)
        assert rule(nJ, top) <= budget < rule(nJ, top + 1)
        for nM in range(max(top - 20, 0), top + 20):
            assert lib.trs_un_fits(nJ, nM) == int(rule(nJ, nM) <= budget), (nJ, nM, rule(nJ, nM))
            seen.add(lib.trs_un_fits(nJ, nM))
    for nM in (0, 1, 5, 942, 20000, 100000, 163824):
        top = largest(lambda nJ: rule(nJ, nM) <= budget)
        assert rule(top, nM) <= budget < rule(top + 1, nM)
        for nJ in range(max(top - 3, 0), top + 5):
            assert lib.trs_un_fits(nJ, nM) == int(rule(nJ, nM) <= budget), (nJ, nM, rule(nJ, nM))
            seen.add(lib.trs_un_fits(nJ, nM))
    assert seen == {0, 1}
    # argument errors come back before any launch; an empty batch is no error
    p8 = ctypes.c_void_p(8)
    bad = lambda **kw: lib.trs_un_step(*_step_args(p8, **kw))
    assert bad(B=0) == 0
    for kw in ({"nJ_max": 0}, {"slack_factor": -1.0}, {"slack_factor": float("nan")}, {"slack_factor": float("inf")},
               {"mode": 3}, {"mode": -1}, {"it": -1}, {"H": -1}, {"nJ_max": 7000, "nM_max": 10}, {"xyz": None}, {"kind": None}):
        assert bad(**kw) != 0, kw


def _step_args(p, B=1, nJ_max=10, nM_max=10, xyz=0, kind=0, slack_factor=0.0, it=0, mode=0, H=1):
    xyz = p if xyz == 0 else xyz
    kind = p if kind == 0 else kind
    return (B, nJ_max, nM_max, xyz, p, p, p, p, p, p, p, 64, p, None, kind, p, slack_factor, None, it, mode, p, p, p, p, p, p,
            H, None)
