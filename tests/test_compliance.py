"""Compliance sizing, the parts that need no GPU: the numpy yardstick (`tests/compliance_reference.py`) against the
properties of the method - a falling objective at a constant measure, the closed form of a determinate truss, the
optimality conditions at convergence, the sensitivities against finite differences - and against the recorded
float64-against-longdouble floors; the refusals of `_check_min_compliance_args`, the LDS rule of `trs_cm_fits` to the
byte, and the C interface of include/trs_compliance.h against its ctypes table and the library."""
import ctypes
import dataclasses
import json
import os

import numpy as np
import pytest

from python_stable_3d_truss_analysis_amd import _capi, batch
from tests import compliance_reference as cref
from tests.helpers import GOLDEN, ROOT, load_json
from tests.test_capi_symbols import declared_prototypes, declared_symbols
from tests.test_sizing import largest

_cache = {}


def full(name, which):
    key = (name, which)
    if key not in _cache:
        data = load_json(name)
        _cache[key] = cref.minimise(data, **cref.config(data, which), **cref.FULL)
    return _cache[key]


def record():
    with open(os.path.join(GOLDEN, "compliance_tol.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("which", sorted(cref.CONFIGS))
def test_the_objective_never_rises_and_the_measure_is_the_target(which):
    """tol 1e-4, 60 resizings at most on the six small fixtures: J falls from analysis to analysis (the problem is convex
    and every resizing is a damped, move-limited step at the same measure), and from analysis 0 on - the target is the
    initial weight - the measure equals the target to 1e-12."""
    for name in cref.BATCH:
        r = full(name, which)
        n = len(r["changes"])
        history = r["objective_history"]
        assert n == r["iterations"] + 1 and not history[n:].any() and (history[:n] > 0).all(), name
        assert (np.diff(history[:n]) <= 0).all(), (which, name)
        assert history[n - 1] == r["objective"] and history[n - 1] < 0.9 * history[0], (which, name)
        assert max(abs(float(m) / float(r["target"]) - 1.0) for m in r["measures"]) <= 1e-12, (which, name)
        assert abs(float(r["measure"]) / float(r["target"]) - 1.0) <= 1e-12
        assert abs(float((np.asarray(cref.CONFIGS[which]) * r["compliance"]).sum()) / float(r["objective"]) - 1.0) <= 1e-14


def determinate():
    """Pin at (0, 0), roller (y held) at (4, 0), apex (2, 3) loaded off every member's axis: statically determinate,
    no zero-force member."""
    return {"joint": [[[0.0, 0.0], "PIN"], [[4.0, 0.0], "ROLLER_Y"], [[2.0, 3.0], "NO"]],
            "force": [[2, [300.0, -1000.0]]],
            "member": [[[0, 1], [1.0, 1.0e7, 0.1]], [[0, 2], [1.5, 1.0e7, 0.1]], [[1, 2], [2.0, 2.0e7, 0.3]]]}


def determinate_answer(target):
    """The member forces of a determinate truss do not depend on the areas, so s_m / w_m = N_m^2 / (E_m rho_m A_m^2) and
    the stationary design is A_m = c |N_m| / sqrt(E_m rho_m), c from sum rho L0 A = target."""
    data = determinate()
    geo = cref.Geometry(data, np.float64)
    an = cref.sref.analyse(geo, geo.A0, cref.cases(data)[:1], 1.0, 1.0)
    shape = np.abs(an["N"][0]) / np.sqrt(geo.E * geo.rho)
    assert (shape > 0).all()
    return shape * (target / (shape * geo.L0 * geo.rho).sum())


DETERMINATE = {"alpha": (1.0,), "target": 3.0, "eta": 0.5, "move": 1.0, "area_min": 1e-6, "area_max": 100.0}
#: the initial design as multiples of the answer: within a factor 2, so the move limit (1 + move) A does not bind
DETERMINATE_START = np.array([1.7, 0.6, 1.2])


def test_determinate_truss_reaches_the_closed_form_after_one_resizing():
    data = determinate()
    want = determinate_answer(DETERMINATE["target"])
    r = cref.minimise(data, cref.cases(data)[:1], areas=DETERMINATE_START * want, **DETERMINATE)
    assert r["status"] == cref.CONVERGED and r["iterations"] == 1 and len(r["changes"]) == 2
    assert np.abs(r["areas"] - want).max() <= 1e-12 * want.max()
    assert abs(r["measure"] - DETERMINATE["target"]) <= 1e-12 * DETERMINATE["target"]
    assert r["changes"][1] <= 1e-12
    geo = cref.Geometry(data, np.float64)
    N = cref.sref.analyse(geo, geo.A0, cref.cases(data)[:1], 1.0, 1.0)["N"][0]
    assert abs(r["objective"] / (N * N * geo.L0 / (geo.E * want)).sum() - 1.0) <= 1e-12      # J = sum N^2 L0 / (E A)
    assert np.abs(r["sensitivity"] / (r["multiplier"] * geo.rho * geo.L0) - 1.0).max() <= 1e-12


@pytest.mark.parametrize("which", sorted(cref.CONFIGS))
def test_optimality_conditions_at_convergence(which):
    """A converged truss has change <= tol < move, so a member whose new area no bound clamps has
    |(s / (multiplier w))^eta - 1| <= tol, that is |s / (multiplier w) - 1| <= 2 tol / eta.  `Strictly inside its bounds`
    is taken with that margin: a_min (1 + 2 tol) < A < a_max (1 - 2 tol)."""
    tol, eta, seen = cref.FULL["tol"], 0.5, 0
    for name in cref.BATCH:
        r = full(name, which)
        if r["status"] != cref.CONVERGED:
            continue
        data = load_json(name)
        kw = cref.config(data, which)
        geo = cref.Geometry(data, np.float64)
        w = cref.measure_weights(geo, "weight")
        inside = (r["areas"] > kw["area_min"] * (1 + 2 * tol)) & (r["areas"] < kw["area_max"] * (1 - 2 * tol))
        assert inside.sum() >= 2 and r["multiplier"] > 0, name
        ratio = r["sensitivity"][inside] / (r["multiplier"] * w[inside])
        print(which, name, int(inside.sum()), len(inside), float(np.abs(ratio - 1.0).max()))
        assert np.abs(ratio - 1.0).max() <= 2 * tol / eta, (which, name)
        # a member on its lower bound wants to shrink: s <= multiplier w there, with the same margin
        low = r["areas"] <= kw["area_min"]
        assert (r["sensitivity"][low] <= r["multiplier"] * w[low] * (1 + 2 * tol / eta)).all(), name
        seen += 1
    assert seen >= 3


@pytest.mark.parametrize("name", ["bar-10_input_0", "bar-25_input_0"])
def test_sensitivity_is_the_gradient_of_the_objective(name):
    """s_m = -dJ/dA_m against a central difference of the yardstick's own J with a step of 1e-4 A_m: the truncation is of
    relative order 1e-8, the rounding of order 1e-16 J / (1e-4 A_m s_max) - both far inside 1e-6 of the largest s."""
    data = load_json(name)
    kw = cref.config(data, "weighted")
    geo = cref.Geometry(data, np.float64)
    A = geo.A0 * (1.0 + 0.3 * np.sin(np.arange(len(geo.A0))))
    _, J, s, _ = cref.analysis(geo, A, kw["loads"], kw["alpha"])
    fd = np.zeros_like(s)
    for m in range(len(A)):
        h = 1e-4 * A[m]
        up, down = A.copy(), A.copy()
        up[m] += h
        down[m] -= h
        fd[m] = -(cref.analysis(geo, up, kw["loads"], kw["alpha"])[1] - cref.analysis(geo, down, kw["loads"], kw["alpha"])[1]) \
            / (up[m] - down[m])
    assert s.max() > 0 and (s >= 0).all()
    assert np.abs(fd - s).max() <= 1e-6 * s.max(), np.abs(fd - s).max() / s.max()
    assert abs((A * s).sum() / J - 1.0) <= 1e-12           # J is homogeneous of degree -1 in A


def test_recorded_floors_are_the_yardsticks_own():
    """tests/golden/compliance_tol.json: the largest max-scaled difference between the yardstick in float64 and in
    longdouble on the inputs of the GPU tests, at depth 6 with tol 0 and on the full runs; for the full runs also what
    the GPU test of the counts leans on: status, iterations and whether any `change` lies within 1 % of `tol`.  The small
    batch and the generated truss are measured again here (the figures of bar-942 and of the wide girder take minutes in
    longdouble and are only read)."""
    rec = record()
    assert rec["trusses"] == list(cref.BATCH) and rec["big_truss"] == cref.BIG and rec["decided"] == cref.DECIDED
    assert 257 <= rec["generated_members"] == len(cref.generated()["member"]) <= 512
    depth = {"tol": 0.0, "max_iters": cref.DEPTH}
    assert rec["wide"]["nx"] == cref.WIDE_NX and rec["wide"]["members"] == len(cref.generated(cref.WIDE_NX)["member"]) > 1024
    for part in ("depth", "generated", "big", "wide"):
        assert {k: rec[part][k] for k in depth} == depth and sorted(rec[part]["configs"]) == sorted(cref.CONFIGS)
    assert {k: rec["full"][k] for k in cref.FULL} == cref.FULL and sorted(rec["full"]["configs"]) == sorted(cref.CONFIGS)
    within = lambda worst, entry: 0.5 * entry["relative_difference"] <= worst <= 2.0 * entry["relative_difference"]
    for which in sorted(cref.CONFIGS):
        worst = max(cref.floor(load_json(name), which, depth)[0] for name in cref.BATCH)
        print("depth", which, worst, rec["depth"]["configs"][which]["relative_difference"])
        assert within(worst, rec["depth"]["configs"][which]), which
        worst = cref.floor(cref.generated(), which, depth)[0]
        print("generated", which, worst, rec["generated"]["configs"][which]["relative_difference"])
        assert within(worst, rec["generated"]["configs"][which]), which
        entry, worst = rec["full"]["configs"][which], 0.0
        for b, name in enumerate(cref.BATCH):
            diff, f64, f80 = cref.floor(load_json(name), which, cref.FULL)
            worst = max(worst, diff)
            assert (f64["status"], f64["iterations"]) == (f80["status"], f80["iterations"]) == \
                (entry["status"][b], entry["iterations"][b]), (which, name)
            tol = cref.FULL["tol"]
            assert entry["decided"][b] == (cref.decided(f64, tol) and cref.decided(f80, tol)), (which, name)
            assert abs(float(f64["changes"][-1]) - entry["last_change"][b]) <= 1e-6 * entry["last_change"][b]
        print("full", which, worst, entry["relative_difference"])
        assert within(worst, entry), which
        assert sum(entry["decided"]) >= 4 and sorted(set(entry["status"])) in ([0], [0, 1])
        assert 0 < rec["big"]["configs"][which]["relative_difference"] < 1e-9
        assert 0 < rec["wide"]["configs"][which]["relative_difference"] < 1e-8


def _refused(word, packed, **kwargs):
    args = {"area_min": 0.1, "area_max": 10.0}
    args.update(kwargs)
    with pytest.raises(ValueError, match=word):
        batch._check_min_compliance_args(packed, **args)


def test_check_min_compliance_args():
    packed = batch.pack_json([load_json("bar-10_input_0"), load_json("bar-25_input_0")])
    B, nJ, nM = packed.B, packed.nJ_max, packed.nM_max
    val = batch._check_min_compliance_args(packed, area_min=0.1, area_max=np.full([B, nM], 5.0))
    assert val["loads"] is None and val["target"] is None and list(val["alpha"]) == [1.0] and val["measure"] == "weight"
    assert (val["eta"], val["move"], val["tol"], val["max_iters"], val["check_every"]) == (0.5, 0.2, 1e-4, 60, 1)
    assert val["area_min"] == 0.1 and val["area_max"].shape == (B, nM)
    loads = np.zeros([B, 2, nJ, 2])
    val = batch._check_min_compliance_args(packed, loads, (0.6, 0.4), 3, "volume", 1.0, 1, 1.0, 1.0, 0.0, 0)
    assert val["loads"].shape == (B, 2, nJ, 3) and list(val["alpha"]) == [0.6, 0.4] and list(val["target"]) == [3.0, 3.0]
    assert (val["measure"], val["eta"], val["move"], val["tol"], val["max_iters"]) == ("volume", 1.0, 1.0, 0.0, 0)
    assert list(batch._check_min_compliance_args(packed, target=np.array([2.0, 3.0]), area_min=1, area_max=1)["target"]) \
        == [2.0, 3.0]
    assert list(batch._check_min_compliance_args(packed, loads, alpha=[0, 2], area_min=1, area_max=1)["alpha"]) == [0.0, 2.0]
    for bad in ((1.0,), (1.0, -0.1), (0.0, 0.0), (1.0, float("nan")), (1.0, float("inf")), 1.0, "ab", [[1.0, 1.0]]):
        _refused("alpha", packed, loads=loads, alpha=bad)
    _refused("alpha", packed, alpha=(0.5, 0.5))                       # (the batch's own loads are one case)
    for bad in (0.0, -1.0, float("nan"), float("inf"), True, "1", np.array([1.0, 0.0]), np.ones(B + 1), np.ones([B, 1])):
        _refused("target", packed, target=bad)
    for bad in ("mass", None, 0, b"weight"):
        _refused("measure", packed, measure=bad)
    for name in ("eta", "move"):
        for bad in (0.0, -0.5, 1.0000001, float("nan"), True, None, "1"):
            _refused(name, packed, **{name: bad})
    for bad in (-1e-9, float("nan"), float("inf"), True, "0", None):
        _refused("tol", packed, tol=bad)
    for bad in (-1, 2.5, True, None):
        _refused("max_iters", packed, max_iters=bad)
    for bad in (0, -1, 2.5, True):
        _refused("check_every", packed, check_every=bad)
    for bad in (None, 0.0, -1.0, float("nan"), True, np.full([B, nM + 1], 0.1), np.zeros([B, nM]), "x"):
        _refused("area_min", packed, area_min=bad)
    for bad in (None, 0.05, float("inf"), True, np.full([B], 5.0), np.full([B, nM], 0.01)):
        _refused("area_max", packed, area_max=bad)
    for bad in (np.zeros([B, 2, nJ]), np.zeros([B + 1, 1, nJ, 3]), np.zeros([B, 0, nJ, 3]), np.zeros([B, 1, nJ + 1, 3]),
                np.zeros([B, 1, nJ, 4]), np.full([B, 1, nJ, 3], float("nan"))):
        _refused("loads", packed, loads=bad)
    _refused("compact", packed, options={"compact": True})
    _refused("sections", packed, sections=[(1.0, 1.0, 1.0)])
    _refused("max_result_bytes", packed, max_result_bytes=100)
    flat = dataclasses.replace(packed, A=packed.A.copy())
    flat.A[1, 3] = 0.0
    _refused("initial design", flat)
    # a member that weighs nothing: refused for the weight, and the refusal names the way out
    light = dataclasses.replace(packed, rho=packed.rho.copy())
    light.rho[0, 2] = 0.0
    _refused("rho <= 0.*measure='volume'", light)
    assert batch._check_min_compliance_args(light, measure="volume", area_min=0.1, area_max=1.0)["measure"] == "volume"
    _refused("rho <= 0", light.table())
    # padding members are not looked at: bounds and densities that are wrong only there pass
    live = np.arange(nM)[None, :] < packed.nM[:, None]
    assert not live.all()
    padded = dataclasses.replace(packed, rho=np.where(live, packed.rho, 0.0))
    assert batch._check_min_compliance_args(padded, area_min=np.where(live, 0.1, -1.0), area_max=1.0)


def test_header_table_and_library_agree():
    names = declared_symbols("trs_compliance.h")
    assert names == ["trs_cm_abi_version", "trs_cm_fits", "trs_cm_step"]
    assert sorted(_capi.CM_SIGNATURES) == names
    protos = declared_prototypes("trs_compliance.h")
    assert sorted(protos) == names
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name, (is_void, n_params) in protos.items():
        restype, argtypes = _capi.CM_SIGNATURES[name]
        assert hasattr(lib, name), name
        assert len(argtypes) == n_params and not is_void and restype is ctypes.c_int, name
    assert protos["trs_cm_step"][1] == 41
    header = open(os.path.join(ROOT, "include", "trs_compliance.h")).read()
    assert "#define TRS_CM_ABI_VERSION %d\n" % _capi.CM_ABI_VERSION in header
    assert _capi.load().trs_cm_abi_version() == _capi.CM_ABI_VERSION == 1
    for word, value in (("ACTIVE", "(-1)"), ("CONVERGED", "0"), ("ITER_LIMIT", "1"), ("NOT_PD", "2")):
        assert "#define TRS_CM_%s %s\n" % (word, value) in header
        assert getattr(_capi, "CM_" + word) == getattr(cref, word) == int(value.strip("()"))
    for word, value in _capi.CM_MEASURES.items():
        assert "#define TRS_CM_%s %d\n" % (word.upper(), value) in header
    assert "#define TRS_CM_BISECTIONS %d\n" % cref.BISECTIONS in header
    # general member form only, a version of its own, and nothing was added to the other headers' tables
    assert not any(name.endswith("_tab") for name in _capi.CM_SIGNATURES)
    assert not any(name.startswith("trs_cm") for table in (_capi.SIGNATURES, _capi.SZ_SIGNATURES) for name in table)
    makefile = open(os.path.join(_capi.CSRC_DIR, "Makefile")).read()
    assert " compliance.hip " in makefile and makefile.count("include/trs_compliance.h") == 2
    # the header, the kernel and the yardstick state the method in the same words
    kernel = open(os.path.join(_capi.CSRC_DIR, "compliance.hip")).read()
    squeeze = lambda text: " ".join(text.replace("*", " ").replace("//", " ").split())
    for line in ("the bisection runs 64 times: xm = sqrt(x0 x1); if V(xm) <= W then x0 = xm, else x1 = xm",
                 "s_m = sum_l alpha_l (E_m / L0_m) proj_ml^2, summed in ascending l",
                 "a member with w_m <= 0 keeps lo_m = hi_m = clamp(A_m, a_min_m, a_max_m)"):
        assert line in squeeze(header) and line in squeeze(cref.__doc__), line
    for line in ("s_m = sum_l alpha_l (E_m / L0_m) proj_ml^2", "a member with w_m <= 0 keeps lo_m = hi_m = clamp(A_m, a_min_m, a_max_m)",
                 "xm = sqrt(x0 x1)"):
        assert line in squeeze(kernel), line
    import python_stable_3d_truss_analysis_amd as pkg
    assert {"solve_min_compliance", "MinComplianceResult"} <= set(pkg.__all__)
    assert pkg.solve_min_compliance is batch.solve_min_compliance and pkg.MinComplianceResult is batch.MinComplianceResult
    assert hasattr(pkg.Truss, "MinimizeCompliance") and hasattr(batch.DeviceBatch, "min_compliance")


def test_fits_rule_in_bytes():
    """The step kernel: two displacement vectors (6 nJ doubles), 64 doubles for the reductions, seven doubles and two
    ints per member, the reduced row of every DOF (3 nJ ints): 60 nJ + 512 + 64 nM bytes, rounded up to 16, within the
    160 KB of a CU - on shapes on both sides of the limit; bar-942 within HALF of it: two work-groups per CU."""
    lib = _capi.load()
    budget = 160 * 1024
    rule = lambda nJ, nM: (8 * (6 * nJ + 64 + 7 * nM) + 4 * (2 * nM + 3 * nJ) + 15) // 16 * 16
    assert rule(244, 942) == (60 * 244 + 512 + 64 * 942 + 15) // 16 * 16 <= budget // 2 and lib.trs_cm_fits(244, 942) == 1
    assert lib.trs_cm_fits(-1, 4) == 0 and lib.trs_cm_fits(4, -1) == 0 and lib.trs_cm_fits(65536, 0) == 0
    seen = set()
    for nJ in (0, 1, 7, 100, 244, 1000, 2000, 2721, 2722, 4000):
        if rule(nJ, 0) > budget:
            assert lib.trs_cm_fits(nJ, 0) == 0
            continue
        top = largest(lambda nM: rule(nJ, nM) <= budget)
        assert rule(nJ, top) <= budget < rule(nJ, top + 1)
        for nM in range(max(top - 3, 0), top + 5):
            assert lib.trs_cm_fits(nJ, nM) == int(rule(nJ, nM) <= budget), (nJ, nM, rule(nJ, nM))
            seen.add(lib.trs_cm_fits(nJ, nM))
    for nM in (0, 1, 5, 942, 2000, 2551):
        top = largest(lambda nJ: rule(nJ, nM) <= budget)
        assert rule(top, nM) <= budget < rule(top + 1, nM)
        for nJ in range(max(top - 3, 0), top + 5):
            assert lib.trs_cm_fits(nJ, nM) == int(rule(nJ, nM) <= budget), (nJ, nM, rule(nJ, nM))
            seen.add(lib.trs_cm_fits(nJ, nM))
    assert seen == {0, 1}
    # argument errors come back before any launch; an empty batch is no error
    p8 = ctypes.c_void_p(8)
    bad = lambda **kw: lib.trs_cm_step(*_step_args(p8, **kw))
    assert bad(B=0) == 0
    for kw in ({"L": 0}, {"measure": 2}, {"measure": -1}, {"eta": 0.0}, {"eta": 1.5}, {"move": 0.0}, {"move": 1.5},
               {"tol": -1.0}, {"tol": float("nan")}, {"a_min_all": 0.0}, {"a_max_all": 0.01}, {"mode": 2}, {"it": -1},
               {"levels": 4}, {"levels": -1}, {"nJ_max": 3000, "nM_max": 3000}, {"xyz": None}, {"alpha": None},
               {"target": None}):
        assert bad(**kw) != 0, kw


def _step_args(p, B=1, L=1, nJ_max=10, nM_max=10, xyz=0, alpha=0, target=0, measure=0, eta=0.5, move=0.2, tol=0.0,
               a_min_all=0.1, a_max_all=1.0, it=0, mode=0, levels=0):
    xyz, alpha, target = (p if x == 0 else x for x in (xyz, alpha, target))
    return (B, L, nJ_max, nM_max, xyz, p, p, p, p, p, p, p, p, p, 64, p, alpha, measure, target, eta, move, tol, None,
            a_min_all, None, a_max_all, it, mode, levels, p, p, p, p, p, p, p, p, 1, p, p, None)
