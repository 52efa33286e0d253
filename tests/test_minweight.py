"""Minimum weight under displacement limits, the parts that need no GPU: the numpy yardstick
(`tests/minweight_reference.py`) against the properties of the method - the closed form of a determinate truss, the
optimality conditions at convergence, the sensitivities against finite differences, the identity g = sum A c, the
weight against the displacement envelope of the stress-ratio sizing - and against the recorded float64-against-longdouble
floors; the refusals of `_check_min_weight_args`, the LDS rule of `trs_mw_fits` to the byte, and the C interface of
include/trs_minweight.h against its ctypes table and the library."""
import ctypes
import dataclasses
import json
import os

import numpy as np
import pytest

from python_stable_3d_truss_analysis_amd import _capi, batch
from tests import minweight_reference as mref
from tests.helpers import GOLDEN, ROOT, load_json
from tests.test_capi_symbols import declared_prototypes, declared_symbols
from tests.test_compliance import determinate
from tests.test_sizing import largest

_cache = {}


def full(name, which):
    key = (name, which)
    if key not in _cache:
        data = load_json(name)
        _cache[key] = mref.minimise(data, **mref.config(data, which), **mref.FULL)
    return _cache[key]


def record():
    with open(os.path.join(GOLDEN, "minweight_tol.json")) as fh:
        return json.load(fh)


#: one limit at the loaded joint along the load, move 1; the initial design as multiples of the answer, within a factor 2
DETERMINATE = {"move": 1.0, "area_min": 1e-6, "area_max": 100.0, "tol": 1e-10, "max_iters": 10}
DETERMINATE_START = np.array([1.7, 0.6, 1.2])
DETERMINATE_VALUE = 2.0e-4


def determinate_answer():
    """The member forces of a determinate truss do not depend on the areas: with the unit load along the load P,
    c_m A_m^2 = q_m = N_m^2 L0_m / (E_m |P|) > 0, the limit is sum q / A <= ubar, and the lightest design is
    A_m = sqrt(q_m / w_m) sum sqrt(q w) / ubar with the weight (sum sqrt(q w))^2 / ubar.  Returns (loads, limits, A, W)."""
    data = determinate()
    geo = mref.Geometry(data, np.float64)
    loads = mref.cases(data)[:1]
    force = loads[0, 2]
    N = mref.sref.analyse(geo, geo.A0, loads, 1.0, 1.0)["N"][0]
    q = N * N * geo.L0 / (geo.E * np.sqrt((force ** 2).sum()))
    w = geo.rho * geo.L0
    assert (q > 0).all()
    total = np.sqrt(q * w).sum()
    return loads, [(0, 2, force, DETERMINATE_VALUE)], np.sqrt(q / w) * total / DETERMINATE_VALUE, total ** 2 / DETERMINATE_VALUE


def test_determinate_truss_reaches_the_closed_form_after_one_resizing():
    loads, limits, want, weight = determinate_answer()
    r = mref.minimise(determinate(), loads, limits, areas=DETERMINATE_START * want, **DETERMINATE)
    assert r["status"] == mref.CONVERGED and r["iterations"] == 1 and len(r["changes"]) == 2
    assert np.abs(r["areas"] - want).max() <= 1e-12 * want.max()
    assert abs(r["measure"] - weight) <= 1e-12 * weight
    assert r["changes"][1] <= 1e-12 and abs(r["ratio"][0] - 1.0) <= 1e-12
    geo = mref.Geometry(determinate(), np.float64)
    assert np.abs(r["multipliers"][0] * r["sensitivity"][0] / (geo.rho * geo.L0) - 1.0).max() <= 1e-12   # mu c = w


@pytest.mark.parametrize("which", sorted(mref.CONFIGS))
def test_optimality_conditions_at_convergence(which):
    """A converged truss has change <= tol < move, so on a member that no bound clamps A'^2 = P / D lies within
    (1 +- tol)^2 of A^2: |sum_j mu_j c_mj - w_m| <= ((1 + tol)^2 - 1) D_m, D_m = w_m + sum_j mu_j max(-c_mj, 0).
    `Strictly inside its bounds` is taken with that margin: a_min (1 + 2 tol) < A < a_max (1 - 2 tol); the move limits
    cannot bind.  A limit with slack beyond limit_tol carries no multiplier."""
    tol, limit_tol, seen = mref.FULL["tol"], mref.FULL["limit_tol"], 0
    for name in mref.BATCH:
        r = full(name, which)
        if r["status"] != mref.CONVERGED:
            continue
        data = load_json(name)
        kw = mref.config(data, which)
        geo = mref.Geometry(data, np.float64)
        w = mref.measure_weights(geo, "weight")
        mu, c = r["multipliers"], r["sensitivity"]
        inside = (r["areas"] > kw["area_min"] * (1 + 2 * tol)) & (r["areas"] < kw["area_max"] * (1 - 2 * tol))
        assert inside.sum() >= 2 and mu.max() > 0, name
        D = w + (mu[:, None] * np.maximum(-c, 0)).sum(axis=0)
        gap = np.abs((mu[:, None] * c).sum(axis=0) - w) / D
        print(which, name, int(inside.sum()), len(inside), float(gap[inside].max()), r["ratio"], mu)
        assert gap[inside].max() <= (1 + tol) ** 2 - 1 + 1e-12, (which, name)
        assert not mu[r["ratio"] < 1 - limit_tol].any(), (which, name)
        assert r["worsts"][-1] <= 1 + limit_tol
        seen += 1
    assert seen >= 4


@pytest.mark.parametrize("name", ["bar-10_input_0", "bar-25_input_0"])
def test_sensitivity_is_the_gradient_of_the_limit_values(name):
    """c_mj = -dg_j/dA_m against a central difference of the yardstick's own g_j in longdouble with a step of 1e-5 A_m:
    the truncation is of relative order 1e-10, the rounding of order 1e-19 g / (1e-5 A_m c_max) - both far inside 1e-7
    of the largest |c_j|.  And g_j = sum_m A_m c_mj (virtual work: g = v.K u) to the solve's own rounding."""
    data = load_json(name)
    kw = mref.config(data, "pair")
    geo = mref.Geometry(data, np.longdouble)
    A = geo.A0 * (1 + np.longdouble(0.3) * np.sin(np.arange(len(geo.A0))))
    c, g, _ = mref.analysis(geo, A, kw["loads"], kw["limits"])
    fd = np.zeros_like(c)
    for m in range(len(A)):
        h = np.longdouble(1e-5) * A[m]
        up, down = A.copy(), A.copy()
        up[m] += h
        down[m] -= h
        fd[:, m] = -(mref.analysis(geo, up, kw["loads"], kw["limits"])[1] -
                     mref.analysis(geo, down, kw["loads"], kw["limits"])[1]) / (up[m] - down[m])
    for j in range(len(g)):
        assert np.abs(c[j]).max() > 0
        assert np.abs(fd[j] - c[j]).max() <= 1e-7 * np.abs(c[j]).max(), (j, float(np.abs(fd[j] - c[j]).max()))
        assert abs((A * c[j]).sum() - g[j]) <= 1e-14 * np.abs(A * c[j]).sum(), j
    assert (c[2] == -c[0]).all() and g[2] == -g[0]      # the third limit is the first with -d
    # the same identity in float64, at the rounding of a float64 solve
    A64 = np.asarray(A, dtype=np.float64)
    c64, g64, _ = mref.analysis(mref.Geometry(data, np.float64), A64, kw["loads"], kw["limits"])
    for j in range(len(g64)):
        assert abs((A64 * c64[j]).sum() - g64[j]) <= 1e-9 * np.abs(A64 * c64[j]).sum(), j


def test_single_limit_ends_feasible_and_lighter_than_the_envelope():
    """For every fixture the "single" run ends converged and within its limit, strictly lighter than what the
    displacement envelope of the stress-ratio sizing ends with at the same value (stress allowables out of reach): the
    envelope scales every member by the one ratio, here 2.  The ratios are those of tests/golden/minweight_tol.json."""
    value = record()["value"]
    for b, name in enumerate(mref.BATCH):
        r = full(name, "single")
        env = mref.envelope(load_json(name), "single")
        assert r["status"] == mref.CONVERGED and r["worsts"][-1] <= 1 + mref.FULL["limit_tol"], name
        assert env["status"] == 0 and abs(env["disp_ratio"] - 1.0) <= 1e-3, name
        ratio = float(r["measure"] / env["weight"])
        print(name, ratio, float(env["weight"] / env["weight_history"][0]), float(r["worsts"][-1]))
        assert ratio < 1.0 and abs(ratio - value["weight_ratio"][b]) <= 1e-6 * ratio, name
        assert abs(env["weight"] / env["weight_history"][0] - value["envelope_over_initial"][b]) <= 1e-6


def _close(new, old):
    least = mref.FLOOR_LEAST
    return all(new[k] <= 2.0 * max(old[k], least) and old[k] <= 2.0 * max(new[k], least) for k in mref.COMPARED)


def test_recorded_floors_are_the_yardsticks_own():
    """tests/golden/minweight_tol.json: the max-scaled differences between the yardstick in float64 and in longdouble on
    the inputs of the GPU tests, per truss and result, at depth 6 with tol 0 and on the full runs; for the full runs also
    what the GPU test of the counts leans on: status, iterations and whether any `change` lies within 1 % of `tol` or any
    `worst` within 1 % of 1 + limit_tol.  The small batch and the generated truss are measured again here (the figures of
    bar-942 take a while in longdouble and are only read)."""
    rec = record()
    assert rec["trusses"] == list(mref.BATCH) and rec["big_truss"] == mref.BIG and rec["decided"] == mref.DECIDED
    assert rec["floor_least"] == mref.FLOOR_LEAST and rec["fractions"] == {k: list(v) for k, v in mref.CONFIGS.items()}
    assert 257 <= rec["generated_members"] == len(mref.generated()["member"]) <= 512
    depth = {"tol": 0.0, "max_iters": mref.DEPTH}
    for part in ("depth", "generated", "big"):
        assert {k: rec[part][k] for k in depth} == depth and sorted(rec[part]["configs"]) == sorted(mref.CONFIGS)
        for entry in rec[part]["configs"].values():
            assert entry["relative_difference"] == max(max(d.values()) for d in entry["per_truss"])
            assert all(sorted(d) == sorted(mref.COMPARED) for d in entry["per_truss"])
    assert {k: rec["full"][k] for k in mref.FULL} == mref.FULL and sorted(rec["full"]["configs"]) == sorted(mref.CONFIGS)
    args = (mref.FULL["tol"], mref.FULL["limit_tol"])
    for which in sorted(mref.CONFIGS):
        for b, name in enumerate(mref.BATCH):
            new = mref.floor(load_json(name), which, depth)[0]
            print("depth", which, name, new)
            assert _close(new, rec["depth"]["configs"][which]["per_truss"][b]), (which, name)
        assert _close(mref.floor(mref.generated(), which, depth)[0], rec["generated"]["configs"][which]["per_truss"][0]), which
        entry = rec["full"]["configs"][which]
        for b, name in enumerate(mref.BATCH):
            new, f64, f80 = mref.floor(load_json(name), which, mref.FULL)
            _cache.setdefault((name, which), f64)
            assert (f64["status"], f64["iterations"]) == (f80["status"], f80["iterations"]) == \
                (entry["status"][b], entry["iterations"][b]), (which, name)
            assert entry["decided"][b] == (mref.decided(f64, *args) and mref.decided(f80, *args)), (which, name)
            assert abs(float(f64["changes"][-1]) - entry["last_change"][b]) <= 1e-6 * entry["last_change"][b]
            if f64["status"] == mref.CONVERGED:     # (a run that ends at the limit may wander: its floor is only read)
                assert _close(new, entry["per_truss"][b]), (which, name)
        assert sum(entry["decided"]) >= 4 and sorted(set(entry["status"])) in ([0], [0, 1])
        assert 0 < rec["big"]["configs"][which]["relative_difference"] < 1e-9
    assert all(rec["full"]["configs"]["single"]["decided"][b] for b in (0, 1, 2, 3, 5))


def _refused(word, packed, **kwargs):
    args = {"limit_case": [0], "limit_joint": [1], "limit_direction": [[0.0, -1.0, 0.0]], "limit_value": 0.5,
            "area_min": 0.1, "area_max": 10.0}
    args.update(kwargs)
    with pytest.raises(ValueError, match=word):
        batch._check_min_weight_args(packed, **args)


def test_check_min_weight_args():
    packed = batch.pack_json([load_json("bar-10_input_0"), load_json("bar-25_input_0")])
    B, nJ, nM = packed.B, packed.nJ_max, packed.nM_max
    ok = {"limit_case": [0], "limit_joint": [1], "limit_direction": [[0.0, -2.0]], "limit_value": 0.5}
    val = batch._check_min_weight_args(packed, area_min=0.1, area_max=np.full([B, nM], 5.0), **ok)
    assert val["loads"] is None and val["measure"] == "weight" and val["want_sensitivity"] is False
    assert (val["move"], val["tol"], val["max_iters"], val["sweeps"], val["limit_tol"], val["check_every"]) == \
        (0.2, 1e-4, 60, 2, 1e-2, 1)
    assert val["area_min"] == 0.1 and val["area_max"].shape == (B, nM)
    lim = val["limits"]
    assert lim["case"].dtype == np.int32 and list(lim["case"]) == [0] and lim["joint"].tolist() == [[1], [1]]
    assert lim["direction"].tolist() == [[[0.0, -1.0, 0.0]]] * 2 and lim["value"].tolist() == [[0.5], [0.5]]
    loads = np.zeros([B, 2, nJ, 2])
    joints = np.array([[2, -1, 0], [1, 3, -1]])
    values = np.array([[1.0, 2.0, np.inf], [np.inf, 1.0, 3.0]])
    val = batch._check_min_weight_args(packed, loads, [0, 1, 1], joints, np.ones([B, 3, 3]), values, "volume", 1.0, 1.0, 1.0,
                                       0.0, 0, 3, 0.0, 2, True)
    lim = val["limits"]
    assert val["loads"].shape == (B, 2, nJ, 3) and lim["joint"].tolist() == joints.tolist() and val["want_sensitivity"]
    assert (val["measure"], val["move"], val["tol"], val["max_iters"], val["sweeps"], val["limit_tol"]) == \
        ("volume", 1.0, 0.0, 0, 3, 0.0)
    on = (joints >= 0) & np.isfinite(values)
    assert np.allclose((lim["direction"] ** 2).sum(axis=2), on) and not lim["direction"][~on].any()
    # a zero direction is fine where the limit is switched off, and only there
    d = np.ones([B, 3, 3])
    d[0, 1] = d[1, 0] = 0.0
    assert batch._check_min_weight_args(packed, loads, [0, 1, 1], joints, d, values, area_min=1, area_max=1)
    d[0, 0] = 0.0
    _refused("limit_direction", packed, loads=loads, limit_case=[0, 1, 1], limit_joint=joints, limit_direction=d,
             limit_value=values)
    for bad in ([], [0] * 9, [1], [-1], [0.0], [True], 0, "a", None):
        _refused("limit_case", packed, limit_case=bad)
    _refused("limit_case", packed, loads=loads, limit_case=[2])
    for bad in ([1, 2], [[1]], [1.0], [-2], [nJ], [[1], [len(load_json("bar-10_input_0")["joint"])]][::-1], "x", None):
        _refused("limit_joint|must be given", packed, limit_joint=bad)
    for bad in (0.0, -1.0, float("nan"), [1.0, 2.0], [[1.0]], "1", None, [float("-inf")]):
        _refused("limit_value|must be given", packed, limit_value=bad)
    for bad in ([[0.0, 0.0, 0.0]], [[1.0]], [[1.0, 0.0, 0.0, 0.0]], [1.0, 0.0, 0.0], [[float("nan"), 1.0, 0.0]], None):
        _refused("limit_direction|must be given", packed, limit_direction=bad)
    for bad in ("mass", None, 0, b"weight"):
        _refused("measure", packed, measure=bad)
    for bad in (0.0, -0.5, 1.0000001, float("nan"), True, None, "1"):
        _refused("move", packed, move=bad)
    for name in ("tol", "limit_tol"):
        for bad in (-1e-9, float("nan"), float("inf"), True, "0", None):
            _refused(name, packed, **{name: bad})
    for bad in (-1, 2.5, True, None):
        _refused("max_iters", packed, max_iters=bad)
    for name in ("check_every", "sweeps"):
        for bad in (0, -1, 2.5, True):
            _refused(name, packed, **{name: bad})
    _refused("want_sensitivity", packed, want_sensitivity=1)
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
    light = dataclasses.replace(packed, rho=packed.rho.copy())
    light.rho[0, 2] = 0.0
    _refused("rho <= 0.*measure='volume'", light)
    assert batch._check_min_weight_args(light, measure="volume", area_min=0.1, area_max=1.0, **ok)["measure"] == "volume"
    _refused("rho <= 0", light.table())


def test_header_table_and_library_agree():
    names = declared_symbols("trs_minweight.h")
    assert names == ["trs_mw_abi_version", "trs_mw_fits", "trs_mw_step"]
    assert sorted(_capi.MW_SIGNATURES) == names
    protos = declared_prototypes("trs_minweight.h")
    assert sorted(protos) == names
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name, (is_void, n_params) in protos.items():
        restype, argtypes = _capi.MW_SIGNATURES[name]
        assert hasattr(lib, name), name
        assert len(argtypes) == n_params and not is_void and restype is ctypes.c_int, name
    assert protos["trs_mw_step"][1] == 46 and protos["trs_mw_fits"][1] == 3
    header = open(os.path.join(ROOT, "include", "trs_minweight.h")).read()
    assert "#define TRS_MW_ABI_VERSION %d\n" % _capi.MW_ABI_VERSION in header
    assert _capi.load().trs_mw_abi_version() == _capi.MW_ABI_VERSION == 1
    for word, value in (("ACTIVE", "(-1)"), ("CONVERGED", "0"), ("ITER_LIMIT", "1"), ("NOT_PD", "2"), ("INFEASIBLE", "3")):
        assert "#define TRS_MW_%s %s\n" % (word, value) in header
        assert getattr(_capi, "MW_" + word) == getattr(mref, word) == int(value.strip("()"))
    for word, value in _capi.MW_MEASURES.items():
        assert "#define TRS_MW_%s %d\n" % (word.upper(), value) in header
    assert "#define TRS_MW_BISECTIONS %d\n" % mref.BISECTIONS in header
    assert "#define TRS_MW_MAX_LIMITS %d\n" % mref.MAX_LIMITS in header and _capi.MW_MAX_LIMITS == mref.MAX_LIMITS == 8
    assert "#define TRS_MW_BRACKET_BITS 300\n" in header and "#define TRS_MW_CUT_BITS %d\n" % mref.CUT_BITS in header
    # general member form only, a version of its own, and nothing was added to the other headers' tables
    assert not any(name.endswith("_tab") for name in _capi.MW_SIGNATURES)
    assert not any(name.startswith("trs_mw") for table in (_capi.SIGNATURES, _capi.SZ_SIGNATURES, _capi.CM_SIGNATURES)
                   for name in table)
    makefile = open(os.path.join(_capi.CSRC_DIR, "Makefile")).read()
    assert " minweight.hip " in makefile and makefile.count("include/trs_minweight.h") == 2
    # the header, the kernel and the yardstick state the method in the same words
    kernel = open(os.path.join(_capi.CSRC_DIR, "minweight.hip")).read()
    squeeze = lambda text: " ".join(text.replace("*", " ").replace("//", " ").split())
    for line in ("xm = sqrt(x0 x1); if gt_j(xm) <= ubar_j then x1 = xm, else x0 = xm",
                 "c_mj = (E_m / L0_m) proj_m(v_j) proj_m(u_{l_j}) = -dg_j/dA_m",
                 "q_mj = max(c_mj, 0) A_m^2 and n_mj = max(-c_mj, 0) where |c_mj| A_m > 2^-30 max_m |c_mj| A_m, else q_mj = n_mj = 0",
                 "A'_m(mu) = clamp(sqrt(P_m / D_m), lo_m, hi_m), and lo_m where P_m <= 0",
                 "a member with w_m <= 0 keeps lo_m = hi_m = clamp(A_m, a_min_m, a_max_m)"):
        assert line in squeeze(header) and line in squeeze(mref.__doc__) and line in squeeze(kernel), line
    import python_stable_3d_truss_analysis_amd as pkg
    assert {"solve_min_weight", "MinWeightResult"} <= set(pkg.__all__)
    assert pkg.solve_min_weight is batch.solve_min_weight and pkg.MinWeightResult is batch.MinWeightResult
    assert hasattr(pkg.Truss, "MinimizeWeight") and hasattr(batch.DeviceBatch, "min_weight")
    fields = {f.name for f in dataclasses.fields(batch.MinWeightResult)}
    assert fields == set(batch.MinWeightResult.FIELDS) | {"info"}


def test_fits_rule_in_bytes():
    """The step kernel: two displacement vectors (6 nJ doubles), 64 doubles for the reductions, 6 + J doubles and two
    ints per member, the reduced row of every DOF (3 nJ ints): 60 nJ + 512 + (56 + 8 J) nM bytes, rounded up to 16,
    within the 160 KB of a CU - on shapes on both sides of the limit, for J = 1, 2 and 8; bar-942 with 8 limits fits."""
    lib = _capi.load()
    budget = 160 * 1024
    rule = lambda nJ, nM, J: (8 * (6 * nJ + 64 + (6 + J) * nM) + 4 * (2 * nM + 3 * nJ) + 15) // 16 * 16
    assert rule(244, 942, 8) == (60 * 244 + 512 + 120 * 942 + 15) // 16 * 16 == 128192 <= budget
    assert lib.trs_mw_fits(244, 942, 8) == 1
    assert lib.trs_mw_fits(-1, 4, 1) == 0 and lib.trs_mw_fits(4, -1, 1) == 0 and lib.trs_mw_fits(65536, 0, 1) == 0
    assert lib.trs_mw_fits(4, 4, 0) == 0 and lib.trs_mw_fits(4, 4, 9) == 0
    seen = set()
    for J in (1, 2, 8):
        for nJ in (0, 1, 7, 244, 1000, 2721, 2722, 4000):
            if rule(nJ, 0, J) > budget:
                assert lib.trs_mw_fits(nJ, 0, J) == 0
                continue
            top = largest(lambda nM: rule(nJ, nM, J) <= budget)
            assert rule(nJ, top, J) <= budget < rule(nJ, top + 1, J)
            for nM in range(max(top - 3, 0), top + 5):
                assert lib.trs_mw_fits(nJ, nM, J) == int(rule(nJ, nM, J) <= budget), (nJ, nM, J)
                seen.add(lib.trs_mw_fits(nJ, nM, J))
        for nM in (0, 1, 942, 1300):
            top = largest(lambda nJ: rule(nJ, nM, J) <= budget)
            for nJ in range(max(top - 3, 0), top + 5):
                assert lib.trs_mw_fits(nJ, nM, J) == int(rule(nJ, nM, J) <= budget), (nJ, nM, J)
                seen.add(lib.trs_mw_fits(nJ, nM, J))
    assert seen == {0, 1}
    # argument errors come back before any launch; an empty batch is no error
    p8 = ctypes.c_void_p(8)
    bad = lambda **kw: lib.trs_mw_step(*_step_args(p8, **kw))
    assert bad(B=0) == 0
    for kw in ({"L": 0}, {"J": 0}, {"J": 9}, {"measure": 2}, {"measure": -1}, {"move": 0.0}, {"move": 1.5}, {"tol": -1.0},
               {"tol": float("nan")}, {"limit_tol": -1.0}, {"sweeps": 0}, {"a_min_all": 0.0}, {"a_max_all": 0.01},
               {"mode": 2}, {"it": -1}, {"nJ_max": 3000, "nM_max": 3000}, {"xyz": None}, {"limit_case": None}, {"mu": None}):
        assert bad(**kw) != 0, kw


def _step_args(p, B=1, L=1, J=1, nJ_max=10, nM_max=10, xyz=0, limit_case=0, mu=0, measure=0, move=0.2, tol=0.0,
               limit_tol=0.01, sweeps=2, a_min_all=0.1, a_max_all=1.0, it=0, mode=0):
    xyz, limit_case, mu = (p if x == 0 else x for x in (xyz, limit_case, mu))
    return (B, L, J, nJ_max, nM_max, xyz, p, p, p, p, p, p, p, p, p, 64, p, limit_case, p, p, p, measure, move, tol,
            limit_tol, sweeps, None, a_min_all, None, a_max_all, it, mode, p, mu, p, p, p, p, p, p, 1, p, p, p, None, None)
