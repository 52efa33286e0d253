"""Member sizing, the parts that need no GPU: the numpy yardstick (`tests/sizing_reference.py`) against a closed form and
against the recorded float64-against-longdouble floors, the refusals of `_check_sizing_args`, the LDS rule of
`trs_sz_fits` to the byte, and the C interface of include/trs_sizing.h against its ctypes table and the library."""
import ctypes
import json
import os

import numpy as np
import pytest

from python_stable_3d_truss_analysis_amd import _capi, batch
from tests import sizing_reference as sref
from tests.helpers import GOLDEN, ROOT, load_json
from tests.test_capi_symbols import declared_prototypes, declared_symbols


def triangle(s=1000.0):
    """Pin at (0, 0), roller (y held) at (4, 0), apex (2, 3) loaded with s towards the roller: statically determinate,
    N = (2 s / sqrt 13, 0, -s) in members 0-1, 0-2, 1-2."""
    pull = np.array([2.0, -3.0]) / np.sqrt(13.0)
    return {"joint": [[[0.0, 0.0], "PIN"], [[4.0, 0.0], "ROLLER_Y"], [[2.0, 3.0], "NO"]],
            "force": [[2, list(s * pull)]],
            "member": [[[0, 1], [1.0, 1.0e7, 0.1]], [[0, 2], [1.5, 1.0e7, 0.1]], [[1, 2], [2.0, 2.0e7, 0.3]]]}


TRIANGLE = {"allow_tension": 250.0, "allow_compression": 160.0, "area_min": 0.05, "area_max": 100.0}


def triangle_areas(s=1000.0):
    return np.array([2.0 * s / np.sqrt(13.0) / TRIANGLE["allow_tension"], TRIANGLE["area_min"],
                     s / TRIANGLE["allow_compression"]])


def test_determinate_triangle_is_fully_stressed_after_one_resizing():
    """The member forces of a determinate truss do not depend on the areas: one resizing gives |N| / allowable, the
    second analysis finds nothing to move."""
    data = triangle()
    loads = sref.cases(data)[:1]
    r = sref.size(data, loads, **TRIANGLE)
    assert r["status"] == sref.CONVERGED and r["iterations"] == 1 and len(r["changes"]) == 2
    want = triangle_areas()
    assert np.abs(r["areas"] - want).max() <= 1e-12 * want.max()
    assert r["areas"][1] == TRIANGLE["area_min"]                      # the zero-force member is on its lower bound
    assert list(r["governing"]) == [0, 0, 0]
    assert np.abs(r["utilisation"][[0, 2]] - 1.0).max() <= 1e-12 and r["utilisation"][1] <= 1e-9
    p = sref.Geometry(data, np.float64)
    assert abs(r["weight"] - (want * p.L0 * p.rho).sum()) <= 1e-12 * r["weight"]
    assert r["weight_history"][1] == r["weight"] and not r["weight_history"][2:].any()


def test_yardstick_statuses_of_the_full_runs():
    """tol 1e-4, 40 iterations on the small fixtures: the (status, iterations) that a throwaway prototype of the method
    gave, and - what the GPU test of the statuses leans on - no truss of the table ends with a `change` within 1e-6
    (relative) of `tol` at its last two analyses."""
    for which in ("stress", "disp"):
        for name in sref.BATCH:
            data = load_json(name)
            r = sref.size(data, **sref.config(data, which), **sref.FULL)
            assert (r["status"], r["iterations"]) == sref.TABLE[which][name.split("_")[0]], (which, name)
            for change in r["changes"][-2:]:
                assert abs(float(change) - sref.FULL["tol"]) > 1e-6 * sref.FULL["tol"], (which, name, change)


def test_recorded_floors_are_the_yardsticks_own():
    """tests/golden/sizing_tol.json: the largest max-scaled difference between the yardstick in float64 and in longdouble
    on the inputs of the GPU tests.  The small batch is measured again here (the bar-942 figures take a minute in
    longdouble and are only read)."""
    with open(os.path.join(GOLDEN, "sizing_tol.json")) as fh:
        rec = json.load(fh)
    assert rec["trusses"] == list(sref.BATCH) and rec["big_truss"] == sref.BIG
    assert (rec["depth"]["tol"], rec["depth"]["max_iters"]) == (0.0, sref.DEPTH)
    assert (rec["full"]["tol"], rec["full"]["max_iters"]) == (sref.FULL["tol"], sref.FULL["max_iters"])
    assert sorted(rec["depth"]["configs"]) == sorted(sref.CONFIGS) and sorted(rec["full"]["configs"]) == ["disp", "stress"]
    assert sorted(rec["big"]["configs"]) == ["disp", "stress"] and rec["catalog"]["config"] == "stress"
    datas = [load_json(n) for n in sref.BATCH]
    ladder = sref.ladder(datas)
    runs = [(rec["depth"]["configs"][w], w, {"tol": 0.0, "max_iters": sref.DEPTH}) for w in sref.CONFIGS]
    runs += [(rec["full"]["configs"][w], w, dict(sref.FULL)) for w in ("stress", "disp")]
    runs += [(rec["catalog"], "stress", dict(sref.FULL, catalog=ladder))]
    for entry, which, run in runs:
        worst = 0.0
        for data in datas:
            kw = sref.config(data, which)
            f64, f80 = sref.size(data, **kw, **run), sref.size(data, dtype=np.longdouble, **kw, **run)
            assert f64["status"] == f80["status"] and f64["iterations"] == f80["iterations"]
            worst = max(worst, sref.relative_difference(f64, f80))
        print(which, run.get("max_iters"), "catalog" in run, worst, entry["relative_difference"])
        assert 0.5 * entry["relative_difference"] <= worst <= 2.0 * entry["relative_difference"], (which, run)
    for which in ("stress", "disp"):
        assert 0 < rec["big"]["configs"][which]["relative_difference"] < 1e-9


def _refused(word, packed, **kwargs):
    args = {"allow_tension": 1.0, "allow_compression": 1.0, "area_min": 0.1, "area_max": 10.0}
    args.update(kwargs)
    with pytest.raises(ValueError, match=word):
        batch._check_sizing_args(packed, **args)


def test_check_sizing_args():
    packed = batch.pack_json([load_json("bar-10_input_0"), load_json("bar-25_input_0")])
    B, nJ, nM = packed.B, packed.nJ_max, packed.nM_max
    val = batch._check_sizing_args(packed, None, 2, 3.5, area_min=0.1, area_max=np.full([B, nM], 5.0), catalog=[1, 2.5])
    assert val["allow_tension"] == 2.0 and val["allow_compression"] == 3.5 and val["loads"] is None
    assert val["area_min"] == 0.1 and val["area_max"].shape == (B, nM) and list(val["catalog"]) == [1.0, 2.5]
    assert (val["relax"], val["tol"], val["max_iters"], val["check_every"]) == (1.0, 1e-4, 40, 1)
    loads = np.zeros([B, 2, nJ, 2])
    assert batch._check_sizing_args(packed, loads, 1.0, 1.0, area_min=0.1, area_max=1.0)["loads"].shape == (B, 2, nJ, 3)
    assert batch._check_sizing_args(packed, None, 1.0, 1.0, area_min=1.0, area_max=1.0, max_iters=0, tol=0.0)["max_iters"] == 0
    per = batch._check_sizing_args(packed, None, np.array([2.0, 3.0]), 1.0, np.array([0.0, 0.5]), area_min=0.1, area_max=1.0)
    assert list(per["allow_tension"]) == [2.0, 3.0] and list(per["allow_displace"]) == [0.0, 0.5]   # one value per truss
    for name in ("allow_tension", "allow_compression"):
        for bad in (0.0, -1.0, float("nan"), float("inf"), True, "1", None, np.array([1.0, 0.0]), np.ones(B + 1), np.ones([B, 1])):
            _refused(name, packed, **{name: bad})
    for name in ("allow_displace", "euler_kappa", "tol"):
        for bad in (-1e-9, float("nan"), float("inf"), True, "0", None, np.ones(B)[:1] if name != "allow_displace" else -np.ones(B)):
            _refused(name, packed, **{name: bad})
    for bad in (0.0, -0.5, 1.0000001, float("nan"), True, None):
        _refused("relax", packed, relax=bad)
    for bad in (-1, 2.5, True, None):
        _refused("max_iters", packed, max_iters=bad)
    for bad in (0, -1, 2.5, True):
        _refused("check_every", packed, check_every=bad)
    for bad in ([], [1.0, 1.0], [2.0, 1.0], [0.0, 1.0], [-1.0], [1.0, float("nan")], [[1.0, 2.0]], list(range(1, 258)), "abc"):
        _refused("catalog", packed, catalog=bad)
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
    import dataclasses
    flat = dataclasses.replace(packed, A=packed.A.copy())
    flat.A[1, 3] = 0.0
    _refused("initial design", flat)
    # padding members are not looked at: bounds that are wrong only there pass
    ragged = np.where(np.arange(nM)[None, :] < packed.nM[:, None], 0.1, -1.0)
    assert batch._check_sizing_args(packed, area_min=ragged, area_max=1.0, allow_tension=1.0, allow_compression=1.0)


def test_header_table_and_library_agree():
    names = declared_symbols("trs_sizing.h")
    assert names == ["trs_sz_abi_version", "trs_sz_fits", "trs_sz_snap", "trs_sz_step"]
    assert sorted(_capi.SZ_SIGNATURES) == names
    protos = declared_prototypes("trs_sizing.h")
    assert sorted(protos) == names
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name, (is_void, n_params) in protos.items():
        restype, argtypes = _capi.SZ_SIGNATURES[name]
        assert hasattr(lib, name), name
        assert len(argtypes) == n_params and not is_void and restype is ctypes.c_int, name
    assert protos["trs_sz_step"][1] == 40 and protos["trs_sz_snap"][1] == 9
    header = open(os.path.join(ROOT, "include", "trs_sizing.h")).read()
    assert "#define TRS_SZ_ABI_VERSION %d\n" % _capi.SZ_ABI_VERSION in header
    assert _capi.load().trs_sz_abi_version() == _capi.SZ_ABI_VERSION == 1
    for word, value in (("ACTIVE", "(-1)"), ("CONVERGED", "0"), ("ITER_LIMIT", "1"), ("NOT_PD", "2")):
        assert "#define TRS_SZ_%s %s\n" % (word, value) in header
        assert getattr(_capi, "SZ_" + word) == getattr(sref, word) == int(value.strip("()"))
    assert "#define TRS_SZ_MAX_CATALOG %d\n" % _capi.SZ_MAX_CATALOG in header
    # general member form only, and nothing was added to trs_solver.h
    assert not any(name.endswith("_tab") for name in _capi.SZ_SIGNATURES)
    assert not any(name.startswith("trs_sz") for name in _capi.SIGNATURES)
    makefile = open(os.path.join(_capi.CSRC_DIR, "Makefile")).read()
    assert " sizing.hip " in makefile and makefile.count("include/trs_sizing.h") == 2
    import python_stable_3d_truss_analysis_amd as pkg
    assert {"solve_sizing", "SizingResult"} <= set(pkg.__all__)
    assert pkg.solve_sizing is batch.solve_sizing and pkg.SizingResult is batch.SizingResult


def largest(fits):
    lo, hi = 0, 1
    while fits(hi):
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


def test_fits_rule_in_bytes():
    """The step kernel: two displacement vectors (6 nJ doubles), eight doubles for the reductions, six doubles and three
    ints per member, the reduced row of every DOF (3 nJ ints): 60 nJ + 64 + 60 nM bytes, rounded up to 16, within the
    160 KB of a CU - on shapes on both sides of the limit."""
    lib = _capi.load()
    budget = 160 * 1024
    rule = lambda nJ, nM: (8 * (6 * nJ + 8 + 6 * nM) + 4 * (3 * nM + 3 * nJ) + 15) // 16 * 16
    assert rule(244, 942) == (60 * 244 + 64 + 60 * 942 + 15) // 16 * 16 <= budget and lib.trs_sz_fits(244, 942) == 1
    assert lib.trs_sz_fits(-1, 4) == 0 and lib.trs_sz_fits(4, -1) == 0 and lib.trs_sz_fits(65536, 0) == 0
    seen = set()
    for nJ in (0, 1, 7, 100, 244, 1000, 2000, 2729, 2730, 4000):
        if rule(nJ, 0) > budget:
            assert lib.trs_sz_fits(nJ, 0) == 0
            continue
        top = largest(lambda nM: rule(nJ, nM) <= budget)
        assert rule(nJ, top) <= budget < rule(nJ, top + 1)
        for nM in range(max(top - 3, 0), top + 5):
            assert lib.trs_sz_fits(nJ, nM) == int(rule(nJ, nM) <= budget), (nJ, nM, rule(nJ, nM))
            seen.add(lib.trs_sz_fits(nJ, nM))
    for nM in (0, 1, 5, 942, 2000, 2729):
        top = largest(lambda nJ: rule(nJ, nM) <= budget)
        assert rule(top, nM) <= budget < rule(top + 1, nM)
        for nJ in range(max(top - 3, 0), top + 5):
            assert lib.trs_sz_fits(nJ, nM) == int(rule(nJ, nM) <= budget), (nJ, nM, rule(nJ, nM))
            seen.add(lib.trs_sz_fits(nJ, nM))
    assert seen == {0, 1}
    # argument errors come back before any launch; an empty batch is no error
    p8 = ctypes.c_void_p(8)
    bad = lambda **kw: lib.trs_sz_step(*_step_args(p8, **kw))
    assert bad(B=0) == 0
    for kw in ({"L": 0}, {"allow_tension": 0.0}, {"allow_compression": -1.0}, {"allow_displace": -1.0}, {"relax": 0.0},
               {"relax": 1.5}, {"tol": -1.0}, {"a_min_all": 0.0}, {"a_max_all": 0.01}, {"mode": 3}, {"it": -1},
               {"euler_kappa": float("nan")}, {"nJ_max": 3000, "nM_max": 3000}, {"xyz": None}):
        assert bad(**kw) != 0, kw
    assert lib.trs_sz_snap(1, 10, None, None, None, 0, None, None, None) != 0
    assert lib.trs_sz_snap(1, 10, p8, p8, p8, 257, p8, p8, None) != 0
    assert lib.trs_sz_snap(0, 10, None, None, None, 4, None, None, None) == 0


def _step_args(p, B=1, L=1, nJ_max=10, nM_max=10, xyz=0, allow_tension=1.0, allow_compression=1.0, allow_displace=0.0,
               euler_kappa=0.0, relax=1.0, tol=0.0, a_min_all=0.1, a_max_all=1.0, it=0, mode=0):
    xyz = p if xyz == 0 else xyz
    return (B, L, nJ_max, nM_max, xyz, p, p, p, p, p, p, p, p, p, 64, p, allow_tension, allow_compression, allow_displace,
            None, euler_kappa, relax, tol, None, a_min_all, None, a_max_all, it, mode, p, p, p, p, p, p, p, p, p, 1, None)
