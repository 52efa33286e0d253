"""Collapse load, the parts that need no GPU: the numpy yardstick (`tests/plastic_reference.py`) against two closed forms,
the admissibility of every parity run of the GPU tests and the recorded float64-against-longdouble floors, the refusals of
`_check_plastic_args` and `Truss.CollapseLoad`, the LDS rule of `trs_pl_fits` to the byte, and the C interface of
include/trs_plastic.h against its ctypes table and the library."""
import ctypes
import json
import os

import numpy as np
import pytest

from python_stable_3d_truss_analysis_amd import _capi, batch
from tests import plastic_reference as pref
from tests.helpers import GOLDEN, ROOT, load_json
from tests.test_capi_symbols import declared_prototypes, declared_symbols
from tests.test_sizing import largest

C = 100.0
ROOT2 = np.sqrt(2.0)


def test_three_bars_closed_form():
    """Three bars to one joint at -45, 0 and +45 degrees, equal A and E, capacity C: the middle bar carries
    P / (1 + 1 / sqrt 2) and yields first, at lambda P = (1 + 1 / sqrt 2) C; then the side bars carry the rest and both
    yield in ONE event (tie_tol) at (1 + sqrt 2) C; the third analysis is of a structure without stiffness."""
    data, caps = pref.three_bars(C)
    for dtype in (np.float64, np.longdouble):
        r = pref.collapse(data, pref.cases(data)[0], caps, caps, lambda_max=1e6, dtype=dtype)
        assert (r["status"], r["events"], r["info"]) == (pref.MECHANISM, 2, 1)
        assert list(r["member_history"][:4]) == [1, 0, -2, 0] and list(r["count_history"][:4]) == [1, 2, 0, 0]
        want = np.array([(1 + 1 / ROOT2) * C, (1 + ROOT2) * C, (1 + ROOT2) * C])
        assert np.abs(r["lambda_history"][:3] - want).max() <= 1e-12 * C and abs(r["lam"] - want[2]) <= 1e-12 * C
        assert list(r["state"]) == [1, 1, 1] and (r["N"] == C).all() and not r["areas_effective"].any()
        assert np.abs(r["residual"][3] - np.array([0.0, -float(r["lam"])])).max() <= 1e-12 * C      # (P is 1 downwards)
        assert r["umax_history"][0] < r["umax_history"][1] == r["umax_history"][2]
    # (no stiffness left at all: the failed pivot is an exact zero, a decision every factorisation shares)
    assert r["trace"][-1]["pivot_ratio"] == 0 and pref.info_clear(r, r)
    # exactly tied side bars need no tolerance; a capacity in compression of its own
    r = pref.collapse(data, -pref.cases(data)[0], caps, 0.5 * caps, lambda_max=1e6, tie_tol=0.0)
    assert list(r["count_history"][:2]) == [1, 2] and list(r["state"]) == [-1, -1, -1] and (r["N"] == -0.5 * C).all()
    assert abs(r["lam"] - 0.5 * (1 + ROOT2) * C) <= 1e-12 * C
    # the caps: lambda_max below the first yield, the displacement limit between the events, the event limit
    r = pref.collapse(data, pref.cases(data)[0], caps, caps, lambda_max=100.0)
    assert (r["status"], r["events"], float(r["lam"])) == (pref.LAMBDA_MAX, 0, 100.0) and not r["state"].any()
    first = pref.collapse(data, pref.cases(data)[0], caps, caps, lambda_max=1e6, max_events=1)
    assert (first["status"], first["events"]) == (pref.EVENT_LIMIT, 1) and list(first["state"]) == [0, 1, 0]
    limit = 1.5 * float(first["umax_history"][0])
    r = pref.collapse(data, pref.cases(data)[0], caps, caps, lambda_max=1e6, disp_limit=limit)
    assert (r["status"], r["events"]) == (pref.DISP_LIMIT, 1) and abs(np.abs(r["u"]).max() - limit) <= 1e-12 * limit
    # hardening: the yielded bars keep a hundredth of their stiffness, nothing collapses
    r = pref.collapse(data, pref.cases(data)[0], caps, caps, hardening=0.01, lambda_max=300.0)
    assert (r["status"], r["events"], float(r["lam"])) == (pref.LAMBDA_MAX, 2, 300.0) and (r["N"] > C).all()


def test_a_determinate_truss_ends_at_its_first_yield():
    data, caps = pref.two_bars(C)
    geo = pref.Geometry(data, np.float64)
    el = pref.Eliminated(geo.stiffness(geo.A0))
    u = np.zeros(6)
    u[geo.mask] = el.solve(pref.cases(data)[0].reshape(-1)[geo.mask])
    linear = geo.forces(geo.A0, u.reshape(1, 3, 2))[0]
    r = pref.collapse(data, pref.cases(data)[0], caps, caps, lambda_max=1e6)
    assert (r["status"], r["events"], r["info"]) == (pref.MECHANISM, 1, 1)
    assert abs(r["lam"] - (C / np.abs(linear)).min()) <= 1e-12 * C and list(r["member_history"][:2]) == [0, -2]


def _runs():
    for name in pref.RUNS:
        if name == "big":
            continue
        for b, (data, load, kw) in enumerate(pref.run_inputs(name)):
            yield name, b, data, load, kw


def test_parity_runs_are_admissible_and_cover_the_method():
    """Every run of the GPU parity tests: float64 and longdouble take the same path and every decision - positive
    definiteness, the softening test, the release test, the gap behind the tie group, cap against yield - has a margin
    of at least 1000 x what float64 itself loses on it.  The results are those of pref.TABLE.  Every fixture is there
    perfectly plastic and with hardening; releases, the softening rule and a failed factorisation all occur."""
    np.seterr(all="ignore")
    with open(os.path.join(GOLDEN, "plastic_tol.json")) as fh:
        rec = json.load(fh)
    assert rec["trusses"] == list(pref.BATCH) and rec["big_truss"] == pref.BIG and rec["max_events"] == pref.MAX_EVENTS
    assert rec["admissible"] == pref.ADMISSIBLE == 1000.0
    assert sorted(rec["runs"]) == sorted(n for n in pref.RUNS if n != "big")
    worst, seen = {}, {"release": 0, "soft": 0, "info": 0}
    for name, b, data, load, kw in _runs():
        f64 = pref.collapse(data, load, **kw)
        f80 = pref.collapse(data, load, dtype=np.longdouble, **kw)
        what = (name, pref.RUNS[name][1][b])
        ok, tightest = pref.admissible(f64, f80)
        print(what, "status", f64["status"], "events", f64["events"], "lambda %.6g" % f64["lam"], "tightest", tightest)
        assert pref.same_path(f64, f80), what
        assert ok, (what, tightest)
        status, events, first = pref.TABLE[name][b]
        assert (f64["status"], f64["events"]) == (status, events) and tuple(f64["member_history"][:4]) == first, what
        worst[name] = max(worst.get(name, 0.0), pref.relative_difference(f64, f80))
        # the end state is in equilibrium with lambda P, and no member yielded at h = 0 is off its capacity
        free = pref.Geometry(data, np.float64).mask.reshape(load.shape)
        unbalanced = np.abs((f64["residual"] - f64["lam"] * load)[free]).max()
        assert unbalanced <= 1e-9 * np.abs(f64["N"]).max(), (what, unbalanced)
        if kw["hardening"] == 0.0:
            caps = np.where(f64["state"] > 0, kw["cap_tension"], -kw["cap_compression"])
            assert np.array_equal(f64["N"][f64["state"] != 0], caps[f64["state"] != 0]), what
        assert rec["runs"][name]["per_truss"][b]["info_clear"] == pref.info_clear(f64, f80), what
        # (every collapse here is a true mechanism: its failed pivot is rounding noise, never a clear decision)
        assert pref.info_clear(f64, f80) == (f64["status"] != pref.MECHANISM), what
        seen["release"] += int((f64["member_history"][:events] == -1).sum())
        seen["soft"] += f64["soft"]
        seen["info"] += f64["info"]
    assert min(seen.values()) >= 1, seen
    for name, rel in worst.items():
        entry = rec["runs"][name]
        assert entry["hardening"] == pref.RUNS[name][0]
        assert [tuple(c) for c in entry["configs"]] == list(pref.RUNS[name][1])
        assert 0.5 * entry["relative_difference"] <= rel <= 2.0 * entry["relative_difference"], (name, rel)
    for name in ("plastic", "hardening"):
        assert [c[0] for c in pref.RUNS[name][1]] == list(pref.BATCH)
    assert pref.RUNS["plastic"][0] == 0.0 and pref.RUNS["hardening"][0] == 1e-3
    # bar-942 takes twenty seconds in longdouble: its record is only read
    big = rec["big"]
    assert [tuple(c) for c in big["configs"]] == list(pref.RUNS["big"][1]) and big["hardening"] == pref.RUNS["big"][0]
    assert 0 < big["relative_difference"] < 1e-9
    one = big["per_truss"][0]
    assert one["admissible"] and one["tightest"][2] >= pref.ADMISSIBLE * one["tightest"][3]
    assert (one["status"], one["events"]) == pref.TABLE["big"][0][:2] == (pref.LAMBDA_MAX, 8)


def _refused(word, packed, *args, **kwargs):
    with pytest.raises(ValueError, match=word):
        batch._check_plastic_args(packed, *args, **kwargs)


def test_check_plastic_args():
    packed = batch.pack_json([load_json("bar-10_input_0"), load_json("bar-25_input_0")])
    B, nJ, nM = packed.B, packed.nJ_max, packed.nM_max
    cap = np.full([B, nM], 5.0)
    val = batch._check_plastic_args(packed, cap, 2.0 * cap)
    assert val["cap_tension"].shape == (B, nM) and val["cap_compression"][0, 0] == 10.0 and val["L"] == 1
    assert val["loads"] is None
    assert (val["hardening"], val["lambda_max"], val["disp_limit"], val["collapse_ratio"], val["tie_tol"],
            val["max_events"], val["check_every"]) == (0.0, 1.0, 0.0, 1e8, 1e-9, 64, 1)
    val = batch._check_plastic_args(packed, cap, cap, np.zeros([B, 2, nJ, 2]), hardening=1e-3, max_events=0)
    assert val["loads"].shape == (B, 2, nJ, 3) and val["L"] == 2 and val["max_events"] == 0
    # the padding members are not looked at
    ragged = np.where(np.arange(nM)[None, :] < packed.nM[:, None], cap, -7.0)
    assert (batch._check_plastic_args(packed, ragged, cap)["cap_tension"][0, packed.nM[0]:] == 1.0).all()
    for name in ("cap_tension", "cap_compression"):
        for bad in (None, np.zeros([B, nM + 1]), np.zeros([B]), np.zeros([B, nM]), np.full([B, nM], -1.0),
                    np.full([B, nM], float("nan")), np.full([B, nM], float("inf")), "abc"):
            args = (bad, cap) if name == "cap_tension" else (cap, bad)
            _refused(name, packed, *args)
    for name, bads in (("hardening", (-1e-9, float("nan"), float("inf"), True, "0", None)),
                       ("lambda_max", (0.0, -1.0, float("nan"), float("inf"), True, None)),
                       ("disp_limit", (-1.0, float("nan"), float("inf"), True)),
                       ("collapse_ratio", (1.0, 0.5, float("nan"), float("inf"), True)),
                       ("tie_tol", (-1e-12, float("nan"), float("inf"), True)),
                       ("max_events", (-1, 2.5, True, None)), ("check_every", (0, -1, 2.5, True))):
        for bad in bads:
            _refused(name, packed, cap, cap, **{name: bad})
    for bad in (np.zeros([B, 2, nJ]), np.zeros([B + 1, 1, nJ, 3]), np.zeros([B, 0, nJ, 3]), np.zeros([B, 1, nJ, 4]),
                np.full([B, 1, nJ, 3], float("nan"))):
        _refused("loads", packed, cap, cap, loads=bad)
    _refused("compact", packed, cap, cap, options={"compact": True})
    _refused("sections", packed, cap, cap, sections=[(1.0, 1.0, 1.0)])
    _refused("max_result_bytes", packed, cap, cap, max_result_bytes=100)


def test_truss_collapse_load_refusals():
    """What `Truss.CollapseLoad` refuses before any device work."""
    from python_stable_3d_truss_analysis_amd import Truss
    data, _ = pref.three_bars(C)
    truss = Truss(2).LoadFromJSON(data=data)
    with pytest.raises(ValueError, match="one number or one per member"):
        truss.CollapseLoad([1.0, 2.0])
    with pytest.raises(ValueError, match="'tension' and 'compression'"):
        truss.CollapseLoad({"tension": 1.0})
    with pytest.raises(ValueError, match="one number or one per member"):
        truss.CollapseLoad(True)
    with pytest.raises(ValueError, match="cap_tension must be positive"):
        truss.CollapseLoad(0.0)
    with pytest.raises(ValueError, match="cap_compression must be positive"):
        truss.CollapseLoad({"tension": 1.0, "compression": [1.0, -1.0, 1.0]})
    with pytest.raises(ValueError, match="hardening"):
        truss.CollapseLoad(C, hardening=-1.0)
    with pytest.raises(ValueError, match="lambda_max"):
        truss.CollapseLoad(C, lambdaMax=0.0)
    assert truss.CollapseLoad(C, []) == []


def test_header_table_and_library_agree():
    names = declared_symbols("trs_plastic.h")
    assert names == ["trs_pl_abi_version", "trs_pl_finish", "trs_pl_fits", "trs_pl_step"]
    assert sorted(_capi.PL_SIGNATURES) == names
    protos = declared_prototypes("trs_plastic.h")
    assert sorted(protos) == names
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name, (is_void, n_params) in protos.items():
        restype, argtypes = _capi.PL_SIGNATURES[name]
        assert hasattr(lib, name), name
        assert len(argtypes) == n_params and not is_void and restype is ctypes.c_int, name
    assert protos["trs_pl_step"][1] == 36 and protos["trs_pl_finish"][1] == 18
    header = open(os.path.join(ROOT, "include", "trs_plastic.h")).read()
    assert "#define TRS_PL_ABI_VERSION %d\n" % _capi.PL_ABI_VERSION in header
    assert _capi.load().trs_pl_abi_version() == _capi.PL_ABI_VERSION == 1
    for word, value in (("ACTIVE", "(-1)"), ("LAMBDA_MAX", "0"), ("EVENT_LIMIT", "1"), ("MECHANISM", "2"),
                        ("DISP_LIMIT", "3")):
        assert "#define TRS_PL_%s %s\n" % (word, value) in header
        assert getattr(_capi, "PL_" + word) == getattr(pref, word) == int(value.strip("()"))
    assert "trs_plastic.h" in _capi.__doc__
    # general member form only, and nothing was added to the other headers' tables
    assert not any(name.endswith("_tab") for name in _capi.PL_SIGNATURES)
    assert not any(name.startswith("trs_pl") for table in (_capi.SIGNATURES, _capi.SZ_SIGNATURES, _capi.UN_SIGNATURES)
                   for name in table)
    makefile = open(os.path.join(_capi.CSRC_DIR, "Makefile")).read()
    assert " plastic.hip " in makefile and makefile.count("include/trs_plastic.h") == 2
    import python_stable_3d_truss_analysis_amd as pkg
    assert {"solve_plastic", "PlasticResult"} <= set(pkg.__all__)
    assert pkg.solve_plastic is batch.solve_plastic and pkg.PlasticResult is batch.PlasticResult
    assert set(batch.PlasticResult.FIELDS) == set(batch.PlasticResult.CASE_FIELDS)
    assert all(shape[0] == "L" for *_, shape in batch.PlasticResult.FIELDS.values())


def _method_lines(text, strip):
    """The numbered steps 1. to 8. of the method as one string of words, the comment marks and line breaks taken out."""
    lines, going = [], False
    for line in text.splitlines():
        line = line.strip()
        for mark in strip:
            if line.startswith(mark):
                line = line[len(mark):].strip()
        if line.startswith("1. A_eff"):
            going = True
        if going and line.startswith("8. the history"):
            break
        if going:
            lines.append(line)
    return " ".join(" ".join(lines).split())


def test_the_method_is_stated_in_the_same_words():
    """Steps 1 to 7 of the method, word for word in the header and in the yardstick; the kernel file's are the same
    steps, shortened only by the remarks in brackets."""
    header = _method_lines(open(os.path.join(ROOT, "include", "trs_plastic.h")).read(), ("*",))
    yardstick = _method_lines(pref.__doc__, ())
    assert header and header == yardstick
    kernel = _method_lines(open(os.path.join(_capi.CSRC_DIR, "plastic.hip")).read(), ("//",))
    for phrase in ("A_eff,m = A_m where s_m = 0, else h A_m", "info != 0: status 2 (mechanism)",
                   "if NOT (r_k <= collapse_ratio r_0)", "a yielded member with s_m de_m < 0 unloads",
                   "dl_m <= dl_y (1 + tie_tol) yields with s_m = sign(dN_m)", "the lowest index that attains it",
                   "at k = max_events: status 1 without advancing"):
        assert phrase in header and phrase in kernel, phrase


def test_fits_rule_in_bytes():
    """The step kernel: one displacement vector (3 nJ doubles), two doubles per member, sixteen doubles and twelve ints:
    24 nJ + 16 nM + 176 bytes, rounded up to 16, within the 160 KB of a CU - on shapes on both sides of the limit.  The
    report's lists (8 nJ + 8 nM + 4 bytes) are always less."""
    lib = _capi.load()
    budget = 160 * 1024
    rule = lambda nJ, nM: (8 * 3 * nJ + 16 * nM + 176 + 15) // 16 * 16
    assert rule(244, 942) <= budget and lib.trs_pl_fits(244, 942) == 1
    assert lib.trs_pl_fits(-1, 4) == 0 and lib.trs_pl_fits(4, -1) == 0 and lib.trs_pl_fits(65536, 0) == 0
    seen = set()
    for nJ in (0, 1, 7, 100, 244, 1000, 4000, 6819, 6820, 7000):
        if rule(nJ, 0) > budget:
            assert lib.trs_pl_fits(nJ, 0) == 0
            continue
        top = largest(lambda nM: rule(nJ, nM) <= budget)
        assert rule(nJ, top) <= budget < rule(nJ, top + 1)
        for nM in range(max(top - 20, 0), top + 20):
            assert lib.trs_pl_fits(nJ, nM) == int(rule(nJ, nM) <= budget), (nJ, nM, rule(nJ, nM))
            seen.add(lib.trs_pl_fits(nJ, nM))
    for nM in (0, 1, 5, 942, 5000, 10229):
        top = largest(lambda nJ: rule(nJ, nM) <= budget)
        assert rule(top, nM) <= budget < rule(top + 1, nM)
        for nJ in range(max(top - 3, 0), top + 5):
            assert lib.trs_pl_fits(nJ, nM) == int(rule(nJ, nM) <= budget), (nJ, nM, rule(nJ, nM))
            seen.add(lib.trs_pl_fits(nJ, nM))
    assert seen == {0, 1}
    # argument errors come back before any launch; an empty batch is no error
    p8 = ctypes.c_void_p(8)
    bad = lambda **kw: lib.trs_pl_step(*_step_args(p8, **kw))
    assert bad(B=0) == 0
    for kw in ({"nJ_max": 0}, {"hardening": -1.0}, {"hardening": float("nan")}, {"lambda_max": 0.0},
               {"lambda_max": float("inf")}, {"disp_limit": -1.0}, {"collapse_ratio": 1.0}, {"tie_tol": -1.0},
               {"tie_tol": float("nan")}, {"mode": 2}, {"mode": -1}, {"it": -1}, {"H": -1},
               {"nJ_max": 7000, "nM_max": 10}, {"xyz": None}, {"cap": None}):
        assert bad(**kw) != 0, kw
    assert lib.trs_pl_finish(0, 10, 10, *([p8] * 6), 64, *([p8] * 7), None) == 0
    assert lib.trs_pl_finish(1, 0, 10, *([p8] * 6), 64, *([p8] * 7), None) != 0
    assert lib.trs_pl_finish(1, 10, 10, None, *([p8] * 5), 64, *([p8] * 7), None) != 0


def _step_args(p, B=1, nJ_max=10, nM_max=10, xyz=0, cap=0, hardening=0.0, lambda_max=1.0, disp_limit=0.0,
               collapse_ratio=1e8, tie_tol=1e-9, it=0, mode=0, H=1):
    xyz = p if xyz == 0 else xyz
    cap = p if cap == 0 else cap
    return (B, nJ_max, nM_max, xyz, p, p, p, p, p, p, p, p, 64, p, cap, p, p, hardening, lambda_max, disp_limit,
            collapse_ratio, tie_tol, it, mode, p, p, p, p, p, p, p, p, p, p, H, None)
