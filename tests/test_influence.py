"""Influence lines and moving-load envelopes, the part that needs no device: the numpy yardstick of the GPU tests
(`tests/influence_reference.py`) against itself and against the statics textbook, the header `include/trs_influence.h`
against its ctypes table and the library's exports, `trs_influence_fits` against its documented rule, and the argument
errors of `solve_influence`."""
import ctypes
import os

import numpy as np
import pytest

from python_stable_3d_truss_analysis_amd import _capi
from tests import helpers as H
from tests import influence_reference as I
from tests.test_capi_symbols import declared_prototypes, declared_symbols

PANEL, HEIGHT = 4.0, 3.0


def warren_truss():
    """A 6-panel 2D Warren truss: bottom chord joints 0 .. 6 at (4 i, 0), top chord joints 7 .. 12 at (4 i + 2, 3); pin at
    joint 0, roller at joint 6.  13 joints, 23 members (statically determinate): bottom chord i = (i, i + 1), members
    0 .. 5; top chord 6 .. 10; rising diagonals (i, 7 + i), members 11 .. 16; falling diagonals (7 + i, i + 1), 17 .. 22."""
    section = [2.5e-3, 2.0e11, 7.8e3]
    joints = [[[PANEL * i, 0.0], "PIN" if i == 0 else "ROLLER_Y" if i == 6 else "NO"] for i in range(7)]
    joints += [[[PANEL * i + PANEL / 2, HEIGHT], "NO"] for i in range(6)]
    members = [[[i, i + 1], section] for i in range(6)] + [[[7 + i, 8 + i], section] for i in range(5)]
    members += [[[i, 7 + i], section] for i in range(6)] + [[[7 + i, i + 1], section] for i in range(6)]
    return {"joint": joints, "force": [[3, [0.0, -1.0]]], "member": members}


WARREN_PATH = list(range(7))          # the bottom chord
DOWN = (0.0, -1.0)

#: name -> (data, path, d, train); the cases of the GPU parity tests
def cases():
    return {
        "warren": (warren_truss(), WARREN_PATH, DOWN, [(1.0, 0.0), (1.0, 1.5), (0.5, 6.0)]),
        "bar-47": (H.load_json("bar-47_input_0"), [16, 17, 18, 19, 20, 21], DOWN, [(2.0, 0.0), (1.0, 45.0)]),
        # 3D, free joints only (the line jumps at both ends; joint 2 recurs), offsets EQUAL to the segment length 75
        "bar-25": (H.load_json("bar-25_input_0"), [2, 3, 4, 5, 2], (0.0, 0.0, -1.0), [(1.0, 0.0), (2.0, 75.0), (1.5, 150.0)]),
    }


@pytest.mark.parametrize("name", ["warren", "bar-47", "bar-25"])
def test_the_two_routes_of_the_yardstick_agree(name):
    data, path, d, train = cases()[name]
    ref = I.by_definition(data, path, d, train)
    print(f"{name}: d_routes = {ref['d_routes']:.3e}")
    assert ref["d_routes"] <= 1e-12
    assert ref["values"].shape == (len(path) * len(train), len(data["member"]))
    # the envelope brackets the response anywhere (where the line has no jump at an end of the path: there the response
    # of a train with an axle just off the path is no candidate), and is attained at the positions it names
    continuous = not ref["eta"][:, [0, -1]].any()
    assert continuous == (name == "warren")
    for x in np.linspace(-1.0, ref["s"][-1] + train[-1][1] + 1.0, 41 if continuous else 0):
        N = I.response(ref["s"], ref["eta"], train, x)
        tol = 1e-12 * np.abs(ref["values"]).max()
        assert (N <= ref["N_max"] + tol).all() and (N >= ref["N_min"] - tol).all()
    for key, at in (("N_max", "x_max"), ("N_min", "x_min")):
        got = np.array([I.response(ref["s"], ref["eta"], train, x)[m] for m, x in enumerate(ref[at])])
        assert H.max_scaled_err(got, ref[key]) <= 1e-12


def test_warren_ordinates_are_the_textbook_values():
    """Method of sections on a simply supported span L = 6 a, unit load down at the bottom joint j (x = j a): the bottom
    chord of panel i carries M / h, M the beam moment under the top joint above it (x = (i + 1/2) a); the rising diagonal
    of panel i carries -V / sin(theta), V the shear just right of joint i."""
    ref = I.by_definition(warren_truss(), WARREN_PATH, DOWN)
    span = 6 * PANEL
    sin = HEIGHT / np.hypot(PANEL / 2, HEIGHT)
    for i in (0, 2, 5):
        for j in range(7):
            x, xc = PANEL * j, PANEL * (i + 0.5)
            moment = (1 - x / span) * xc if xc <= x else (x / span) * (span - xc)
            assert abs(ref["eta"][i, j] - moment / HEIGHT) <= 1e-12, (i, j)
            shear = (1 - x / span) - (1.0 if j <= i else 0.0)
            assert abs(ref["eta"][11 + i, j] - (-shear / sin)) <= 1e-12, (i, j)
    # the ordinates vanish over the supports, and one unit axle's envelope is the extreme ordinate
    assert not ref["eta"][:, [0, 6]].any()
    np.testing.assert_array_equal(ref["N_max"], ref["eta"].max(axis=1))
    np.testing.assert_array_equal(ref["N_min"], ref["eta"].min(axis=1))
    assert ref["x_max"][2] == 3 * PANEL or ref["x_max"][2] == 2 * PANEL      # bottom chord of panel 2: under joint 2 or 3


def test_the_areas_of_a_diagonal_sum_to_the_signed_integral():
    ref = I.by_definition(warren_truss(), WARREN_PATH, DOWN)
    for m in (12, 13, 19):                    # diagonals of inner panels: their lines change sign
        eta = ref["eta"][m]
        assert eta.max() > 0 > eta.min() and ref["area_pos"][m] > 0 > ref["area_neg"][m]
        signed = float((0.5 * np.diff(ref["s"]) * (eta[1:] + eta[:-1])).sum())
        assert abs(ref["area_pos"][m] + ref["area_neg"][m] - signed) <= 1e-12 * np.abs(eta).max() * ref["s"][-1]
    # a bottom chord is in tension wherever the load stands
    assert ref["area_neg"][2] == 0 and ref["area_pos"][2] > 0


def test_solve_influence_argument_errors_need_no_gpu(monkeypatch):
    import python_stable_3d_truss_analysis_amd as pkg
    from python_stable_3d_truss_analysis_amd import batch
    assert {"solve_influence", "InfluenceResult"} <= set(pkg.__all__)
    assert pkg.solve_influence is batch.solve_influence and pkg.InfluenceResult is batch.InfluenceResult
    assert hasattr(pkg.Truss, "InfluenceLines") and hasattr(batch.DeviceBatch, "influence")

    def no_device(*_a, **_k):
        raise AssertionError("a device was asked for before the arguments were checked")
    monkeypatch.setattr(batch, "_require_gpu", no_device)
    same_place = warren_truss()
    same_place["joint"][8][0] = list(same_place["joint"][7][0])
    packed, twins = batch.pack_json([warren_truss()]), batch.pack_json([same_place])
    ok = dict(path=[WARREN_PATH], direction=DOWN, train=[(1.0, 0.0), (2.0, 3.0)])
    bad = [dict(path=[[0, 1, 13]]), dict(path=[[0, -1, 2]]), dict(path=np.array([[0, -1, 2]])),     # out of range
           dict(path=[[0, 1], [1, 2]]),                                                             # one list per truss
           dict(path=[[3, 3]]),                                                                     # the same joint twice
           dict(direction=(0.0, np.nan)), dict(direction=(0.0, np.inf, 0.0)), dict(direction=(1.0,)),
           dict(train=[]), dict(train=[(1.0, 1.0)]), dict(train=[(1.0, 0.0), (1.0, 2.0), (1.0, 1.0)]),
           dict(train=[(np.inf, 0.0)]), dict(train=[(1.0, 0.0), (1.0, np.nan)]),
           dict(sections=[(1.0, 1.0, 1.0)]), dict(chunk=0),
           dict(want_lines=True, max_result_bytes=100),
           dict(path=[[0, 1] * 10000])]                                                             # trs_influence_fits
    for kw in bad:
        with pytest.raises(ValueError):
            batch.solve_influence(packed, **dict(ok, **kw))
    with pytest.raises(ValueError, match="same position"):
        batch.solve_influence(twins, **dict(ok, path=[[0, 7, 8, 1]]))
    with pytest.raises(AssertionError, match="a device was asked for"):       # the good arguments pass every check
        batch.solve_influence(packed, **ok)


def influence_lds_rule(nJ_max, P_max, A):
    """The LDS rule as include/trs_influence.h states it, in bytes (rounded up to 16)."""
    return (8 * (8 * P_max + 2 * A) + 4 * (4 * P_max + nJ_max) + 15) // 16 * 16


def test_header_table_exports_and_the_fits_rule_agree():
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    names = declared_symbols("trs_influence.h")
    protos = declared_prototypes("trs_influence.h")
    assert sorted(protos) == names == sorted(_capi.INFLUENCE_SIGNATURES)
    assert names == ["trs_influence_abi_version", "trs_influence_apply", "trs_influence_fits", "trs_influence_tab_apply"]
    for name in names:
        assert hasattr(lib, name), f"{name} declared in trs_influence.h but not exported"
        restype, argtypes = _capi.INFLUENCE_SIGNATURES[name]
        is_void, n_params = protos[name]
        assert len(argtypes) == n_params and not is_void and restype is ctypes.c_int, name
    assert _capi.INFLUENCE_SIGNATURES["trs_influence_tab_apply"][1] == _capi.INFLUENCE_SIGNATURES["trs_influence_apply"][1]
    others = set(_capi.SIGNATURES) | set(_capi.MODES_SIGNATURES) | set(_capi.EFFECTS_SIGNATURES) | set(_capi.LOSS_SIGNATURES)
    assert not set(_capi.INFLUENCE_SIGNATURES) & others
    header = open(os.path.join(H.ROOT, "include", "trs_influence.h")).read()
    assert "#define TRS_INFLUENCE_ABI_VERSION 1\n" in header
    loaded = _capi.load()
    assert loaded.trs_influence_abi_version() == _capi.INFLUENCE_ABI_VERSION == 1
    makefile = open(os.path.join(_capi.CSRC_DIR, "Makefile")).read()
    assert " influence.hip " in makefile and "../../include/trs_influence.h" in makefile
    # trs_influence_fits is its documented rule, on both sides of the limit
    shapes = [(244, 32, 3), (13, 7, 1), (0, 0, 1), (244, 2000, 3), (244, 2100, 3), (40000, 10, 2), (41000, 10, 2),
              (10, 10, 9000), (10, 10, 11000), (-1, 5, 1), (5, -1, 1), (5, 5, 0)]
    for nJ_max, P_max, A in shapes:
        want = nJ_max >= 0 and P_max >= 0 and A >= 1 and influence_lds_rule(nJ_max, P_max, A) <= 160 * 1024
        assert loaded.trs_influence_fits(nJ_max, P_max, A) == int(want), (nJ_max, P_max, A)
    assert {bool(loaded.trs_influence_fits(*s)) for s in shapes if min(s) >= 0 and s[2] >= 1} == {True, False}
    # refused before any launch; an empty call is no error
    nothing = [None] * 13
    assert loaded.trs_influence_apply(1, 0, 16, 10, 20, 100000, 1, *nothing, 64, *[None] * 9) != 0
    assert loaded.trs_influence_apply(1, 0, 16, 10, 20, 8, 0, *nothing, 64, *[None] * 9) != 0          # no axle
    assert loaded.trs_influence_tab_apply(1, 0, 16, 10, 20, 8, 1, *nothing, 64, *[None] * 9) != 0      # no member table
    assert loaded.trs_influence_apply(0, 0, 16, 10, 20, 8, 1, *nothing, 64, *[None] * 9) == 0


def sweep_as_the_header_states_it(s, eta, train):
    """The envelope and the areas of ONE member by the steps include/trs_influence.h spells out (and csrc/influence.hip
    takes): the segment by bisection on the s_p, the lever rule as one fused multiply-add, the axle sum ascending from 0,
    the first of equal candidates, the areas segment by segment.  Plain Python floats; fma written as a * b + c."""
    P, A = len(s), len(train)
    S = s[-1]
    eps = 1e-12 * S

    def line_at(t):
        if t < -eps or t > S + eps:
            return 0.0
        if P == 1:
            return eta[0]
        t = min(max(t, 0.0), S)
        lo, hi = 0, P - 1
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            lo, hi = (mid, hi) if s[mid] <= t else (lo, mid)
        if t == s[lo + 1]:
            return eta[lo + 1]
        return (t - s[lo]) / (s[lo + 1] - s[lo]) * (eta[lo + 1] - eta[lo]) + eta[lo]

    best = {}
    for cand in range(P * A):
        p, a = divmod(cand, A)
        n = 0.0
        for a2, (w, o) in enumerate(train):
            n = w * (eta[p] if a2 == a else line_at(s[p] + (train[a][1] - o))) + n
        for key, better in (("max", lambda x, y: x > y), ("min", lambda x, y: x < y)):
            if key not in best or better(n, best[key][0]):
                best[key] = (n, s[p] + train[a][1])
    pos = neg = 0.0
    for p in range(P - 1):
        h, u, v = s[p + 1] - s[p], eta[p], eta[p + 1]
        if u >= 0 and v >= 0:
            pos += 0.5 * h * (u + v)
        elif u <= 0 and v <= 0:
            neg += 0.5 * h * (u + v)
        else:
            cut = h * (u / (u - v))
            au, av = 0.5 * u * cut, 0.5 * v * (h - cut)
            pos, neg = pos + (au if u > 0 else av), neg + (av if u > 0 else au)
    return best["max"], best["min"], pos, neg


@pytest.mark.parametrize("name", ["warren", "bar-47", "bar-25"])
def test_the_headers_steps_give_the_definitions_numbers(name):
    """What the kernel is written to do, on the host: within the GPU tests' bound (1e-11 of max|eta| sum|w|) of the
    yardstick, areas included, on the column route's ordinates."""
    data, path, d, train = cases()[name]
    ref = I.by_definition(data, path, d, train)
    eta = I.ordinates_by_column(data, path, d)
    tol = 1e-11 * np.abs(ref["eta"]).max() * sum(abs(w) for w, _o in train)
    for m in range(len(data["member"])):
        (hi, x_hi), (lo, x_lo), pos, neg = sweep_as_the_header_states_it(list(ref["s"]), list(eta[m]), train)
        worst = max(abs(hi - ref["N_max"][m]), abs(lo - ref["N_min"][m]), abs(pos - ref["area_pos"][m]),
                    abs(neg - ref["area_neg"][m]))
        assert worst <= tol, (name, m, worst, tol)
        assert abs(I.response(ref["s"], ref["eta"], train, x_hi)[m] - hi) <= tol
        assert abs(I.response(ref["s"], ref["eta"], train, x_lo)[m] - lo) <= tol
