"""Gradients of the natural frequencies, the parts that need no GPU: the header `include/trs_modegrad.h` against its
ctypes table and the library, the refusals of `_check_mode_gradient_args`, and the numpy yardstick of the GPU tests
(`tests/mode_gradients_reference.py`) against central differences of the eigenvalues and against the identities that
hold without any reference - so that parity with it means something.

`python -m tests.test_mode_gradients` measures the float64 floor of the restatement and what the block iteration's
shapes cost against `eigh`'s, and writes tests/golden/mode_gradients_tol.json, which the GPU tests read."""
import ctypes
import json
import os

import numpy as np
import pytest

from python_stable_3d_truss_analysis_amd import _capi, batch
from tests import helpers as H
from tests import mode_gradients_reference as G
from tests import modes_reference as R
from tests.test_capi_symbols import declared_prototypes, declared_symbols

P = 8
FD_BOUND = 1e-4       # 7 x the worst central-difference noise measured (1.5e-5, bar-47 mode 0)
GAP_MIN = 1e-3        # single modes are differentiated only where the eigenvalue is simple
FIXTURES = [n for n in H.data_case_names() if n.endswith("_input_0") and n != "bar-942_input_0"]
CLUSTERS = {"bar-72_input_0": [(0, 1), (4, 5)], "bar-120_input_0": [(0, 1), (3, 4), (5, 6)]}
TOL_FILE = os.path.join(H.GOLDEN, "mode_gradients_tol.json")
TOL_SMALL, TOL_BIG = ("bar-120_input_0", [2]), ("bar-942_input_0", list(range(8)))

_cache = {}


def exact(name, with_mass=False):
    """(arrays, mass_scale, lam [p], gap [p], exact gradients) of a fixture, computed once.  `with_mass`: seeded joint
    masses of the order of the lumped ones and mass_scale = 0.5, so that every formula has every term."""
    if (name, with_mass) not in _cache:
        d = G.arrays(H.load_json(name))
        mu = 1.0
        if with_mass:
            rng = np.random.default_rng(len(d["conn"]))
            d["joint_mass"] = rng.uniform(0.2, 1.0, size=len(d["xyz"])) * G.system(d)[1].max()
            mu = 0.5
        _cache[name, with_mass] = (d, mu) + G.exact_gradients(d, P, mu)
    return _cache[name, with_mass]


# ---- the C interface ---------------------------------------------------------------------------------------------------
def test_header_table_and_library_agree():
    names = declared_symbols("trs_modegrad.h")
    assert names == ["trs_mg_abi_version", "trs_mg_fits", "trs_mg_grad", "trs_mg_tab_grad"]
    assert sorted(_capi.MG_SIGNATURES) == names
    protos = declared_prototypes("trs_modegrad.h")
    assert sorted(protos) == names
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name, (is_void, n_params) in protos.items():
        restype, argtypes = _capi.MG_SIGNATURES[name]
        assert hasattr(lib, name), name
        assert len(argtypes) == n_params and not is_void and restype is ctypes.c_int, name
    # (conn16, type_idx, types) for (conn, E, A, rho): one pointer fewer, the rest alike
    general, table = _capi.MG_SIGNATURES["trs_mg_grad"][1], _capi.MG_SIGNATURES["trs_mg_tab_grad"][1]
    assert len(general) == 26 and general[:4] + general[5:] == table
    # disjoint from every other table
    others = [getattr(_capi, t) for t in dir(_capi) if t.endswith("SIGNATURES") and t != "MG_SIGNATURES"]
    assert len(others) >= 9
    for table in others:
        assert not set(table) & set(_capi.MG_SIGNATURES)
    assert not any(name.startswith("trs_mg") for table in others for name in table)
    header = open(os.path.join(H.ROOT, "include", "trs_modegrad.h")).read()
    assert "#define TRS_MG_ABI_VERSION %d\n" % _capi.MG_ABI_VERSION in header
    assert "#define TRS_MG_BLOCK %d " % _capi.MODES_BLOCK in header
    assert _capi.load().trs_mg_abi_version() == _capi.MG_ABI_VERSION == 1
    # trs_modes.h is what it was
    assert len(declared_symbols("trs_modes.h")) == 6 and _capi.MODES_ABI_VERSION == 1
    import python_stable_3d_truss_analysis_amd as pkg
    assert {"solve_mode_gradients", "ModeGradientResult"} <= set(pkg.__all__)
    assert pkg.solve_mode_gradients is batch.solve_mode_gradients and hasattr(pkg.Truss, "FrequencyGradients")
    assert batch.DeviceBatch.MODE_GRADIENTS == G.KEYS
    assert sorted(key for key, *_ in batch.ModeGradientResult.FIELDS.values()) == \
        sorted(("lam", "omega", "gap", "resid", "n_modes", "iters") + G.KEYS)


def test_fits_rule_in_bytes_and_argument_errors():
    """The member table (48 nM), the clamped end joints (8 nM), the end lists (4 (2 nJ + 1 + 2 nM)) and one mode in joint
    layout (24 nJ), rounded up to 16, within 160 KB; p in 1 .. 8."""
    lib = _capi.load()
    need = lambda nJ, nM, pc=1: (64 * nM + 8 * nJ + 4 + 24 * nJ * pc + 15) // 16 * 16
    budget = 160 * 1024
    assert lib.trs_mg_fits(244, 942, 8) == 1 and need(244, 942, 8) <= budget          # bar-942: all eight modes at once
    assert lib.trs_mg_fits(488, 1884, 8) == 1 and need(488, 1884, 3) <= budget < need(488, 1884, 4)   # three per pass
    for nJ, nM in ((100, 2510), (100, 2511), (100, 2512), (5119, 0), (5120, 0), (5121, 0), (2000, 1559), (2000, 1560),
                   (2000, 1561)):
        assert lib.trs_mg_fits(nJ, nM, 4) == int(need(nJ, nM) <= budget), (nJ, nM)
    assert need(2000, 1559) <= budget < need(2000, 1561)
    for bad in ((-1, 0, 4), (0, -1, 4), (10, 10, 0), (10, 10, 9)):
        assert lib.trs_mg_fits(*bad) == 0
    some = ctypes.c_void_p(8)
    call = lambda B, nJ, nM, p, X=some: lib.trs_mg_grad(B, nJ, nM, some, some, some, some, some, some, some, some, some,
                                                        None, X, 64, some, some, p, 1.0, None, some, None, None, None,
                                                        None, None)
    assert call(1, 10, 10, 0) != 0 and call(1, 10, 10, 9) != 0 and call(1, 10, 1 << 20, 4) != 0
    assert call(1, 10, 10, 4, X=None) != 0
    assert call(0, 10, 10, 4) == 0                                                   # an empty batch is no error


def test_check_mode_gradient_args():
    ok = batch._check_mode_gradient_args
    B, nJ = 2, 10
    assert ok(B, nJ, 4, None, 1.0, 1e-10, 256, want=("A", "xyz")) == ("A", "xyz")
    assert ok(B, nJ, np.int64(8), (B, nJ), 0.5, 1e-8, 3, weights=np.ones([B, 8]), want=["joint_mass"]) == ("joint_mass",)
    for bad in (0, 9, 2.5, True):
        with pytest.raises(ValueError, match="p must"):
            ok(B, nJ, bad, None, 1.0, 1e-10, 256)
    with pytest.raises(ValueError, match="joint_mass"):
        ok(B, nJ, 4, (B, nJ + 1), 1.0, 1e-10, 256)
    with pytest.raises(ValueError, match="joint_mass"):
        ok(B, nJ, 4, (B, nJ), 1.0, 1e-10, 256, joint_mass_min=-1.0)
    with pytest.raises(ValueError, match="mass_scale"):
        ok(B, nJ, 4, None, -1.0, 1e-10, 256)
    with pytest.raises(ValueError, match="tol"):
        ok(B, nJ, 4, None, 1.0, 0.0, 256)
    with pytest.raises(ValueError, match="max_iters"):
        ok(B, nJ, 4, None, 1.0, 1e-10, 0)
    for bad in (np.ones([B, 5]), np.ones([B + 1, 4]), np.ones([4]), np.ones([B, 4, 1])):
        with pytest.raises(ValueError, match="weights must be"):
            ok(B, nJ, 4, None, 1.0, 1e-10, 256, weights=bad)
    for bad in (np.nan, np.inf):
        w = np.ones([B, 4])
        w[1, 2] = bad
        with pytest.raises(ValueError, match="finite"):
            ok(B, nJ, 4, None, 1.0, 1e-10, 256, weights=w)
    for bad in (("A", "loads"), ("mass",), "xyz"):
        with pytest.raises(ValueError, match="want"):
            ok(B, nJ, 4, None, 1.0, 1e-10, 256, want=bad)
    with pytest.raises(ValueError, match="joint_mass"):
        ok(B, nJ, 4, None, 1.0, 1e-10, 256, want=("A", "joint_mass"))
    with pytest.raises(ValueError, match="sections"):
        ok(B, nJ, 4, None, 1.0, 1e-10, 256, sections=[])
    # `solve_mode_gradients` refuses before it asks for a device
    packed = batch.pack_json([H.load_json("bar-25_input_0")] * 2)
    for kw in (dict(p=9), dict(weights=np.ones([2, 5])), dict(weights=np.full([2, 6], np.nan)), dict(want=("u",)),
               dict(want=("joint_mass",)), dict(sections=[]), dict(joint_mass=np.zeros([2, packed.nJ_max]) - 1.0),
               dict(mass_scale=float("nan")), dict(tol=-1.0)):
        with pytest.raises(ValueError):
            batch.solve_mode_gradients(packed, **kw)


# ---- the restatement against central differences ----------------------------------------------------------------------
CASES = [(name, False) for name in FIXTURES] + [("bar-25_input_0", True), ("bar-72_input_0", True)]


@pytest.mark.parametrize("name, with_mass", CASES, ids=[f"{n}{'-masses' if w else ''}" for n, w in CASES])
def test_restatement_against_central_differences(name, with_mass):
    d, mu, lam, gap, g = exact(name, with_mass)
    n = len(lam)
    simple = [k for k in range(n) if gap[k] >= GAP_MIN]
    assert simple, name
    for key in G.KEYS:
        fd = G.central_differences(d, key, lambda l: l[:n], mu)
        for k in simple:
            if not np.abs(fd[k]).max() > 0:        # (nothing depends on it: joint masses at zero density never occur)
                assert not np.abs(g[key][k]).max() > 0, (name, key, k)
                continue
            diff = G.scaled_difference(g[key][k], fd[k])
            print(f"{name} mode {k} gap {gap[k]:.1e} d/d{key}: scaled difference {diff:.2e}")
            assert diff <= FD_BOUND, (name, key, k, diff)
    if orc_dim(name) == 2:
        assert not g["xyz"][:, :, 2].any()


def orc_dim(name):
    return len(H.load_json(name)["joint"][0][0])


@pytest.mark.parametrize("name, pair", [(n, c) for n, cs in CLUSTERS.items() for c in cs],
                         ids=[f"{n}-{c[0]}{c[1]}" for n, cs in CLUSTERS.items() for c in cs])
def test_cluster_sums_against_differences_of_the_summed_eigenvalues(name, pair):
    """A member of a repeated pair has no derivative; the sum over the closed cluster has, whatever basis `eigh` chose."""
    d, mu, lam, gap, g = exact(name)
    ks = list(pair)
    assert max(gap[k] for k in ks) < 1e-9 and abs(lam[ks[1]] - lam[ks[0]]) < 1e-9 * lam[ks[0]]
    outside = np.delete(lam, ks)
    assert np.abs(outside - lam[ks[0]]).min() >= GAP_MIN * lam[ks[0]]       # the cluster is closed
    for key in ("A", "E", "rho", "xyz"):
        fd = G.central_differences(d, key, lambda l: l[ks].sum(keepdims=True), mu)[0]
        diff = G.scaled_difference(g[key][ks].sum(0), fd)
        print(f"{name} cluster {pair} d/d{key}: scaled difference {diff:.2e}")
        assert diff <= FD_BOUND, (name, pair, key, diff)


def assert_identities(d, mu, lam, g, rows, rtol, what):
    """The four identities of the issue, per row, each against the size of its own terms."""
    for k in rows:
        l = lam[k]
        dm = float((d["joint_mass"] * g["joint_mass"][k]).sum())
        checks = {"sum E dE = lam": ((d["E"] * g["E"][k]).sum() - l, l),
                  "sum A dA = -sum m dm": ((d["A"] * g["A"][k]).sum() + dm, l),
                  "sum rho drho = -(lam + sum m dm)": ((d["rho"] * g["rho"][k]).sum() + l + dm, l)}
        for axis in range(3):
            checks[f"translation {axis}"] = (g["xyz"][k, :, axis].sum(), np.abs(g["xyz"][k]).sum())
        for label, (err, scale) in checks.items():
            assert abs(err) <= rtol * abs(scale), (what, k, label, err, scale)


@pytest.mark.parametrize("with_mass", [False, True])
def test_identities_hold_for_every_mode(with_mass):
    """Also for the members of a cluster: each identity is a statement about phi^T K phi and phi^T M phi of ONE
    M-orthonormal vector, whichever one of the subspace it is."""
    for name in FIXTURES:
        d, mu, lam, gap, g = exact(name, with_mass)
        assert_identities(d, mu, lam, g, range(len(lam)), 1e-10, name)
        if not with_mass:
            assert not g["joint_mass"][:, d["free"].any(1) == 0].any()       # held joints carry no phi


# ---- the recorded tolerances ------------------------------------------------------------------------------------------
def measure(name, modes):
    """(a) the scaled float64 - longdouble difference of the restatement on FIXED shapes (eigh's), (b) the scaled
    difference between the restatement on the block iteration's shapes and on eigh's; the worst over `modes` and the
    five quantities, each scaled by its own largest entry."""
    data = H.load_json(name)
    d = G.arrays(data)
    lam, Phi = G.eigen_pairs(d, 1.0, P)
    gap = G.gaps(lam)[:P]
    g64, g80 = G.gradients(d, Phi, lam[:P]), G.gradients(d, Phi, lam[:P], dtype=np.longdouble)
    K_ff, m, mask = R.matrices(data)
    it_lam, it_Phi, resid, n_modes, iters = R.block_iteration(K_ff, m, p=P, tol=1e-10, check_every=8)
    assert iters > 0 and n_modes == P
    shapes = np.zeros([P, d["free"].size])
    shapes[:, d["free"].ravel()] = it_Phi.T
    git = G.gradients(d, shapes.reshape(P, -1, 3), it_lam)
    a = max(G.scaled_difference(g64[key][k], g80[key][k]) for key in G.KEYS[:4] for k in modes)
    b = max(G.scaled_difference(git[key][k], g64[key][k]) for key in G.KEYS[:4] for k in modes)
    return {"truss": name, "modes": list(modes), "iterations": int(iters), "smallest_gap": float(gap[list(modes)].min()),
            "a_float64_against_longdouble": a, "b_iteration_against_eigh": b}


def record_tolerance():
    """Writes tests/golden/mode_gradients_tol.json (about a minute: the block iteration on bar-942 in numpy)."""
    rec = {"what": "tests/mode_gradients_reference.gradients, differences scaled by the largest entry of each (mode, "
                   "quantity), the worst over the modes named and over A, E, rho, xyz: (a) float64 against longdouble on "
                   "the shapes of numpy.linalg.eigh; (b) on the shapes of tests/modes_reference.block_iteration (p = 8, "
                   "tol 1e-10, check_every 8) against those of eigh.  The device is allowed max(1e-11, 100 x a) "
                   "against the restatement on its own shapes and max(1e-9, 100 x b) against eigh, of its size class",
           "small": measure(*TOL_SMALL), "big": measure(*TOL_BIG)}
    with open(TOL_FILE, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    return rec


def test_recorded_tolerances_name_their_inputs():
    """The small truss is measured again here; the bar-942 figures (a minute of numpy) are only read."""
    with open(TOL_FILE) as fh:
        rec = json.load(fh)
    assert (rec["small"]["truss"], rec["small"]["modes"]) == TOL_SMALL
    assert (rec["big"]["truss"], rec["big"]["modes"]) == TOL_BIG
    assert "block_iteration" in rec["what"] and "longdouble" in rec["what"] and "eigh" in rec["what"]
    again = measure(*TOL_SMALL)
    assert again["iterations"] == rec["small"]["iterations"]
    for key in ("a_float64_against_longdouble", "b_iteration_against_eigh"):
        for size in ("small", "big"):
            assert 0 < rec[size][key] < 1e-9, (size, key)
        assert again[key] <= 10 * rec["small"][key] + 1e-15, key
    assert rec["small"]["smallest_gap"] >= 1e-2 and rec["big"]["smallest_gap"] >= GAP_MIN


if __name__ == "__main__":
    print(json.dumps(record_tolerance(), indent=1))
