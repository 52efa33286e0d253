"""Response spectrum analysis, the parts that need no GPU: the header `include/trs_spectrum.h` against its ctypes table and
the library, the fits rule to the byte, the refusals of the C entry points and of `_check_spectrum_args`, and the numpy
yardstick of the GPU tests (`tests/spectrum_reference.py`) against four truths that need no restatement - so that parity
with it means something.

`python -m tests.test_spectrum` measures the float64 floor of the restatement, what the block iteration's shapes cost
against `eigh`'s and how well the four identities hold, and writes tests/golden/spectrum_tol.json, which these tests and
the GPU tests read.

bar-120's eigenvalue 7 is half of the repeated pair (7, 8): with eight modes the set is not closed and the response
depends on which vector of the pair came out.  Wherever shapes of two origins are compared, bar-120 therefore uses its
seven lowest modes (`modes_of`); the clusters inside them are (0, 1), (3, 4) and (5, 6)."""
import ctypes
import json
import os

import numpy as np
import pytest

from python_stable_3d_truss_analysis_amd import _capi, batch
from tests import helpers as H
from tests import mode_gradients_reference as G
from tests import modes_reference as R
from tests import spectrum_reference as S
from tests.test_capi_symbols import declared_prototypes, declared_symbols
from tests.test_mode_gradients import CLUSTERS, GAP_MIN

P = 8
FIXTURES = [n for n in H.data_case_names() if n.endswith("_input_0") and n != "bar-942_input_0"]
SIMPLE = [n for n in FIXTURES if n not in CLUSTERS]          # every gap of the first eight >= GAP_MIN (checked below)
TOL_FILE = os.path.join(H.GOLDEN, "spectrum_tol.json")
TOL_SMALL, TOL_BIG = "bar-120_input_0", "bar-942_input_0"
FACTOR = 100          # a bound = FACTOR x what `record_tolerance` measured
RULES = ("srss", "cqc", "abs")
# The table shared by every test: periods that bracket the fixtures' (bar-47's modes 6, 7 lie below T[0], bar-942's
# first beyond T[K - 1], the others inside), three directions of which the last is no axis, one spectrum shape per direction
PERIODS = np.array([0.05, 0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 60.0])
ACCEL = np.array([[0.4, 1.0, 1.0, 0.8, 0.4, 0.2, 0.08, 0.01],
                  [0.3, 0.8, 0.9, 0.6, 0.35, 0.15, 0.05, 0.02],
                  [0.25, 0.7, 0.6, 0.5, 0.2, 0.1, 0.06, 0.0]])
DIRS = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.6, -0.3, 0.5]])
ZETA = 0.05
COMBINED = ("u", "N", "R", "base")


def modes_of(name, p=P):
    return min(p, 7) if name == "bar-120_input_0" else p


_cache = {}


def arrays_of(name, with_mass=False):
    """(arrays, mass_scale) of a fixture; `with_mass`: seeded joint masses and mass_scale = 0.5 (test_mode_gradients)."""
    if (name, with_mass) not in _cache:
        d = G.arrays(H.load_json(name))
        mu = 1.0
        if with_mass:
            rng = np.random.default_rng(len(d["conn"]))
            d["joint_mass"] = rng.uniform(0.2, 1.0, size=len(d["xyz"])) * G.system(d)[1].max()
            mu = 0.5
        _cache[name, with_mass] = (d, mu)
    return _cache[name, with_mass]


def pairs_of(name, with_mass=False):
    if ("pairs", name, with_mass) not in _cache:
        d, mu = arrays_of(name, with_mass)
        _cache["pairs", name, with_mass] = G.eigen_pairs(d, mu, None)
    return _cache["pairs", name, with_mass]


# ---- the C interface ---------------------------------------------------------------------------------------------------
def test_header_table_and_library_agree():
    names = declared_symbols("trs_spectrum.h")
    assert names == ["trs_rs_abi_version", "trs_rs_combine", "trs_rs_combine_tab", "trs_rs_fits", "trs_rs_modal"]
    assert sorted(_capi.RS_SIGNATURES) == names
    protos = declared_prototypes("trs_spectrum.h")
    assert sorted(protos) == names
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name, (is_void, n_params) in protos.items():
        restype, argtypes = _capi.RS_SIGNATURES[name]
        assert hasattr(lib, name), name
        assert len(argtypes) == n_params and not is_void and restype is ctypes.c_int, name
    # (conn16, type_idx, types) for (conn, E, A): the member pointers only
    general, table = _capi.RS_SIGNATURES["trs_rs_combine"][1], _capi.RS_SIGNATURES["trs_rs_combine_tab"][1]
    assert len(general) == 29 and general == table
    # disjoint from every other table
    others = [getattr(_capi, t) for t in dir(_capi) if t.endswith("SIGNATURES") and t != "RS_SIGNATURES"]
    assert len(others) >= 10
    for table in others:
        assert not set(table) & set(_capi.RS_SIGNATURES)
    assert not any(name.startswith("trs_rs") for table in others for name in table)
    header = open(os.path.join(H.ROOT, "include", "trs_spectrum.h")).read()
    assert "#define TRS_RS_ABI_VERSION %d\n" % _capi.RS_ABI_VERSION in header
    assert "#define TRS_RS_BLOCK %d " % _capi.MODES_BLOCK in header
    for rule, code in _capi.RS_RULES.items():
        assert "#define TRS_RS_%s %d\n" % (rule.upper(), code) in header
    assert _capi.RS_RULES == S.RULES
    assert _capi.load().trs_rs_abi_version() == _capi.RS_ABI_VERSION == 1
    assert "`include/trs_spectrum.h`" in _capi.__doc__
    assert "include/trs_spectrum.h" in open(os.path.join(_capi.CSRC_DIR, "Makefile")).readline()
    # the headers it builds on are what they were
    assert len(declared_symbols("trs_modes.h")) == 6 and len(declared_symbols("trs_modegrad.h")) == 4
    import python_stable_3d_truss_analysis_amd as pkg
    assert {"solve_response_spectrum", "SpectrumResult"} <= set(pkg.__all__)
    assert pkg.solve_response_spectrum is batch.solve_response_spectrum and hasattr(pkg.Truss, "ResponseSpectrum")
    keys = sorted(key for key, *_ in batch.SpectrumResult.FIELDS.values())
    assert keys == sorted(("lam", "omega", "resid", "n_modes", "iters", "u_all", "N_all", "R_all") + S.KEYS)


def test_fits_rule_in_bytes_and_argument_errors():
    """All p + 3 response vectors in joint layout (24 nJ each), rho [8][8] and q [3][8] (704 bytes) and the end lists
    (4 (2 nJ + 1 + 2 nM)), rounded up to 16, within 160 KB; p in 1 .. 8."""
    lib = _capi.load()
    need = lambda nJ, nM, p: (24 * nJ * (p + 3) + 8 * 64 + 8 * 24 + 4 * (2 * nJ + 1 + 2 * nM) + 15) // 16 * 16
    budget = 160 * 1024
    assert lib.trs_rs_fits(244, 942, 8) == 1 and need(244, 942, 8) == 74624 <= budget // 2      # bar-942: two per CU
    inside = outside = 0
    for nJ, nM, p in ((100, 16991, 8), (100, 16992, 8), (100, 16993, 8), (599, 0, 8), (600, 0, 8), (1568, 0, 1),
                      (1569, 0, 1), (488, 1884, 8), (1000, 3000, 2), (1000, 3000, 3)):
        fits = need(nJ, nM, p) <= budget
        assert lib.trs_rs_fits(nJ, nM, p) == int(fits), (nJ, nM, p)
        inside, outside = inside + fits, outside + (not fits)
    assert inside >= 5 and outside >= 5
    assert need(100, 16991, 8) == budget < need(100, 16992, 8)                  # just inside, just outside
    for bad in ((-1, 0, 4), (0, -1, 4), (10, 10, 0), (10, 10, 9)):
        assert lib.trs_rs_fits(*bad) == 0
    some = ctypes.c_void_p(8)

    def modal(B=1, p=4, G=3, K=8, rule=1, X=some, zeta=0.05):
        return lib.trs_rs_modal(B, 10, some, some, some, X, 64, some, some, some, p, G, some, K, some, some, some, zeta,
                                rule, 1, None, None, None, None, None, some, some, some, None)

    def comb(B=1, nM=10, p=4, G=3, rule=1, X=some):
        return lib.trs_rs_combine(B, 10, nM, some, some, some, some, some, some, some, some, None, X, 64, some, p, G,
                                  some, some, rule, 1, some, some, None, None, None, None, None, None)

    for call in (modal, comb):
        for kw in (dict(p=0), dict(p=9), dict(G=0), dict(G=4), dict(rule=-1), dict(rule=3), dict(X=None)):
            assert call(**kw) != 0, (call.__name__, kw)
        assert call(B=0) == 0                                                    # an empty batch is no error
    assert modal(K=1) != 0 and modal(K=65) != 0 and modal(zeta=0.0) != 0 and modal(zeta=0.0, rule=0, B=0) == 0
    assert comb(nM=1 << 20) != 0                                                 # the vectors do not fit: refused


def test_check_spectrum_args():
    ok = batch._check_spectrum_args
    dirs, T, Sa, zpa, code, want = ok(8, DIRS, PERIODS, ACCEL)
    assert dirs.shape == (3, 3) and T.shape == (8,) and Sa.shape == (3, 8) and code == 1 and want == ("u", "N", "R")
    np.testing.assert_array_equal(zpa, ACCEL[:, 0])                             # the default zero-period acceleration
    assert ok(np.int64(1), [[1.0, 2.0]], [0.0, 1.0], [[1.0, 0.0]], 0.0, "SRSS", [3.0], ["N"])[2:] != ()
    d2 = ok(1, [[1.0, 2.0]], [0.0, 1.0], [[1.0, 0.0]], 0.0, "abs")
    np.testing.assert_array_equal(d2[0], [[1.0, 2.0, 0.0]])
    assert d2[4] == 2
    for bad in (0, 9, 2.5, True):
        with pytest.raises(ValueError, match="p must"):
            ok(bad, DIRS, PERIODS, ACCEL)
    for bad in (DIRS[0], np.zeros([0, 3]), np.zeros([4, 3]), np.zeros([2, 4]), np.full([1, 3], np.nan)):
        with pytest.raises(ValueError, match="directions"):
            ok(8, bad, PERIODS, ACCEL[:1])
    for bad in (PERIODS[:1], np.arange(65.0), PERIODS[::-1], np.array([0.0, 1.0, 1.0]), np.array([-1.0, 1.0]),
                np.array([0.0, np.inf]), PERIODS.reshape(2, 4)):
        with pytest.raises(ValueError, match="periods"):
            ok(8, DIRS, bad, np.ones([3, np.size(bad)]))
    for bad in (ACCEL[:2], ACCEL[:, :7], -ACCEL, np.where(ACCEL > 0.9, np.nan, ACCEL), np.where(ACCEL > 0.9, np.inf, ACCEL)):
        with pytest.raises(ValueError, match="accel"):
            ok(8, DIRS, PERIODS, bad)
    for bad in ([1.0, 2.0], [1.0, 2.0, -1.0], [1.0, np.nan, 1.0]):
        with pytest.raises(ValueError, match="zpa"):
            ok(8, DIRS, PERIODS, ACCEL, zpa=bad)
    for bad in ("sum", "", None, 1):
        with pytest.raises(ValueError, match="rule"):
            ok(8, DIRS, PERIODS, ACCEL, rule=bad)
    for bad in (0.0, -0.1, np.nan, "0.05", None, [0.05]):
        with pytest.raises(ValueError, match="damping"):
            ok(8, DIRS, PERIODS, ACCEL, damping=bad, rule="cqc")
    assert ok(8, DIRS, PERIODS, ACCEL, damping=0.0, rule="srss")[4] == 0
    for bad in (("u", "f_ext"), ("modal_u",), "u"):
        with pytest.raises(ValueError, match="want"):
            ok(8, DIRS, PERIODS, ACCEL, want=bad)
    # `solve_response_spectrum` refuses before it asks for a device
    packed = batch.pack_json([H.load_json("bar-25_input_0")] * 2)
    for kw in (dict(p=9), dict(rule="sum"), dict(damping=0.0), dict(zpa=[1.0]), dict(mass_scale=float("nan")),
               dict(joint_mass=np.zeros([2, packed.nJ_max]) - 1.0), dict(tol=-1.0)):
        with pytest.raises(ValueError):
            batch.solve_response_spectrum(packed, DIRS, PERIODS, ACCEL, **kw)
    with pytest.raises(ValueError):
        batch.solve_response_spectrum(packed, DIRS, PERIODS[::-1], ACCEL)


# ---- the restatement against truths that need no restatement -----------------------------------------------------------
def rotated(Phi, pair, angle):
    """The shapes with the two of `pair` rotated inside their plane: as good a basis of a repeated eigenvalue."""
    out = Phi.copy()
    i, j = pair
    out[i] = np.cos(angle) * Phi[i] + np.sin(angle) * Phi[j]
    out[j] = -np.sin(angle) * Phi[i] + np.cos(angle) * Phi[j]
    return out


def identities(name, with_mass=False):
    """How well the four truths hold for the restatement on a fixture, each error against the size of its own terms:
    (a) all modes: sum_k Gamma_k^2 = mtot; (b) flat spectrum Sa = zpa = a0, p = 1, 3, 8: the plain sum of the signed
    modal displacements plus the missing-mass vector = inv(K_ff) (a0 M iota); (c) every slot: sum_j modal_R . dir =
    -(the slot's base shear); (d) a rotation inside every repeated pair leaves the CQC results where they were (and
    moves the SRSS ones: `d_srss_moves`, the largest relative change)."""
    d, mu = arrays_of(name, with_mass)
    lam, Phi = pairs_of(name, with_mass)
    n = len(lam)
    K_ff, m = G.system(d, mu)
    free = d["free"].ravel()
    axis = np.tile(np.arange(3), len(d["xyz"]))[free]
    out = {"a": 0.0, "b": 0.0, "c": 0.0, "d": 0.0, "d_srss_moves": 0.0}
    full = S.response(d, Phi, lam, DIRS, PERIODS, ACCEL, ZETA, "srss", False, mass_scale=mu)
    out["a"] = float(np.abs((full["gamma"] ** 2).sum(1) - full["mtot"]).max() / full["mtot"].max())
    a0 = 0.7
    flat = np.full([len(DIRS), 2], a0)
    for p in sorted({1, min(3, n), min(P, n)}):
        r = S.response(d, Phi[:p], lam[:p], DIRS, [0.0, 1.0], flat, ZETA, "abs", True, mass_scale=mu)
        for g in range(len(DIRS)):
            want = np.zeros(free.size)
            want[free] = np.linalg.solve(K_ff, a0 * m * DIRS[g][axis])
            out["b"] = max(out["b"], G.scaled_difference(r["modal_u"][g].sum(0).ravel(), want))
    p = min(P, n) if with_mass else modes_of(name, min(P, n))
    for rule in RULES:
        r = S.response(d, Phi[:p], lam[:p], DIRS, PERIODS, ACCEL, ZETA, rule, True, mass_scale=mu)
        shear = -np.einsum("gvja,ga->gv", r["modal_R"], DIRS)
        out["c"] = max(out["c"], G.scaled_difference(shear, r["modal_base"]))
    for pair in ([] if with_mass else CLUSTERS.get(name, [])):      # (seeded joint masses break the symmetry)
        assert abs(lam[pair[1]] - lam[pair[0]]) < 1e-9 * lam[pair[0]]
        turned = rotated(Phi[:p], pair, 0.6)
        for rule in ("cqc", "srss"):
            r0 = S.response(d, Phi[:p], lam[:p], DIRS, PERIODS, ACCEL, ZETA, rule, True, mass_scale=mu)
            r1 = S.response(d, turned, lam[:p], DIRS, PERIODS, ACCEL, ZETA, rule, True, mass_scale=mu)
            worst = max(G.scaled_difference(r1[key], r0[key]) for key in COMBINED)
            key = "d" if rule == "cqc" else "d_srss_moves"
            out[key] = max(out[key], worst)
    return out


def tolerances():
    """tests/golden/spectrum_tol.json, as `record_tolerance` wrote it."""
    if "tol" not in _cache:
        with open(TOL_FILE) as fh:
            _cache["tol"] = json.load(fh)
    return _cache["tol"]


@pytest.mark.parametrize("name, with_mass", [(n, False) for n in FIXTURES] + [("bar-25_input_0", True), ("bar-72_input_0", True)])
def test_restatement_against_the_four_identities(name, with_mass):
    got = identities(name, with_mass)
    print(name, with_mass, got)
    for key in "abcd":
        bound = FACTOR * tolerances()["identities"][key]
        assert got[key] <= bound, (name, key, got[key], bound)
    if name in CLUSTERS and not with_mass:
        assert got["d_srss_moves"] > 0.05, (name, got)       # the same rotation moves SRSS: only CQC is compared there


def test_which_fixtures_have_simple_spectra():
    """SRSS and ABS are compared with `eigh` only where the gaps are >= GAP_MIN; the clusters are closed inside the modes
    that are compared."""
    for name in SIMPLE + [TOL_BIG]:
        lam = pairs_of(name)[0] if name != TOL_BIG else G.eigenvalues(arrays_of(name)[0])
        n = min(P, len(lam))
        assert (G.gaps(lam)[:n] >= GAP_MIN).all(), name
    assert SIMPLE == ["bar-10_input_0", "bar-25_input_0", "bar-47_input_0", "bar-6_input_0"]
    for name, clusters in CLUSTERS.items():
        lam = pairs_of(name)[0]
        p = modes_of(name)
        gap = G.gaps(lam)
        inside = sorted(k for c in clusters for k in c)
        assert [k for k in range(p) if gap[k] < GAP_MIN] == inside, name
        assert abs(lam[p] - lam[p - 1]) >= GAP_MIN * lam[p - 1], name          # closed at the top
    lam = pairs_of("bar-120_input_0")[0]
    assert abs(lam[8] - lam[7]) < 1e-9 * lam[7]                                # why bar-120 stops at seven


# ---- the recorded tolerances ------------------------------------------------------------------------------------------
def cluster_sums(name, x, p):
    """[G, p] per-mode values with every cluster's entries replaced by the cluster's sum."""
    x = np.array(x[:, :p], dtype=float)
    for pair in CLUSTERS.get(name, []):
        x[:, list(pair)] = x[:, list(pair)].sum(1, keepdims=True)
    return x


def difference(key, got, want):
    """`scaled_difference` of one quantity; gamma up to its sign, which is the sign of the shape it was formed with (every
    response carries Gamma phi, where it cancels)."""
    return G.scaled_difference(np.abs(got), np.abs(want)) if key == "gamma" else G.scaled_difference(got, want)


def truth_differences(name, got, want, p, rule):
    """Scaled differences between two responses of one truss whose shapes have different origins: everything on a simple
    spectrum; on a clustered one the combined CQC results, sa, mtot and the cluster sums of meff and gamma^2."""
    out = {}
    if name in CLUSTERS:
        if rule != "cqc":
            return out
        keys = ("sa", "mtot") + COMBINED
        out["meff"] = G.scaled_difference(cluster_sums(name, got["meff"], p), cluster_sums(name, want["meff"], p))
        out["gamma"] = G.scaled_difference(cluster_sums(name, got["gamma"] ** 2, p), cluster_sums(name, want["gamma"] ** 2, p))
    else:
        keys = S.KEYS
    for key in keys:
        out[key] = difference(key, got[key], want[key])
    return out


def measure(name):
    """(a) the scaled float64 - longdouble difference of the restatement on FIXED shapes (eigh's), (b) the scaled
    difference between the restatement on the block iteration's shapes and on eigh's; the worst over the rules and the
    quantities, each scaled by its own largest entry."""
    data = H.load_json(name)
    d = G.arrays(data)
    p = modes_of(name)
    lam, Phi = G.eigen_pairs(d, 1.0, p)
    K_ff, m, mask = R.matrices(data)
    it_lam, it_Phi, resid, n_modes, iters = R.block_iteration(K_ff, m, p=P, tol=1e-10, check_every=8)
    assert iters > 0 and n_modes == P
    shapes = np.zeros([p, d["free"].size])
    shapes[:, d["free"].ravel()] = it_Phi.T[:p]
    a = b = 0.0
    for rule in RULES:
        r64 = S.response(d, Phi, lam[:p], DIRS, PERIODS, ACCEL, ZETA, rule, True)
        r80 = S.response(d, Phi, lam[:p], DIRS, PERIODS, ACCEL, ZETA, rule, True, dtype=np.longdouble)
        a = max([a] + [difference(key, r64[key], r80[key]) for key in S.KEYS])
        rit = S.response(d, shapes.reshape(p, -1, 3), it_lam[:p], DIRS, PERIODS, ACCEL, ZETA, rule, True)
        b = max([b] + list(truth_differences(name, rit, r64, p, rule).values()))
    return {"truss": name, "modes": p, "iterations": int(iters), "a_float64_against_longdouble": a,
            "b_iteration_against_eigh": b}


def record_tolerance():
    """Writes tests/golden/spectrum_tol.json (about a minute: the block iteration on bar-942 in numpy)."""
    worst = {key: 0.0 for key in "abcd"}
    cases = [(n, False) for n in FIXTURES] + [("bar-25_input_0", True), ("bar-72_input_0", True)]
    for name, with_mass in cases:
        for key, value in identities(name, with_mass).items():
            if key in worst:
                worst[key] = max(worst[key], value)
    rec = {"what": "tests/spectrum_reference.response on tests/test_spectrum's table (three directions, missing mass on), "
                   "differences scaled by the largest entry of each quantity, the worst over the rules srss, cqc, abs and "
                   "the quantities: (a) float64 against longdouble on the shapes of numpy.linalg.eigh; (b) on the shapes "
                   "of tests/modes_reference.block_iteration (p = 8, tol 1e-10, check_every 8) against those of eigh - on "
                   "bar-120 its seven lowest modes (eigenvalue 7 is half of the pair (7, 8)), cqc only and per-mode "
                   "values by cluster sums.  The device is allowed max(1e-11, 100 x a) against the restatement on its "
                   "own shapes and max(1e-9, 100 x b) against eigh, of its size class.  identities: the worst error over "
                   "bar-6 ... bar-120 of (a) sum Gamma^2 = mtot, (b) flat spectrum: modal sum + missing mass = the "
                   "static solution, (c) reactions . direction = -base shear per slot, (d) cqc under a rotation inside a "
                   "repeated pair; the tests allow 100 x each",
           "small": measure(TOL_SMALL), "big": measure(TOL_BIG), "identities": worst}
    with open(TOL_FILE, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    return rec


def test_recorded_tolerances_name_their_inputs():
    """The small truss is measured again here; the bar-942 figures (a minute of numpy) are only read."""
    rec = tolerances()
    assert (rec["small"]["truss"], rec["small"]["modes"]) == (TOL_SMALL, 7)
    assert (rec["big"]["truss"], rec["big"]["modes"]) == (TOL_BIG, 8)
    assert "block_iteration" in rec["what"] and "longdouble" in rec["what"] and "eigh" in rec["what"]
    again = measure(TOL_SMALL)
    assert again["iterations"] == rec["small"]["iterations"]
    for key in ("a_float64_against_longdouble", "b_iteration_against_eigh"):
        for size in ("small", "big"):
            assert 0 < rec[size][key] < 1e-9, (size, key)
        assert again[key] <= 10 * rec["small"][key] + 1e-15, key
    # (d) alone is a root of a sum that cancels (a member at rest by symmetry): the root of float64's epsilon, not epsilon
    assert sorted(rec["identities"]) == list("abcd") and all(0 < rec["identities"][k] < 1e-11 for k in "abc")
    assert 0 < rec["identities"]["d"] < 1e-8


if __name__ == "__main__":
    print(json.dumps(record_tolerance(), indent=1))
