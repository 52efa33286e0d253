"""Harmonic response analysis, the parts that need no GPU: the header `include/trs_harmonic.h` against its ctypes table
and the library, the fits rule to the byte, the refusals of the C entry points and of `_check_harmonic_args`, and the
numpy yardstick of the GPU tests (`tests/harmonic_reference.py`) against four truths that need no restatement - so that
parity with it means something.

`python -m tests.test_harmonic` measures the float64 floor of the restatement, what the block iteration's shapes cost
against `eigh`'s and how well the four identities hold, and writes tests/golden/harmonic_tol.json, which these tests and
the GPU tests read.  As in tests/test_spectrum.py, bar-120 is compared through its seven lowest modes wherever shapes of
two origins meet (`modes_of`), and bar-942 takes no part in the identities: its own conditioning (1e-10 for the static
solution, 2e-8 for the complex solve) would set their bounds."""
import ctypes
import json
import os

import numpy as np
import pytest

from python_stable_3d_truss_analysis_amd import _capi, batch
from tests import harmonic_reference as HR
from tests import helpers as H
from tests import mode_gradients_reference as G
from tests import modes_reference as R
from tests.test_capi_symbols import declared_prototypes, declared_symbols
from tests.test_spectrum import CLUSTERS, FIXTURES, P, arrays_of, modes_of, pairs_of, rotated

TOL_FILE = os.path.join(H.GOLDEN, "harmonic_tol.json")
TOL_SMALL, TOL_BIG = "bar-120_input_0", "bar-942_input_0"
FACTOR = 100          # a bound = FACTOR x what `record_tolerance` measured
ZETA = 0.02
S_TEST = 130          # more than two table chunks of 64, and no multiple of 64
L_TEST = 3            # a load pattern, a ground acceleration, both together
AG = np.array([0.7, -0.4, 0.5])

_cache = {}


def frequencies_of(name, with_mass=False):
    """The p lowest circular frequencies of a fixture from `eigh` (fewer when it has fewer)."""
    lam = pairs_of(name, with_mass)[0] if name != TOL_BIG else G.eigenvalues(arrays_of(name, with_mass)[0])
    return np.sqrt(lam[:P])


def sweep_of(name, with_mass=False, S=S_TEST):
    """The test sweep of a fixture from its own frequencies w_1 .. w_p: 0, w_1 / 2, every w_k, every 1.001 w_k, the
    midpoints, 2 w_p, then a linear grid inside (0, 2 w_p) up to S values - the special values first, so the order is not
    ascending."""
    if ("sweep", name, with_mass, S) not in _cache:
        _cache["sweep", name, with_mass, S] = sweep_from(frequencies_of(name, with_mass), S)
    return _cache["sweep", name, with_mass, S]


def sweep_from(w, S=S_TEST):
    """The test sweep from the frequencies w_1 .. w_p themselves (a ragged batch: those of its first truss).
    The two frequencies of a repeated eigenvalue (bar-72, bar-120) give one value, not two a rounding error apart, and a
    grid point that falls on a value already there moves on by 0.37 of the grid's step: every value stands apart from the
    others by more than 1e-6 w_p, so that no two of them tie for an envelope."""
    vals = []
    apart = lambda x: all(abs(x - y) > 1e-6 * w[-1] for y in vals)
    for x in [0.0, 0.5 * w[0]] + list(w) + list(1.001 * w) + list(0.5 * (w[1:] + w[:-1])) + [2.0 * w[-1]]:
        if apart(x) and len(vals) < S:
            vals.append(float(x))
    grid = np.linspace(0.0, 2.0 * w[-1], S - len(vals) + 2)[1:-1] if S > len(vals) else []
    for x in grid:
        while not apart(x):
            x += 0.37 * (grid[1] - grid[0])
        vals.append(float(x))
    return np.array(vals)


def dampings_from(w):
    return {"modal": (ZETA, 0.0, 0.0), "all": (ZETA, 0.006 * w[0], 0.02 / w[-1])}


def dampings_of(name, with_mass=False):
    """The two damping configurations of the tests: modal alone, and all three."""
    return dampings_from(frequencies_of(name, with_mass))


def cases_of(d, mass_scale=1.0):
    """(patterns [3, nJ, 3], ground accelerations [3, 3]) of the three test cases of a truss: a seeded load pattern on
    its free DOFs, a ground acceleration, both together - the pattern sized like the inertia load, so that both count."""
    nJ = len(d["xyz"])
    rng = np.random.default_rng(3 * nJ + len(d["conn"]))
    m = G.system(d, mass_scale)[1]
    pat = rng.uniform(-1.0, 1.0, size=[nJ, 3]) * d["free"] * (m.mean() * np.abs(AG).max())
    return np.stack([pat, np.zeros_like(pat), 0.5 * pat]), np.stack([np.zeros(3), AG, AG])


def loads_of(d, mass_scale=1.0, dtype=np.float64):
    pats, ags = cases_of(d, mass_scale)
    return [HR.load(d, pats[l], ags[l], mass_scale, dtype) for l in range(L_TEST)]


def scaled(got, want):
    """max |got - want| / max |want| of complex arrays (0 when both are all zero)."""
    scale = np.abs(want).max() if want.size else 0.0
    diff = np.abs(got - want).max() if want.size else 0.0
    return float(diff / scale) if scale > 0 else float(diff)


# ---- the C interface ---------------------------------------------------------------------------------------------------
def test_header_table_and_library_agree():
    names = declared_symbols("trs_harmonic.h")
    assert names == ["trs_hr_abi_version", "trs_hr_fits", "trs_hr_modal", "trs_hr_sweep", "trs_hr_sweep_tab"]
    assert sorted(_capi.HR_SIGNATURES) == names
    protos = declared_prototypes("trs_harmonic.h")
    assert sorted(protos) == names
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name, (is_void, n_params) in protos.items():
        restype, argtypes = _capi.HR_SIGNATURES[name]
        assert hasattr(lib, name), name
        assert len(argtypes) == n_params and not is_void and restype is ctypes.c_int, name
    # (conn16, type_idx, types) for (conn, E, A): the member pointers only
    general, table = _capi.HR_SIGNATURES["trs_hr_sweep"][1], _capi.HR_SIGNATURES["trs_hr_sweep_tab"][1]
    assert len(general) == 38 and general == table and len(_capi.HR_SIGNATURES["trs_hr_modal"][1]) == 18
    # disjoint from every other table
    others = [getattr(_capi, t) for t in dir(_capi) if t.endswith("SIGNATURES") and t != "HR_SIGNATURES"]
    assert len(others) >= 11
    for table in others:
        assert not set(table) & set(_capi.HR_SIGNATURES)
    assert not any(name.startswith("trs_hr") for table in others for name in table)
    header = open(os.path.join(H.ROOT, "include", "trs_harmonic.h")).read()
    assert "#define TRS_HR_ABI_VERSION %d\n" % _capi.HR_ABI_VERSION in header
    assert "#define TRS_HR_BLOCK %d " % _capi.MODES_BLOCK in header and "#define TRS_HR_CHUNK 64 " in header
    assert _capi.load().trs_hr_abi_version() == _capi.HR_ABI_VERSION == 1
    assert "`include/trs_harmonic.h`" in _capi.__doc__
    makefile = open(os.path.join(_capi.CSRC_DIR, "Makefile")).read()
    assert "include/trs_harmonic.h" in makefile.splitlines()[0] and " harmonic.hip " in makefile
    assert makefile.count("../../include/trs_harmonic.h") == 1
    # the headers it builds on are what they were
    assert len(declared_symbols("trs_modes.h")) == 6 and len(declared_symbols("trs_spectrum.h")) == 5
    import python_stable_3d_truss_analysis_amd as pkg
    assert {"solve_harmonic", "HarmonicResult"} <= set(pkg.__all__)
    assert pkg.solve_harmonic is batch.solve_harmonic and hasattr(pkg.Truss, "HarmonicResponse")
    keys = sorted(key for key, *_ in batch.HarmonicResult.FIELDS.values())
    assert keys == sorted(["lam", "omega", "n_modes", "iters", "frf_u", "frf_N"]
                          + [k + tail for k in HR.KEYS for tail in ("_amp", "_at", "_omega")])
    for text in (batch.DeviceBatch.harmonic.__doc__, batch.solve_harmonic.__doc__, pkg.Truss.HarmonicResponse.__doc__):
        assert "static" in text.lower() and "first" in text and "left out" in text      # what the residual does not cover


def test_fits_rule_in_bytes_and_argument_errors():
    """The p + 1 response vectors in joint layout (24 nJ each), the coefficient table of one chunk (64 x 8 complex: 8192
    bytes), g (64 bytes) and the end lists (4 (2 nJ + 1 + 2 nM)), rounded up to 16, within 160 KB; p in 1 .. 8."""
    lib = _capi.load()
    need = lambda nJ, nM, p: (24 * nJ * (p + 1) + 8192 + 64 + 4 * (2 * nJ + 1 + 2 * nM) + 15) // 16 * 16
    budget = 160 * 1024
    assert lib.trs_hr_fits(244, 942, 8) == 1 and need(244, 942, 8) == 70464 <= budget // 2      # bar-942: two per CU
    inside = outside = 0
    for nJ, nM, p in ((100, 16646, 8), (100, 16647, 8), (100, 16648, 8), (694, 0, 8), (695, 0, 8), (2778, 0, 1),
                      (2779, 0, 1), (488, 1884, 8), (732, 2826, 8), (1000, 3000, 4), (1000, 3000, 5)):
        fits = need(nJ, nM, p) <= budget
        assert lib.trs_hr_fits(nJ, nM, p) == int(fits), (nJ, nM, p)
        inside, outside = inside + fits, outside + (not fits)
    assert inside >= 5 and outside >= 5
    assert need(100, 16647, 8) == budget < need(100, 16648, 8)                  # just inside, just outside
    for bad in ((-1, 0, 4), (0, -1, 4), (10, 10, 0), (10, 10, 9)):
        assert lib.trs_hr_fits(*bad) == 0
    some = ctypes.c_void_p(8)

    def modal(B=1, L=3, p=4, X=some, Pr=some, ag=some, residual=1, g=some, F=some):
        return lib.trs_hr_modal(B, L, 10, some, some, some, X, 64, some, some, some, p, Pr, ag, residual, g, F, None)

    def sweep(B=1, L=3, nM=10, p=4, X=some, S=5, omega=some, damp=(0.02, 0.0, 0.0), Pj=0, Pm=0, g=some, tab=False, **kw):
        fn = lib.trs_hr_sweep_tab if tab else lib.trs_hr_sweep
        mon_j, mon_m = kw.get("mon_j", None), kw.get("mon_m", None)
        return fn(B, L, 10, nM, some, some, some, some, some, some, some, some, None, X, 64, some, some, p, g, some, S,
                  omega, damp[0], damp[1], damp[2], some, some, None, None, some, some, mon_j, Pj, mon_m, Pm,
                  kw.get("frf_u", None), kw.get("frf_N", None), None)

    for call in (modal, sweep):
        for kw in (dict(p=0), dict(p=9), dict(L=0), dict(L=17), dict(X=None), dict(g=None)):
            assert call(**kw) != 0, (call.__name__, kw)
        assert call(B=0) == 0 and call(B=0, p=0) == 0                            # an empty batch is no error
    assert modal(Pr=None, ag=None) != 0 and modal(F=None) != 0                   # no load at all; residual without F
    for kw in (dict(S=0), dict(omega=None), dict(Pj=-1), dict(Pm=-1), dict(damp=(0.0, 0.0, 0.0)),
               dict(damp=(-0.1, 1.0, 0.0)), dict(damp=(0.1, -1.0, 0.0)), dict(damp=(0.1, 0.0, -1.0)),
               dict(damp=(float("nan"), 0.0, 0.0)), dict(nM=1 << 20), dict(Pj=2, frf_u=some), dict(Pm=2, frf_N=some)):
        assert sweep(**kw) != 0, kw
        assert sweep(tab=True, **kw) != 0, kw


def test_check_harmonic_args():
    ok = batch._check_harmonic_args
    W, ag, L, want = ok(2, 10, 8, [0.0, 3.0, 1.0], None, [[1.0, 0.0, 0.0]])
    assert W.tolist() == [0.0, 3.0, 1.0] and ag.shape == (2, 1, 3) and L == 1 and want == ("u", "N", "R")
    W, ag, L, want = ok(2, 10, np.int64(1), np.array([2.0]), (2, 4, 10, 3), None, 0.0, 0.1, 0.0, ["N"])
    assert ag is None and L == 4 and want == ("N",)
    assert ok(2, 10, 8, [1.0], (2, 3, 10, 3), np.ones([2, 3, 2]))[1].shape == (2, 3, 3)       # 2D accelerations get z = 0
    for bad in (0, 9, 2.5, True):
        with pytest.raises(ValueError, match="p must"):
            ok(2, 10, bad, [1.0], None, [[1.0, 0.0, 0.0]])
    for bad in ([], [[1.0]], [-1.0], [np.nan], [np.inf, 1.0], 1.0):
        with pytest.raises(ValueError, match="omegas"):
            ok(2, 10, 8, bad, None, [[1.0, 0.0, 0.0]])
    with pytest.raises(ValueError, match="at least one of pattern and accel"):
        ok(2, 10, 8, [1.0])
    for bad in ((2, 3, 10), (3, 3, 10, 3), (2, 3, 11, 3), (2, 3, 10, 4)):
        with pytest.raises(ValueError, match="pattern"):
            ok(2, 10, 8, [1.0], bad)
    for bad in ([1.0, 0.0, 0.0], np.ones([3, 1, 3]), np.ones([2, 4, 3]), np.ones([3, 4]), np.full([3, 3], np.nan)):
        with pytest.raises(ValueError, match="accel"):
            ok(2, 10, 8, [1.0], (2, 3, 10, 3), bad)
    for shape, acc in (((2, 0, 10, 3), None), ((2, 17, 10, 3), None), (None, np.ones([17, 3]))):
        with pytest.raises(ValueError, match="L must"):
            ok(2, 10, 8, [1.0], shape, acc)
    for name in ("damping", "damp_mass", "damp_stiff"):
        for bad in (-0.1, np.nan, np.inf, "0.05", None, [0.05], True):
            with pytest.raises(ValueError, match=name):
                ok(2, 10, 8, [1.0], (2, 3, 10, 3), **{name: bad})
    with pytest.raises(ValueError, match="at least one of damping"):
        ok(2, 10, 8, [1.0], (2, 3, 10, 3), damping=0.0)
    assert ok(2, 10, 8, [1.0], (2, 3, 10, 3), damping=0.0, damp_stiff=1e-3)[2] == 3
    for bad in (("u", "f_ext"), ("frf_u",), "u"):
        with pytest.raises(ValueError, match="want"):
            ok(2, 10, 8, [1.0], (2, 3, 10, 3), want=bad)
    with pytest.raises(ValueError, match="max_result_bytes"):
        ok(2, 10, 8, np.arange(100.0), (2, 3, 10, 3), Pj=4, Pm=1, max_result_bytes=16 * 2 * 3 * 100 * 13 - 1)
    assert ok(2, 10, 8, np.arange(100.0), (2, 3, 10, 3), Pj=4, Pm=1, max_result_bytes=16 * 2 * 3 * 100 * 13)[2] == 3
    # `solve_harmonic` refuses before it asks for a device
    packed = batch.pack_json([H.load_json("bar-25_input_0")] * 2)
    acc = [[1.0, 0.0, 0.0]]
    for kw in (dict(p=9), dict(damping=0.0), dict(damp_mass=-1.0), dict(mass_scale=float("nan")), dict(tol=-1.0),
               dict(joint_mass=np.zeros([2, packed.nJ_max]) - 1.0), dict(monitor_joints=np.array([[99], [0]])),
               dict(monitor_members=np.array([[0.5], [0.0]])), dict(pattern=np.zeros([2, 1, packed.nJ_max + 1, 3]))):
        with pytest.raises(ValueError):
            batch.solve_harmonic(packed, [1.0, 2.0], accel=acc, **kw)
    with pytest.raises(ValueError):
        batch.solve_harmonic(packed, [1.0, -2.0], accel=acc)
    with pytest.raises(ValueError):
        batch.solve_harmonic(packed, [1.0, 2.0])


# ---- the restatement against truths that need no restatement -----------------------------------------------------------
def identities(name):
    """How well the four truths hold for the restatement on a fixture, each error scaled by the largest modulus of its
    quantity: (a) at W = 0, Re = the static solution of f and Im = 0 EXACTLY (asserted), truncated basis, residual on;
    (b) ALL modes, zeta = 0, Rayleigh damping: `response` = the direct complex solve, and u_res vanishes; (c) reciprocity:
    the FRF at DOF i from a unit load at DOF j = the FRF at j from a unit load at i, truncated basis, residual on;
    (d) rotating the two vectors of every repeated pair changes nothing."""
    d, mu = arrays_of(name)
    lam, Phi = pairs_of(name)
    n = len(lam)
    W = sweep_of(name)
    damp = dampings_of(name)
    fs = loads_of(d, mu)
    K_ff, m = G.system(d, mu)
    free = d["free"].ravel()
    out = {"a": 0.0, "b": 0.0, "c": 0.0, "d": 0.0}
    p = modes_of(name, min(P, n))
    for f in fs:
        for pp in sorted({1, min(3, n), p}):
            r = HR.response(d, Phi[:pp], lam[:pp], [0.0], f, *damp["all"], True, mu)
            assert not r["u"].imag.any() and not r["N"].imag.any() and not r["R"].imag.any(), name
            static = np.zeros(free.size)
            static[free] = np.linalg.solve(K_ff, f.reshape(-1)[free])
            sN, sR = HR.forces(d, static.reshape(1, -1, 3))
            out["a"] = max(out["a"], scaled(r["u"].real.ravel(), static), scaled(r["N"].real, sN), scaled(r["R"].real, sR))
        full = HR.response(d, Phi, lam, W, f, 0.0, damp["all"][1], damp["all"][2], True, mu)
        want = HR.direct(d, W, f, damp["all"][1], damp["all"][2], mu)
        no_residual = float(np.abs(full["u_res"]).max() / np.abs(full["u"]).max())
        out["b"] = max([out["b"], no_residual] + [scaled(full[k], want[k]) for k in HR.KEYS])
    dofs = np.flatnonzero(free)
    i, j = int(dofs[0]), int(dofs[-1])
    unit = lambda q: np.eye(1, free.size, q).reshape(-1, 3)
    pp = min(3, n - 1)
    ri = HR.response(d, Phi[:pp], lam[:pp], W, unit(i), *damp["all"], True, mu)["u"].reshape(len(W), -1)
    rj = HR.response(d, Phi[:pp], lam[:pp], W, unit(j), *damp["all"], True, mu)["u"].reshape(len(W), -1)
    out["c"] = float(np.abs(ri[:, j] - rj[:, i]).max() / max(np.abs(ri).max(), np.abs(rj).max()))
    for pair in CLUSTERS.get(name, []):
        assert abs(lam[pair[1]] - lam[pair[0]]) < 1e-9 * lam[pair[0]]
        turned = rotated(Phi[:p], pair, 0.6)
        for f in fs:
            r0 = HR.response(d, Phi[:p], lam[:p], W, f, *damp["all"], True, mu)
            r1 = HR.response(d, turned, lam[:p], W, f, *damp["all"], True, mu)
            out["d"] = max([out["d"]] + [scaled(r1[k], r0[k]) for k in HR.KEYS])
    return out


def tolerances():
    """tests/golden/harmonic_tol.json, as `record_tolerance` wrote it."""
    if "tol" not in _cache:
        with open(TOL_FILE) as fh:
            _cache["tol"] = json.load(fh)
    return _cache["tol"]


def class_bound(n_members, key, floor):
    return max(floor, FACTOR * tolerances()["big" if n_members >= 942 else "small"][key])


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_against_the_four_identities(name):
    got = identities(name)
    print(name, got)
    for key in "abcd":
        bound = FACTOR * tolerances()["identities"][key]
        assert got[key] <= bound, (name, key, got[key], bound)


def test_the_sweep_and_the_cases_are_what_the_issue_sets():
    for name in FIXTURES + [TOL_BIG]:
        W, w = sweep_of(name), frequencies_of(name)
        assert W.shape == (S_TEST,) and S_TEST > 2 * 64 and S_TEST % 64
        assert W[0] == 0.0 and (W >= 0).all() and W.max() == 2 * w[-1] and (np.diff(W) < 0).any()      # any order
        for x in [0.5 * w[0]] + list(w) + list(1.001 * w) + list(0.5 * (w[1:] + w[:-1])):
            assert np.abs(W - x).min() <= 1e-6 * w[-1], (name, x)
        gaps = np.diff(np.sort(W))
        assert (gaps > 1e-6 * w[-1]).all(), name                                  # no two values tie for an envelope
        damp = dampings_of(name)
        assert damp["modal"] == (0.02, 0.0, 0.0) and damp["all"] == (0.02, 0.006 * w[0], 0.02 / w[-1])
    pats, ags = cases_of(arrays_of("bar-25_input_0")[0])
    assert pats[0].any() and not pats[1].any() and pats[2].any() and not ags[0].any() and ags[1].any() and ags[2].any()


@pytest.mark.parametrize("name", FIXTURES + [TOL_BIG])
def test_the_envelope_indices_are_decided_on_the_test_sweep(name):
    """What the GPU test of the envelope indices relies on: on the test sweep the restatement's best amplitude and its
    runner-up differ by more than 2 x bound x scale for at least 90 % of the non-zero entries of every quantity, so the
    device's index must EQUAL the restatement's there.  A condition on the inputs, checked here with the restatement."""
    d, mu = arrays_of(name)
    p = modes_of(name)
    W = sweep_of(name)
    bound = class_bound(len(d["conn"]), "a_float64_against_longdouble", 1e-11)
    for f in loads_of(d, mu):
        r = HR.exact_response(d, p, W, f, mu, zeta=ZETA)
        for key in HR.KEYS:
            share = decided(r[key], bound)[1]
            assert share >= 0.9, (name, key, share)


def decided(y, bound):
    """(mask of the entries whose best and runner-up amplitudes differ by more than 2 x bound x scale, its share of the
    non-zero entries) of complex y [S, ...]."""
    amp = np.abs(y)
    scale = amp.max()
    top = np.sort(amp, axis=0)[-2:]
    mask = (top[1] - top[0]) > 2 * bound * scale
    nonzero = amp.max(0) > 0
    return mask, float((mask & nonzero).sum() / max(1, nonzero.sum()))


# ---- the recorded tolerances ------------------------------------------------------------------------------------------
def measure(name):
    """(a) the scaled float64 - longdouble difference of the restatement on FIXED shapes (eigh's), (b) the scaled
    difference between the restatement on the block iteration's shapes and on eigh's; on the test sweep, the worst over
    the three cases, the two damping configurations and u, N, R (complex: both parts), each scaled by the quantity's
    largest modulus over the sweep."""
    data = H.load_json(name)
    d = G.arrays(data)
    p = modes_of(name)
    lam, Phi = G.eigen_pairs(d, 1.0, p)
    K_ff, m, mask = R.matrices(data)
    it_lam, it_Phi, resid, n_modes, iters = R.block_iteration(K_ff, m, p=P, tol=1e-10, check_every=8)
    assert iters > 0 and n_modes == P
    shapes = np.zeros([p, d["free"].size])
    shapes[:, d["free"].ravel()] = it_Phi.T[:p]
    W = sweep_of(name)
    a = b = 0.0
    for damp in dampings_of(name).values():
        for l in range(L_TEST):
            pats, ags = cases_of(d)
            f64, f80 = HR.load(d, pats[l], ags[l]), HR.load(d, pats[l], ags[l], dtype=np.longdouble)
            r64 = HR.response(d, Phi, lam[:p], W, f64, *damp, True)
            r80 = HR.response(d, Phi, lam[:p], W, f80, *damp, True, dtype=np.longdouble)
            a = max([a] + [scaled(r64[k], r80[k]) for k in HR.KEYS])
            rit = HR.response(d, shapes.reshape(p, -1, 3), it_lam[:p], W, f64, *damp, True)
            b = max([b] + [scaled(rit[k], r64[k]) for k in HR.KEYS])
    return {"truss": name, "modes": p, "iterations": int(iters), "a_float64_against_longdouble": a,
            "b_iteration_against_eigh": b}


def record_tolerance():
    """Writes tests/golden/harmonic_tol.json (a few minutes: the block iteration and longdouble on bar-942 in numpy)."""
    worst = {key: 0.0 for key in "abcd"}
    for name in FIXTURES:
        for key, value in identities(name).items():
            worst[key] = max(worst[key], value)
    rec = {"what": "tests/harmonic_reference.response on tests/test_harmonic's sweep (S = 130 from the truss's own eigh "
                   "frequencies), three cases (a load pattern, a ground acceleration, both), residual on, zeta = 0.02 "
                   "alone and with damp_mass = 0.006 w_1 and damp_stiff = 0.02 / w_p; complex differences scaled by the "
                   "largest modulus of each quantity over the sweep, the worst over the cases, the dampings and u, N, R: "
                   "(a) float64 against longdouble on the shapes of numpy.linalg.eigh; (b) on the shapes of "
                   "tests/modes_reference.block_iteration (p = 8, tol 1e-10, check_every 8) against those of eigh - on "
                   "bar-120 its seven lowest modes (eigenvalue 7 is half of the pair (7, 8)).  The device is allowed "
                   "max(1e-11, 100 x a) against the restatement on its own shapes and max(1e-9, 100 x b) against eigh, of "
                   "its size class.  identities: the worst error over bar-6 ... bar-120 of (a) W = 0: Re = the static "
                   "solution (Im = 0 exactly is asserted), (b) all modes, zeta = 0: the direct complex solve under "
                   "Rayleigh damping, and no residual, (c) reciprocity with a truncated basis and the residual, (d) a "
                   "rotation inside a repeated pair; the tests allow 100 x each",
           "small": measure(TOL_SMALL), "big": measure(TOL_BIG), "identities": worst}
    with open(TOL_FILE, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    return rec


def test_recorded_tolerances_name_their_inputs():
    """The small truss is measured again here; the bar-942 figures (minutes of numpy) are only read."""
    rec = tolerances()
    assert (rec["small"]["truss"], rec["small"]["modes"]) == (TOL_SMALL, 7)
    assert (rec["big"]["truss"], rec["big"]["modes"]) == (TOL_BIG, 8)
    assert "block_iteration" in rec["what"] and "longdouble" in rec["what"] and "eigh" in rec["what"]
    again = measure(TOL_SMALL)
    assert again["iterations"] == rec["small"]["iterations"]
    for key in ("a_float64_against_longdouble", "b_iteration_against_eigh"):
        for size in ("small", "big"):
            assert 0 < rec[size][key] < 1e-7, (size, key)
        assert again[key] <= 10 * rec["small"][key] + 1e-15, key
    assert sorted(rec["identities"]) == list("abcd") and all(0 < rec["identities"][k] < 1e-10 for k in "abcd")


if __name__ == "__main__":
    print(json.dumps(record_tolerance(), indent=1))
