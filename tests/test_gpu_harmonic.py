"""Harmonic response analysis on the GPU (`DeviceBatch.harmonic`, `solve_harmonic`, `Truss.HarmonicResponse`; C ABI
include/trs_harmonic.h) against the numpy restatement of `tests/harmonic_reference.py`: on the device's own shapes
(kernel parity), on `eigh`'s and against the direct complex solve (truth), by the identities that need no reference, and
bit for bit where the interface promises bits.

The parity bound is max(1e-11, 100 x a) of the size class (tests/golden/harmonic_tol.json), entry by entry, scaled by
the largest modulus of the quantity over the sweep; the truth bound max(1e-9, 100 x b); an identity gets 100 x what the
restatement itself reaches (tests/test_harmonic.py)."""
import os

import numpy as np
import pytest

from tests import harmonic_reference as HR
from tests import helpers as H
from tests import mode_gradients_reference as G
from tests.test_gpu_mode_gradients import CONFIGS, RAGGED, RAGGED_SCALE, Run, ragged_masses, run_of
from tests.test_gpu_spectrum import truth_run
from tests.test_harmonic import (FACTOR, L_TEST, P, ZETA, cases_of, class_bound, dampings_from, decided, sweep_from,
                                 tolerances)
from tests.test_spectrum import DIRS, PERIODS, ACCEL

pytestmark = pytest.mark.gpu
SINGLE = [n for n in H.data_case_names() if n.endswith("_input_0")]
BIG = "bar-942_input_0"
AMPS = ("u_amp", "N_amp", "R_amp")


def frequencies(run):
    """The p lowest circular frequencies of the run's FIRST truss from `eigh`: what its sweep and dampings are built on."""
    if not hasattr(run, "_hr_w"):
        run._hr_w = np.sqrt(G.eigen_pairs(run.arrays[0], run.mass_scale, P)[0][:P])
    return run._hr_w


def inputs(run, L=L_TEST):
    """(patterns [B, L, nJ_max, 3], accelerations [B, L, 3]) of the test cases of every truss of a run (zeros for none)."""
    B, nJ_max = len(run.arrays), run.packed.nJ_max
    pat, ag = np.zeros([B, L_TEST, nJ_max, 3]), np.zeros([B, L_TEST, 3])
    for b, d in enumerate(run.arrays):
        pat[b, :, :len(d["xyz"])], ag[b] = cases_of(d, run.mass_scale)
    return pat[:, :L], ag[:, :L]


def monitors(run):
    """Caller's ids [B, 3] of each truss: its first joint with a free DOF, its last joint and none; members 0, last, none."""
    mj = np.array([[int(np.flatnonzero(d["free"].any(1))[0]), len(d["xyz"]) - 1, -1] for d in run.arrays], dtype=np.int32)
    mm = np.array([[0, len(d["conn"]) - 1, -1] for d in run.arrays], dtype=np.int32)
    return mj, mm


def harmonic(run, W, damp, residual=True, pat=None, ag=None, mon=True, **kw):
    """`harmonic` of a run with the tests' cases (or others), as host arrays."""
    import torch
    dev = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    if pat is None and ag is None:
        pat, ag = inputs(run)
    mj, mm = monitors(run) if mon is True else mon if mon else (None, None)
    out = run.db.harmonic(W, pattern=dev(pat), accel=ag, damping=damp[0], damp_mass=damp[1], damp_stiff=damp[2],
                          residual=residual, monitor_joints=dev(mj), monitor_members=dev(mm), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


_restated = {}


def restated(run, b, l, W, damp, residual, pat=None, ag=None):
    """The restatement of case l of truss b on the device's OWN shapes and eigenvalues, once per set of inputs."""
    d = run.arrays[b]
    nJ = len(d["xyz"])
    if pat is None and ag is None:
        pat, ag = inputs(run)
    phi, lam = np.ascontiguousarray(run.phi[b, :, :nJ]), run.lam[b]
    f = HR.load(d, None if pat is None else pat[b, l], None if ag is None else ag[b, l], run.mass_scale)
    key = (phi.tobytes(), lam.tobytes(), W.tobytes(), f.tobytes(), damp, residual, run.mass_scale)
    if key not in _restated:
        _restated[key] = HR.response(d, phi, lam, W, f, *damp, residual, run.mass_scale)
    return _restated[key]


def cut(out, b, l, key, d):
    """Case l of truss b of an envelope output, trimmed to the truss's own joints / members."""
    return out[key][b, l, :len(d["conn"])] if key[0] == "N" else out[key][b, l, :len(d["xyz"])]


def assert_entries(what, got, want, scale, bound):
    """Entry by entry |got - want| <= bound x scale, both parts of a complex value; prints the worst."""
    err = np.maximum(np.abs(np.real(got) - np.real(want)), np.abs(np.imag(got) - np.imag(want))) / (scale if scale > 0 else 1.0)
    worst = float(err.max()) if err.size else 0.0
    print(f"{what}: {worst:.2e} (bound {bound:.1e})")
    assert worst <= bound, (what, worst, bound)


def check_against(run, what, out, wants, tol_key, floor, indices=True):
    """The outputs of one call against `wants[b][l]` (a response of the restatement), within the bound of each truss's
    size class (`class_bound(., tol_key, floor)`): the envelopes and the monitored complex values entry by entry, and the
    envelope indices: the reference's amplitude AT the device's index within the bound of the reference's peak, the index
    EQUAL wherever best and runner-up differ by more than 2 x bound x scale."""
    mj, mm = monitors(run)
    for b, d in enumerate(run.arrays):
        bound = class_bound(len(d["conn"]), tol_key, floor)
        for l in range(out["g"].shape[1]):
            want = wants[b][l]
            for key in HR.KEYS:
                scale = float(np.abs(want[key]).max())
                got = cut(out, b, l, key + "_amp", d)
                assert_entries(f"{what} truss {b} case {l} {key}_amp", got, want[key + "_amp"], scale, bound)
                at = cut(out, b, l, key + "_at", d).astype(np.int64)
                amp = np.abs(want[key])
                there = np.take_along_axis(amp, at[None], axis=0)[0]
                assert (want[key + "_amp"] - there <= bound * scale).all(), (what, b, l, key)
                if indices:
                    mask, share = decided(want[key], bound)
                    assert (at[mask] == want[key + "_at"][mask]).all(), (what, b, l, key)
                    assert share >= 0.9, (what, b, l, key, share)
            if "frf_u" in out:
                for i, j in enumerate(mj[b]):
                    ref = want["u"][:, j] if j >= 0 else np.zeros([len(want["u"]), 3])
                    assert_entries(f"{what} truss {b} case {l} frf_u {i}", out["frf_u"][b, l, :, i], ref,
                                   float(np.abs(want["u"]).max()), bound)
                for i, m in enumerate(mm[b]):
                    ref = want["N"][:, m] if m >= 0 else np.zeros(len(want["N"]))
                    assert_entries(f"{what} truss {b} case {l} frf_N {i}", out["frf_N"][b, l, :, i], ref,
                                   float(np.abs(want["N"]).max()), bound)


def check_parity(run, what, W=None, configs=("modal", "all"), residuals=(True, False)):
    W = sweep_from(frequencies(run)) if W is None else W
    for name in configs:
        damp = dampings_from(frequencies(run))[name]
        for residual in residuals:
            out = harmonic(run, W, damp, residual)
            np.testing.assert_array_equal(out["n_modes"], run.n_modes)
            wants = [[restated(run, b, l, W, damp, residual) for l in range(L_TEST)] for b in range(len(run.arrays))]
            for b, d in enumerate(run.arrays):
                bound = class_bound(len(d["conn"]), "a_float64_against_longdouble", 1e-11)
                n = int(run.n_modes[b])
                gs = np.array([wants[b][l]["g"] for l in range(L_TEST)])
                # (g up to its sign, which is that of the shape: `modes()` hands out phi with its largest component
                # positive, the block X keeps the sign the iteration left; every response carries g phi, where it cancels)
                assert_entries(f"{what} {name} residual={residual} truss {b} g", np.abs(out["g"][b][:, :n]),
                               np.abs(gs[:, :n]), float(np.abs(gs).max()), bound)
                assert not out["g"][b][:, n:].any()
            check_against(run, f"{what} {name} residual={residual}", out, wants, "a_float64_against_longdouble", 1e-11,
                          indices=len(W) > 3)


# ---- kernel parity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["general", "table"])
def test_parity_of_every_fixture(config):
    """bar-6 has 5 free DOFs < p (n_modes < p, NaN eigenvalues), bar-10 exactly 8; bar-942 once."""
    for name in SINGLE:
        if name != BIG or config == "general":
            check_parity(run_of(name, config), f"{name} [{config}]")


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_parity_of_the_ragged_batch(config):
    """bar-6, bar-25, bar-72 and two cube-7 cases in one padded batch, with joint masses and mass_scale = 0.5; the sweep
    is that of the first truss."""
    run = run_of("ragged", config)
    assert run.packed.nJ_max > min(len(d["joint"]) for d in run.datas)
    check_parity(run, f"ragged [{config}]")


def test_parity_of_a_truss_of_more_than_256_joints():
    """Two copies of bar-942 in one truss (test_gpu_spectrum): 488 joints, 1884 members - every stride loop strides; S = 3."""
    base = H.load_json(BIG)
    nJ = len(base["joint"])
    data = {"joint": base["joint"] + base["joint"], "force": base["force"],
            "member": base["member"] + [[[j0 + nJ, j1 + nJ], [a, 1.3 * e, rho]] for (j0, j1), (a, e, rho) in base["member"]]}
    run = Run([data])
    assert run.packed.nJ_max == 488 > 256 and run.packed.nM_max == 1884
    check_parity(run, "bar-942 twice", W=sweep_from(frequencies(run), 3), configs=("all",), residuals=(True,))


# ---- truth -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SINGLE)
def test_truth_against_eigh(name):
    run = truth_run(name)
    d = run.arrays[0]
    W, damp = sweep_from(frequencies(run)), dampings_from(frequencies(run))["all"]
    out = harmonic(run, W, damp)
    pat, ag = inputs(run)
    wants = [[HR.exact_response(d, run.p, W, HR.load(d, pat[0, l], ag[0, l]), 1.0, zeta=damp[0], damp_mass=damp[1],
                                damp_stiff=damp[2]) for l in range(L_TEST)]]
    check_against(run, f"{name} truth", out, wants, "b_iteration_against_eigh", 1e-9, indices=False)


@pytest.mark.parametrize("name", ["bar-6_input_0", "bar-10_input_0"])
def test_truth_against_the_direct_complex_solve(name):
    """p = 8 covers every free DOF of bar-6 (5) and bar-10 (8): with Rayleigh damping alone the modal answer IS the
    solution of (K - W^2 M + i W (alpha M + beta K)) U = f, and residual on and off agree."""
    run = run_of(name)
    d = run.arrays[0]
    assert int(run.n_modes[0]) == int(d["free"].sum()) <= P
    W, (_, alpha, beta) = sweep_from(frequencies(run)), dampings_from(frequencies(run))["all"]
    pat, ag = inputs(run)
    wants = [[HR.direct(d, W, HR.load(d, pat[0, l], ag[0, l]), alpha, beta) for l in range(L_TEST)]]
    on, off = harmonic(run, W, (0.0, alpha, beta), True), harmonic(run, W, (0.0, alpha, beta), False)
    check_against(run, f"{name} direct", on, wants, "b_iteration_against_eigh", 1e-9, indices=False)
    check_against(run, f"{name} direct, no residual", off, wants, "b_iteration_against_eigh", 1e-9, indices=False)


# ---- the identities on the device's numbers ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ragged", "bar-47_input_0"])
def test_the_static_limit_and_reciprocity(kind):
    """At W = 0 with the residual on, Im is exactly 0 and the amplitude is |the static answer| of `solve_cases` - another
    kernel family on the same factor; reciprocity from two unit-load cases and two monitored joints.

    Both are identities of EXACT eigenpairs: with a truncated basis the residual flexibility inv(K) (I - M X X^T) is
    symmetric only as far as K X = M X lam holds, and the asymmetry is about 1.5e-3 of the pairs' residual.  The restatement
    on bar-72 of the ragged batch: 2e-17 on `eigh`'s pairs, 1.1e-14 on `modes_reference.block_iteration`'s (residual 7e-12).
    The device's block at the default tol = 1e-10 gave 1.3e-13 there on the MI355X, above 100 x the recorded identity
    (6e-14), while bar-6 (all modes) and bar-25 gave 1.2e-17 and 1.5e-17: the shapes, not the sweep kernel.  The modes of
    this test are therefore iterated to tol = 1e-12, which asks as much of `harmonic` and no less of the identity."""
    import torch
    if kind == "ragged":
        datas, jm = ragged_masses()
        run = Run(datas, joint_mass=jm, mass_scale=RAGGED_SCALE, reorder="device")
    else:
        run = Run([H.load_json(kind)], reorder="device")
    tight = run.db.modes(P, tol=1e-12, joint_mass=run.jm, mass_scale=run.mass_scale)
    assert bool((tight["iters"] > 0).all())                                      # converged at the tighter tolerance
    damp = dampings_from(frequencies(run))["all"]
    W = sweep_from(frequencies(run))
    assert W[0] == 0.0
    out = harmonic(run, W, damp)
    assert not out["frf_u"][:, :, 0].imag.any() and not out["frf_N"][:, :, 0].imag.any()
    assert out["frf_u"][:, :, 1:].imag.any()
    # reciprocity: unit loads at a free DOF of two joints, the same two joints monitored
    B, nJ_max = len(run.arrays), run.packed.nJ_max
    pat, mj, axes = np.zeros([B, 2, nJ_max, 3]), np.zeros([B, 2], dtype=np.int32), np.zeros([B, 2], dtype=np.int64)
    for b, d in enumerate(run.arrays):
        dofs = np.argwhere(d["free"])
        (mj[b, 0], axes[b, 0]), (mj[b, 1], axes[b, 1]) = dofs[0], dofs[-1]
        pat[b, 0, mj[b, 0], axes[b, 0]] = pat[b, 1, mj[b, 1], axes[b, 1]] = 1.0
    rec = harmonic(run, W, damp, pat=pat, mon=(mj, None))["frf_u"]
    bound = FACTOR * tolerances()["identities"]["c"]
    for b in range(B):
        ij, ji = rec[b, 1, :, 0, axes[b, 0]], rec[b, 0, :, 1, axes[b, 1]]        # at i from the load at j, and the reverse
        diff = float(np.abs(ij - ji).max() / np.abs(rec[b]).max())
        print(f"{kind} truss {b} reciprocity: {diff:.2e} (bound {bound:.1e})")
        assert diff <= bound, (kind, b, diff, bound)
    # the one-point sweep W = 0 against the static solve
    pats, ags = inputs(run)
    one = harmonic(run, np.array([0.0]), damp, mon=False)
    loads = np.zeros([B, L_TEST, nJ_max, 3])
    for b, d in enumerate(run.arrays):
        for l in range(L_TEST):
            loads[b, l, :len(d["xyz"])] = HR.load(d, pats[b, l], ags[b, l], run.mass_scale)
    static = run.db.solve_cases(torch.from_numpy(loads).to("cuda:0"))      # (bumps the generation)
    static = {k: v.cpu().numpy() for k, v in static.items()}
    bound = FACTOR * tolerances()["identities"]["a"]
    for b in range(B):
        for l in range(L_TEST):
            for key, ref in (("u_amp", static["u"]), ("N_amp", static["N"])):
                diff = np.abs(one[key][b, l] - np.abs(ref[b, l])).max() / np.abs(ref[b, l]).max()
                print(f"{kind} truss {b} case {l} {key} against solve_cases: {diff:.2e} (bound {bound:.1e})")
                assert diff <= bound, (kind, b, l, key, diff, bound)
    assert not one["u_at"].any() and not one["N_at"].any() and not one["R_at"].any()
    with pytest.raises(ValueError, match="stale"):
        run.db.harmonic(W, accel=[[1.0, 0.0, 0.0]])


# ---- bits --------------------------------------------------------------------------------------------------------------
def assert_same(a, b, what):
    assert sorted(a) == sorted(b)
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=f"{what} {key}")


def standard(run, **kw):
    return harmonic(run, sweep_from(frequencies(run)), dampings_from(frequencies(run))["all"], **kw)


@pytest.mark.parametrize("kind", ["ragged", BIG, "bar-47_input_0"])
def test_the_general_form_equals_the_table_form(kind):
    for reorder in ("", "-reorder"):
        for residual in (True, False):
            assert_same(standard(run_of(kind, "general" + reorder), residual=residual),
                        standard(run_of(kind, "table" + reorder), residual=residual), f"{kind}{reorder}")


@pytest.mark.parametrize("config", ["general", "general-reorder"])
def test_a_truss_alone_and_a_case_alone(config):
    """A truss alone = the truss in the ragged batch; case l alone = case l among L = 5."""
    run = run_of("ragged", config)
    W, damp = sweep_from(frequencies(run)), dampings_from(frequencies(run))["all"]
    whole = harmonic(run, W, damp)
    datas, jm = ragged_masses()
    for b in (0, 2, 4):
        d = run.arrays[b]
        nJ = len(datas[b]["joint"])
        alone = Run([datas[b]], joint_mass=jm[b:b + 1, :nJ], mass_scale=RAGGED_SCALE, **CONFIGS[config])
        mine = harmonic(alone, W, damp)
        for key in ("u_amp", "u_at", "N_amp", "N_at", "R_amp", "R_at"):
            n = len(d["conn"]) if key[0] == "N" else nJ
            np.testing.assert_array_equal(mine[key][0][:, :n], whole[key][b][:, :n], err_msg=f"truss {b} {key}")
        for key in ("frf_u", "frf_N", "g"):
            np.testing.assert_array_equal(mine[key][0], whole[key][b], err_msg=f"truss {b} {key}")
    pat, ag = inputs(run)
    five = lambda x: np.concatenate([x[:, 1:2], x[:, :1], x], axis=1)       # the cases 1, 0, 0, 1, 2 of the three
    among = harmonic(run, W, damp, pat=five(pat), ag=five(ag))
    assert among["g"].shape[1] == 5
    for key in whole:
        if key != "n_modes":
            np.testing.assert_array_equal(among[key][:, 2:5], whole[key], err_msg=key)
            np.testing.assert_array_equal(among[key][:, 0], whole[key][:, 1], err_msg=key)
    single = harmonic(run, W, damp, pat=pat[:, 1:2], ag=ag[:, 1:2])
    for key in whole:
        if key != "n_modes":
            np.testing.assert_array_equal(single[key][:, 0], whole[key][:, 1], err_msg=key)


def test_repeats_streams_and_the_other_analyses_afterwards():
    """A second call gives the first one's bits, a call on a side stream those of the current stream, and
    `mode_gradients` and `response_spectrum` the same bits before and after: nothing they read is touched, nothing is
    bumped.  A narrow `want` gives the same bits and no other key.  At the envelope's index the monitored (Re, Im) give
    the envelope's amplitude through sqrt(fma(.)): the kernel shares one function between them."""
    import torch
    run = run_of("ragged", "table-reorder")
    spectrum = lambda: {k: v.cpu().numpy() for k, v in run.db.response_spectrum(DIRS, PERIODS, ACCEL).items()}
    before, before_rs = run.gradients(), spectrum()
    seen = run.db.generation
    first = standard(run)
    assert run.db.generation == seen
    assert_same(first, standard(run, generation=seen), "second call")
    assert_same(before, run.gradients(), "mode_gradients")
    assert_same(before_rs, spectrum(), "response_spectrum")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        got = standard(run)
    assert_same(first, got, "side stream")
    only = standard(run, want=("N",), mon=False)
    assert sorted(only) == ["N_amp", "N_at", "g", "n_modes"]
    np.testing.assert_array_equal(only["N_amp"], first["N_amp"])
    np.testing.assert_array_equal(only["N_at"], first["N_at"])
    # the monitors and the envelopes are the same numbers
    mj, mm = monitors(run)
    checked = 0
    for b in range(len(run.arrays)):
        for l in range(L_TEST):
            for i, m in enumerate(mm[b][:2]):
                z = first["frf_N"][b, l, first["N_at"][b, l, m], i]
                re, im = np.longdouble(z.real), np.longdouble(z.imag)
                amp = float(np.sqrt(re * re + im * im))
                assert abs(amp - first["N_amp"][b, l, m]) <= 2 * np.spacing(first["N_amp"][b, l, m]), (b, l, m)
                assert np.abs(first["frf_N"][b, l, :, i]).max() <= first["N_amp"][b, l, m] * (1 + 4e-16)
                checked += 1
            for i, j in enumerate(mj[b][:2]):
                for a in range(3):
                    z = first["frf_u"][b, l, first["u_at"][b, l, j, a], i, a]
                    re, im = np.longdouble(z.real), np.longdouble(z.imag)
                    amp = float(np.sqrt(re * re + im * im))
                    assert abs(amp - first["u_amp"][b, l, j, a]) <= 2 * np.spacing(first["u_amp"][b, l, j, a]), (b, l, j, a)
                    checked += 1
    assert checked == len(run.arrays) * L_TEST * 8


# ---- zeros, NaN and padding --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["general", "table-reorder"])
def test_zeros_under_poisoned_outputs(config):
    """Every entry is written: padding joints and members, held DOFs of u, free DOFs of R, the monitor -1 and the modes
    k >= n_modes of g (bar-6: five) - under `out` tensors full of NaN (indices: full of -7)."""
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    run = run_of("ragged", config)
    b6 = RAGGED.index("bar-6_input_0")
    assert int(run.n_modes[b6]) == 5 and np.isnan(run.lam[b6, 5:]).all()
    W = sweep_from(frequencies(run))
    for residual in (True, False):
        shapes = batch._field_shapes(batch.HarmonicResult.FIELDS, run.db.B,
                                     run.db._sizes(P=P, L=L_TEST, S=len(W), Pj=3, Pm=3),
                                     ("u_amp", "u_at", "N_amp", "N_at", "R_amp", "R_at", "frf_u", "frf_N"))
        shapes["g"] = ([run.db.B, L_TEST, P], torch.float64)   # (the modal loads: no field of the result)
        poison = {k: torch.full(shape, float("nan") if dtype == torch.float64 else -7, dtype=dtype, device="cuda:0")
                  for k, (shape, dtype) in shapes.items()}
        out = standard(run, residual=residual, out=poison)
        for key, x in out.items():
            assert np.isfinite(x).all(), (residual, key)                         # no NaN anywhere, healthy trusses
        assert not out["g"][b6, :, 5:].any() and out["g"][b6, :, :5].any()
        assert not out["frf_u"][:, :, :, 2].any() and not out["frf_N"][:, :, :, 2].any()        # the monitor -1
        assert out["frf_u"][:, :, :, :2].any() and out["frf_N"][:, :, :, :2].any()
        for b, d in enumerate(run.arrays):
            nJ, nM = len(d["xyz"]), len(d["conn"])
            for tail in ("_amp", "_at"):
                assert not out["u" + tail][b, :, nJ:].any() and not out["R" + tail][b, :, nJ:].any()
                assert not out["N" + tail][b, :, nM:].any()
                assert not out["u" + tail][b, :, :nJ][:, ~d["free"]].any()
                assert not out["R" + tail][b, :, :nJ][:, d["free"]].any()
            assert out["u_amp"][b].any() and out["R_amp"][b].any() and out["N_amp"][b].any()
        for key in AMPS:
            assert (out[key] >= 0).all()
        for key in ("u_at", "N_at", "R_at"):
            assert (out[key] >= 0).all() and (out[key] < len(W)).all() and out[key].any()


# ---- guards ------------------------------------------------------------------------------------------------------------
def test_guards_of_the_resident_state():
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    from python_stable_3d_truss_analysis_amd.utils import HipExtensionError
    data = H.load_json("bar-25_input_0")
    packed = batch.pack_json([data] * 2)
    db = batch.DeviceBatch(packed, "cuda:0", use_small=False)
    acc = [[1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    call = lambda **kw: db.harmonic([0.0, 5.0, 9.0], accel=acc, **kw)
    with pytest.raises(ValueError, match="no modes"):
        call()
    db.factor()
    with pytest.raises(ValueError, match="no modes"):
        call()
    db.modes(4)
    seen = db.generation
    out = call(generation=seen)
    assert db.generation == seen                                                     # nothing is bumped
    assert sorted(out) == ["N_amp", "N_at", "R_amp", "R_at", "g", "n_modes", "u_amp", "u_at"]
    assert list(out["u_amp"].shape) == [2, 2, packed.nJ_max, 3] and list(out["g"].shape) == [2, 2, 4]
    assert out["u_at"].dtype == torch.int32
    again = call(out=out)                                                            # and the call can be repeated
    assert again["u_amp"] is out["u_amp"]
    mon = torch.tensor([[0, 3], [-1, 2]], dtype=torch.int32, device="cuda:0")
    frf = call(monitor_joints=mon, monitor_members=mon[:, :1], want=())
    assert sorted(frf) == ["frf_N", "frf_u", "g", "n_modes"]
    assert frf["frf_u"].dtype == torch.complex128 and list(frf["frf_u"].shape) == [2, 2, 3, 2, 3]
    assert list(frf["frf_N"].shape) == [2, 2, 3, 1]
    back = call(monitor_joints=mon, monitor_members=mon[:, :1], want=(), out=frf)      # the complex views come back
    assert back["frf_u"].data_ptr() == frf["frf_u"].data_ptr()
    for kw, match in ((dict(damping=0.0), "at least one of damping"), (dict(damp_mass=-1.0), "damp_mass"),
                      (dict(want=("f_ext",)), "want"), (dict(generation=seen - 1), "stale"),
                      (dict(monitor_joints=mon, max_result_bytes=10), "max_result_bytes"),
                      (dict(out={"u_amp": torch.zeros([2, 2, packed.nJ_max, 3], dtype=torch.float32, device="cuda:0")}), "out"),
                      (dict(out={"N_at": torch.zeros([2, 2, packed.nM_max], dtype=torch.int32)}), "out")):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    with pytest.raises(ValueError, match="omegas"):
        db.harmonic([-1.0], accel=acc)
    with pytest.raises(ValueError, match="at least one of pattern"):
        db.harmonic([1.0])
    db.factor()
    with pytest.raises(ValueError, match="stale"):
        call()
    db.modes(4)
    call()
    db.solve_cases(torch.zeros([2, 1, packed.nJ_max, 3], dtype=torch.float64, device="cuda:0"))
    with pytest.raises(ValueError, match="stale"):
        call()
    # a shape whose vectors do not fit the LDS is refused by name: three copies of bar-942 in one truss (moduli x 1, 1.3,
    # 1.7: a simple spectrum), 732 joints - nine vectors take 190 KB
    base = H.load_json(BIG)
    nJ = len(base["joint"])
    data = {"joint": base["joint"] * 3, "force": base["force"],
            "member": [[[j0 + c * nJ, j1 + c * nJ], [a, f * e, rho]] for c, f in enumerate((1.0, 1.3, 1.7))
                       for (j0, j1), (a, e, rho) in base["member"]]}
    big = batch.DeviceBatch(batch.pack_json([data]), "cuda:0", use_small=False)
    assert big.lib.trs_hr_fits(big.nJ_max, big.nM_max, 8) == 0 and big.lib.trs_hr_fits(big.nJ_max, big.nM_max, 1) == 1
    big.factor()
    big.modes(8)
    with pytest.raises(HipExtensionError, match="trs_hr_fits"):
        big.harmonic([1.0], accel=acc)
    big.modes(1)
    assert bool(big.harmonic([1.0], accel=acc)["N_amp"].isfinite().all())


# ---- the drivers above the resident batch -----------------------------------------------------------------------------
def test_solve_harmonic_and_the_truss_method():
    from python_stable_3d_truss_analysis_amd import Truss, batch
    from oracle import truss_oracle as orc
    run = run_of("ragged", "general")
    W, damp = sweep_from(frequencies(run)), dampings_from(frequencies(run))["all"]
    want = harmonic(run, W, damp)
    datas, jm = ragged_masses()
    pat, ag = inputs(run)
    mj, mm = monitors(run)
    res = batch.solve_harmonic(batch.pack_json(datas), W, pattern=pat, accel=ag, p=P, damping=damp[0], damp_mass=damp[1],
                               damp_stiff=damp[2], joint_mass=jm, mass_scale=RAGGED_SCALE, monitor_joints=mj,
                               monitor_members=mm)
    np.testing.assert_array_equal(res.eigenvalue, run.lam)
    np.testing.assert_array_equal(res.omega, np.sqrt(run.lam))
    np.testing.assert_array_equal(res.n_modes, run.n_modes)
    assert (res.info == 0).all() and (res.iters > 0).all()
    fields = {"u_amp": res.displace, "N_amp": res.force, "R_amp": res.reaction, "u_at": res.displace_at,
              "N_at": res.force_at, "R_at": res.reaction_at, "frf_u": res.frf_displace, "frf_N": res.frf_force}
    for key, got in fields.items():
        np.testing.assert_array_equal(got, want[key], err_msg=key)               # the buckets trim; the bits stay
    np.testing.assert_array_equal(res.force_omega, W[want["N_at"]])
    np.testing.assert_array_equal(res.displace_omega, W[want["u_at"]])
    np.testing.assert_array_equal(res.reaction_omega, W[want["R_at"]])
    # two size buckets, results left on the device
    import torch
    from python_stable_3d_truss_analysis_amd.batch import size_buckets
    mixed = batch.pack_json(datas + [H.load_json(BIG)])
    assert len(list(size_buckets(mixed, 64 << 30))) >= 2
    dev = batch.solve_harmonic(mixed, W[:5], accel=[[1.0, 0.0, 0.0]], p=4, residual=False, on_device=True)
    assert isinstance(dev.force, torch.Tensor) and dev.force.is_cuda and list(dev.frf_force.shape) == [6, 1, 5, 0]
    assert list(dev.force.shape) == [6, 1, mixed.nM_max] and (dev.info == 0).all() and bool(dev.force[5].any())
    one = batch.solve_harmonic(batch.pack_json([H.load_json(BIG)]), W[:5], accel=[[1.0, 0.0, 0.0]], p=4, residual=False)
    np.testing.assert_array_equal(dev.force[5].cpu().numpy(), one.force[0])
    # the model's method, in the truss's own ids, against the restatement on eigh's shapes
    name = "bar-25_input_0"
    data = H.load_json(name)
    truss = Truss(orc.truss_dim(data)).LoadFromJSON(os.path.join(H.GOLDEN, "data", name + ".json"))
    before = truss.Serialize()
    d = G.arrays(data)
    w = np.sqrt(G.eigen_pairs(d, 1.0, 6)[0][:6])
    Wt = sweep_from(w, 40)
    out = truss.HarmonicResponse(Wt, nModes=6, damping=ZETA, monitorJoints=[0, 1], monitorMembers=[3])
    assert truss.Serialize() == before
    assert sorted(out) == sorted(["eigenvalue", "omega", "frf_displace", "frf_force"]
                                 + [k + t for k in ("displace", "force", "reaction") for t in ("", "_at", "_omega")])
    own = np.zeros([len(d["xyz"]), 3])
    for j, vec in truss._loads.items():
        own[j, :len(vec)] = vec
    ref = HR.exact_response(d, 6, Wt, HR.load(d, own), zeta=ZETA)
    bound = class_bound(len(d["conn"]), "b_iteration_against_eigh", 1e-9)
    for mine, key in (("displace", "u"), ("force", "N"), ("reaction", "R")):
        assert out[mine].shape == (1,) + ref[key + "_amp"].shape, mine
        assert G.scaled_difference(out[mine][0], ref[key + "_amp"]) <= bound, mine
    assert np.abs(out["frf_displace"][0, :, 1] - ref["u"][:, 1]).max() <= bound * np.abs(ref["u"]).max()
    assert np.abs(out["frf_force"][0, :, 0] - ref["N"][:, 3]).max() <= bound * np.abs(ref["N"]).max()
    np.testing.assert_array_equal(out["force_omega"], Wt[out["force_at"]])
    masses = {j: 2.0 + j for j in range(0, len(data["joint"]), 3)}
    out2 = truss.HarmonicResponse(Wt[:4], loads=[{0: [1.0, 0.0, 0.0]}, {1: [0.0, 2.0, 0.0]}], accel=[[0.0, 0.0, 1.0]] * 2,
                                  nModes=3, damping=0.0, dampStiff=1e-4, residual=False, jointMasses=masses, massScale=0.5)
    assert out2["force"].shape == (2, len(data["member"])) and "frf_force" not in out2
    assert np.isfinite(out2["force"]).all() and out2["force"].any()
