"""The resident-factor analyses (`solve_load_cases`, `solve_effect_cases`, `solve_gradients`, `solve_modes`,
`solve_buckling`, `solve_transient`, `solve_nonlinear`, `solve_mode_gradients`, `solve_response_spectrum`, `solve_harmonic`,
`solve_sizing`, `solve_min_compliance`, `solve_unilateral`, `solve_plastic` and the three on the columns
inv(K_ff) b_e: `solve_member_loss`, `solve_member_sets`, `solve_influence`) give the SAME BITS as the
build that recorded `tests/golden/analysis_bits.json`: SHA-256 digests of every field (that is not None) of the result
dataclasses, for both member forms and with and without a joint order.  The kernels use no floating-point
atomics, so the digests are stable from run to run; they are promised per compiler only, so the fixture names the stack
that recorded it and the tests skip on any other.  A change that is meant to keep the bits is checked by recording at
the commit before it and running the tests after it:

    python -m tests.test_gpu_analysis_bits --record
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H

FIXTURE = os.path.join(H.GOLDEN, "analysis_bits.json")
# one ragged batch: a truss with a roller (a constrained joint that keeps free DOFs: bar-6), 2D trusses (bar-10,
# bar-47), 3D ones, and bar-942, which the size buckets keep apart from the small ones; every truss once
NAMES = ["bar-6_input_0", "bar-10_input_0", "bar-25_input_0", "bar-47_input_0", "bar-72_input_0", "bar-120_input_0",
         "bar-942_input_0"]
L, P = 17, 3   # two case groups of the substitution (16 + 1); three modes
CONFIGS = {"general": dict(table=False, reorder=False), "general-profile": dict(table=False, reorder="profile"),
           "table": dict(table=True, reorder=False), "table-profile": dict(table=True, reorder="profile")}
ANALYSES = ("load_cases", "effect_cases", "gradients", "modes", "buckling", "member_loss", "member_sets", "influence",
            "transient", "nonlinear", "mode_gradients", "response_spectrum", "harmonic", "sizing", "min_compliance",
            "unilateral", "plastic")
# the three iterated analyses beside the sizing run on batches of their own, whose yardstick answers the CPU suites hold:
# every status and count below is an integer the yardstick decides with a margin (tests/test_unilateral.py,
# tests/test_plastic.py) or that tests/golden/compliance_tol.json records (tests/test_compliance.py forms it again), and
# no truss ends with status 2 (which would only hash the fallback).  Each has a ragged batch bar-6 .. bar-120 and bar-942
# alone: unilateral the runs "slack" and "big" of tests/unilateral_reference.py (slack factor 1e-3), plastic the runs
# "hardening" and "big" of tests/plastic_reference.py, compliance the configuration "weighted" resized to tol 1e-4 within
# 60 iterations (compliance_reference.FULL).
OWN_BATCH = ("min_compliance", "unilateral", "plastic")
UN_RUNS, PL_RUNS = ("slack", "big"), ("hardening", "big")
# the transient response: two excitations (the first two load cases as patterns), five Newmark steps, stiffness
# damping (so the end lists of the members are built), two monitored joints and two monitored members (first and last)
L_DYN, STEPS, DT, DAMP_STIFF = 2, 5, 1e-3, 1e-4
# the nonlinear statics: two load steps of the trusses' own loads.  (0.5, 1.0) halved until every truss converged in both
# steps at the commit that recorded the fixture: down to (1/32, 1/16) bar-942's tangent lost definiteness in the first
# step, at (1/64, 1/32) in the second.  At this pair that commit took, per truss in NAMES' order and per step,
# (2, 2), (3, 3), (2, 2), (2, 2), (2, 2), (2, 2), (11, 7) Newton iterations, in all four configs.
NL_FACTORS = (1.0 / 128, 1.0 / 64)
# the column analyses: nine cases are two uneven passes of their apply kernels (8 at most per pass: 5 + 4); chunk 48
# leaves a partial last range of members; 40 scenarios are two slices of 32, the second partial; the path is the first
# twelve joints and back to joint 0
L_COL, CHUNK, S_SETS, P_PATH = 9, 48, 40, 12
# the response spectrum: two ground directions (x and y: the 2D trusses have no z) and a five-point table of periods
RS_DIRS = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
RS_PERIODS = [0.0, 0.02, 0.1, 0.5, 2.0]
# the harmonic response: two cases (the first two load cases as patterns, the first two accelerations as ground motion)
# over 70 forcing frequencies - two chunks of the sweep's table of 64, the second partial - with all three dampings
L_HR, HR_OMEGAS, HR_DAMPING = 2, np.linspace(0.0, 2000.0, 70), dict(damping=0.02, damp_mass=0.5, damp_stiff=1e-5)
# the member sizing: the first two load cases, one allowable of each kind per truss (SZ_ALLOW, in NAMES' order), tensor
# bounds (a row per truss: 0.1 x its smallest to 1000 x its largest initial area), the member buckling check, a damped
# resizing, a look at the active count every second iteration, six resizings at most and a catalogue of 8 areas, so every
# host branch of `DeviceBatch.sizing` is in the digests.  The allowables are 0.5 and 0.4 of the truss's largest initial
# stress and half its largest initial joint displacement under these two cases, as tests/sizing_reference.py gives them
# on the CPU, rounded to two digits; there no truss ends with status 2 (which would only hash the fallback).  The commit
# that recorded the fixture ended every truss, in all four configs, as the yardstick does: status 1 (the iteration limit)
# after 6 resizings, info 0, and the members spread over seven of the catalogue's eight areas.
SZ_L, SZ_ITERS, SZ_CATALOG = 2, 6, 8
SZ_ALLOW = {"allow_tension": [1.9e4, 5.8e4, 1.4e4, 2.1e5, 3.6e4, 6.3e4, 1.0e6],
            "allow_compression": [1.6e4, 4.6e4, 1.1e4, 1.7e5, 2.9e4, 5.1e4, 8.1e5],
            "allow_displace": [0.14, 22.0, 0.53, 1.7, 1.8, 3.6, 1.1e6]}
SMALL = 6   # the trusses before bar-942: one bucket, where the results per member pair and per scenario are small
TRAIN = [(1.0, 0.0), (2.0, 30.0), (1.5, 75.0)]


def packed_batch(table):
    from python_stable_3d_truss_analysis_amd import batch
    return batch.pack_json([H.load_json(n) for n in NAMES], members="auto" if table else "general")


def inputs(packed):
    """Seeded inputs of every analysis, padded to the batch: settlements at constrained DOFs only, nothing along z in a
    2D truss."""
    rng = np.random.default_rng(17)
    B, nJ_max, nM_max = packed.B, packed.nJ_max, packed.nM_max
    joints = np.arange(nJ_max)[None, :] < np.asarray(packed.nJ).reshape(B, 1)                    # [B, nJ_max]
    axes = np.arange(3)[None, :] < np.asarray(packed.dim).reshape(B, 1)                           # [B, 3]
    live = (joints[:, :, None] & axes[:, None, :])[:, None]                                       # [B, 1, nJ_max, 3]
    members = (np.arange(nM_max)[None, :] < np.asarray(packed.nM).reshape(B, 1))[:, None]         # [B, 1, nM_max]
    vec = lambda scale: rng.uniform(-scale, scale, size=(B, L, nJ_max, 3)) * live
    per_member = lambda scale: rng.uniform(-scale, scale, size=(B, L, nM_max)) * members
    return {"loads": vec(3e4), "settlement": vec(0.02) * packed.constrained()[:, None],
            "prestrain": per_member(5e-4), "accel": rng.uniform(-2.0, 2.0, size=(B, L, 3)) * axes[:, None],
            "grad_u": vec(1.0), "grad_f_ext": vec(1e-4), "grad_N": per_member(1e-4),
            "joint_mass": rng.uniform(0.0, 50.0, size=(B, nJ_max)) * joints,
            # (drawn after everything above, so the inputs of the earlier analyses are what they were)
            "scale": rng.uniform(-1.0, 1.0, size=(B, L_DYN, STEPS + 1)),
            "ground": rng.uniform(-2.0, 2.0, size=(B, L_DYN, STEPS + 1, 3)) * axes[:, None, None],
            "weights": rng.uniform(-1.0, 1.0, size=(B, P))}


def scenarios(packed):
    """Seeded scenarios of `solve_member_sets`: sets int64 [B, S_SETS, 8] (-1 padding) of 0 .. min(8, nM) distinct
    members - the first empty, the second a single removal - and factors from {0, 0, 0.5, 2}."""
    rng = np.random.default_rng(7)
    sets = np.full([packed.B, S_SETS, 8], -1, dtype=np.int64)
    for b in range(packed.B):
        nM = int(packed.nM[b])
        for s in range(S_SETS):
            k = s if s < 2 else int(rng.integers(0, min(8, nM) + 1))
            sets[b, s, :k] = rng.choice(nM, size=k, replace=False)
    factors = rng.choice([0.0, 0.0, 0.5, 2.0], size=sets.shape)
    factors[:, 1] = 0.0
    return sets, factors


def moving_load(packed):
    """The path of `solve_influence` per truss (joints 0 .. min(nJ, P_PATH) - 1 in id order, then joint 0 again; -1
    padding) and a seeded load vector [B, 3], nothing along z on a 2D truss."""
    rng = np.random.default_rng(11)
    path = np.full([packed.B, P_PATH + 1], -1, dtype=np.int64)
    for b in range(packed.B):
        n = min(int(packed.nJ[b]), P_PATH)
        path[b, :n + 1] = list(range(n)) + [0]
    axes = np.arange(3)[None, :] < np.asarray(packed.dim).reshape(packed.B, 1)
    return path, rng.uniform(-1.0, 1.0, size=(packed.B, 3)) * axes


def spectrum_table():
    """The seeded spectral accelerations [2, 5] of `solve_response_spectrum`, from a generator of their own (the inputs
    of the other analyses stay what they were)."""
    return np.random.default_rng(23).uniform(0.5, 10.0, size=(len(RS_DIRS), len(RS_PERIODS)))


def sizing_arguments(packed, x):
    """The keyword arguments of `solve_sizing` (see SZ_ALLOW): bounds and catalogue from the batch's own areas."""
    A = np.asarray((packed.general() if packed.is_table else packed).A, dtype=np.float64)
    live = np.arange(packed.nM_max)[None, :] < np.asarray(packed.nM).reshape(-1, 1)
    lo, hi = np.where(live, A, np.inf).min(axis=1), np.where(live, A, 0.0).max(axis=1)
    return dict(loads=x["loads"][:, :SZ_L], **{k: np.array(v) for k, v in SZ_ALLOW.items()},
                euler_kappa=1.0 / (4.0 * np.pi), area_min=np.repeat(0.1 * lo[:, None], packed.nM_max, axis=1),
                area_max=np.repeat(1000.0 * hi[:, None], packed.nM_max, axis=1), relax=0.7, tol=1e-4, max_iters=SZ_ITERS,
                check_every=2, catalog=np.geomspace(0.1 * lo.min(), 30.0 * hi.max(), SZ_CATALOG))


_yardstick = {}


def own_batch_runs(analysis, table, reorder):
    """{name: (result dataclass, [(status, count)] of the yardstick per truss)} of an analysis of OWN_BATCH, through its
    `solve_*` function: the ragged batch and bar-942 alone.  The count is `iterations`, for plastic `events`."""
    from python_stable_3d_truss_analysis_amd import batch
    from tests import compliance_reference as cref, plastic_reference as pref, unilateral_reference as uref
    form = lambda packed: packed.table() if table else packed
    runs = {}
    if analysis == "unilateral":
        for name in UN_RUNS:
            packed, kind, loads, pre, slack, _ = uref.batch_inputs(name)
            res = batch.solve_unilateral(form(packed), kind, loads[:, None], None if pre is None else pre[:, None],
                                         slack_factor=slack, max_iters=uref.MAX_ITERS, reorder=reorder)
            runs[name] = (res, [row[:2] for row in uref.TABLE[name]])
    elif analysis == "plastic":
        for name in PL_RUNS:
            packed, ct, cc, loads, scalars, _ = pref.batch_inputs(name)
            res = batch.solve_plastic(form(packed), ct, cc, loads[:, None], reorder=reorder, **scalars)
            runs[name] = (res, [row[:2] for row in pref.TABLE[name]])
    else:
        with open(os.path.join(H.GOLDEN, "compliance_tol.json")) as fh:
            entry = json.load(fh)["full"]["configs"]["weighted"]
        if "big" not in _yardstick:      # (not in the record: the yardstick itself, once - LAPACK for its 696 unknowns)
            data = H.load_json(cref.BIG)
            ref = cref.minimise(data, solve=np.linalg.solve, **cref.config(data, "weighted"), **cref.FULL)
            _yardstick["big"] = [(ref["status"], ref["iterations"])]
        want = {"batch": list(zip(entry["status"], entry["iterations"])), "big": _yardstick["big"]}
        for name, names in (("batch", cref.BATCH), ("big", (cref.BIG,))):
            packed, kw = cref.batch_arguments(names, "weighted")
            runs[name] = (batch.solve_min_compliance(form(packed), reorder=reorder, **kw, **cref.FULL), want[name])
    return runs


def column_calls(analysis, packed, x):
    """{name: (function name, arguments, keywords)} of a column analysis: "full" on the whole batch with chunk 48 and
    no result per member pair, "small" on the trusses before bar-942 with the default chunk and every optional result."""
    small = packed.take(np.arange(SMALL)).trimmed()
    loads = x["loads"][:, :L_COL]
    loads_small = loads[:SMALL, :, :small.nJ_max]
    if analysis == "member_loss":
        return {"full": ("solve_member_loss", (packed, loads), dict(chunk=CHUNK, want_forces=False)),
                "small": ("solve_member_loss", (small, loads_small), dict(want_forces=True))}
    if analysis == "member_sets":
        sets, factors = scenarios(packed)
        return {"full": ("solve_member_sets", (packed, sets, factors, loads), dict(chunk=CHUNK)),
                "small": ("solve_member_sets", (small, sets[:SMALL], factors[:SMALL], loads_small),
                          dict(want_forces=True, want_displace=True))}
    path, direction = moving_load(packed)
    return {"full": ("solve_influence", (packed, path, direction, TRAIN), dict(chunk=CHUNK)),
            "small": ("solve_influence", (small, path[:SMALL], direction[:SMALL], TRAIN), dict(want_lines=True))}


def run(analysis, packed, x, reorder):
    """The result dataclasses of one analysis, as {name: dataclass}."""
    from python_stable_3d_truss_analysis_amd import batch
    if analysis == "load_cases":
        return {"cases": batch.solve_load_cases(packed, x["loads"], reorder=reorder)}
    if analysis == "effect_cases":
        return {"effects": batch.solve_effect_cases(packed, x["loads"], x["prestrain"], x["settlement"], x["accel"],
                                                    reorder=reorder)}
    if analysis == "gradients":
        forward, grads = batch.solve_gradients(packed, x["loads"], x["grad_u"], x["grad_f_ext"], x["grad_N"],
                                               reorder=reorder)
        return {"forward": forward, "grads": grads}
    if analysis in ("member_loss", "member_sets", "influence"):
        return {name: getattr(batch, fn)(*args, reorder=reorder, **kw)
                for name, (fn, args, kw) in column_calls(analysis, packed, x).items()}
    if analysis == "buckling":
        # under the loads as they are, and reversed: there several trusses have only negative factors near zero and take
        # two or three rounds, so the shifted factors, the trusses left out of a round and the merge are in the digests
        reversed_ = packed._map(lambda f, a: -a if f == "loads" else a)
        return {"loaded": batch.solve_buckling(packed, p=P, reorder=reorder),
                "reversed": batch.solve_buckling(reversed_, p=P, reorder=reorder)}
    if analysis == "transient":
        last = lambda counts: np.stack([np.zeros(packed.B, dtype=np.int64), np.asarray(counts).reshape(-1) - 1], axis=1)
        return {"transient": batch.solve_transient(packed, x["loads"][:, :L_DYN], DT, STEPS, scale=x["scale"],
                                                   accel=x["ground"], damp_stiff=DAMP_STIFF,
                                                   monitor_joints=last(packed.nJ), monitor_members=last(packed.nM),
                                                   reorder=reorder)}
    if analysis == "nonlinear":
        return {"nonlinear": batch.solve_nonlinear(packed, NL_FACTORS, reorder=reorder)}
    if analysis == "mode_gradients":
        return {"rows": batch.solve_mode_gradients(packed, p=P, joint_mass=x["joint_mass"], reorder=reorder),
                "weighted": batch.solve_mode_gradients(packed, p=P, weights=x["weights"], joint_mass=x["joint_mass"],
                                                       reorder=reorder)}
    if analysis == "response_spectrum":
        # CQC with the missing mass and the modal values; the absolute sum without either (the other branch of the
        # combination, and no response vector behind the p mode shapes)
        return {"spectrum": batch.solve_response_spectrum(packed, RS_DIRS, RS_PERIODS, spectrum_table(), p=P, rule="cqc",
                                                          missing_mass=True, want_modal=True,
                                                          joint_mass=x["joint_mass"], reorder=reorder),
                "abs": batch.solve_response_spectrum(packed, RS_DIRS, RS_PERIODS, spectrum_table(), p=P, rule="abs",
                                                     missing_mass=False, want_modal=False, joint_mass=x["joint_mass"],
                                                     reorder=reorder)}
    if analysis == "harmonic":
        # "full": patterns and ground accelerations together, the static correction, the first and last joint and member
        # monitored; "bare": ground accelerations alone, no correction, no monitors (no pattern, no residual block and no
        # monitor arrays reach the kernels)
        last = lambda counts: np.stack([np.zeros(packed.B, dtype=np.int64), np.asarray(counts).reshape(-1) - 1], axis=1)
        accel = x["accel"][:, :L_HR]
        return {"full": batch.solve_harmonic(packed, HR_OMEGAS, pattern=x["loads"][:, :L_HR], accel=accel, p=P,
                                             residual=True, monitor_joints=last(packed.nJ),
                                             monitor_members=last(packed.nM), joint_mass=x["joint_mass"],
                                             reorder=reorder, **HR_DAMPING),
                "bare": batch.solve_harmonic(packed, HR_OMEGAS, accel=accel, p=P, residual=False,
                                             joint_mass=x["joint_mass"], reorder=reorder, **HR_DAMPING)}
    if analysis == "sizing":
        return {"sizing": batch.solve_sizing(packed, reorder=reorder, **sizing_arguments(packed, x))}
    if analysis in OWN_BATCH:
        return {name: res for name, (res, _) in own_batch_runs(analysis, packed.is_table, reorder).items()}
    return {"modes": batch.solve_modes(packed, p=P, joint_mass=x["joint_mass"], reorder=reorder)}


def digests(results):
    """{"<result>.<field>": SHA-256 of the field's dtype, shape and raw bytes}, every field of every dataclass that is
    not None (an optional result that was not asked for)."""
    out = {}
    for name, res in results.items():
        for field, value in vars(res).items():
            if value is None:
                continue
            a = np.ascontiguousarray(value)
            h = hashlib.sha256(f"{a.dtype.str} {a.shape} ".encode())
            h.update(a.tobytes())
            out[f"{name}.{field}"] = h.hexdigest()
    return out


def stack():
    """What the digests are promised for: the HIP runtime torch was built against and the compiler that builds the
    library - the hipcc installed NOW ($HIPCC, else /opt/rocm/bin/hipcc), the one `build()` uses, not a version read out
    of the loaded libtrs_hip.so (it records none).  A hipcc that cannot be run gives an empty line, which matches no
    recording: the tests then skip, as on any other stack."""
    import torch
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        text = subprocess.run([hipcc, "--version"], capture_output=True, text=True, timeout=60).stdout
    except (OSError, subprocess.SubprocessError):
        text = ""
    line = next((ln.strip() for ln in text.splitlines() if ln.startswith("HIP version")), "")
    return {"torch_hip": torch.version.hip, "hipcc": line}


def record(path=FIXTURE):
    os.environ.setdefault("TRS_DEBUG_POISON", "1")   # as the suite runs (tests/conftest.py)
    found = {}
    for config, kw in CONFIGS.items():
        packed = packed_batch(kw["table"])
        x = inputs(packed)
        found[config] = {a: digests(run(a, packed, x, kw["reorder"])) for a in ANALYSES}
    with open(path, "w") as fh:
        json.dump({"stack": stack(), "digests": found}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"recorded {sum(len(d) for c in found.values() for d in c.values())} digests to {path}")


def test_the_batch_exercises_every_fold():
    """From the packing and `size_buckets` alone (no GPU): two or more buckets, a 2D and a 3D truss, a constrained joint
    with free DOFs, every truss at most three times, and the table member form where it is asked for."""
    from python_stable_3d_truss_analysis_amd import batch
    assert max(NAMES.count(n) for n in NAMES) <= 3
    packed = packed_batch(False)
    assert len(list(batch.size_buckets(packed))) >= 2
    assert {2, 3} <= set(np.asarray(packed.dim).reshape(-1).tolist())
    held = packed.constrained()   # [B, nJ_max, 3]
    assert (held.any(axis=2) & ~held.all(axis=2))[0, :packed.nJ[0]].any() and packed.dim.reshape(-1)[0] == 3
    assert packed_batch(True).is_table and not packed.is_table
    assert L > 16 and L % 16 != 0
    assert 64 < HR_OMEGAS.size < 128 and 1 < L_HR <= L   # (two chunks of the sweep's table of 64, the second partial)
    # the column analyses: more cases than one pass of the apply kernels holds, a partial last chunk of members and a
    # partial last slice of scenarios in every bucket, several ranges of scenarios, every set size, a valid path
    assert 8 < L_COL < 16 and S_SETS > 32 and S_SETS % 32 != 0 and CHUNK % 16 == 0
    buckets = [packed.take(idx).trimmed() for idx in batch.size_buckets(packed)]
    assert sorted(b.nM_max for b in buckets) == [120, 942] and packed.take(np.arange(SMALL)).trimmed().nM_max == 120
    assert all(b.nM_max > CHUNK and b.nM_max % CHUNK != 0 for b in buckets)
    x = inputs(packed)
    sets, factors = scenarios(packed)
    assert not (sets[:, 0] >= 0).any() and ((sets[:, 1] >= 0).sum(axis=1) == 1).all()
    assert {int(k) for k in (sets >= 0).sum(axis=2).reshape(-1)} == set(range(9))
    assert {0.0, 0.5, 2.0} == set(factors.reshape(-1).tolist())
    for chunk, part in ((CHUNK, packed), (64, packed.take(np.arange(SMALL)).trimmed())):
        got = batch._check_member_sets_args(part, sets[:part.B], factors[:part.B], x["loads"][:part.B, :L_COL, :part.nJ_max],
                                            batch.MEMBER_LOSS_R_TOL, None, chunk=chunk)
        assert len(batch.plan_member_sets(got[0], chunk, part.nM_max)) > 1
    path, direction = moving_load(packed)
    path, path_len = batch._check_influence_args(packed, path, direction, TRAIN, None, chunk=CHUNK)[:2]
    assert path_len.tolist() == [min(int(n), P_PATH) + 1 for n in packed.nJ]
    assert not direction[packed.dim.reshape(-1) == 2, 2].any()


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        fixture = json.load(fh)
    if fixture["stack"] != stack():
        pytest.skip(f"digests are promised per compiler: recorded on {fixture['stack']}, running on {stack()}")
    return fixture["digests"]


@pytest.fixture(scope="module")
def batches():
    made = {}

    def get(table):
        if table not in made:
            packed = packed_batch(table)
            made[table] = (packed, inputs(packed))
        return made[table]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("analysis", ANALYSES)
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_same_bits_as_recorded(recorded, batches, config, analysis):
    kw = CONFIGS[config]
    packed, x = batches(kw["table"])
    if analysis in OWN_BATCH:
        runs = own_batch_runs(analysis, kw["table"], kw["reorder"])
        results = {name: res for name, (res, _) in runs.items()}
        for name, (res, want) in runs.items():   # (the yardstick's, truss by truss; its status is never 2)
            count = res.events if analysis == "plastic" else res.iterations
            got = list(zip(res.status.reshape(-1).tolist(), count.reshape(-1).tolist()))
            print(f"{config} / {analysis} / {name}: status, count {got}, the yardstick's {want}")
            assert got == [tuple(w) for w in want] and 2 not in res.status, (name, got, want)
    else:
        results = run(analysis, packed, x, kw["reorder"])
    assert all(not res.info.any() for res in results.values())
    if analysis == "buckling":   # (else the batch would never shift, or never find a factor)
        from python_stable_3d_truss_analysis_amd import batch
        assert results["reversed"].rounds.max() >= 2 and (results["loaded"].status == batch.BK_FOUND).any()
    if analysis == "nonlinear":   # (info only speaks of a tangent that was not positive definite)
        assert not results["nonlinear"].status.any() and results["nonlinear"].iterations.min() >= 1
    if analysis == "sizing":   # (status 2 would only hash the design a truss fell back to)
        assert (results["sizing"].status == 1).all() and (results["sizing"].iterations == SZ_ITERS).all()
    got, want = digests(results), recorded[config][analysis]
    assert sorted(got) == sorted(want)
    differing = [k for k in got if got[k] != want[k]]
    assert not differing, f"{config} / {analysis}: other bits than recorded in {differing}"


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"] or len(sys.argv) > 3:
        sys.exit("usage: python -m tests.test_gpu_analysis_bits --record [FILE]")
    record(*sys.argv[2:3])
