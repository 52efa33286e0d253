"""Minimum weight under stress and displacement limits in one run on the GPU (`DeviceBatch.min_weight`,
`solve_min_weight`, `Truss.MinimizeWeight` with `allow_tension` / `allow_compression` / `euler_kappa`; C ABI
trs_mw_step_stress of include/trs_minweight_stress.h) against the numpy yardstick `tests/minweight_stress_reference.py`.

The parity tolerance of a truss is 100 x the largest max-scaled difference between the yardstick in float64 and in
longdouble on the same inputs, over its results (tests/golden/minweight_stress_tol.json, which names them and keeps the
figure of every result; tests/test_minweight_stress.py measures the small batch and the generated truss again; never
less than 100 x FLOOR_LEAST).  The device's own output never sets a bound.  Every fixture keeps its own limits, area
bounds and allowables: inside one `DeviceBatch` they go in as one row per truss."""
import json
import os
import threading

import numpy as np
import pytest

from tests import minweight_reference as mref
from tests import minweight_stress_reference as sref
from tests.helpers import GOLDEN, edge_cases, load_json

pytestmark = pytest.mark.gpu
FLOATS = sref.COMPARED
INTS = ("governing", "iterations", "status")
KEYS = FLOATS + INTS
PER_MEMBER = ("areas", "sensitivity", "utilisation", "governing")
HISTORIES = ("measure_history", "worst_history", "stress_history")
DEPTH = {"tol": 0.0, "max_iters": sref.DEPTH}
GENERATED = sref.GENERATED

_cache = {}
_data, _arguments = sref.fixture, sref.batch_arguments


def _solver(name):
    return np.linalg.solve if name == sref.BIG else None      # (696 unknowns: a float64 run may use LAPACK)


def _reference(name, which, **run):
    key = (name, which, tuple(sorted(run.items())))
    if key not in _cache:
        data = _data(name)
        _cache[key] = sref.minimise(data, solve=_solver(name), **sref.config(data, which, solve=_solver(name)), **run)
    return _cache[key]


def _record():
    if "record" not in _cache:
        with open(os.path.join(GOLDEN, "minweight_stress_tol.json")) as fh:
            _cache["record"] = json.load(fh)
    rec = _cache["record"]
    assert rec["trusses"] == list(sref.BATCH) and rec["big_truss"] == sref.BIG
    return rec


def _tolerance(per):
    return dict.fromkeys(FLOATS, 100.0 * max(max(per.values()), sref.FLOOR_LEAST))


def _floors(part, which, b=0):
    """key -> the tolerance of truss b of a part and configuration: 100 x the largest of the truss's own figures."""
    return _tolerance(_record()[part]["configs"][which]["per_truss"][b])


def _on_device(torch, dev, kw):
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return dict(kw, loads=up(kw["loads"]), area_min=up(kw["area_min"]), area_max=up(kw["area_max"]))


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _launch(packed, kw, dbkw=None, **run):
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    db = batch.DeviceBatch(packed, use_small=False, **(dbkw or {}))
    out = db.min_weight(**_on_device(torch, db.device, kw), want_sensitivity=True, **run)
    torch.cuda.synchronize(db.device)
    return dict(_host(out), info=db.info.cpu().numpy()), db


def _run(names, which, rows=None, dbkw=None, **run):
    """`min_weight` with stress limits on ONE DeviceBatch over the trusses `names` (`rows`: only these of them).  Returns
    (numpy results, db)."""
    names = list(names) if rows is None else [names[r] for r in rows]
    packed, kw = _arguments(names, which)
    return _launch(packed, kw, dbkw, **run)


def _scaled(mine, ref):
    ref = np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max())
    diff = float(np.abs(np.asarray(mine) - ref).max())
    return diff if scale == 0 else diff / scale


def _compare(got, b, ref, tols, what, counts=True):
    """Truss b of the device results against its yardstick: every float result max-scaled within its tolerance, the
    governing case exactly wherever the yardstick's two largest case requirements of the member differ by more than the
    tolerance (max-scaled; one case: against 0), zeros and -1 on the padding."""
    nM, H = len(ref["areas"]), len(ref["measure_history"])
    if counts:
        assert (got["status"][b], got["iterations"][b]) == (ref["status"], ref["iterations"]), (what, got["status"][b],
                                                                                             got["iterations"][b])
    worst = {"areas": _scaled(got["areas"][b, :nM], ref["areas"]),
             "sensitivity": _scaled(got["sensitivity"][b, :, :nM], ref["sensitivity"]),
             "utilisation": _scaled(got["utilisation"][b, :nM], ref["utilisation"])}
    for key in ("measure", "displacement", "ratio", "multipliers"):
        worst[key] = _scaled(got[key][b], ref[key])
    for key in HISTORIES:
        worst[key] = _scaled(got[key][b, :H], ref[key])
    print(f"{what}: " + " ".join(f"{k} {v:.2e}/{tols[k]:.2e}" for k, v in worst.items())
          + f" status {got['status'][b]} iterations {got['iterations'][b]}")
    assert sorted(worst) == sorted(FLOATS)
    for key, value in worst.items():
        assert value <= tols[key], (what, key, value, tols[key])
    required = np.sort(np.asarray(ref["required"], dtype=np.float64), axis=0)[::-1]
    second = required[1] if len(required) > 1 else np.zeros(nM)
    clear = required[0] - second > tols["utilisation"] * max(float(required.max()), 0.0)
    assert np.array_equal(got["governing"][b, :nM][clear], ref["governing"][clear]), what
    assert set(np.unique(got["governing"][b, :nM]).tolist()) <= set(range(-1, len(required))), what
    assert not got["areas"][b, nM:].any() and not got["sensitivity"][b, :, nM:].any(), what
    assert not got["utilisation"][b, nM:].any() and (got["governing"][b, nM:] == -1).all(), what
    return int(clear.sum())


def _same(a, b, what, rows_a=slice(None), rows_b=slice(None), nM=None, history=None, keys=KEYS + ("info",)):
    for key in keys:
        x, y = a[key][rows_a], b[key][rows_b]
        if key in PER_MEMBER:
            x, y = x[..., :nM], y[..., :nM]
        if key in HISTORIES and history is not None:   # (zero beyond the shorter run)
            assert not x[:, history:].any() and not y[:, history:].any(), (what, key)
            x, y = x[:, :history], y[:, :history]
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        same = np.array_equal(x.view(np.uint64), y.view(np.uint64)) if x.dtype == np.float64 else np.array_equal(x, y)
        assert same, (what, key)


@pytest.fixture(scope="module")
def full():
    """The ragged batch resized to tol 1e-4 within 200 iterations, every configuration."""
    return {which: _run(sref.BATCH, which, **sref.FULL)[0] for which in sref.CONFIGS}


def _stress_check(names, which, areas):
    """The utilisation [B] that an INDEPENDENT kernel gives the designs `areas`: a fresh batch, `sizing(max_iters=0)`."""
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    packed, kw = _arguments(list(names), which)
    db = batch.DeviceBatch(packed, use_small=False)
    db.A.copy_(torch.from_numpy(np.ascontiguousarray(areas)).to(db.device))
    dev = _on_device(torch, db.device, kw)
    check = _host(db.sizing(dev["loads"], allow_tension=kw["allow_tension"], allow_compression=kw["allow_compression"],
                            euler_kappa=kw["euler_kappa"], area_min=dev["area_min"], area_max=dev["area_max"], tol=1e-4,
                            max_iters=0))
    return check["utilisation"].max(axis=1)


# ---- 1. parity at a fixed depth ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(sref.CONFIGS))
def test_parity_at_a_fixed_depth(which):
    """bar-6 .. bar-120 in ONE DeviceBatch (ragged padding, the allowables as [B] arrays), tol = 0, six resizings: status
    1 and 6 iterations; members on the stress floor and members sized by the multipliers in the same truss."""
    got, db = _run(sref.BATCH, which, **DEPTH)
    assert db.env is not None and not db.table
    assert (got["status"] == 1).all() and (got["iterations"] == sref.DEPTH).all() and not got["info"].any()
    compared = 0
    for b, name in enumerate(sref.BATCH):
        compared += _compare(got, b, _reference(name, which, **DEPTH), _floors("depth", which, b), f"{which} {name}")
    assert compared > 100      # (the governing cases that are compared exactly)
    if which != "single":
        assert {0, 1} <= set(np.unique(got["governing"]).tolist())


# ---- 2. the strides and the largest carve --------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(sref.CONFIGS))
def test_parity_at_a_fixed_depth_on_the_large_truss(which):
    """bar-942 alone (n_free 696): four members per thread, and the LDS fit with three limits under "pair"."""
    got, db = _run((sref.BIG,), which, **DEPTH)
    assert db.nM_max > 3 * 256
    _compare(got, 0, _reference(sref.BIG, which, **DEPTH), _floors("big", which), f"{which} bar-942")


@pytest.mark.parametrize("which", sorted(sref.CONFIGS))
def test_parity_at_a_fixed_depth_on_the_generated_truss(which):
    """A girder of 305 members: the second stride, and a last pass that not every thread takes."""
    got, db = _run((GENERATED,), which, **DEPTH)
    assert 256 < db.nM_max <= 512 and db.nM_max % 256
    _compare(got, 0, _reference(GENERATED, which, **DEPTH), _floors("generated", which), f"{which} generated")


def test_eight_limits_for_the_largest_carve():
    """J = 8 on three small trusses under "euler": the three limits of "pair" and five more copies, one of them at 0.9 of
    its value, one switched off by an infinite value on truss 0 and one by joint -1 on truss 1.  The tolerance is measured
    here, 100 x the float64-against-longdouble difference of these very runs."""
    names = sref.BATCH[:3]
    packed, kw = _arguments(names, "euler")
    B, J = len(names), 8
    wide = {"limit_case": np.zeros(J, dtype=np.int64), "limit_joint": np.zeros([B, J], dtype=np.int64),
            "limit_direction": np.zeros([B, J, 3]), "limit_value": np.zeros([B, J])}
    for j, s in enumerate([0, 1, 2, 0, 0, 1, 1, 0]):
        wide["limit_case"][j] = kw["limit_case"][s]
        for key in ("limit_joint", "limit_direction", "limit_value"):
            wide[key][:, j] = kw[key][:, s]
    wide["limit_value"][:, 4] *= 0.9
    wide["limit_value"][0, 5] = np.inf
    wide["limit_joint"][1, 6] = -1
    got, _ = _launch(packed, dict(kw, **wide), **DEPTH)
    for b, name in enumerate(names):
        data = load_json(name)
        one = sref.config(data, "euler")
        dim = one["loads"].shape[2]
        one["limits"] = [(int(wide["limit_case"][j]), int(wide["limit_joint"][b, j]), wide["limit_direction"][b, j, :dim],
                          float(wide["limit_value"][b, j])) for j in range(J)]
        f64 = sref.minimise(data, **one, **DEPTH)
        f80 = sref.minimise(data, dtype=np.longdouble, **one, **DEPTH)
        _compare(got, b, f64, _tolerance(sref.differences(f64, f80)), f"eight limits {name}")
    assert got["ratio"][0, 5] == 0.0 and got["multipliers"][0, 5] == 0.0 and not got["sensitivity"][0, 5].any()
    assert got["ratio"][1, 6] == 0.0 and got["displacement"][1, 6] == 0.0 and not got["sensitivity"][1, 6].any()


# ---- 3. the classical 10-bar truss ---------------------------------------------------------------------------------------
def test_the_classical_ten_bar_truss():
    """Bays of 360, E = 1e7, rho = 0.1, 100 000 down at the two lower free joints, +-25 000 stress, 2.0 on the downward
    displacement of the four free joints, area_min 0.1, move 0.1: status 0 at the yardstick's count and weight, which is
    the recorded 5076.54 - 0.31 % above the literature's optimum 5060.85 -, within both kinds of limit."""
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    data, kw = sref.ten_bar()
    rec = _record()["ten_bar"]
    tols = _tolerance(rec["per_truss"][0])
    ref = sref.minimise(data, **kw, **sref.FULL)
    # (the last change, 0.99367e-4, lies 0.63 % under tol - inside the 1 % band of `decided`, so the record says
    # decided: false; float64 and longdouble agree on that change to 1e-11 and both end at 66, which is compared)
    assert (ref["status"], ref["iterations"]) == (rec["status"], rec["iterations"]) == (0, 66)
    assert abs(float(ref["measure"]) - rec["weight"]) <= tols["measure"] * rec["weight"]
    assert abs(rec["weight"] - 5076.54) < 0.005 and abs(float(ref["measure"]) / sref.TEN_BAR["optimum"] - 1.0031) < 5e-5
    db = batch.DeviceBatch(batch.pack_json([data]), use_small=False)
    loads = torch.zeros([1, 1, db.nJ_max, 3], dtype=torch.float64, device=db.device)
    loads[0, :, :, :2] = torch.from_numpy(kw["loads"]).to(db.device)
    joints = [joint for _, joint, _, _ in kw["limits"]]
    got = _host(db.min_weight(loads, limit_case=[0] * 4, limit_joint=joints, limit_direction=[[0.0, -1.0, 0.0]] * 4,
                              limit_value=sref.TEN_BAR["deflection"], move=kw["move"], area_min=kw["area_min"],
                              area_max=kw["area_max"], allow_tension=kw["allow_tension"],
                              allow_compression=kw["allow_compression"], want_sensitivity=True, **sref.FULL))
    got["info"] = db.info.cpu().numpy()
    assert got["status"][0] == 0
    _compare(got, 0, ref, tols, "ten-bar")
    weight, edge = got["measure"][0], 1.0 + sref.FULL["limit_tol"]
    print("ten-bar: weight", weight, "over the optimum", weight / sref.TEN_BAR["optimum"], "iterations", got["iterations"][0])
    assert weight <= 1.01 * sref.TEN_BAR["optimum"]
    u = db.solve_cases(loads)["u"].cpu().numpy()[0, 0]        # no factor() in between
    print("ten-bar: largest downward displacement", (-u[:, 1]).max(), "utilisation", got["utilisation"][0].max())
    assert (np.abs(u[:, 1]) <= sref.TEN_BAR["deflection"] * edge).all()
    assert got["utilisation"][0].max() <= edge and got["stress_history"][0, got["iterations"][0]] <= edge


# ---- 4. full runs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(sref.CONFIGS))
def test_statuses_and_counts(full, which):
    """Status and iterations equal the yardstick's for every truss that tests/golden/minweight_stress_tol.json records as
    decided (tests/test_minweight_stress.py measures that again); where such a truss converged its results agree too,
    and an INDEPENDENT kernel - `sizing(max_iters=0)` on a fresh batch with the returned areas - finds the design
    within its stress limits."""
    got = full[which]
    entry = _record()["full"]["configs"][which]
    assert sum(entry["decided"]) >= 4
    independent = _stress_check(sref.BATCH, which, got["areas"])
    edge = 1 + sref.FULL["limit_tol"]
    converged = 0
    for b, name in enumerate(sref.BATCH):
        ref = _reference(name, which, **sref.FULL)
        assert (ref["status"], ref["iterations"]) == (entry["status"][b], entry["iterations"][b]), (which, name)
        if got["status"][b] == sref.CONVERGED:
            print(f"{which} {name}: converged; the stress sizing kernel's utilisation {independent[b]:.6f}")
            assert independent[b] <= edge and got["worst_history"][b, got["iterations"][b]] <= edge, (which, name)
            assert got["utilisation"][b].max() <= edge and got["ratio"][b].max() <= edge, (which, name)
            converged += 1
        if not entry["decided"][b]:
            print(f"{which} {name}: not decided - the count is not compared; device status {got['status'][b]} iterations "
                  f"{got['iterations'][b]}, yardstick {ref['status']} {ref['iterations']}")
        elif ref["status"] == sref.CONVERGED:
            _compare(got, b, ref, _floors("full", which, b), f"{which} {name}")
        else:
            assert (got["status"][b], got["iterations"][b]) == (ref["status"], ref["iterations"]), (which, name)
    assert converged >= 3
    n = got["iterations"] + 1
    for b in range(len(sref.BATCH)):
        for key in HISTORIES:
            assert not got[key][b, n[b]:].any(), (b, key)
        assert got["measure_history"][b, n[b] - 1] == got["measure"][b], b
        assert got["stress_history"][b, n[b] - 1] == got["utilisation"][b].max(), b


def test_what_the_stress_limits_are_for():
    """Today's `min_weight` without stress limits on bar-25, checked by the same independent kernel: overstressed more
    than a hundred times (the yardstick: 1237)."""
    name = "bar-25_input_0"
    packed, kw = mref.batch_arguments([name], "single")
    plain, _ = _launch(packed, kw, **mref.FULL)
    assert plain["status"][0] == 0 and "utilisation" not in plain
    over = _stress_check([name], "single", plain["areas"])
    print("bar-25 without stress limits: utilisation", over[0])
    assert over[0] > 100.0


# ---- 5. status 3 -----------------------------------------------------------------------------------------------------------
def test_a_truss_whose_area_max_cannot_carry_its_stress():
    """Every member of the middle truss may grow by 5 % at most, its allowables ask for twice the area: it converges on
    its bounds with a utilisation near 1.9 and status 3; the neighbours keep the bits of a run without the cap."""
    names = sref.BATCH[:3]
    packed, kw = _arguments(names, "single")
    capped = dict(kw, area_max=kw["area_max"].copy(), limit_value=kw["limit_value"].copy())
    nM = len(load_json(names[1])["member"])
    capped["area_max"][1, :nM] = 1.05 * packed.A[1, :nM]
    capped["limit_value"][1] = np.inf           # (no displacement limit on it: the stress alone gives the status)
    got, _ = _launch(packed, capped, **sref.FULL)
    clean, _ = _launch(packed, kw, **sref.FULL)
    assert got["status"].tolist() == [0, 3, 0] and clean["status"].tolist() == [0, 0, 0]
    last = got["iterations"][1]
    assert got["utilisation"][1].max() > 1.5 and got["stress_history"][1, last] == got["utilisation"][1].max()
    assert got["worst_history"][1, last] == 0.0
    assert (got["areas"][1, :nM] <= capped["area_max"][1, :nM]).all()
    assert (got["areas"][1, :nM] >= capped["area_min"][1, :nM]).all()
    _same(got, clean, "neighbours of status 3", rows_a=[0, 2], rows_b=[0, 2])


# ---- 6. independence, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 3, 5])
def test_a_truss_alone_has_the_bits_it_has_in_the_batch(full, b):
    alone, _ = _run(sref.BATCH, "euler", rows=[b], **sref.FULL)
    nM = len(load_json(sref.BATCH[b])["member"])
    _same(full["euler"], alone, sref.BATCH[b], rows_a=slice(b, b + 1), nM=nM)


def test_results_depend_neither_on_check_every_nor_on_max_iters(full):
    sparse, _ = _run(sref.BATCH, "pair", **dict(sref.FULL, check_every=7))
    _same(full["pair"], sparse, "check_every 7")
    longer, _ = _run(sref.BATCH, "pair", **dict(sref.FULL, max_iters=sref.FULL["max_iters"] + 10))
    done = np.flatnonzero(full["pair"]["status"] == 0)
    assert len(done) >= 2
    _same(full["pair"], longer, "ten more", rows_a=done, rows_b=done, history=sref.FULL["max_iters"] + 1)


def test_a_mechanism_among_healthy_trusses():
    """status 2 with 0 iterations, its initial areas, utilisation 0 and governing -1; the neighbours keep the bits of a
    run without it."""
    from python_stable_3d_truss_analysis_amd import batch
    names = ("bar-25_input_0", "bar-72_input_0")
    bad = edge_cases()["3d_mechanism_singular"]["input"]
    packed2, kw2 = _arguments(names, "single")
    packed3 = batch.pack_json([load_json(names[0]), bad, load_json(names[1])])
    assert (packed3.nJ_max, packed3.nM_max) == (packed2.nJ_max, packed2.nM_max)
    kw3 = dict(kw2)
    for key in ("loads", "area_min", "area_max", "limit_joint", "limit_direction", "limit_value", "allow_tension",
                "allow_compression"):
        row = np.ones_like(kw2[key][:1])
        if key == "loads":
            row[:] = 0.0
            row[0, 0, 2, 2] = -10.0
        kw3[key] = np.concatenate([kw2[key][:1], row, kw2[key][1:]], axis=0)
    kw3["area_min"][1], kw3["area_max"][1] = 0.1, 10.0
    got, _ = _launch(packed3, kw3, **sref.FULL)
    clean, _ = _launch(packed2, kw2, **sref.FULL)
    assert got["status"][1] == 2 and got["iterations"][1] == 0 and got["info"][1] != 0
    nM = len(bad["member"])
    assert np.array_equal(got["areas"][1, :nM], np.array([m[1][0] for m in bad["member"]]))
    for key in FLOATS:
        assert key == "areas" or not np.any(got[key][1]), key
    assert (got["governing"][1] == -1).all()
    assert not clean["info"].any() and 2 not in clean["status"]
    _same(got, clean, "neighbours", rows_a=[0, 2])


def test_two_streams_at_once_give_the_bits_of_one_after_the_other():
    """Each run has a host thread of its own (a stream context is per thread); the two interleave on the device."""
    import torch
    halves = (sref.BATCH[:3], sref.BATCH[3:])
    run = dict(sref.FULL, max_iters=40)
    one_by_one = [_run(names, "pair", **run)[0] for names in halves]
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs, errors = [None, None], []
    ready = threading.Barrier(2)

    def work(k):
        try:
            with torch.cuda.stream(streams[k]):
                ready.wait(timeout=60)
                for _ in range(2):
                    outs[k] = _run(halves[k], "pair", **run)[0]
        except Exception as exc:   # noqa: BLE001
            errors.append(exc)

    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for k in range(2):
        _same(one_by_one[k], outs[k], f"stream {k}")


# ---- 7. switched-off limits ----------------------------------------------------------------------------------------------
def test_a_truss_with_both_allowables_infinite():
    """Truss 1 of three with both allowables inf: utilisation 0, governing -1, and its float results agree with the run
    without stress limits within the parity tolerance (not bit for bit: the two instantiations of the kernel are compiled
    apart and may contract their products differently); its neighbours keep their floors."""
    names = sref.BATCH[:3]
    packed, kw = _arguments(names, "pair")
    off = dict(kw, allow_tension=kw["allow_tension"].copy(), allow_compression=kw["allow_compression"].copy())
    off["allow_tension"][1] = off["allow_compression"][1] = np.inf
    got, _ = _launch(packed, off, **DEPTH)
    plain, _ = _launch(packed, {k: v for k, v in kw.items() if k not in ("allow_tension", "allow_compression",
                                                                          "euler_kappa")}, **DEPTH)
    assert not got["utilisation"][1].any() and (got["governing"][1] == -1).all() and not got["stress_history"][1].any()
    assert got["utilisation"][0].max() > 0 and got["utilisation"][2].max() > 0
    tols = _floors("depth", "pair", 1)
    for key in mref.COMPARED:
        assert _scaled(got[key][1], plain[key][1]) <= tols[key], key
    assert (got["status"][1], got["iterations"][1]) == (plain["status"][1], plain["iterations"][1])


def test_allowables_of_none_are_the_plain_call():
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    packed, kw = mref.batch_arguments(mref.BATCH[:3], "pair")
    plain, _ = _launch(packed, kw, **DEPTH)
    none, _ = _launch(packed, dict(kw, allow_tension=None, allow_compression=None, euler_kappa=0.0), **DEPTH)
    assert sorted(plain) == sorted(none) and not set(none) & {"utilisation", "governing", "stress_history"}
    _same(plain, none, "None", keys=mref.COMPARED + ("iterations", "status", "info"))
    res = batch.solve_min_weight(packed, **kw, **DEPTH)
    assert res.utilisation is None and res.governing is None and res.stress_history is None


# ---- 8. the public layers --------------------------------------------------------------------------------------------------
def test_solve_min_weight_over_buckets_orders_and_member_forms():
    from python_stable_3d_truss_analysis_amd import batch
    names = ("bar-25_input_0", "bar-72_input_0", sref.BIG)
    packed, kw = _arguments(names, "euler")
    small = 1 << 20
    assert len(batch.size_buckets(packed, small)) >= 2
    direct, _ = _run(names, "euler", **DEPTH)

    def fields(res):
        assert isinstance(res, batch.MinWeightResult)
        return {key: getattr(res, key) for key in KEYS + ("info",)}

    more = dict(max_slab_bytes=small, want_sensitivity=True, **DEPTH)
    bucketed = fields(batch.solve_min_weight(packed, **kw, **more))
    _same(direct, bucketed, "buckets")
    table = packed.table()
    assert table.is_table
    _same(bucketed, fields(batch.solve_min_weight(table, **kw, **more)), "table form")
    ordered = fields(batch.solve_min_weight(packed, **kw, reorder=True, **more))
    for b, name in enumerate(names):
        tols = _floors("big", "euler") if name == sref.BIG else _floors("depth", "euler", sref.BATCH.index(name))
        _compare(ordered, b, _reference(name, "euler", **DEPTH), tols, f"reorder {name}")
        _compare(bucketed, b, _reference(name, "euler", **DEPTH), tols, f"buckets {name}")


def test_truss_minimize_weight():
    from python_stable_3d_truss_analysis_amd import Truss
    name = "bar-72_input_0"
    data = load_json(name)
    kw = sref.config(data, "pair")
    truss = Truss(3).LoadFromJSON(data=data)
    before = truss.Serialize()
    listed = [{j: tuple(f[j]) for j in range(len(f)) if np.any(f[j] != 0)} for f in kw["loads"]]
    limits = [(case, joint, tuple(2.0 * d), value) for case, joint, d, value in kw["limits"]]
    run = sref.FULL
    one = truss.MinimizeWeight(listed, limits, move=sref.MOVE, areaMin=kw["area_min"], areaMax=kw["area_max"], tol=run["tol"],
                               maxIters=run["max_iters"], limitTol=run["limit_tol"], returnSensitivity=True,
                               allowTension=kw["allow_tension"], allowCompression=kw["allow_compression"],
                               eulerKappa=kw["euler_kappa"])
    assert truss.Serialize() == before and not truss.isSolved
    ref = _reference(name, "pair", **run)
    b = sref.BATCH.index(name)
    assert _record()["full"]["configs"]["pair"]["decided"][b]
    assert (one["status"], one["iterations"]) == (ref["status"], ref["iterations"]) and one["status"] == 0
    tols = _floors("full", "pair", b)
    for key in FLOATS:
        assert np.shape(one[key]) == np.shape(ref[key]) and _scaled(one[key], ref[key]) <= tols[key], key
    assert one["governing"].shape == ref["governing"].shape and one["utilisation"].max() <= 1 + run["limit_tol"]
    plain = truss.MinimizeWeight(listed, limits, areaMin=kw["area_min"], areaMax=kw["area_max"], maxIters=2)
    assert "utilisation" not in plain and "governing" not in plain and "stress_history" not in plain
    with pytest.raises(ValueError, match="together"):
        truss.MinimizeWeight(listed, limits, areaMin=kw["area_min"], areaMax=kw["area_max"], allowTension=1.0)


def test_refusals():
    from python_stable_3d_truss_analysis_amd import batch
    packed, kw = _arguments(sref.BATCH[:3], "single")
    ok = dict(limit_case=[0], limit_joint=[1], limit_direction=[[0.0, -1.0, 0.0]], limit_value=1.0, area_min=0.1,
              area_max=10.0, allow_tension=1.0, allow_compression=1.0)
    with pytest.raises(ValueError, match="small-system"):
        batch.DeviceBatch(packed, use_small=True).min_weight(**ok)
    with pytest.raises(ValueError, match="compact"):
        batch.DeviceBatch(packed, use_small=False, options={"compact": True}).min_weight(**ok)
    with pytest.raises(ValueError, match="table member form"):
        batch.DeviceBatch(packed.table(), use_small=False).min_weight(**ok)
    db = batch.DeviceBatch(packed, use_small=False)
    for word, bad in (("together", {"allow_tension": None}), ("together", {"allow_compression": None}),
                      ("allow_tension", {"allow_tension": 0.0}), ("allow_compression", {"allow_compression": -1.0}),
                      ("allow_compression", {"allow_compression": np.array([1.0, 0.0, 1.0])}),
                      ("allow_tension", {"allow_tension": float("nan")}), ("allow_tension", {"allow_tension": -np.inf}),
                      ("euler_kappa", {"euler_kappa": -0.1}), ("euler_kappa", {"euler_kappa": float("inf")}),
                      ("allow_tension", {"allow_tension": np.ones(4)}), ("allow_tension", {"allow_tension": np.ones([3, 1])}),
                      ("allow_tension", {"allow_tension": "1"}), ("move", {"move": 1.5})):
        with pytest.raises(ValueError, match=word):
            db.min_weight(**dict(ok, **bad))
    with pytest.raises(ValueError, match="euler_kappa"):
        db.min_weight(**dict(ok, allow_tension=None, allow_compression=None, euler_kappa=0.1))
    for word, bad in (("together", {"allow_tension": None}), ("allow_compression", {"allow_compression": 0.0}),
                      ("euler_kappa", {"euler_kappa": -1.0}), ("allow_tension", {"allow_tension": np.ones(2)})):
        with pytest.raises(ValueError, match=word):
            batch.solve_min_weight(packed, **dict(kw, **bad))
