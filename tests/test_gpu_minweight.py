"""Minimum weight under displacement limits on the GPU (`DeviceBatch.min_weight`, `solve_min_weight`,
`Truss.MinimizeWeight`; C ABI include/trs_minweight.h) against the numpy yardstick `tests/minweight_reference.py`.

The parity tolerance of a truss is 100 x the largest max-scaled difference between the yardstick in float64 and in
longdouble on the same inputs, over its results (tests/golden/minweight_tol.json, which names them and keeps the figure
of every result; tests/test_minweight.py measures the small batch and the generated truss again; never less than
100 x FLOOR_LEAST) - what float64 itself loses, times the
project's margin for a different summation order.  The device's own output never sets a bound.  Every fixture keeps its
own limits and area bounds: inside one `DeviceBatch` they go in as one row per truss."""
import json
import os
import threading

import numpy as np
import pytest

from tests import minweight_reference as mref
from tests.helpers import GOLDEN, edge_cases, load_json

pytestmark = pytest.mark.gpu
FLOATS = mref.COMPARED
KEYS = FLOATS + ("iterations", "status")
DEPTH = {"tol": 0.0, "max_iters": mref.DEPTH}
GENERATED = mref.GENERATED

_cache = {}
_data, _arguments = mref.fixture, mref.batch_arguments


def _solver(name):
    return np.linalg.solve if name == mref.BIG else None      # (696 unknowns: a float64 run may use LAPACK)


def _reference(name, which, **run):
    key = (name, which, tuple(sorted(run.items())))
    if key not in _cache:
        data = _data(name)
        _cache[key] = mref.minimise(data, solve=_solver(name), **mref.config(data, which, solve=_solver(name)), **run)
    return _cache[key]


def _record():
    with open(os.path.join(GOLDEN, "minweight_tol.json")) as fh:
        rec = json.load(fh)
    assert rec["trusses"] == list(mref.BATCH) and rec["big_truss"] == mref.BIG
    return rec


def _floors(part, which, b=0):
    """key -> the tolerance of truss b of a part and configuration: 100 x the largest of the truss's own figures."""
    per = _record()[part]["configs"][which]["per_truss"][b]
    return dict.fromkeys(FLOATS, 100.0 * max(max(per.values()), mref.FLOOR_LEAST))


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
    """`min_weight` on ONE DeviceBatch over the trusses `names` (`rows`: only these of them).  Returns (numpy results,
    db)."""
    names = list(names) if rows is None else [names[r] for r in rows]
    packed, kw = _arguments(names, which)
    return _launch(packed, kw, dbkw, **run)


def _scaled(mine, ref):
    ref = np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max())
    diff = float(np.abs(np.asarray(mine) - ref).max())
    return diff if scale == 0 else diff / scale


def _compare(got, b, ref, tols, what, counts=True):
    """Truss b of the device results against its yardstick: every float result max-scaled within its tolerance, zeros
    on the padding."""
    nM, H = len(ref["areas"]), len(ref["measure_history"])
    if counts:
        assert (got["status"][b], got["iterations"][b]) == (ref["status"], ref["iterations"]), (what, got["status"][b],
                                                                                             got["iterations"][b])
    worst = {"areas": _scaled(got["areas"][b, :nM], ref["areas"]),
             "sensitivity": _scaled(got["sensitivity"][b, :, :nM], ref["sensitivity"])}
    for key in ("measure", "displacement", "ratio", "multipliers"):
        worst[key] = _scaled(got[key][b], ref[key])
    for key in ("measure_history", "worst_history"):
        worst[key] = _scaled(got[key][b, :H], ref[key])
    print(f"{what}: " + " ".join(f"{k} {v:.2e}/{tols[k]:.2e}" for k, v in worst.items())
          + f" status {got['status'][b]} iterations {got['iterations'][b]}")
    assert sorted(worst) == sorted(FLOATS)
    for key, value in worst.items():
        assert value <= tols[key], (what, key, value, tols[key])
    assert not got["areas"][b, nM:].any() and not got["sensitivity"][b, :, nM:].any(), what


def _same(a, b, what, rows_a=slice(None), rows_b=slice(None), nM=None, history=None):
    for key in KEYS + ("info",):
        x, y = a[key][rows_a], b[key][rows_b]
        if key in ("areas", "sensitivity"):
            x, y = x[..., :nM], y[..., :nM]
        if key in ("measure_history", "worst_history") and history is not None:   # (zero beyond the shorter run)
            assert not x[:, history:].any() and not y[:, history:].any(), (what, key)
            x, y = x[:, :history], y[:, :history]
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        same = np.array_equal(x.view(np.uint64), y.view(np.uint64)) if x.dtype == np.float64 else np.array_equal(x, y)
        assert same, (what, key)


@pytest.fixture(scope="module")
def full():
    """The ragged batch resized to tol 1e-4 within 100 iterations, both configurations."""
    return {which: _run(mref.BATCH, which, **mref.FULL)[0] for which in mref.CONFIGS}


# ---- 1. parity at a fixed depth ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(mref.CONFIGS))
def test_parity_at_a_fixed_depth(which):
    """bar-6 .. bar-120 in ONE DeviceBatch (ragged padding; bar-72 and bar-120 take more than one wave; bar-47 has
    members with c < 0; zero-force members end on lo), tol = 0, six resizings: status 1 and 6 iterations."""
    got, db = _run(mref.BATCH, which, **DEPTH)
    assert db.env is not None and not db.table
    assert (got["status"] == 1).all() and (got["iterations"] == mref.DEPTH).all() and not got["info"].any()
    ref47 = _reference("bar-47_input_0", which, **DEPTH)
    assert (ref47["sensitivity"][0] < 0).any()
    for b, name in enumerate(mref.BATCH):
        _compare(got, b, _reference(name, which, **DEPTH), _floors("depth", which, b), f"{which} {name}")


@pytest.mark.parametrize("which", sorted(mref.CONFIGS))
def test_parity_at_a_fixed_depth_on_the_large_truss(which):
    """bar-942 alone (n_free 696): four members per thread."""
    got, db = _run((mref.BIG,), which, **DEPTH)
    assert db.nM_max > 3 * 256
    _compare(got, 0, _reference(mref.BIG, which, **DEPTH), _floors("big", which), f"{which} bar-942")


@pytest.mark.parametrize("which", sorted(mref.CONFIGS))
def test_parity_at_a_fixed_depth_on_the_generated_truss(which):
    """A girder of 305 members: the second stride, and a last pass that not every thread takes."""
    got, db = _run((GENERATED,), which, **DEPTH)
    assert 256 < db.nM_max <= 512 and db.nM_max % 256
    _compare(got, 0, _reference(GENERATED, which, **DEPTH), _floors("generated", which), f"{which} generated")


# ---- 2. edge limits ------------------------------------------------------------------------------------------------------
def test_eight_limits_some_switched_off_and_one_on_a_held_dof():
    """J = 8 on three small trusses: the three limits of "pair", a limit on a held DOF (g = 0, mu = 0), the first limit
    at 0.9 of its value, and three more copies of which truss 0 has one at an infinite value and truss 1 one at joint
    -1.  Against the yardstick of every truss with its own eight limits; the tolerance is measured here, 100 x the
    float64-against-longdouble difference of these very runs."""
    names = mref.BATCH[:3]
    packed, kw = _arguments(names, "pair")
    B, J = len(names), 8
    wide = {"limit_case": np.zeros(J, dtype=np.int64), "limit_joint": np.zeros([B, J], dtype=np.int64),
            "limit_direction": np.zeros([B, J, 3]), "limit_value": np.zeros([B, J])}
    source = [0, 1, 2, 0, 0, 1, 1, 0]
    for j, s in enumerate(source):
        wide["limit_case"][j] = kw["limit_case"][s]
        for key in ("limit_joint", "limit_direction", "limit_value"):
            wide[key][:, j] = kw[key][:, s]
    wide["limit_value"][:, 4] *= 0.9
    wide["limit_value"][0, 5] = np.inf
    wide["limit_joint"][1, 6] = -1
    held = []
    for b, name in enumerate(names):
        geo = mref.Geometry(load_json(name), np.float64)
        dof = int(np.flatnonzero(~geo.mask)[0])
        held.append(divmod(dof, geo.dim))
        wide["limit_joint"][b, 3] = held[b][0]
        wide["limit_direction"][b, 3] = 0.0
        wide["limit_direction"][b, 3, held[b][1]] = 1.0
        wide["limit_value"][b, 3] = 1.0
    got, _ = _launch(packed, dict(kw, **wide), **DEPTH)
    for b, name in enumerate(names):
        data = load_json(name)
        one = mref.config(data, "pair")
        dim = one["loads"].shape[2]
        one["limits"] = [(int(wide["limit_case"][j]), int(wide["limit_joint"][b, j]), wide["limit_direction"][b, j, :dim],
                          float(wide["limit_value"][b, j])) for j in range(J)]
        f64 = mref.minimise(data, **one, **DEPTH)
        f80 = mref.minimise(data, dtype=np.longdouble, **one, **DEPTH)
        tols = dict.fromkeys(FLOATS, 100.0 * max(mref.relative_difference(f64, f80), mref.FLOOR_LEAST))
        _compare(got, b, f64, tols, f"eight limits {name}")
        assert got["displacement"][b, 3] == 0.0 and got["multipliers"][b, 3] == 0.0 and got["ratio"][b, 3] == 0.0
        assert not got["sensitivity"][b, 3].any()
    assert got["ratio"][0, 5] == 0.0 and got["multipliers"][0, 5] == 0.0 and not got["sensitivity"][0, 5].any()
    assert got["ratio"][1, 6] == 0.0 and got["displacement"][1, 6] == 0.0 and not got["sensitivity"][1, 6].any()
    assert got["ratio"][1, 5] != 0.0 and got["ratio"][0, 6] != 0.0


# ---- 3. statuses and counts ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(mref.CONFIGS))
def test_statuses_and_counts(full, which):
    """Status and iterations equal the yardstick's for every truss of which tests/golden/minweight_tol.json records that
    no `change` of its run lies within 1 % of `tol` and no `worst` within 1 % of 1 + limit_tol (tests/test_minweight.py
    measures that again); where such a truss converged its results agree too (a run that ends at the iteration limit is
    compared in status and count alone: bar-25 and bar-120 under "pair" wander inside their move limits)."""
    got = full[which]
    entry = _record()["full"]["configs"][which]
    assert sum(entry["decided"]) >= 4
    for b, name in enumerate(mref.BATCH):
        ref = _reference(name, which, **mref.FULL)
        assert (ref["status"], ref["iterations"]) == (entry["status"][b], entry["iterations"][b]), (which, name)
        if not entry["decided"][b]:
            print(f"{which} {name}: not decided - the count is not compared; device status {got['status'][b]} iterations "
                  f"{got['iterations'][b]}, yardstick {ref['status']} {ref['iterations']}")
        elif ref["status"] == mref.CONVERGED:
            _compare(got, b, ref, _floors("full", which, b), f"{which} {name}")
            assert got["worst_history"][b, got["iterations"][b]] <= 1 + mref.FULL["limit_tol"]
        else:
            assert (got["status"][b], got["iterations"][b]) == (ref["status"], ref["iterations"]), (which, name)
    if which == "pair":
        assert sorted(set(got["status"].tolist())) == [0, 1]      # the batch mixes converged trusses and the limit
    n = got["iterations"] + 1
    for b in range(len(mref.BATCH)):
        assert not got["measure_history"][b, n[b]:].any() and not got["worst_history"][b, n[b]:].any(), b
        assert got["measure_history"][b, n[b] - 1] == got["measure"][b], b


# ---- 4. the determinate truss --------------------------------------------------------------------------------------------
def test_determinate_truss():
    """The closed form after ONE resizing with move 1 from a design within a factor 2 of it; converged at the next
    analysis (as the yardstick: tests/test_minweight.py)."""
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    from tests.test_minweight import DETERMINATE, DETERMINATE_START, determinate, determinate_answer
    loads, limits, want, weight = determinate_answer()
    data = determinate()
    for member, area in zip(data["member"], DETERMINATE_START * want):
        member[1][0] = float(area)
    db = batch.DeviceBatch(batch.pack_json([data]), use_small=False)
    (case, joint, d, value), = limits
    out = _host(db.min_weight(limit_case=[case], limit_joint=[joint], limit_direction=[d], limit_value=value, **DETERMINATE))
    assert out["status"][0] == 0 and out["iterations"][0] == 1
    assert np.abs(out["areas"][0] - want).max() <= 1e-12 * want.max()
    assert abs(out["measure"][0] - weight) <= 1e-12 * weight and abs(out["ratio"][0, 0] - 1.0) <= 1e-12
    assert out["measure_history"][0, 1] == out["measure"][0] and not out["measure_history"][0, 2:].any()
    assert torch.equal(db.A, torch.from_numpy(out["areas"]).to(db.device)) and "sensitivity" not in out


# ---- 5. status 3 -----------------------------------------------------------------------------------------------------------
def test_a_truss_whose_area_max_cannot_meet_its_limit():
    """Every member of the middle truss may grow by 5 % at most, its limit asks for half the displacement: it converges
    on its bounds with worst near 1.9 and status 3; the neighbours keep the bits of a run without the cap."""
    names = mref.BATCH[:3]
    packed, kw = _arguments(names, "single")
    capped = dict(kw, area_max=kw["area_max"].copy())
    nM = len(load_json(names[1])["member"])
    capped["area_max"][1, :nM] = 1.05 * packed.A[1, :nM]
    got, _ = _launch(packed, capped, **mref.FULL)
    clean, _ = _launch(packed, kw, **mref.FULL)
    assert got["status"].tolist() == [0, 3, 0] and clean["status"].tolist() == [0, 0, 0]
    assert got["ratio"][1, 0] > 1.5      # (the yardstick: 1 / 1.05 of the initial 2)
    assert (got["areas"][1, :nM] <= capped["area_max"][1, :nM]).all()
    _same(got, clean, "neighbours of status 3", rows_a=[0, 2], rows_b=[0, 2])


# ---- 6. independence, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 3, 5])
def test_a_truss_alone_has_the_bits_it_has_in_the_batch(full, b):
    alone, _ = _run(mref.BATCH, "pair", rows=[b], **mref.FULL)
    nM = len(load_json(mref.BATCH[b])["member"])
    _same(full["pair"], alone, mref.BATCH[b], rows_a=slice(b, b + 1), nM=nM)


def test_results_depend_neither_on_check_every_nor_on_max_iters(full):
    sparse, _ = _run(mref.BATCH, "pair", **dict(mref.FULL, check_every=7))
    _same(full["pair"], sparse, "check_every 7")
    longer, _ = _run(mref.BATCH, "pair", **dict(mref.FULL, max_iters=110))
    done = np.flatnonzero(full["pair"]["status"] == 0)
    assert len(done) >= 2
    _same(full["pair"], longer, "max_iters 110", rows_a=done, rows_b=done, history=mref.FULL["max_iters"] + 1)


def test_two_streams_at_once_give_the_bits_of_one_after_the_other():
    """`min_weight` waits for its own stream at every look at the active count, so each run has a host thread of its
    own (a stream context is per thread) and the two interleave on the device."""
    import torch
    halves = (mref.BATCH[:3], mref.BATCH[3:])
    one_by_one = [_run(names, "single", **mref.FULL)[0] for names in halves]
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs, errors = [None, None], []
    ready = threading.Barrier(2)

    def work(k):
        try:
            with torch.cuda.stream(streams[k]):
                ready.wait(timeout=60)
                for _ in range(2):
                    outs[k] = _run(halves[k], "single", **mref.FULL)[0]
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


# ---- 7. the factor left behind -------------------------------------------------------------------------------------------
def test_the_factor_left_behind_serves_solve_cases():
    """`displacement` equals d.u(joint) of a `solve_cases` that follows without a `factor()`."""
    import torch
    packed, kw = _arguments(mref.BATCH, "pair")
    got, db = _run(mref.BATCH, "pair", **mref.FULL)
    assert db.generation >= 1
    u = db.solve_cases(torch.from_numpy(kw["loads"]).to(db.device))["u"].cpu().numpy()     # no factor() in between
    A = db.A.cpu().numpy()
    for b, name in enumerate(mref.BATCH):
        nM = len(load_json(name)["member"])
        assert np.array_equal(A[b, :nM].view(np.uint64), got["areas"][b, :nM].view(np.uint64)), name
        g = np.array([(kw["limit_direction"][b, j] * u[b, kw["limit_case"][j], kw["limit_joint"][b, j]]).sum()
                      for j in range(len(kw["limit_case"]))])
        tol = _floors("full", "pair", b)["displacement"]
        assert _scaled(got["displacement"][b], g) <= tol, (name, _scaled(got["displacement"][b], g), tol)


# ---- 8. a truss that cannot be factored ----------------------------------------------------------------------------------
def test_a_mechanism_among_healthy_trusses():
    """status 2 with 0 iterations, its initial areas and a nonzero info - an ordinary info != 0, not a fault; the
    neighbours keep the bits of a run without it."""
    from python_stable_3d_truss_analysis_amd import batch
    names = ("bar-25_input_0", "bar-72_input_0")
    bad = edge_cases()["3d_mechanism_singular"]["input"]
    packed2, kw2 = _arguments(names, "single")
    packed3 = batch.pack_json([load_json(names[0]), bad, load_json(names[1])])
    assert (packed3.nJ_max, packed3.nM_max) == (packed2.nJ_max, packed2.nM_max)
    kw3 = dict(kw2)
    for key in ("loads", "area_min", "area_max", "limit_joint", "limit_direction", "limit_value"):
        row = np.ones_like(kw2[key][:1])
        if key == "loads":
            row[:] = 0.0
            row[0, 0, 2, 2] = -10.0
        kw3[key] = np.concatenate([kw2[key][:1], row, kw2[key][1:]], axis=0)
    kw3["area_min"][1], kw3["area_max"][1] = 0.1, 10.0
    outs = []
    for packed, kw in ((packed3, kw3), (packed2, kw2)):
        got, db = _launch(packed, kw, **mref.FULL)
        outs.append(dict(got, A=db.A.cpu().numpy()))
    got, clean = outs
    assert got["status"][1] == 2 and got["iterations"][1] == 0 and got["info"][1] != 0
    nM = len(bad["member"])
    initial = np.array([m[1][0] for m in bad["member"]])
    assert np.array_equal(got["areas"][1, :nM], initial) and np.array_equal(got["A"][1, :nM], initial)
    for key in ("sensitivity", "measure", "measure_history", "worst_history", "displacement", "ratio", "multipliers"):
        assert not np.any(got[key][1]), key
    assert list(clean["status"]) == [0, 0] and not clean["info"].any()
    _same(got, clean, "neighbours", rows_a=[0, 2])


# ---- 9. the composition with the stress sizing ---------------------------------------------------------------------------
def test_stress_sizing_first_then_its_areas_as_area_min():
    """`sizing` with stress limits only, then `min_weight` with those areas as `area_min`, on bar-6 and bar-10: the
    result is within the displacement limit (status 0) and within the stress allowables (the yardstick's utilisation
    of the composed design is 0.90 and 0.94), and it is no heavier than `sizing` with the displacement envelope at the
    same value.  (The composition does not GUARANTEE the stress limits on a redundant truss - growing members draw
    force: the yardstick gives 1.11 on bar-25, DESIGN 3s - so the stress check afterwards is part of it.)"""
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    from tests import sizing_reference as sref
    names = mref.BATCH[:2]
    packed, kw = _arguments(names, "single")
    allow = {"allow_tension": np.zeros(len(names)), "allow_compression": np.zeros(len(names))}
    for b, name in enumerate(names):
        one = sref.config(load_json(name), "stress")
        allow["allow_tension"][b], allow["allow_compression"][b] = one["allow_tension"], one["allow_compression"]
    db = batch.DeviceBatch(packed, use_small=False)
    dev_kw = _on_device(torch, db.device, kw)
    bounds = dict(area_min=dev_kw["area_min"], area_max=dev_kw["area_max"])
    stress = db.sizing(dev_kw["loads"], **allow, **bounds, tol=1e-4, max_iters=60)
    assert (stress["status"].cpu().numpy() == 0).all()
    sized = stress["areas"].clone()
    live = torch.from_numpy(np.arange(packed.nM_max)[None, :] < packed.nM[:, None]).to(db.device)
    floor = torch.where(live, sized, dev_kw["area_min"])
    limits = {k: kw[k] for k in ("limit_case", "limit_joint", "limit_direction", "limit_value")}
    light = _host(db.min_weight(dev_kw["loads"], **limits, move=mref.MOVE, area_min=floor, area_max=dev_kw["area_max"],
                                **mref.FULL))
    assert (light["status"] == 0).all() and (light["ratio"][:, 0] <= 1 + mref.FULL["limit_tol"]).all()
    assert (light["areas"] >= sized.cpu().numpy() * (1 - 1e-12)).all()
    # feasible in the stress sense: one more stress analysis of the returned design asks for no growth
    db2 = batch.DeviceBatch(packed, use_small=False)
    db2.A.copy_(torch.from_numpy(light["areas"]).to(db2.device))
    check = _host(db2.sizing(dev_kw["loads"], **allow, **bounds, tol=1e-4, max_iters=0))
    print("composition: utilisation", check["utilisation"].max(axis=1))
    assert (check["utilisation"].max(axis=1) <= 1.0).all()
    db3 = batch.DeviceBatch(packed, use_small=False)
    envelope = _host(db3.sizing(dev_kw["loads"], **allow, allow_displace=kw["limit_value"][:, 0].copy(), **bounds,
                                tol=1e-4, max_iters=60))
    print("composition: weight", light["measure"], "envelope", envelope["weight"])
    assert (light["measure"] <= envelope["weight"] * (1 + 1e-9)).all()


# ---- 10. the public layers -------------------------------------------------------------------------------------------------
def test_solve_min_weight_over_buckets_orders_and_member_forms():
    from python_stable_3d_truss_analysis_amd import batch
    names = ("bar-25_input_0", "bar-72_input_0", mref.BIG)
    packed, kw = _arguments(names, "pair")
    small = 1 << 20
    assert len(batch.size_buckets(packed, small)) >= 2
    direct, _ = _run(names, "pair", **DEPTH)

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
        tols = _floors("big", "pair") if name == mref.BIG else _floors("depth", "pair", mref.BATCH.index(name))
        _compare(ordered, b, _reference(name, "pair", **DEPTH), tols, f"reorder {name}")
        _compare(bucketed, b, _reference(name, "pair", **DEPTH), tols, f"buckets {name}")
    assert batch.solve_min_weight(packed, **kw, **DEPTH).sensitivity is None


def test_truss_minimize_weight():
    from python_stable_3d_truss_analysis_amd import Truss
    name = "bar-72_input_0"
    data = load_json(name)
    kw = mref.config(data, "pair")
    truss = Truss(3).LoadFromJSON(data=data)
    before = truss.Serialize()
    listed = [{j: tuple(f[j]) for j in range(len(f)) if np.any(f[j] != 0)} for f in kw["loads"]]
    limits = [(case, joint, tuple(2.0 * d), value) for case, joint, d, value in kw["limits"]]
    run = {k: v for k, v in mref.FULL.items()}
    one = truss.MinimizeWeight(listed, limits, move=mref.MOVE, areaMin=kw["area_min"], areaMax=kw["area_max"], tol=run["tol"],
                               maxIters=run["max_iters"], limitTol=run["limit_tol"], returnSensitivity=True)
    assert truss.Serialize() == before and not truss.isSolved
    ref = _reference(name, "pair", **mref.FULL)
    b = mref.BATCH.index(name)
    assert _record()["full"]["configs"]["pair"]["decided"][b]
    assert (one["status"], one["iterations"]) == (ref["status"], ref["iterations"]) == (0, 59)
    tols = _floors("full", "pair", b)
    for key in FLOATS:
        assert np.shape(one[key]) == np.shape(ref[key]) and _scaled(one[key], ref[key]) <= tols[key], key
    with pytest.raises(ValueError, match="limit_value"):
        truss.MinimizeWeight(listed, [(0, 1, (0.0, 0.0, 1.0), -1.0)], areaMin=kw["area_min"], areaMax=kw["area_max"])
    with pytest.raises(ValueError, match="limits"):
        truss.MinimizeWeight(listed, [(0, 1, (0.0, 1.0), 1.0)], areaMin=kw["area_min"], areaMax=kw["area_max"])


def test_refusals():
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    packed, kw = _arguments(mref.BATCH[:3], "single")
    ok = dict(limit_case=[0], limit_joint=[1], limit_direction=[[0.0, -1.0, 0.0]], limit_value=1.0, area_min=0.1,
              area_max=10.0)
    with pytest.raises(ValueError, match="small-system"):
        batch.DeviceBatch(packed, use_small=True).min_weight(**ok)
    with pytest.raises(ValueError, match="compact"):
        batch.DeviceBatch(packed, use_small=False, options={"compact": True}).min_weight(**ok)
    with pytest.raises(ValueError, match="table member form"):
        batch.DeviceBatch(packed.table(), use_small=False).min_weight(**ok)
    db = batch.DeviceBatch(packed, use_small=False)
    for word, bad in (("move", {"move": 1.5}), ("limit_case", {"limit_case": [1]}), ("limit_case", {"limit_case": [0] * 9}),
                      ("limit_joint", {"limit_joint": [packed.nJ_max]}), ("limit_value", {"limit_value": -1.0}),
                      ("limit_direction", {"limit_direction": [[0.0, 0.0, 0.0]]}), ("measure", {"measure": "mass"}),
                      ("sweeps", {"sweeps": 0}), ("limit_tol", {"limit_tol": -0.1}), ("area_max", {"area_max": 0.01}),
                      ("max_iters", {"max_iters": -1})):
        with pytest.raises(ValueError, match=word):
            db.min_weight(**dict(ok, **bad))
    with pytest.raises(ValueError, match="out\\['areas'\\]"):
        db.min_weight(**ok, out={"areas": torch.zeros([1], device=db.device)})
    with pytest.raises(ValueError, match="sections"):
        batch.solve_min_weight(packed, **kw, sections=[(1.0, 1.0, 1.0)])
    import dataclasses
    light = dataclasses.replace(packed, rho=packed.rho.copy())
    light.rho[0, 0] = 0.0
    with pytest.raises(ValueError, match="rho <= 0"):
        batch.solve_min_weight(light, **kw)
