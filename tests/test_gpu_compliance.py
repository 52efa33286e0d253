"""Compliance sizing on the GPU (`DeviceBatch.min_compliance`, `solve_min_compliance`, `Truss.MinimizeCompliance`; C ABI
include/trs_compliance.h) against the numpy yardstick `tests/compliance_reference.py`.

The parity tolerance is 100 x the largest max-scaled difference between the yardstick in float64 and in longdouble on
the same inputs (tests/golden/compliance_tol.json, which names them; tests/test_compliance.py measures the small batch
and the generated truss again) - what float64 itself loses, times the project's margin for a different summation order.
The device's own output never sets a bound.  Every fixture keeps its own area bounds (1e-3 of ITS smallest and 1000 x
ITS largest initial area) and its own target, its initial weight: inside one `DeviceBatch` the bounds go in as one row
per truss and the targets are left to the kernel."""
import json
import os
import threading

import numpy as np
import pytest

from tests import compliance_reference as cref
from tests.helpers import GOLDEN, edge_cases, load_json
from tests.test_compliance import DETERMINATE, DETERMINATE_START, determinate, determinate_answer

pytestmark = pytest.mark.gpu
FLOATS = ("areas", "measure", "compliance", "objective", "objective_history", "sensitivity", "multiplier")
KEYS = FLOATS + ("iterations", "status")
DEPTH = {"tol": 0.0, "max_iters": cref.DEPTH}
GENERATED, WIDE = cref.GENERATED, cref.WIDE

_cache = {}


_data, _arguments = cref.fixture, cref.batch_arguments


def _solver(name):
    return np.linalg.solve if name in (cref.BIG, WIDE) else None      # (696, 1041 unknowns: a float64 run may use LAPACK)


def _reference(name, which, **run):
    key = (name, which, tuple(sorted(run.items())))
    if key not in _cache:
        data = _data(name)
        _cache[key] = cref.minimise(data, solve=_solver(name), **cref.config(data, which), **run)
    return _cache[key]


def _record():
    with open(os.path.join(GOLDEN, "compliance_tol.json")) as fh:
        rec = json.load(fh)
    assert rec["trusses"] == list(cref.BATCH) and rec["big_truss"] == cref.BIG
    return rec


def _floor(part, which):
    return 100.0 * _record()[part]["configs"][which]["relative_difference"]


def _on_device(torch, dev, kw):
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return dict(kw, loads=up(kw["loads"]), area_min=up(kw["area_min"]), area_max=up(kw["area_max"]))


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _run(names, which, rows=None, dbkw=None, **run):
    """`min_compliance` on ONE DeviceBatch over the trusses `names` (`rows`: only these of them).  Returns (numpy
    results, db)."""
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    names = list(names) if rows is None else [names[r] for r in rows]
    packed, kw = _arguments(names, which)
    db = batch.DeviceBatch(packed, use_small=False, **(dbkw or {}))
    out = db.min_compliance(**_on_device(torch, db.device, kw), **run)
    torch.cuda.synchronize(db.device)
    return dict(_host(out), info=db.info.cpu().numpy()), db


def _scaled(mine, ref):
    ref = np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max())
    diff = float(np.abs(np.asarray(mine) - ref).max())
    return diff if scale == 0 else diff / scale


def _compare(got, b, ref, tol, what, counts=True):
    """Truss b of the device results against its yardstick: every float result max-scaled within `tol`, zeros on the
    padding."""
    nM = len(ref["areas"])
    if counts:
        assert (got["status"][b], got["iterations"][b]) == (ref["status"], ref["iterations"]), (what, got["status"][b],
                                                                                             got["iterations"][b])
    worst = {key: _scaled(got[key][b, :nM], ref[key]) for key in ("areas", "sensitivity")}
    for key in ("measure", "compliance", "objective", "multiplier"):
        worst[key] = _scaled(got[key][b], ref[key])
    H = len(ref["objective_history"])
    worst["objective_history"] = _scaled(got["objective_history"][b, :H], ref["objective_history"])
    print(f"{what}: tol {tol:.2e} worst " + " ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + f" status {got['status'][b]} iterations {got['iterations'][b]}")
    assert sorted(worst) == sorted(FLOATS)
    for key, value in worst.items():
        assert value <= tol, (what, key, value, tol)
    assert not got["areas"][b, nM:].any() and not got["sensitivity"][b, nM:].any(), what


def _same(a, b, what, rows_a=slice(None), rows_b=slice(None), nM=None, history=None):
    for key in KEYS + ("info",):
        x, y = a[key][rows_a], b[key][rows_b]
        if key in ("areas", "sensitivity"):
            x, y = x[:, :nM], y[:, :nM]
        if key == "objective_history" and history is not None:   # (runs of different max_iters: zero beyond the shorter)
            assert not x[:, history:].any() and not y[:, history:].any(), (what, key)
            x, y = x[:, :history], y[:, :history]
        same = np.array_equal(x.view(np.uint64), y.view(np.uint64)) if x.dtype == np.float64 else np.array_equal(x, y)
        assert same, (what, key)


@pytest.fixture(scope="module")
def full():
    """The ragged batch resized to tol 1e-4 within 60 iterations, both configurations."""
    return {which: _run(cref.BATCH, which, **cref.FULL)[0] for which in cref.CONFIGS}


# ---- 1. parity at a fixed depth ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(cref.CONFIGS))
def test_parity_at_a_fixed_depth(which):
    """bar-6 .. bar-120 in ONE DeviceBatch (ragged padding; bar-72 and bar-120 take more than one wave), tol = 0, six
    resizings: every truss ends with status 1 and 6 iterations."""
    got, db = _run(cref.BATCH, which, **DEPTH)
    assert db.env is not None and not db.table
    assert (got["status"] == 1).all() and (got["iterations"] == cref.DEPTH).all() and not got["info"].any()
    tol = _floor("depth", which)
    for b, name in enumerate(cref.BATCH):
        _compare(got, b, _reference(name, which, **DEPTH), tol, f"{which} {name}")


@pytest.mark.parametrize("which", sorted(cref.CONFIGS))
def test_parity_at_a_fixed_depth_on_the_large_truss(which):
    """bar-942 alone (n_free 696): four members per thread."""
    got, db = _run((cref.BIG,), which, **DEPTH)
    assert db.nM_max > 3 * 256
    _compare(got, 0, _reference(cref.BIG, which, **DEPTH), _floor("big", which), f"{which} bar-942")


@pytest.mark.parametrize("which", sorted(cref.CONFIGS))
def test_parity_at_a_fixed_depth_on_the_generated_truss(which):
    """A girder of 305 members: the second stride, and a last pass that not every thread takes."""
    got, db = _run((GENERATED,), which, **DEPTH)
    assert 256 < db.nM_max <= 512 and db.nM_max % 256
    _compare(got, 0, _reference(GENERATED, which, **DEPTH), _floor("generated", which), f"{which} generated")


# ---- 2. statuses and counts ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(cref.CONFIGS))
def test_statuses_and_counts(full, which):
    """Status and iterations equal the yardstick's for every truss of which tests/golden/compliance_tol.json records that
    no `change` of its run lies within 1 % of `tol` (tests/test_compliance.py measures that again); the results agree."""
    got = full[which]
    entry = _record()["full"]["configs"][which]
    tol = _floor("full", which)
    assert sum(entry["decided"]) >= 4
    for b, name in enumerate(cref.BATCH):
        ref = _reference(name, which, **cref.FULL)
        assert (ref["status"], ref["iterations"]) == (entry["status"][b], entry["iterations"][b]), (which, name)
        if entry["decided"][b]:
            _compare(got, b, ref, tol, f"{which} {name}")
        else:
            print(f"{which} {name}: a change within 1 % of tol - the count is not compared; device status "
                  f"{got['status'][b]} iterations {got['iterations'][b]}, yardstick {ref['status']} {ref['iterations']}")
    assert sorted(set(got["status"].tolist())) == [0, 1]      # the batch mixes converged trusses and the limit
    n = got["iterations"] + 1
    for b in range(len(cref.BATCH)):
        # the yardstick's history never rises and the device's lies within tol of it: no rise beyond 2 tol of the largest
        history = got["objective_history"][b]
        assert (np.diff(history[:n[b]]) <= 2 * tol * history[0]).all() and not history[n[b]:].any(), b
        assert history[n[b] - 1] == got["objective"][b] and history[n[b] - 1] < 0.9 * history[0], b


# ---- 3. the determinate truss --------------------------------------------------------------------------------------------
def test_determinate_truss():
    """The closed form A_m = c |N_m| / sqrt(E_m rho_m) after ONE resizing with move 1 from a design within a factor 2 of
    it, at an explicit target; converged at the next analysis (as the yardstick: tests/test_compliance.py)."""
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    want = determinate_answer(DETERMINATE["target"])
    data = determinate()
    for member, area in zip(data["member"], DETERMINATE_START * want):
        member[1][0] = float(area)
    db = batch.DeviceBatch(batch.pack_json([data]), use_small=False)
    out = _host(db.min_compliance(**DETERMINATE))
    assert out["status"][0] == 0 and out["iterations"][0] == 1
    assert np.abs(out["areas"][0] - want).max() <= 1e-12 * want.max()
    assert abs(out["measure"][0] - DETERMINATE["target"]) <= 1e-12 * DETERMINATE["target"]
    assert out["objective_history"][0, 1] == out["objective"][0] and not out["objective_history"][0, 2:].any()
    assert torch.equal(db.A, torch.from_numpy(out["areas"]).to(db.device))
    # the volume as the measure: A_m = c |N_m| / sqrt(E_m), at a target per truss
    vol = _host(db.min_compliance(**dict(DETERMINATE, measure="volume", target=np.array([7.0]))))
    geo = cref.Geometry(data, np.float64)
    shape = want * np.sqrt(geo.rho)
    assert vol["status"][0] == 0 and abs(vol["measure"][0] - 7.0) <= 1e-12 * 7.0
    assert np.abs(vol["areas"][0] - shape * (7.0 / (shape * geo.L0).sum())).max() <= 1e-12 * vol["areas"][0].max()


# ---- 4. independence, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 3, 5])
def test_a_truss_alone_has_the_bits_it_has_in_the_batch(full, b):
    alone, _ = _run(cref.BATCH, "weighted", rows=[b], **cref.FULL)
    nM = len(load_json(cref.BATCH[b])["member"])
    _same(full["weighted"], alone, cref.BATCH[b], rows_a=slice(b, b + 1), nM=nM)


def test_results_depend_neither_on_check_every_nor_on_max_iters(full):
    sparse, _ = _run(cref.BATCH, "weighted", **dict(cref.FULL, check_every=7))
    _same(full["weighted"], sparse, "check_every 7")
    longer, _ = _run(cref.BATCH, "weighted", **dict(cref.FULL, max_iters=75))
    done = np.flatnonzero(full["weighted"]["status"] == 0)
    assert len(done) >= 2
    _same(full["weighted"], longer, "max_iters 75", rows_a=done, rows_b=done, history=cref.FULL["max_iters"] + 1)


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_the_search_gives_the_same_bits_at_every_number_of_levels(full, levels):
    """One, two or three levels of the bisection per round take the decisions of the definition on the same operands."""
    got, _ = _run(cref.BATCH, "weighted", levels=levels, **cref.FULL)
    _same(full["weighted"], got, f"levels {levels}")
    big = [_run((cref.BIG,), "single", levels=k, **DEPTH)[0] for k in (0, levels)]
    _same(big[0], big[1], f"bar-942 levels {levels}")


def test_a_batch_of_more_than_1024_members_gives_the_same_bits(full):
    """Above 4 x 256 members per truss the bisection reads p, lo, hi, w from LDS instead of holding them in registers -
    decided by the batch's nM_max, so the six fixtures beside a girder of 1128 members take that path: the bits of the
    narrow batch.  The girder itself (five members per thread) keeps its measure at the target and its objective
    falling, and alone at depth 6 it meets the yardstick within 100 x its own recorded floor."""
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    wide = _data(WIDE)
    datas = [load_json(n) for n in cref.BATCH] + [wide]
    packed = batch.pack_json(datas)
    assert packed.nM_max == len(wide["member"]) == 1128
    _, narrow = _arguments(cref.BATCH, "weighted")
    B, nJ, nM = packed.B, packed.nJ_max, packed.nM_max
    one = cref.config(wide, "weighted")
    kw = {"loads": np.zeros([B, 2, nJ, 3]), "alpha": narrow["alpha"], "area_min": np.ones([B, nM]),
          "area_max": np.ones([B, nM])}
    kw["loads"][:-1, :, :narrow["loads"].shape[2]] = narrow["loads"]
    kw["loads"][-1, :, :, :2] = one["loads"]
    for key in ("area_min", "area_max"):
        kw[key][:-1] = narrow[key][:, :1]
        kw[key][-1] = one[key]
    db = batch.DeviceBatch(packed, use_small=False)
    got = _host(db.min_compliance(**_on_device(torch, db.device, kw), **cref.FULL))
    got["info"] = db.info.cpu().numpy()
    for b, name in enumerate(cref.BATCH):
        _same(full["weighted"], got, f"wide {name}", rows_a=slice(b, b + 1), rows_b=slice(b, b + 1),
              nM=len(load_json(name)["member"]))
    n = got["iterations"][-1] + 1
    history = got["objective_history"][-1, :n]
    geo = cref.Geometry(wide, np.float64)
    target = float((geo.A0 * geo.L0 * geo.rho).sum())
    assert got["status"][-1] in (0, 1) and n > 10 and got["info"][-1] == 0
    assert abs(got["measure"][-1] / target - 1.0) <= 1e-12
    assert abs((got["areas"][-1] * geo.L0 * geo.rho).sum() / target - 1.0) <= 1e-12
    # the yardstick's history of this run never rises and ends at 0.30 of its start; the device's lies within tol of it
    tol = _floor("wide", "weighted")
    assert (np.diff(history) <= 2 * tol * history[0]).all() and history[-1] < 0.9 * history[0]
    alone, db = _run((WIDE,), "weighted", **DEPTH)
    assert db.nM_max > 4 * 256
    _compare(alone, 0, _reference(WIDE, "weighted", **DEPTH), tol, "weighted wide")


def test_two_streams_at_once_give_the_bits_of_one_after_the_other():
    """`min_compliance` waits for its own stream at every look at the active count, so each run has a host thread of its
    own (a stream context is per thread) and the two interleave on the device."""
    import torch
    halves = (cref.BATCH[:3], cref.BATCH[3:])
    one_by_one = [_run(names, "single", **cref.FULL)[0] for names in halves]
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs, errors = [None, None], []
    ready = threading.Barrier(2)

    def work(k):
        try:
            with torch.cuda.stream(streams[k]):
                ready.wait(timeout=60)
                for _ in range(2):
                    outs[k] = _run(halves[k], "single", **cref.FULL)[0]
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


# ---- 5. the factor left behind -------------------------------------------------------------------------------------------
def test_the_factor_left_behind_serves_solve_cases():
    """`compliance` (twice the strain energy) equals f.u of a `solve_cases` that follows without a `factor()`."""
    import torch
    packed, kw = _arguments(cref.BATCH, "weighted")
    got, db = _run(cref.BATCH, "weighted", **cref.FULL)
    assert db.generation >= 1
    loads = torch.from_numpy(kw["loads"]).to(db.device)
    u = db.solve_cases(loads)["u"].cpu().numpy()                    # no factor() in between
    A = db.A.cpu().numpy()
    tol = _floor("full", "weighted")
    for b, name in enumerate(cref.BATCH):
        nM = len(load_json(name)["member"])
        assert np.array_equal(A[b, :nM].view(np.uint64), got["areas"][b, :nM].view(np.uint64)), name
        work = (kw["loads"][b] * u[b]).sum(axis=(1, 2))
        assert _scaled(got["compliance"][b], work) <= tol, (name, _scaled(got["compliance"][b], work))


# ---- 6. a truss that cannot be factored ----------------------------------------------------------------------------------
def test_a_mechanism_among_healthy_trusses():
    """status 2 with 0 iterations, its initial areas and a nonzero info - an ordinary info != 0, not a fault; the
    neighbours keep the bits of a run without it."""
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    names = ("bar-25_input_0", "bar-72_input_0")
    bad = edge_cases()["3d_mechanism_singular"]["input"]
    packed2, kw2 = _arguments(names, "single")
    packed3 = batch.pack_json([load_json(names[0]), bad, load_json(names[1])])
    assert (packed3.nJ_max, packed3.nM_max) == (packed2.nJ_max, packed2.nM_max)
    kw3 = {"alpha": kw2["alpha"]}
    for key in ("loads", "area_min", "area_max"):
        row = np.ones_like(kw2[key][:1])
        if key == "loads":
            row[:] = 0.0
            row[0, 0, 2, 2] = -10.0
        kw3[key] = np.concatenate([kw2[key][:1], row, kw2[key][1:]], axis=0)
    kw3["area_min"][1], kw3["area_max"][1] = 0.1, 10.0
    outs = []
    for packed, kw in ((packed3, kw3), (packed2, kw2)):
        db = batch.DeviceBatch(packed, use_small=False)
        out = db.min_compliance(**_on_device(torch, db.device, kw), **cref.FULL)
        torch.cuda.synchronize(db.device)
        outs.append(dict(_host(out), info=db.info.cpu().numpy(), A=db.A.cpu().numpy()))
    got, clean = outs
    assert got["status"][1] == 2 and got["iterations"][1] == 0 and got["info"][1] != 0
    nM = len(bad["member"])
    initial = np.array([m[1][0] for m in bad["member"]])
    assert np.array_equal(got["areas"][1, :nM], initial) and np.array_equal(got["A"][1, :nM], initial)
    for key in ("sensitivity", "measure", "compliance", "objective", "objective_history", "multiplier"):
        assert not np.any(got[key][1]), key
    assert list(clean["status"]) == [0, 0] and not clean["info"].any()
    _same(got, clean, "neighbours", rows_a=[0, 2])


# ---- 7. the public layers --------------------------------------------------------------------------------------------------
def test_solve_min_compliance_over_buckets_orders_and_member_forms():
    from python_stable_3d_truss_analysis_amd import batch
    names = ("bar-25_input_0", "bar-72_input_0", cref.BIG)
    packed, kw = _arguments(names, "weighted")
    small = 1 << 20
    assert len(batch.size_buckets(packed, small)) >= 2
    direct, _ = _run(names, "weighted", **DEPTH)

    def fields(res):
        assert isinstance(res, batch.MinComplianceResult)
        return {key: getattr(res, key) for key in KEYS + ("info",)}

    bucketed = fields(batch.solve_min_compliance(packed, **kw, max_slab_bytes=small, **DEPTH))
    _same(direct, bucketed, "buckets")
    table = packed.table()
    assert table.is_table
    _same(bucketed, fields(batch.solve_min_compliance(table, **kw, max_slab_bytes=small, **DEPTH)), "table form")
    ordered = fields(batch.solve_min_compliance(packed, **kw, max_slab_bytes=small, reorder=True, **DEPTH))
    for b, name in enumerate(names):
        tol = _floor("big", "weighted") if name == cref.BIG else _floor("depth", "weighted")
        _compare(ordered, b, _reference(name, "weighted", **DEPTH), tol, f"reorder {name}")
        _compare(bucketed, b, _reference(name, "weighted", **DEPTH), tol, f"buckets {name}")


def test_truss_minimize_compliance():
    from python_stable_3d_truss_analysis_amd import Truss
    name = "bar-72_input_0"
    data = load_json(name)
    kw = cref.config(data, "weighted")
    truss = Truss(3).LoadFromJSON(data=data)
    before = truss.Serialize()
    f0, f1 = kw["loads"]
    listed = [{j: tuple(f[j]) for j in range(len(f)) if np.any(f[j] != 0)} for f in (f0, f1)]
    one = truss.MinimizeCompliance(listed, alpha=kw["alpha"], areaMin=kw["area_min"], areaMax=kw["area_max"])
    assert truss.Serialize() == before and not truss.isSolved
    ref = _reference(name, "weighted", **cref.FULL)
    assert (one["status"], one["iterations"]) == (ref["status"], ref["iterations"]) == (0, 35)
    tol = _floor("full", "weighted")
    for key in FLOATS:
        assert np.shape(one[key]) == np.shape(ref[key]) and _scaled(one[key], ref[key]) <= tol, key
    with pytest.raises(ValueError, match="alpha"):
        truss.MinimizeCompliance(listed, alpha=(1.0, -1.0), areaMin=kw["area_min"], areaMax=kw["area_max"])


def test_refusals():
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    packed, kw = _arguments(cref.BATCH[:3], "single")
    ok = dict(area_min=0.1, area_max=10.0)
    with pytest.raises(ValueError, match="small-system"):
        batch.DeviceBatch(packed, use_small=True).min_compliance(**ok)
    with pytest.raises(ValueError, match="compact"):
        batch.DeviceBatch(packed, use_small=False, options={"compact": True}).min_compliance(**ok)
    with pytest.raises(ValueError, match="table member form"):
        batch.DeviceBatch(packed.table(), use_small=False).min_compliance(**ok)
    db = batch.DeviceBatch(packed, use_small=False)
    for word, bad in (("eta", {"eta": 0.0}), ("move", {"move": 1.5}), ("alpha", {"alpha": (1.0, 1.0)}),
                      ("measure", {"measure": "mass"}), ("target", {"target": -1.0}), ("levels", {"levels": 4}),
                      ("target", {"target": torch.ones([packed.B + 1], dtype=torch.float64, device=db.device)}),
                      ("area_max", {"area_max": 0.01}), ("max_iters", {"max_iters": -1})):
        with pytest.raises(ValueError, match=word):
            db.min_compliance(**dict(ok, **bad))
    with pytest.raises(ValueError, match="out\\['areas'\\]"):
        db.min_compliance(**ok, out={"areas": torch.zeros([1], device=db.device)})
    with pytest.raises(ValueError, match="sections"):
        batch.solve_min_compliance(packed, **kw, sections=[(1.0, 1.0, 1.0)])
    import dataclasses
    light = dataclasses.replace(packed, rho=packed.rho.copy())
    light.rho[0, 0] = 0.0
    with pytest.raises(ValueError, match="rho <= 0"):
        batch.solve_min_compliance(light, **kw)
