"""Collapse load on the GPU (`DeviceBatch.plastic`, `solve_plastic`, `Truss.CollapseLoad`; C ABI include/trs_plastic.h)
against the numpy yardstick `tests/plastic_reference.py`.

The parity runs are those of `pref.RUNS`; tests/test_plastic.py asserts that each is admissible - every decision of every
analysis has a margin of 1000 x what float64 itself loses on it - so state, status, events, member_history and
count_history compare EQUAL.  u, N, f_ext, the load factor and the float histories are held to 100 x the largest max-scaled
difference between the yardstick in float64 and in longdouble on the same inputs (tests/golden/plastic_tol.json, which
names them; tests/test_plastic.py measures the small runs again).  The device's own output never sets a bound.  `info` is
compared where the yardstick's decision did not rest on the softening rule and a failed pivot, if any, is clear of rounding
(`pref.info_clear`): the pivot of a true mechanism is rounding noise of either sign - in the runs here |pivot| / diagonal is
1e-16 to 1e-13, and float64 and longdouble themselves disagree on three of the six -, so one factorisation fails on it and
another passes and leaves it to the softening rule; the truss ends in the same state with status 2 either way."""
import dataclasses
import json
import os

import numpy as np
import pytest

from tests import plastic_reference as pref
from tests.helpers import GOLDEN, load_json

pytestmark = pytest.mark.gpu
FLOATS = ("u", "f_ext", "N", "load_factor", "lambda_history", "umax_history", "areas_effective")
KEYS = FLOATS + ("state", "status", "events", "member_history", "count_history")
HISTORIES = ("lambda_history", "umax_history", "member_history", "count_history")

_cache = {}


_inputs = pref.batch_inputs


def _reference(name, b, **kw):
    key = (name, b, tuple(sorted(kw.items())))
    if key not in _cache:
        data, load, run = _inputs(name)[5][b]
        with np.errstate(all="ignore"):
            _cache[key] = pref.collapse(data, load, **dict(run, **kw))
    return _cache[key]


def _floor(name):
    with open(os.path.join(GOLDEN, "plastic_tol.json")) as fh:
        rec = json.load(fh)
    assert rec["trusses"] == list(pref.BATCH) and rec["big_truss"] == pref.BIG
    entry = rec["big"] if name == "big" else rec["runs"][name]
    assert [tuple(c) for c in entry["configs"]] == list(pref.RUNS[name][1])
    return 100.0 * entry["relative_difference"]


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _run(name, rows=None, dbkw=None, **kw):
    """`plastic` on ONE DeviceBatch over the trusses of run `name` (`rows`: only these).  Returns (numpy results, db, the
    device arguments)."""
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    packed, ct, cc, loads, scalars, _ = _inputs(name)
    if rows is not None:      # (trimmed: a truss alone has a padding of its own)
        packed = packed.take(rows).trimmed()
        nJ, nM = packed.nJ_max, packed.nM_max
        ct, cc, loads = ct[rows][:, :nM], cc[rows][:, :nM], loads[rows][:, :nJ]
    db = batch.DeviceBatch(packed, use_small=False, **(dbkw or {}))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(db.device)
    args = {"cap_tension": up(ct), "cap_compression": up(cc), "loads": up(loads)}
    out = db.plastic(**args, **dict(scalars, **kw))
    torch.cuda.synchronize(db.device)
    return dict(_host(out), info=db.info.cpu().numpy()), db, args


def _scaled(mine, ref):
    ref = np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max())
    diff = float(np.abs(np.asarray(mine) - ref).max())
    return diff if scale == 0 else diff / scale


def _failed_pivot_is_clear(name, b):
    """What tests/golden/plastic_tol.json records of truss b of run `name` (tests/test_plastic.py forms it again)."""
    with open(os.path.join(GOLDEN, "plastic_tol.json")) as fh:
        rec = json.load(fh)
    return (rec["big"] if name == "big" else rec["runs"][name])["per_truss"][b]["info_clear"]


def _compare(got, b, ref, tol, what, row, what_run):
    """Truss b of the device results against its yardstick: the integers equal, the float results max-scaled within
    `tol`, zeros on the padding; then the invariants of the device output alone (`row`: the truss's inputs;
    `what_run`: (run, truss) of the record)."""
    nM, (nJ, dim) = len(ref["N"]), ref["u"].shape
    H = len(ref["lambda_history"])
    worst = {"u": _scaled(got["u"][b, :nJ, :dim], ref["u"]), "N": _scaled(got["N"][b, :nM], ref["N"]),
             "f_ext": _scaled(got["f_ext"][b, :nJ, :dim], ref["f_ext"]),
             "load_factor": _scaled(got["load_factor"][b], ref["lam"]),
             "lambda_history": _scaled(got["lambda_history"][b, :H], ref["lambda_history"]),
             "umax_history": _scaled(got["umax_history"][b, :H], ref["umax_history"])}
    print(f"{what}: tol {tol:.2e} worst " + " ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + f" status {got['status'][b]} events {got['events'][b]} info {got['info'][b]} lambda {got['load_factor'][b]:.6g} "
          + f"members {got['member_history'][b][:got['events'][b] + 1]}")
    assert (got["status"][b], got["events"][b]) == (ref["status"], ref["events"]), what
    for key in ("member_history", "count_history"):
        assert np.array_equal(got[key][b, :H], ref[key]) and not got[key][b, H:].any(), (what, key)
    assert np.array_equal(got["state"][b, :nM], ref["state"]), what
    assert np.array_equal(got["areas_effective"][b, :nM], ref["areas_effective"]), what
    # (a failed pivot that is rounding noise is no decision another factorisation must share: pref.info_clear)
    if not ref["soft"] and (ref["info"] == 0 or _failed_pivot_is_clear(*what_run)):
        assert (got["info"][b] != 0) == (ref["info"] != 0), what
    if ref["info"] == 0 and not ref["soft"]:
        assert got["info"][b] == 0, what
    for key, value in worst.items():
        assert value <= tol, (what, key, value, tol)
    for key in ("state", "N", "areas_effective"):
        assert not got[key][b, nM:].any(), (what, key)
    for key in ("u", "f_ext"):
        assert not got[key][b, nJ:].any() and not got[key][b, :, dim:].any(), (what, key)
    _invariants(got, b, row, tol, what)


def _invariants(got, b, row, tol, what):
    """Of the device output alone: the member forces balance lambda P at every free DOF, no force lies beyond its
    capacity - exactly for the members yielded at h = 0 -, and lambda_history never decreases."""
    data, load, kw = row
    geo = pref.Geometry(data, np.float64)
    nM, nJ, dim = len(geo.A0), geo.nJ, geo.dim
    N, lam = got["N"][b, :nM], got["load_factor"][b]
    R = np.zeros([nJ, dim])
    np.add.at(R, geo.j1, N[:, None] * geo.c)
    np.add.at(R, geo.j0, -N[:, None] * geo.c)
    free = geo.mask.reshape(nJ, dim)
    scale = max(float(np.abs(N).max()), float(np.abs(lam * load).max()))
    assert np.abs((R - lam * load)[free]).max() <= tol * scale, (what, "equilibrium")
    assert np.abs((R - got["f_ext"][b, :nJ, :dim])[~free]).max() <= tol * scale, (what, "reactions")
    ct, cc = kw["cap_tension"], kw["cap_compression"]
    state = got["state"][b, :nM]
    if kw["hardening"] == 0.0:
        assert np.array_equal(N[state > 0], ct[state > 0]) and np.array_equal(N[state < 0], -cc[state < 0]), what
        elastic = state == 0
        assert (N[elastic] <= ct[elastic] * (1 + tol)).all() and (N[elastic] >= -cc[elastic] * (1 + tol)).all(), what
    else:      # (a member that hardened beyond its capacity and was released may still lie beyond it)
        assert (N[state > 0] >= ct[state > 0]).all() and (N[state < 0] <= -cc[state < 0]).all(), what
    count = got["events"][b] + 1
    assert (np.diff(got["lambda_history"][b, :count]) >= 0).all(), what
    assert got["lambda_history"][b, count - 1] == lam and not got["lambda_history"][b, count:].any(), what
    assert got["member_history"][b, count - 1] == -2 and (got["member_history"][b, :count - 1] >= -1).all(), what


def _same(a, b, what, rows_a=slice(None), rows_b=slice(None), history=None, keys=KEYS + ("info",)):
    for key in keys:
        x, y = a[key][rows_a], b[key][rows_b]
        if key in HISTORIES and history is not None:      # (runs of different max_events: zero beyond the shorter)
            assert not x[:, history:].any() and not y[:, history:].any(), (what, key)
            x, y = x[:, :history], y[:, :history]
        same = np.array_equal(x.view(np.uint64), y.view(np.uint64)) if x.dtype == np.float64 else np.array_equal(x, y)
        assert same, (what, key)


@pytest.fixture(scope="module")
def full():
    """The two ragged runs, each on one DeviceBatch."""
    return {name: _run(name) for name in ("plastic", "hardening")}


# ---- 1. parity, 3. the invariants of every end state ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plastic", "hardening"])
def test_parity_on_the_ragged_batch(full, name):
    """bar-6 .. bar-120 in ONE DeviceBatch (ragged padding).  plastic: perfectly plastic members, removed exactly; every
    truss ends as a mechanism, by the factorisation or by the softening rule; bar-72 and bar-120 release members on the
    way.  hardening: a thousandth of the stiffness kept, every truss runs into the displacement limit."""
    got, db, _ = full[name]
    assert db.env is not None and not db.table
    tol = _floor(name)
    for b, config in enumerate(pref.RUNS[name][1]):
        ref = _reference(name, b)
        assert (ref["status"], ref["events"]) == pref.TABLE[name][b][:2]
        _compare(got, b, ref, tol, f"{name} {config}", _inputs(name)[5][b], (name, b))
    want = pref.MECHANISM if name == "plastic" else pref.DISP_LIMIT
    assert (got["status"] == want).all() and (got["member_history"] == -1).any()
    if name == "hardening":
        assert not got["info"].any()
        assert np.abs(np.abs(got["u"]).max(axis=(1, 2)) - pref.DISP_LIMIT_RULE).max() <= tol * pref.DISP_LIMIT_RULE


@pytest.mark.parametrize("reorder", [False, True])
def test_parity_on_the_large_truss(reorder):
    """bar-942 alone (n_free 696): four members per thread, joints beyond one pass, eight events, then lambda_max.  With a
    joint order the loads and the results keep the caller's numbering."""
    got, db, _ = _run("big", dbkw={"reorder": reorder})
    assert (db.joint_out is not None) == reorder
    assert db.nM_max > 3 * 256 and db.rows > 256
    ref = _reference("big", 0)
    assert (ref["status"], ref["events"]) == pref.TABLE["big"][0][:2]
    _compare(got, 0, ref, _floor("big"), "bar-942", _inputs("big")[5][0], ("big", 0))
    assert got["load_factor"][0] == 1.2


# ---- 2. the closed forms through the model ------------------------------------------------------------------------------------
def test_closed_forms_through_the_truss_model():
    from python_stable_3d_truss_analysis_amd import Truss
    C, root2 = 100.0, np.sqrt(2.0)
    data, _ = pref.three_bars(C)
    truss = Truss(2).LoadFromJSON(data=data)
    before = truss.Serialize()
    (one,) = truss.CollapseLoad(C, lambdaMax=1e6)
    assert truss.Serialize() == before and not truss.isSolved
    assert (one["status"], one["events"]) == (2, 2) and one["yielded"] == {0: 1, 1: 1, 2: 1}
    assert [m for _, m in one["sequence"]] == [1, 0]
    assert abs(one["sequence"][0][0] - (1 + 1 / root2) * C) <= 1e-12 * C
    assert abs(one["sequence"][1][0] - (1 + root2) * C) <= 1e-12 * C and abs(one["loadFactor"] - (1 + root2) * C) <= 1e-12 * C
    assert (one["forces"] == C).all() and len(one["curve"]) == 3 and one["curve"][0][1] < one["curve"][1][1]
    want = one["loadFactor"] * np.array([[0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]])
    want[:3] = C * np.array([[-1 / root2, 1 / root2], [0.0, 1.0], [1 / root2, 1 / root2]])
    assert np.abs(one["reactions"] - want).max() <= 1e-12 * C and one["displacements"].shape == (4, 2)
    from python_stable_3d_truss_analysis_amd import batch
    res = batch.solve_plastic([truss], np.full([1, 3], C), np.full([1, 3], C), lambda_max=1e6)
    assert res.count_history[0, 0, :3].tolist() == [1, 2, 0] and res.member_history[0, 0, :3].tolist() == [1, 0, -2]
    assert res.info[0] != 0                  # (no stiffness left at all: a failed pivot that is clear of rounding)
    # pushed upwards with half the capacity in compression
    up, = truss.CollapseLoad({"tension": C, "compression": 0.5 * C}, [{3: (0.0, 1.0)}], lambdaMax=1e6)
    assert up["yielded"] == {0: -1, 1: -1, 2: -1} and abs(up["loadFactor"] - 0.5 * (1 + root2) * C) <= 1e-12 * C
    # a statically determinate truss ends at its first yield
    data, _ = pref.two_bars(C)
    two = Truss(2).LoadFromJSON(data=data)
    ref = pref.collapse(data, pref.cases(data)[0], np.full(2, C), np.full(2, C), lambda_max=1e6)
    (end,) = two.CollapseLoad(C, lambdaMax=1e6)
    assert (end["status"], end["events"], end["sequence"][0][1]) == (2, 1, 0)
    assert abs(end["loadFactor"] - float(ref["lam"])) <= 1e-12 * C and end["yielded"] == {0: 1}
    assert abs(end["loadFactor"] - C / (0.65 * root2)) <= 1e-12 * C      # (statics: N = (0.65, 0.35) sqrt 2 P)


# ---- 4. lambda_max below the first yield ---------------------------------------------------------------------------------------
def test_lambda_max_below_the_first_yield_is_the_linear_solve():
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    packed, ct, cc, loads, _, _ = _inputs("plastic")
    db = batch.DeviceBatch(packed, use_small=False)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(db.device)
    got = _host(db.plastic(up(1e3 * ct), up(1e3 * cc), up(loads), lambda_max=1.0))
    assert not got["status"].any() and not got["events"].any() and not got["state"].any()
    assert (got["load_factor"] == 1.0).all() and (got["member_history"][:, 0] == -2).all()
    assert not db.info.cpu().numpy().any()
    fresh = batch.DeviceBatch(packed, use_small=False)
    fresh.factor()
    ref = _host(fresh.solve_cases(up(loads[:, None])))
    assert np.array_equal(got["u"].view(np.uint64), ref["u"][:, 0].view(np.uint64))
    tol = _floor("plastic")
    for b in range(packed.B):
        assert _scaled(got["N"][b], ref["N"][b, 0]) <= tol and _scaled(got["f_ext"][b], ref["f_ext"][b, 0]) <= tol
    assert np.array_equal(got["umax_history"][:, 0], np.abs(got["u"]).max(axis=(1, 2)))


# ---- 5. independence, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 4, 5])
def test_a_truss_alone_has_the_bits_it_has_in_the_batch(full, b):
    alone, _, _ = _run("plastic", rows=[b])
    got = full["plastic"][0]
    nJ, nM = alone["u"].shape[1], alone["N"].shape[1]
    cut = {k: (v[:, :nJ] if k in ("u", "f_ext") else v[:, :nM] if k in ("N", "state", "areas_effective") else v)
           for k, v in got.items()}
    _same(cut, alone, pref.RUNS["plastic"][1][b], rows_a=slice(b, b + 1))


def test_max_events_cut_short_and_longer(full):
    """Three events allowed: the trusses that need more end with status 1 in the yardstick's state, those that ended
    earlier keep their bits.  Sixty events allowed change nothing."""
    got = full["plastic"][0]
    cut, _, _ = _run("plastic", max_events=3)
    tol = _floor("plastic")
    for b, config in enumerate(pref.RUNS["plastic"][1]):
        _compare(cut, b, _reference("plastic", b, max_events=3), tol, f"max_events 3 {config}", _inputs("plastic")[5][b],
                 ("plastic", b))
    assert list(cut["status"]) == [2, 2, 1, 1, 1, 1] and list(cut["events"]) == [2, 2, 3, 3, 3, 3]
    early = np.flatnonzero(got["events"] < 3)
    assert len(early) == 2
    _same(got, cut, "max_events 3", rows_a=early, rows_b=early, history=4)
    longer, _, _ = _run("plastic", max_events=60)
    _same(got, longer, "max_events 60", history=pref.MAX_EVENTS + 1)


@pytest.mark.parametrize("name", ["plastic", "hardening"])
def test_check_every_does_not_change_the_bits(full, name):
    sparse, _, _ = _run(name, check_every=3)
    _same(full[name][0], sparse, "check_every 3")


def test_solve_plastic_with_two_cases_equals_two_runs():
    """Two load patterns: each case is an independent run from the nominal areas.  The table member form gives the same
    bits; the batch's own loads are the pattern where none is given, also under a joint order."""
    from python_stable_3d_truss_analysis_amd import batch
    names = ("bar-25_input_0", "bar-72_input_0")
    datas = [load_json(n) for n in names]
    packed = batch.pack_json(datas)
    B, nJ, nM = packed.B, packed.nJ_max, packed.nM_max
    ct, cc, loads = np.ones([B, nM]), np.ones([B, nM]), np.zeros([B, 2, nJ, 3])
    for b, data in enumerate(datas):
        for case in (0, 1):
            load, kw = pref.rule(data, case)
            loads[b, case, :load.shape[0], :load.shape[1]] = load
        ct[b, :len(kw["cap_tension"])], cc[b, :len(kw["cap_compression"])] = kw["cap_tension"], kw["cap_compression"]
    kw = dict(hardening=1e-3, lambda_max=10.0, disp_limit=pref.DISP_LIMIT_RULE, max_events=pref.MAX_EVENTS)
    two = batch.solve_plastic(packed, ct, cc, loads, **kw)
    assert isinstance(two, batch.PlasticResult) and two.status.shape == (B, 2) and two.displace.shape == (B, 2, nJ, 3)
    assert not two.info.any() and (two.events > 0).all()
    same = lambda x, y: np.array_equal(x.view(np.uint64), y.view(np.uint64)) if x.dtype == np.float64 else np.array_equal(x, y)
    for l in range(2):
        one = batch.solve_plastic(packed, ct, cc, loads[:, l:l + 1], **kw)
        for field in batch.PlasticResult.FIELDS:
            assert same(getattr(two, field)[:, l], getattr(one, field)[:, 0]), (l, field)
    assert (two.member_history[:, 0] != two.member_history[:, 1]).any()          # the sequences differ per case
    table = batch.solve_plastic(packed.table(), ct, cc, loads, **kw)
    for field in batch.PlasticResult.FIELDS:
        assert same(getattr(two, field), getattr(table, field)), field
    # the batch's own loads as the one case, also under a joint order
    for reorder in (False, True):
        own = batch.solve_plastic(packed, ct, cc, reorder=reorder, **kw)
        given = batch.solve_plastic(packed, ct, cc, packed.loads[:, None], reorder=reorder, **kw)
        for field in batch.PlasticResult.FIELDS:
            assert same(getattr(own, field), getattr(given, field)), (reorder, field)


# ---- 6. the factor left behind -------------------------------------------------------------------------------------------------
def test_the_factor_left_behind_serves_solve_cases():
    """Afterwards `solve_cases` on the same DeviceBatch - no `factor()` in between - gives the bits of a fresh linear
    solve of the effective areas, for the trusses whose info is 0."""
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    for name in ("hardening", "plastic"):
        got, db, args = _run(name)
        packed = _inputs(name)[0]
        live = np.arange(packed.nM_max)[None, :] < packed.nM[:, None]
        assert np.array_equal(db.A.cpu().numpy()[live], got["areas_effective"][live])
        generation = db.generation
        loads = args["loads"][:, None].contiguous()
        mine = _host(db.solve_cases(loads))
        assert db.generation == generation + 1
        fresh = batch.DeviceBatch(dataclasses.replace(packed, A=np.where(live, got["areas_effective"], packed.A)),
                                  use_small=False)
        fresh.factor()
        ref = _host(fresh.solve_cases(loads))
        good = got["info"] == 0
        assert np.array_equal(fresh.info.cpu().numpy() == 0, good) and good.any()
        for key in ("u", "f_ext", "N"):
            assert np.array_equal(mine[key][good].view(np.uint64), ref[key][good].view(np.uint64)), (name, key)
        torch.cuda.synchronize(db.device)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    packed, ct, cc, loads, _, _ = _inputs("plastic")
    packed = packed.take([0, 1, 2]).trimmed()
    ct = np.ascontiguousarray(ct[:3, :packed.nM_max])
    with pytest.raises(ValueError, match="small-system"):
        db = batch.DeviceBatch(packed, use_small=True)
        db.plastic(torch.from_numpy(ct).to(db.device), torch.from_numpy(ct).to(db.device))
    with pytest.raises(ValueError, match="compact"):
        db = batch.DeviceBatch(packed, use_small=False, options={"compact": True})
        db.plastic(torch.from_numpy(ct).to(db.device), torch.from_numpy(ct).to(db.device))
    with pytest.raises(ValueError, match="table member form cannot hold one area per member"):
        db = batch.DeviceBatch(packed.table(), use_small=False)
        db.plastic(torch.from_numpy(ct).to(db.device), torch.from_numpy(ct).to(db.device))
    db = batch.DeviceBatch(packed, use_small=False)
    on = torch.from_numpy(ct).to(db.device)
    for name in ("cap_tension", "cap_compression"):
        for bad in (on * 0, -on, on * float("nan")):
            with pytest.raises(ValueError, match=f"{name} must be positive"):
                db.plastic(**dict({"cap_tension": on, "cap_compression": on}, **{name: bad}))
        for bad in (on[:, :-1], on.to(torch.float32), ct):
            with pytest.raises(ValueError, match=f"{name} must be float64"):
                db.plastic(**dict({"cap_tension": on, "cap_compression": on}, **{name: bad}))
    for name, bads in (("hardening", (-1e-9, float("nan"), float("inf"), True)), ("lambda_max", (0.0, -1.0, True)),
                       ("disp_limit", (-1.0, float("nan"), True)), ("collapse_ratio", (1.0, float("inf"), True)),
                       ("tie_tol", (-1e-12, True)), ("max_events", (-1, 2.5, True)), ("check_every", (0, True))):
        for bad in bads:
            with pytest.raises(ValueError, match=name):
                db.plastic(on, on, **{name: bad})
    with pytest.raises(ValueError, match="loads must be float64"):
        db.plastic(on, on, loads=torch.zeros([3, 2, 3], device=db.device, dtype=torch.float64))
    with pytest.raises(ValueError, match="out\\['state'\\]"):
        db.plastic(on, on, out={"state": torch.zeros([1], device=db.device)})
    with pytest.raises(ValueError, match="sections"):
        batch.solve_plastic(packed, ct, ct, sections=[(1.0, 1.0, 1.0)])
