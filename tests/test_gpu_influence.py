"""Influence lines and moving-load envelopes on the device (`solve_influence`, `DeviceBatch.influence`,
`Truss.InfluenceLines`; C ABI include/trs_influence.h) against the numpy yardstick's definition
(`tests/influence_reference.py`), against the existing load-case solver, and the bit guarantees of the analyses on the
resident factor.

Tolerance of the parity tests, per truss: max(1e-11, 10 d) relative to the truss's largest |eta| times sum |w_a|, d the
discrepancy between the yardstick's own two numpy routes on that truss (about 1e-14 on these trusses, so the project's
parity bound 1e-11 is what holds).  Every test prints its errors before it asserts (`-s`); EXPERIMENTS R15 records them."""
import copy

import numpy as np
import pytest

from tests import helpers as H
from tests import influence_reference as I
from tests.test_influence import DOWN, WARREN_PATH, cases, warren_truss

pytestmark = pytest.mark.gpu

KEYS = ("N_max", "N_min", "x_max", "x_min", "area_pos", "area_neg", "lines")
RAGGED_TRAIN = [(1.0, 0.0), (2.0, 75.0), (1.5, 150.0)]
_REF, _ALONE = {}, {}


def bar10_with_a_held_member():
    """bar-10 with one more member between its two pinned joints 4 and 5: both of its ends are held."""
    data = copy.deepcopy(H.load_json("bar-10_input_0"))
    data["member"].append([[4, 5], data["member"][0][1]])
    return data


def all_cases():
    """name -> (data, path, d, train): the three parity cases, and the trusses of the ragged batch under its one train."""
    out = dict(cases())
    out["warren-ragged"] = (warren_truss(), WARREN_PATH, DOWN, RAGGED_TRAIN)
    out["bar-10"] = (bar10_with_a_held_member(), [4, 2, 0], DOWN, RAGGED_TRAIN)          # joint 4 is pinned
    out["bar-25-ragged"] = cases()["bar-25"][:3] + (RAGGED_TRAIN,)
    out["no-path"] = (H.load_json("bar-25_input_0"), [], (0.0, 0.0, -1.0), RAGGED_TRAIN)
    out["one-joint"] = (H.load_json("bar-47_input_0"), [18], DOWN, RAGGED_TRAIN)
    return out


def ref(name):
    """(data, path, d, train, yardstick, absolute tolerance) of a case, once per session."""
    if name not in _REF:
        data, path, d, train = all_cases()[name]
        want = I.by_definition(data, path, d, train)
        rel = max(1e-11, 10 * want["d_routes"])
        scale = (np.abs(want["eta"]).max() if want["eta"].size else 0.0) * sum(abs(w) for w, _o in train)
        print(f"{name}: yardstick discrepancy d = {want['d_routes']:.3e}, relative tolerance {rel:.2e}, scale {scale:.3e}")
        _REF[name] = (data, path, d, train, want, rel * scale)
    return _REF[name]


def solve(names, members="general", want_lines=True, **kw):
    """The named cases as one batch (they share the first one's train)."""
    from python_stable_3d_truss_analysis_amd import batch
    packed = batch.pack_json([ref(n)[0] for n in names], members=members)
    direction = np.zeros([len(names), 3])
    for b, n in enumerate(names):
        direction[b, :len(ref(n)[2])] = ref(n)[2]
    assert all(ref(n)[3] == ref(names[0])[3] for n in names)
    return packed, batch.solve_influence(packed, [ref(n)[1] for n in names], direction, train=ref(names[0])[3],
                                         want_lines=want_lines, **kw)


def alone(name):
    if name not in _ALONE:
        _ALONE[name] = solve([name])
    return _ALONE[name]


def _bits(x):
    x = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def same_bits(a, b, b_of_a, b_of_b, nM, P):
    """Truss b_of_a of result a and truss b_of_b of result b: the same bits (NaN positions included)."""
    for key in KEYS:
        x, y = getattr(a, key)[b_of_a, :nM], getattr(b, key)[b_of_b, :nM]
        if key == "lines":
            x, y = x[:, :P], y[:, :P]
        np.testing.assert_array_equal(_bits(np.ascontiguousarray(x)), _bits(np.ascontiguousarray(y)), err_msg=key)


def check(res, b, name):
    """Truss b of a result against the yardstick's definition.  Returns the largest error, relative to the scale."""
    data, path, _d, train, want, tol = ref(name)
    nM, P = len(data["member"]), len(path)
    assert not res.info[b]
    errs = {"eta": np.abs(res.lines[b, :nM, :P] - want["eta"]).max(initial=0.0)}
    for key in ("N_max", "N_min"):
        errs[key] = np.abs(getattr(res, key)[b, :nM] - want[key]).max()
    for key in ("area_pos", "area_neg"):
        errs[key] = np.abs(getattr(res, key)[b, :nM] - want[key]).max()
    print(f"{name}: tolerance {tol:.3e}, errors " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for key, err in errs.items():
        assert err <= tol, (name, key, err, tol)
    # positions, without a tie rule: the yardstick's response at the device's position is the device's extreme, and no
    # candidate of the yardstick lies beyond it
    if P:
        for m in range(nM):
            for key, at, sign in (("N_max", "x_max", 1.0), ("N_min", "x_min", -1.0)):
                got, x = getattr(res, key)[b, m], getattr(res, at)[b, m]
                assert abs(I.response(want["s"], want["eta"], train, x)[m] - got) <= tol, (name, m, key)
                assert (sign * (want["values"][:, m] - got)).max() <= tol, (name, m, key)
    else:
        assert np.isnan(res.x_max[b, :nM]).all() and np.isnan(res.x_min[b, :nM]).all()
    # padding members and padding path entries: zeros, no position
    for key in ("N_max", "N_min", "area_pos", "area_neg"):
        assert not getattr(res, key)[b, nM:].any()
    assert np.isnan(res.x_max[b, nM:]).all() and np.isnan(res.x_min[b, nM:]).all()
    assert not res.lines[b, nM:].any() and not res.lines[b, :, P:].any()
    scale = tol / max(1e-11, 10 * want["d_routes"])
    return max(errs.values()) / scale if scale else 0.0


# ---- 1. parity against the definition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["warren", "bar-47", "bar-25"])
def test_a_truss_against_the_definition(name):
    packed, res = alone(name)
    assert res.lines.shape == (1, packed.nM_max, len(ref(name)[1]))
    print(f"{name}: worst error relative to max|eta| sum|w| = {check(res, 0, name):.3e}")


def test_the_end_clamp_rule_on_bar25():
    """Offsets equal to the segment length: at every candidate the other axles stand on path joints too, or exactly one
    or two segments off an end - the envelope is then a maximum over sums of ordinates."""
    _data, path, _d, train, want, tol = ref("bar-25")
    _, res = alone("bar-25")
    eta, P = res.lines[0, :25], len(path)
    best = np.full([25], -np.inf)
    for p in range(P):
        for a in range(3):
            total = np.zeros([25])
            for a2, (w, _o) in enumerate(train):
                q = p + (a - a2)
                if 0 <= q < P:
                    total += w * eta[:, q]
            best = np.maximum(best, total)
    assert np.abs(best - res.N_max[0, :25]).max() <= tol


# ---- 2. against the existing solver --------------------------------------------------------------------------------------
def test_the_train_as_joint_loads_through_solve_load_cases():
    from python_stable_3d_truss_analysis_amd import batch
    data, path, d, train, want, tol = ref("warren")
    packed, res = alone("warren")
    s, nJ, nM = want["s"], len(data["joint"]), len(data["member"])
    # lead positions: axles on joints; an axle between two joints; an axle off the path behind; the lead axle off ahead
    leads = [8.0, 13.3, 3.0, 24.0, 27.0]
    loads = np.zeros([1, len(leads), packed.nJ_max, 3])
    between = off = 0
    for k, x in enumerate(leads):
        for w, o in train:
            t = x - o
            if t < 0.0 or t > s[-1]:
                off += 1
                continue
            q = min(int(np.searchsorted(s, t, side="right")) - 1, len(s) - 2)
            lam = (t - s[q]) / (s[q + 1] - s[q])
            between += 0.0 < lam < 1.0
            loads[0, k, path[q], :2] += w * (1.0 - lam) * np.asarray(d)
            loads[0, k, path[q + 1], :2] += w * lam * np.asarray(d)
    assert between and off
    solved = batch.solve_load_cases(packed, loads)
    assert not solved.info.any()
    for k, x in enumerate(leads):
        N = solved.internal[0, k, :nM]
        assert np.abs(N - I.response(s, res.lines[0, :nM, :len(path)], train, x)).max() <= tol, x
        assert (N <= res.N_max[0, :nM] + tol).all() and (N >= res.N_min[0, :nM] - tol).all(), x


# ---- 3. bits -------------------------------------------------------------------------------------------------------------
def test_the_chunk_does_not_change_a_bit():
    """nM = 23: chunk 16 gives two passes, the second partial."""
    _, whole = alone("warren")
    _, split = solve(["warren"], chunk=16)
    same_bits(split, whole, 0, 0, 23, 7)
    _, odd = solve(["warren"], chunk=1)          # (rounded up to 16)
    same_bits(odd, whole, 0, 0, 23, 7)


RAGGED = ["warren-ragged", "bar-10", "bar-25-ragged", "no-path", "one-joint"]


def test_the_ragged_batch_truss_by_truss():
    packed, res = solve(RAGGED)
    assert res.lines.shape == (5, packed.nM_max, 7) and len({int(n) for n in packed.nM}) >= 4
    for b, name in enumerate(RAGGED):
        data, path = ref(name)[:2]
        check(res, b, name)
        same_bits(res, alone(name)[1], b, 0, len(data["member"]), len(path))
    # one joint on the path: the candidates are x = o_a, the areas zero; no path: zeros
    one, none = RAGGED.index("one-joint"), RAGGED.index("no-path")
    assert set(np.unique(res.x_max[one, :47])) <= {0.0, 75.0, 150.0} and res.N_max[one, :47].any()
    assert not res.area_pos[one].any() and not res.area_neg[one].any()
    assert not res.N_max[none].any() and not res.N_min[none].any() and not res.area_pos[none].any()


def test_supports_and_members_between_supports():
    _, res = alone("bar-10")
    assert not res.lines[0, :, 0].any() and res.lines[0, :10, 1:].any()      # the path starts on the pinned joint 4
    for key in ("N_max", "N_min", "area_pos", "area_neg"):                    # member 10: both ends held
        assert getattr(res, key)[0, 10] == 0.0
    assert not res.lines[0, 10].any() and not np.isnan(res.x_max[0, 10])
    check(res, 0, "bar-10")


def test_the_two_member_forms_give_the_same_bits():
    names = ["bar-47", "bar-47"]
    packed, table = solve(names, members="table")
    assert packed.is_table
    _, general = solve(names)
    for b in range(2):
        same_bits(table, general, b, b, 47, 6)
    same_bits(table, table, 0, 1, 47, 6)


def test_a_joint_order_does_not_change_what_the_path_means():
    """`reorder=True` (whatever order the solver finds) and an explicit reversal of the joints, which is no identity by
    construction: the kernel translates the path through the inverse of the order, and every result stays what it was."""
    for name in ("bar-47", "bar-25"):
        nJ = len(ref(name)[0]["joint"])
        reversal = np.arange(nJ, dtype=np.int32)[::-1].reshape(1, nJ).copy()
        assert (reversal != np.arange(nJ)).all() or nJ % 2
        tol = ref(name)[5]
        _, plain = solve([name], reorder=False)
        for order in (True, reversal):
            _, ordered = solve([name], reorder=order)
            check(ordered, 0, name)
            for key in ("lines", "N_max", "N_min", "area_pos", "area_neg"):
                assert np.abs(getattr(ordered, key) - getattr(plain, key)).max() <= tol, (name, key)


def _resident(name):
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    data, path, d, train = ref(name)[:4]
    packed = batch.pack_json([data, data])
    db = batch.DeviceBatch(packed, "cuda:0", use_small=False)
    db.factor()
    dev = db.device
    d3 = np.zeros([2, 3])
    d3[:, :len(d)] = d
    args = (torch.tensor([path, path], dtype=torch.int32, device=dev),
            torch.full([2], len(path), dtype=torch.int32, device=dev), torch.from_numpy(d3).to(dev),
            torch.tensor([w for w, _o in train], dtype=torch.float64, device=dev),
            torch.tensor([o for _w, o in train], dtype=torch.float64, device=dev))
    return packed, db, args


def _same(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        np.testing.assert_array_equal(_bits(a[key]), _bits(b[key]), err_msg=key)


def test_repeated_calls_and_a_side_stream_give_the_same_bits():
    import torch
    _, db1, args = _resident("bar-25")
    _, db2, _ = _resident("bar-25")
    first = {k: v.clone() for k, v in db1.influence(*args, want_lines=True).items()}
    again = db1.influence(*args, want_lines=True)
    torch.cuda.synchronize()
    _same(again, first)
    _same({k: v[:1] for k, v in first.items()}, {k: v[1:] for k, v in first.items()})
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = db2.influence(*args, want_lines=True)
    torch.cuda.synchronize()
    _same(other, first)


def test_the_forward_state_of_solve_cases_survives():
    import torch
    packed, db, args = _resident("bar-47")
    loads = torch.zeros([2, 2, packed.nJ_max, 3], dtype=torch.float64, device=db.device)
    loads[:, 0, 18, 1], loads[:, 1, 21, 0] = -1.0e3, 2.0e2
    cot = torch.ones_like(loads)
    db.solve_cases(loads)
    want = {k: v.clone() for k, v in db.adjoint_cases(grad_u=cot).items()}
    db.solve_cases(loads)
    kept, before = db.cases_F.clone(), db.generation
    out = db.influence(*args)
    assert "eta" not in out and db.generation == before
    got = db.adjoint_cases(grad_u=cot, generation=before)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(db.cases_F), _bits(kept))
    _same(got, want)
    # results go into a caller's dict, whose tensors are checked; no factor, no analysis
    given = {"N_max": torch.zeros([2, 47], dtype=torch.float64, device=db.device)}
    assert db.influence(*args, out=given)["N_max"] is given["N_max"] and given["N_max"].any().item()
    with pytest.raises(ValueError):
        db.influence(*args, out={"N_min": torch.zeros([2, 47], dtype=torch.float32, device=db.device)})
    with pytest.raises(ValueError):
        db.influence(args[0].long(), *args[1:])
    from python_stable_3d_truss_analysis_amd import batch
    with pytest.raises(ValueError, match="factor"):
        batch.DeviceBatch(packed, "cuda:0", use_small=False).influence(*args)


# ---- 4. the object model -------------------------------------------------------------------------------------------------
def test_truss_influence_lines_on_the_warren_truss():
    from python_stable_3d_truss_analysis_amd import Truss
    data, path, d, train = ref("warren")[:4]
    truss = Truss(2).LoadFromJSON(data=data)
    truss.Solve()
    before, forces = truss.Serialize(), dict(truss.GetInternalForces())
    got = truss.InfluenceLines(path, d, train=train, returnLines=True)
    assert truss.Serialize() == before and truss.GetInternalForces() == forces and truss.isSolved
    _, res = alone("warren")
    assert sorted(got) == list(range(23))
    for m, rec in got.items():
        assert rec["max"] == res.N_max[0, m] and rec["maxAt"] == res.x_max[0, m]
        assert rec["min"] == res.N_min[0, m] and rec["minAt"] == res.x_min[0, m]
        assert rec["areaPositive"] == res.area_pos[0, m] and rec["areaNegative"] == res.area_neg[0, m]
        assert rec["ordinates"] == res.lines[0, m, :7].tolist()
    # one unit axle: the envelope is the extreme ordinate
    unit = truss.InfluenceLines(path, d)
    assert "ordinates" not in unit[0]
    for m, rec in unit.items():
        assert rec["max"] == max(got[m]["ordinates"]) and rec["min"] == min(got[m]["ordinates"])
