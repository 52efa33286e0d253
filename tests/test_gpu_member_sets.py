"""Member-set scenarios on the device (`solve_member_sets`, `DeviceBatch.member_sets`, `Truss.MemberSets`; C ABI
include/trs_sets.h) against the numpy yardstick's re-solve (`tests/member_sets_reference.py`), against `member_loss` on
the same factor, and the bit guarantees of the analyses on the resident factor.

Tolerance of the parity tests, per fixture: max(1e-11, 100 d) relative to the largest magnitude of the compared array,
d the discrepancy between the yardstick's own two numpy routes on that fixture and those scenarios (computed here from
reference code alone) - the rule of tests/test_gpu_member_loss.py.

Every test prints its figures before it asserts (`-s`); EXPERIMENTS R16 records what has been measured."""
import numpy as np
import pytest

from oracle import truss_oracle as orc
from tests import helpers as H
from tests import member_sets_reference as R
from tests.test_gpu_member_loss import cases_of

pytestmark = pytest.mark.gpu

SMALL = ["bar-6_input_0", "bar-10_input_0", "bar-25_input_0", "bar-47_input_0", "bar-72_input_0", "bar-120_input_0",
         "cube-7_case_3", "cube-7_case_10"]
L = 2
R_TOL = 1e-8
N_RANDOM = 24      # seeded random scenarios per fixture; then the empty set; then every singleton of a small fixture
KEYS = ("pivot", "unstable", "first_unstable", "peak_stress", "peak_member", "peak_displace", "peak_joint", "N_after",
        "u_after")
_REF = {}


def ref(name):
    """(data, scenarios, loads, re-solve, closed form, tolerance) of a fixture, once per session."""
    if name not in _REF:
        data, loads = cases_of(name)
        scen = R.scenarios(name, 7, N_RANDOM)
        a, b = R.resolve(data, scen, loads), R.closed_form(data, scen, loads)
        d = R.discrepancy(a, b)
        print(f"{name}: {len(scen)} scenarios, {int(a['unstable'].sum())} unstable, yardstick discrepancy d = {d:.3e}")
        _REF[name] = (data, scen, loads, a, b, max(1e-11, 100 * d))
    return _REF[name]


def arrays(scen_lists):
    """Scenario lists per truss as sets int [B, S, 8] (-1 padding, short lists padded with empty sets), gamma [B, S, 8]."""
    S = max(len(x) for x in scen_lists)
    sets, gamma = np.full([len(scen_lists), S, 8], -1, dtype=np.int64), np.zeros([len(scen_lists), S, 8])
    for b, scen in enumerate(scen_lists):
        for s, (members, factors) in enumerate(scen):
            sets[b, s, :len(members)], gamma[b, s, :len(members)] = members, factors
    return sets, gamma


def batch_loads(names, nJ_max):
    loads = np.zeros([len(names), L, nJ_max, 3])
    for b, name in enumerate(names):
        x = ref(name)[2]
        loads[b, :, :x.shape[1]] = x
    return loads


def solve(names, members="general", **kw):
    from python_stable_3d_truss_analysis_amd import batch
    packed = batch.pack_json([ref(n)[0] for n in names], members=members)
    sets, gamma = arrays([ref(n)[1] for n in names])
    return packed, batch.solve_member_sets(packed, sets, gamma, batch_loads(names, packed.nJ_max), want_forces=True,
                                           want_displace=True, **kw)


def check(res, b, name):
    """Truss b of a result against the yardstick's re-solve."""
    data, scen, _loads, want, closed, tol = ref(name)
    dim, nJ, nM, S = orc.truss_dim(data), len(data["joint"]), len(data["member"]), len(scen)
    bad = want["unstable"]
    assert not res.info[b]
    np.testing.assert_array_equal(res.unstable[b, :S], bad)
    np.testing.assert_array_equal(res.first_unstable[b, :S], want["first_unstable"])
    # the pivots: the default r_tol lies a factor 100 from either class, on the device
    sizes = np.array([len(m) for m, _f in scen])
    stable_min, fail_max = np.inf, 0.0
    for s in range(S):
        p = res.pivot[b, s]
        if bad[s]:
            j = want["first_unstable"][s]
            fail_max = max(fail_max, abs(p[j]))
            assert np.isnan(p[j + 1:]).all() and (p[:j] >= 100 * R_TOL).all()
        else:
            assert np.isnan(p[sizes[s]:]).all()
            stable_min = min(stable_min, p[:sizes[s]].min(initial=np.inf))
    print(f"{name}: smallest pivot of a stable scenario {stable_min:.2e}, largest failing pivot {fail_max:.2e}")
    assert stable_min >= 100 * R_TOL and fail_max <= R_TOL / 100
    ok = ~bad
    errs = {"pivot": H.max_scaled_err(np.nan_to_num(res.pivot[b, :S][ok]), np.nan_to_num(closed["pivot"][ok])),
            "u": H.max_scaled_err(res.displace[b, :, :nJ, :dim], closed["u"]),
            "N": H.max_scaled_err(res.internal[b, :, :nM], closed["N"]),
            "N_after": H.max_scaled_err(res.internal_after[b, :, :S, :nM][:, ok], want["N_after"][:, ok]),
            "u_after": H.max_scaled_err(res.displace_after[b, :, :S, :nJ, :dim][:, ok], want["U_after"][:, ok]),
            "peak_stress": H.max_scaled_err(res.peak_stress[b, :, :S][:, ok], want["peak_stress"][:, ok]),
            "peak_displace": H.max_scaled_err(res.peak_displace[b, :, :S][:, ok], want["peak_displace"][:, ok])}
    print(f"{name}: tolerance {tol:.2e}, errors " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for key, err in errs.items():
        assert err <= tol, (name, key, err, tol)
    # where the yardstick's best and second best differ by more than the tolerance, the places agree
    for got, key, gap, peak in ((res.peak_member, "peak_member", "stress_gap", "peak_stress"),
                                (res.peak_joint, "peak_joint", "displace_gap", "peak_displace")):
        clear = (want[gap] > tol * want[peak][:, ok].max()) & ok[None, :]
        np.testing.assert_array_equal(got[b, :, :S][clear], want[key][clear])
    # unstable scenarios: inf, -1 and NaN rows (zeros at the padding)
    assert np.isinf(res.peak_stress[b, :, :S][:, bad]).all() and np.isinf(res.peak_displace[b, :, :S][:, bad]).all()
    assert (res.peak_member[b, :, :S][:, bad] == -1).all() and (res.peak_joint[b, :, :S][:, bad] == -1).all()
    assert np.isnan(res.internal_after[b, :, :S, :nM][:, bad]).all()
    assert np.isnan(res.displace_after[b, :, :S, :nJ][:, bad]).all()
    assert not res.internal_after[b, :, :, nM:].any() and not res.displace_after[b, :, :, nJ:].any()
    # the scenarios past the truss's own list are empty sets: the intact state
    if S < res.unstable.shape[1]:
        assert not res.unstable[b, S:].any() and (res.first_unstable[b, S:] == -1).all() and np.isnan(res.pivot[b, S:]).all()
        np.testing.assert_array_equal(res.internal_after[b, :, S:, :nM], res.internal_after[b, :, N_RANDOM:N_RANDOM + 1, :nM]
                                      .repeat(res.unstable.shape[1] - S, axis=1))


# ---- 1. parity against the yardstick's re-solve ------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_a_truss_alone_against_the_resolve(name):
    packed, res = solve([name])
    S = len(ref(name)[1])
    assert res.internal_after.shape == (1, L, S, packed.nM_max) and res.displace_after.shape == (1, L, S, packed.nJ_max, 3)
    check(res, 0, name)


def test_the_ragged_batch_against_the_resolve():
    """All the small fixtures together: several size buckets, padding joints, members and scenarios, 2D beside 3D."""
    packed, res = solve(SMALL)
    assert len({int(n) for n in packed.nM}) > 3
    for b, name in enumerate(SMALL):
        check(res, b, name)


@pytest.mark.parametrize("config", ["reorder-device", "table"])
def test_bar942_against_the_resolve(config):
    """bar-942 x 2 with 24 random scenarios and the empty set: the envelope, a joint order, several n_pad blocks."""
    from tests.test_gpu_load_cases import CONFIGS
    kw = dict(CONFIGS[config])
    packed, res = solve(["bar-942_input_0"] * 2, members="auto" if kw.pop("table", False) else "general", **kw)
    assert packed.is_table == (config == "table") and len(ref("bar-942_input_0")[1]) == N_RANDOM + 1
    for b in range(2):
        check(res, b, "bar-942_input_0")
    for key in ("pivot", "peak_stress", "peak_displace", "internal_after", "displace_after"):
        np.testing.assert_array_equal(getattr(res, key)[0].view(np.uint64), getattr(res, key)[1].view(np.uint64))


# ---- 2. on one resident factor --------------------------------------------------------------------------------------------
def _bits(t):
    t = t.cpu().numpy()
    return t.view(np.uint64) if t.dtype == np.float64 else t


def _resident(names, table=False, reorder=False):
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    packed = batch.pack_json([ref(n)[0] for n in names], members="table" if table else "general")
    db = batch.DeviceBatch(packed, "cuda:0", use_small=False, reorder=reorder)
    db.factor()
    return packed, db, torch.from_numpy(batch_loads(names, packed.nJ_max)).to(db.device)


def _keep(out):
    return {k: v.clone() for k, v in out.items()}


def _same(a, b, keys=KEYS, pick_a=slice(None), pick_b=slice(None), axis=1):
    """The scenarios `pick_a` of a and `pick_b` of b hold the same bits (the scenario axis is 1 for the per-scenario
    arrays and 2 for the per-case ones)."""
    for key in keys:
        x, y = _bits(a[key]), _bits(b[key])
        if key in ("u", "f_ext", "N"):
            np.testing.assert_array_equal(x, y, err_msg=key)
            continue
        ax = 1 if key in ("pivot", "unstable", "first_unstable") else 2
        np.testing.assert_array_equal(np.take(x, pick_a, axis=ax) if not isinstance(pick_a, slice) else x,
                                      np.take(y, pick_b, axis=ax) if not isinstance(pick_b, slice) else y, err_msg=key)


def _run(db, loads, sets, gamma, **kw):
    import torch
    out = _keep(db.member_sets(loads, sets, gamma, want_forces=True, want_displace=True, **kw))
    torch.cuda.synchronize()
    return out


def test_singleton_removals_are_member_loss_on_the_same_factor():
    """pivot[:, :, 0] of the set {e} is r_e BIT FOR BIT, unstable is critical, and the state agrees within the tolerance."""
    import torch
    names = SMALL
    packed, db, loads = _resident(names)
    nM_max = packed.nM_max
    sets = np.full([len(names), nM_max, 1], -1)
    for b in range(len(names)):
        sets[b, :int(packed.nM[b]), 0] = np.arange(int(packed.nM[b]))
    loss = _keep(db.member_loss(loads, want_forces=True))
    got = _run(db, loads, sets, None)
    np.testing.assert_array_equal(_bits(got["pivot"][:, :, 0]), np.where(sets[:, :, 0] >= 0, _bits(loss["r"]),
                                                                        _bits(torch.full_like(loss["r"], float("nan")))))
    np.testing.assert_array_equal(_bits(got["unstable"]), _bits(loss["critical"]))
    assert (_bits(got["first_unstable"]) == np.where(_bits(loss["critical"]) != 0, 0, -1)).all()
    _same(got, loss, ("u", "f_ext", "N"))
    for b, name in enumerate(names):
        nM, tol = int(packed.nM[b]), ref(name)[5]
        ok = _bits(loss["critical"])[b, :nM] == 0
        errs = {}
        for key in ("peak_stress", "peak_displace"):
            errs[key] = H.max_scaled_err(got[key][b, :, :nM][:, ok].cpu().numpy(), loss[key][b, :, :nM][:, ok].cpu().numpy())
            assert np.isinf(got[key][b, :, :nM][:, ~ok].cpu().numpy()).all()
        errs["N_after"] = H.max_scaled_err(got["N_after"][b, :, :nM, :nM][:, ok].cpu().numpy(),
                                           loss["N_after"][b, :, :nM, :nM][:, ok].cpu().numpy())
        print(f"{name}: singletons against member_loss, tolerance {tol:.2e}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert max(errs.values()) <= tol
        after = got["N_after"][b].cpu().numpy()
        assert not after[:, np.arange(nM), np.arange(nM)][:, ok].any()      # the removed member carries nothing


def test_an_empty_set_and_factor_one_return_the_intact_state():
    names = ["bar-72_input_0", "bar-47_input_0", "cube-7_case_3"]
    packed, db, loads = _resident(names, reorder="device")
    sets = np.full([3, 3, 8], -1)
    sets[:, 1, :5] = [4, 0, 17, 9, 30]
    sets[:, 2, :8] = np.arange(8) * 3
    got = _run(db, loads, sets, np.ones([3, 3, 8]))
    assert not got["unstable"].any().item() and (got["first_unstable"] == -1).all().item()
    piv = got["pivot"].cpu().numpy()
    assert np.isnan(piv[:, 0]).all() and (piv[:, 1, :5] == 1.0).all() and np.isnan(piv[:, 1, 5:]).all() and (piv[:, 2] == 1.0).all()
    N, u = got["N"].cpu().numpy(), got["u"].cpu().numpy()
    area = np.where(np.arange(packed.nM_max)[None, :] < np.asarray(packed.nM)[:, None], np.asarray(packed.A), np.inf)
    stress = np.abs(N) / area[:, None, :]
    norm = np.sqrt((u ** 2).sum(axis=-1))
    for s in range(3):
        assert H.max_scaled_err(got["N_after"][:, :, s].cpu().numpy(), N) <= 1e-13
        assert H.max_scaled_err(got["u_after"][:, :, s].cpu().numpy(), u) <= 1e-13
        assert H.max_scaled_err(got["peak_stress"][:, :, s].cpu().numpy(), stress.max(axis=-1)) <= 1e-13
        assert H.max_scaled_err(got["peak_displace"][:, :, s].cpu().numpy(), norm.max(axis=-1)) <= 1e-13
    np.testing.assert_array_equal(got["u_after"][:, :, 0].cpu().numpy(), u)       # the empty set: u' = u exactly


def test_the_order_within_a_set_changes_the_pivots_but_not_their_product_or_the_state():
    name = "bar-25_input_0"
    _, db, loads = _resident([name])
    members, factors = [3, 11, 20, 7], [0.0, 0.5, 2.0, 0.0]
    sets, gamma = arrays([[(members, factors), (members[::-1], factors[::-1])]])
    got = _run(db, loads, sets, gamma)
    piv = got["pivot"].cpu().numpy()[0, :, :4]
    tol = ref(name)[5]
    assert not got["unstable"].any().item() and np.abs(piv[0] - piv[1, ::-1]).max() > 1e-3
    assert abs(np.prod(piv[0]) / np.prod(piv[1]) - 1.0) <= tol
    for key in ("N_after", "u_after", "peak_stress", "peak_displace"):
        x = got[key].cpu().numpy()
        assert H.max_scaled_err(x[:, :, 0], x[:, :, 1]) <= tol, key


# ---- 3. bits ----------------------------------------------------------------------------------------------------------
def _scenario_arrays(names):
    return arrays([ref(n)[1] for n in names])


def test_the_chunk_the_company_and_the_order_of_the_scenarios_do_not_change_a_bit():
    names = ["bar-47_input_0", "bar-72_input_0", "cube-7_case_3"]
    _, db, loads = _resident(names)
    sets, gamma = _scenario_arrays(names)
    S = sets.shape[1]
    outs = {c: _run(db, loads, sets, gamma, chunk=c) for c in (16, 64, 128)}
    _same(outs[16], outs[64])
    _same(outs[128], outs[64])
    # a scenario alone, and a few among fewer others
    for pick in ([5], [0, 30, S - 1], list(range(20, 40))):
        part = _run(db, loads, sets[:, pick], gamma[:, pick])
        _same(part, outs[64], pick_b=np.array(pick))
    # permuted
    perm = np.random.default_rng(3).permutation(S)
    shuffled = _run(db, loads, sets[:, perm], gamma[:, perm], chunk=16)
    _same(shuffled, outs[64], pick_b=perm)


def test_a_case_does_not_depend_on_the_other_cases():
    """Two cases together, each alone, and nine (two passes of the apply kernel) - bit for bit."""
    import torch
    names = ["bar-72_input_0", "bar-47_input_0"]
    _, db, loads = _resident(names)
    sets, gamma = _scenario_arrays(names)
    both = _run(db, loads, sets, gamma)
    per_case = ("peak_stress", "peak_member", "peak_displace", "peak_joint", "N_after", "u_after")
    for k in range(L):
        one = _run(db, loads[:, k:k + 1].contiguous(), sets, gamma)
        _same(one, both, ("pivot", "unstable", "first_unstable"))
        for key in per_case:
            np.testing.assert_array_equal(_bits(one[key]), _bits(both[key][:, k:k + 1]), err_msg=key)
    nine = _run(db, torch.cat([loads] * 4 + [loads[:, :1]], dim=1).contiguous(), sets, gamma)
    for k in range(9):
        for key in per_case:
            np.testing.assert_array_equal(_bits(nine[key][:, k]), _bits(both[key][:, k % L]), err_msg=(key, k))
    _same(nine, both, ("pivot", "unstable", "first_unstable"))


def test_a_truss_does_not_depend_on_the_batch():
    from python_stable_3d_truss_analysis_amd import batch
    names = SMALL
    packed, db, loads = _resident(names)
    sets, gamma = _scenario_arrays(names)
    whole = _run(db, loads, sets, gamma)
    for b in (1, 3, 6):
        one = batch.DeviceBatch(packed.take([b]), "cuda:0", use_small=False)
        one.factor()
        single = _run(one, loads[b:b + 1].contiguous(), sets[b:b + 1], gamma[b:b + 1])
        for key in KEYS:
            np.testing.assert_array_equal(_bits(single[key]), _bits(whole[key][b:b + 1]), err_msg=key)


def test_the_two_member_forms_give_the_same_bits():
    names = ["bar-942_input_0", "bar-72_input_0"]
    _, db, loads = _resident(names, reorder="device")
    _, tdb, _ = _resident(names, table=True, reorder="device")
    assert tdb.table and not db.table
    sets, gamma = _scenario_arrays(names)
    _same(_run(db, loads, sets, gamma), _run(tdb, loads, sets, gamma), KEYS + ("u", "f_ext", "N"))


def test_repeated_calls_and_a_side_stream_give_the_same_bits():
    import torch
    names = ["bar-72_input_0", "cube-7_case_3"]
    _, db1, loads = _resident(names)
    _, db2, _ = _resident(names)
    sets, gamma = _scenario_arrays(names)
    first = _run(db1, loads, sets, gamma)
    _same(_run(db1, loads, sets, gamma), first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = db2.member_sets(loads, sets, gamma, want_forces=True, want_displace=True)
    torch.cuda.synchronize()
    _same(other, first)


# ---- 4. the state left behind, errors and edges ----------------------------------------------------------------------------
def test_the_intact_state_is_solve_cases_and_survives():
    import torch
    names = ["bar-942_input_0", "bar-47_input_0"]
    _, db, loads = _resident(names, reorder="device")
    sets, gamma = _scenario_arrays(names)
    plain = _keep(db.solve_cases(loads))
    kept = db.cases_F.clone()
    before = db.generation
    out = db.member_sets(loads, sets, gamma)
    torch.cuda.synchronize()
    assert "N_after" not in out and "u_after" not in out and db.generation == before + 1
    _same(out, plain, ("u", "f_ext", "N"))
    np.testing.assert_array_equal(_bits(db.cases_F), _bits(kept))      # the ranges work on a buffer of their own
    grads = _keep(db.adjoint_cases(grad_u=torch.ones_like(loads), want=("A",)))
    db.solve_cases(loads)
    _same(db.adjoint_cases(grad_u=torch.ones_like(loads), want=("A",)), grads, ("A",))
    with pytest.raises(ValueError):
        db.member_sets(loads, sets, gamma, out={"unstable": torch.zeros(list(sets.shape[:2]), dtype=torch.int64, device=db.device)})


def test_no_factor_and_bad_arguments():
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    packed = batch.pack_json([H.load_json("bar-72_input_0")] * 2)
    db = batch.DeviceBatch(packed, "cuda:0", use_small=False)
    loads = torch.zeros([2, 1, packed.nJ_max, 3], dtype=torch.float64, device=db.device)
    sets = np.zeros([2, 3, 1], dtype=np.int64)
    with pytest.raises(ValueError, match="factor"):
        db.member_sets(loads, sets)
    db.factor()
    for kw in (dict(r_tol=0.0), dict(r_tol=1.0), dict(chunk=0), dict(gamma=-np.ones([2, 3, 1]))):
        with pytest.raises(ValueError):
            db.member_sets(loads, sets, **kw)
    for wrong in (np.full([2, 3, 1], 72), np.zeros([2, 3, 9], dtype=np.int64), np.zeros([2, 1, 2], dtype=np.int64)):
        with pytest.raises(ValueError):
            db.member_sets(loads, wrong)
    with pytest.raises(ValueError, match=str(2 * 3 * 72 * 8)):
        db.member_sets(loads, sets, want_forces=True, max_result_bytes=1000)
    assert db.member_sets(loads, np.zeros([2, 0, 8], dtype=np.int64))["pivot"].shape == (2, 0, 8)


def test_a_singular_truss_leaves_the_others_bits_unchanged():
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    good = "bar-72_input_0"
    singular = H.edge_cases()["3d_mechanism_singular"]["input"]
    packed3 = batch.pack_json([ref(good)[0], singular, ref(good)[0]])
    packed2 = packed3.take([0, 2])
    loads3 = torch.from_numpy(batch_loads([good] * 3, packed3.nJ_max))
    loads3[1] = 0.0
    sets, gamma = _scenario_arrays([good] * 3)
    sets[1], gamma[1] = -1, 0.0
    sets[1, :, 0] = 0
    outs = []
    for packed, rows in ((packed3, [0, 1, 2]), (packed2, [0, 2])):
        db = batch.DeviceBatch(packed, "cuda:0", use_small=False)
        db.factor()
        outs.append((db, _run(db, loads3[rows].contiguous().to(db.device), sets[rows], gamma[rows])))
    info = outs[0][0].info.cpu().numpy()
    assert info[0] == 0 and info[2] == 0 and info[1] > 0 and not outs[1][0].info.any().item()
    for key in KEYS:
        np.testing.assert_array_equal(_bits(outs[0][1][key][[0, 2]]), _bits(outs[1][1][key]), err_msg=key)


# ---- 5. the object model ------------------------------------------------------------------------------------------------
def test_truss_member_sets_on_bar72_and_bar47():
    from python_stable_3d_truss_analysis_amd import Truss
    data, scen, loads, want, _closed, tol = ref("bar-72_input_0")
    truss = Truss(3).LoadFromJSON(data=data)
    before = truss.Serialize()
    cases = [{j: tuple(loads[k, j]) for j in range(len(data["joint"])) if loads[k, j].any()} for k in range(L)]
    pick = list(range(N_RANDOM + 1))
    got = truss.MemberSets([scen[s][0] for s in pick], [scen[s][1] for s in pick], cases, returnForces=True)
    assert len(got) == L and truss.Serialize() == before and not truss.isSolved
    for k in range(L):
        assert len(got[k]) == len(pick)
        for s, rec in zip(pick, got[k]):
            assert rec["members"] == scen[s][0] and rec["factors"] == scen[s][1] and len(rec["pivots"]) == len(scen[s][0])
            assert rec["unstable"] is False and rec["firstUnstable"] is None
            dense = np.zeros([72])
            for m, v in rec["forces"].items():
                dense[m] = v
            assert all(abs(v) >= 1e-10 for v in rec["forces"].values())
            assert not any(m in rec["forces"] for m, g in zip(*scen[s]) if g == 0.0)
            assert H.max_scaled_err(dense, want["N_after"][k, s]) <= tol
            assert abs(rec["peakStress"] - want["peak_stress"][k, s]) <= tol * want["peak_stress"][k].max()
            assert abs(rec["peakDisplacement"] - want["peak_displace"][k, s]) <= tol * want["peak_displace"][k].max()
    # bar-47 (2D), removals only, the truss's own forces as the one case: stable and unstable scenarios
    data47, scen47, _loads, want47, _c, _t = ref("bar-47_input_0")
    only = Truss(2).LoadFromJSON(data=data47).MemberSets([m for m, _f in scen47[:N_RANDOM]])
    removed = R.closed_form(data47, [(m, [0.0] * len(m)) for m, _f in scen47[:N_RANDOM]])
    assert len(only) == 1 and "forces" not in only[0][0]
    assert [rec["unstable"] for rec in only[0]] == removed["unstable"].tolist() and 0 < removed["unstable"].sum() < N_RANDOM
    for s, rec in enumerate(only[0]):
        if rec["unstable"]:
            assert rec["firstUnstable"] == scen47[s][0][removed["first_unstable"][s]]
            assert rec["peakStress"] == np.inf and rec["peakStressMember"] is None
            assert rec["peakDisplacement"] == np.inf and rec["peakDisplacementJoint"] is None
            assert rec["pivots"][removed["first_unstable"][s] + 1:] == [None] * (len(rec["pivots"]) - removed["first_unstable"][s] - 1)
        else:
            assert rec["firstUnstable"] is None and rec["factors"] == [0.0] * len(rec["members"])
