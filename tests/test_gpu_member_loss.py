"""Member-loss analysis on the device (`solve_member_loss`, `DeviceBatch.member_loss`, `Truss.MemberLoss`; C ABI
include/trs_loss.h) against the numpy yardstick's re-solve (`tests/member_loss_reference.py`), the exact invariant, and
the bit guarantees of the analyses on the resident factor.

Tolerance of the parity tests, per fixture: max(1e-11, 100 d) relative to the largest magnitude of the compared array,
d the discrepancy between the yardstick's own two numpy routes on that fixture (computed here from reference code
alone; about 1e-10 on bar-942 and <= 1e-12 elsewhere).  The factor 100 covers a different elimination order and the
1 / r amplification (up to 2 700) of the weakest member."""
import numpy as np
import pytest

from oracle import truss_oracle as orc
from tests import helpers as H
from tests import member_loss_reference as M
from tests.test_gpu_load_cases import CONFIGS

pytestmark = pytest.mark.gpu

SMALL = ["bar-6_input_0", "bar-10_input_0", "bar-25_input_0", "bar-47_input_0", "bar-72_input_0", "cube-7_case_3",
         "cube-7_case_10"]
CRITICAL = {"bar-47_input_0": 12, "bar-942_input_0": 1, "cube-7_case_3": 9, "cube-7_case_10": 3}
L = 2
R_TOL = 1e-8      # the default (`batch.MEMBER_LOSS_R_TOL`, asserted equal below)
KEYS = ("r", "critical", "peak_stress", "peak_member", "peak_displace", "peak_joint", "N_after")
_REF, _ALONE = {}, {}


def cases_of(name):
    """The two load cases [2, nJ, 3] of a fixture: bar-72's two shipped ones; elsewhere the truss's own forces and one
    seeded case."""
    data = H.load_json(name)
    dim, nJ = orc.truss_dim(data), len(data["joint"])
    loads = np.zeros([L, nJ, 3])
    loads[0, :, :dim] = orc.force_vector(data).reshape(nJ, dim)
    if name == "bar-72_input_0":
        loads[1, :, :dim] = orc.force_vector(H.load_json("bar-72_input_1")).reshape(nJ, dim)
    else:
        loads[1, :, :dim] = np.random.default_rng(len(name) + nJ).uniform(-3e4, 3e4, size=(nJ, dim))
    return data, loads


def ref(name):
    """(data, loads, re-solve, closed form, tolerance) of a fixture, once per session."""
    if name not in _REF:
        data, loads = cases_of(name)
        a, b = M.resolve(data, loads), M.closed_form(data, loads)
        d = M.discrepancy(a, b)
        print(f"{name}: yardstick discrepancy d = {d:.3e}")
        _REF[name] = (data, loads, a, b, max(1e-11, 100 * d))
    return _REF[name]


def batch_loads(names, nJ_max):
    loads = np.zeros([len(names), L, nJ_max, 3])
    for b, name in enumerate(names):
        x = ref(name)[1]
        loads[b, :, :x.shape[1]] = x
    return loads


def solve(names, members="general", **kw):
    from python_stable_3d_truss_analysis_amd import batch
    assert batch.MEMBER_LOSS_R_TOL == R_TOL
    packed = batch.pack_json([ref(n)[0] for n in names], members=members)
    return packed, batch.solve_member_loss(packed, batch_loads(names, packed.nJ_max), want_forces=True, **kw)


def alone(name):
    if name not in _ALONE:
        _ALONE[name] = solve([name])
    return _ALONE[name]


def check(res, b, name):
    """Truss b of a result against the yardstick's re-solve.  Returns the largest error seen."""
    data, _loads, want, closed, tol = ref(name)
    dim, nJ, nM = orc.truss_dim(data), len(data["joint"]), len(data["member"])
    crit = want["critical"]
    assert not res.info[b]
    np.testing.assert_array_equal(res.critical[b, :nM], crit)
    assert int(crit.sum()) == CRITICAL.get(name, 0)
    errs = {"r": H.max_scaled_err(res.redundancy[b, :nM], closed["r"])}
    # the default r_tol lies a factor 100 from either class, on the device
    r_crit, r_rest = np.abs(res.redundancy[b, :nM][crit]).max(initial=0.0), res.redundancy[b, :nM][~crit].min()
    print(f"{name}: largest |r| among critical {r_crit:.2e}, smallest other r {r_rest:.2e}")
    assert r_crit <= R_TOL / 100 and r_rest >= 100 * R_TOL
    assert abs(res.redundancy[b, :nM].sum() - (nM - closed["n_free"])) <= 1e-8
    # the intact state
    errs["u"] = H.max_scaled_err(res.displace[b, :, :nJ, :dim], closed["u"])
    errs["N"] = H.max_scaled_err(res.internal[b, :, :nM], closed["N"])
    ok = ~crit
    errs["N_after"] = H.max_scaled_err(res.internal_after[b, :, :nM, :nM][:, ok], want["N_after"][:, ok])
    errs["peak_stress"] = H.max_scaled_err(res.peak_stress[b, :, :nM][:, ok], want["peak_stress"][:, ok])
    errs["peak_displace"] = H.max_scaled_err(res.peak_displace[b, :, :nM][:, ok], want["peak_displace"][:, ok])
    print(f"{name}: tolerance {tol:.2e}, errors " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for key, err in errs.items():
        assert err <= tol, (name, key, err, tol)
    # where the yardstick's best and second best differ by more than the tolerance - an absolute difference above
    # tol times the largest peak of the compared array, the scale every tolerance here is relative to - the places agree
    for got, key, gap, peak in ((res.peak_member, "peak_member", "stress_gap", "peak_stress"),
                                (res.peak_joint, "peak_joint", "displace_gap", "peak_displace")):
        clear = (want[gap] > tol * want[peak][:, ok].max()) & ok[None, :]
        np.testing.assert_array_equal(got[b, :, :nM][clear], want[key][clear])
    # critical members: inf, -1 and NaN rows; entry e of row e is zero
    assert np.isinf(res.peak_stress[b, :, :nM][:, crit]).all() and np.isinf(res.peak_displace[b, :, :nM][:, crit]).all()
    assert (res.peak_member[b, :, :nM][:, crit] == -1).all() and (res.peak_joint[b, :, :nM][:, crit] == -1).all()
    assert np.isnan(res.internal_after[b, :, :nM, :nM][:, crit]).all()
    assert not res.internal_after[b, :, np.arange(nM), np.arange(nM)][ok].any()
    # padding members and padding columns: zeros, ids -1
    assert not res.redundancy[b, nM:].any() and not res.critical[b, nM:].any()
    assert not res.peak_stress[b, :, nM:].any() and not res.peak_displace[b, :, nM:].any()
    assert (res.peak_member[b, :, nM:] == -1).all() and (res.peak_joint[b, :, nM:] == -1).all()
    assert not res.internal_after[b, :, nM:].any() and not res.internal_after[b, :, :nM, nM:].any()
    return max(errs.values())


# ---- 1. parity against the yardstick's re-solve ------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_a_truss_alone_against_the_resolve(name):
    packed, res = alone(name)
    assert res.internal_after.shape == (1, L, packed.nM_max, packed.nM_max)
    check(res, 0, name)


def test_the_ragged_batch_against_the_resolve():
    """All the small fixtures together: several size buckets, padding joints and members, 2D beside 3D."""
    packed, res = solve(SMALL)
    assert len({int(n) for n in packed.nM}) > 3
    for b, name in enumerate(SMALL):
        check(res, b, name)


@pytest.mark.parametrize("config", ["plain", "reorder-device", "table", "dense"])
def test_bar942_against_the_resolve(config):
    """bar-942 x 2: the envelope, several n_pad blocks, and 942 = 14 * 64 + 46 - the last chunk is partial."""
    kw = dict(CONFIGS[config])
    packed, res = solve(["bar-942_input_0"] * 2, members="auto" if kw.pop("table", False) else "general", **kw)
    assert packed.is_table == (config == "table")
    for b in range(2):
        check(res, b, "bar-942_input_0")
    for key in ("redundancy", "peak_stress", "peak_displace", "internal_after"):
        np.testing.assert_array_equal(getattr(res, key)[0].view(np.uint64), getattr(res, key)[1].view(np.uint64))


# ---- 3. the invariant on the device (also inside `check`) ---------------------------------------------------------------
def test_the_redundancies_sum_to_the_degree_of_indeterminacy():
    from python_stable_3d_truss_analysis_amd import batch
    datas = [H.load_json(n) for n in SMALL]
    packed = batch.pack_json(datas)
    res = batch.solve_member_loss(packed)        # the batch's own loads as one case
    assert res.peak_stress.shape == (len(SMALL), 1, packed.nM_max) and res.internal_after is None
    for b, data in enumerate(datas):
        want = len(data["member"]) - int(orc.free_mask(data).sum())
        assert abs(res.redundancy[b].sum() - want) <= 1e-8, (SMALL[b], res.redundancy[b].sum(), want)
        assert (res.redundancy[b] >= -1e-12).all() and (res.redundancy[b] <= 1 + 1e-12).all()


# ---- 4. bits ----------------------------------------------------------------------------------------------------------
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


def _same(a, b, keys=KEYS):
    for key in keys:
        np.testing.assert_array_equal(_bits(a[key]), _bits(b[key]), err_msg=key)


def test_the_chunk_does_not_change_a_bit():
    import torch
    _, db, loads = _resident(SMALL)
    outs = {c: _keep(db.member_loss(loads, want_forces=True, chunk=c)) for c in (16, 64, 1024)}
    torch.cuda.synchronize()
    _same(outs[16], outs[64])
    _same(outs[1024], outs[64])
    # a chunk is rounded up to a multiple of 16
    _same(_keep(db.member_loss(loads, want_forces=True, chunk=17)), db.member_loss(loads, want_forces=True, chunk=32))


def test_a_case_does_not_depend_on_the_other_cases():
    """Two cases together, each alone, and nine (two passes of the apply kernel) - bit for bit."""
    import torch
    _, db, loads = _resident(["bar-72_input_0", "bar-47_input_0", "bar-942_input_0"])
    both = _keep(db.member_loss(loads, want_forces=True))
    per_case = ("peak_stress", "peak_member", "peak_displace", "peak_joint", "N_after")
    for k in range(L):
        one = db.member_loss(loads[:, k:k + 1].contiguous(), want_forces=True)
        torch.cuda.synchronize()
        _same(one, both, ("r", "critical"))
        for key in per_case:
            np.testing.assert_array_equal(_bits(one[key]), _bits(both[key][:, k:k + 1]), err_msg=key)
    nine = db.member_loss(torch.cat([loads] * 4 + [loads[:, :1]], dim=1).contiguous())
    torch.cuda.synchronize()
    for k in range(9):
        for key in per_case[:-1]:
            np.testing.assert_array_equal(_bits(nine[key][:, k]), _bits(both[key][:, k % L]), err_msg=(key, k))
    _same(nine, both, ("r", "critical"))


def test_a_truss_does_not_depend_on_the_batch():
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    packed, db, loads = _resident(SMALL)
    whole = _keep(db.member_loss(loads, want_forces=True))
    for b in (1, 3, 4):
        one = batch.DeviceBatch(packed.take([b]), "cuda:0", use_small=False)
        one.factor()
        single = one.member_loss(loads[b:b + 1].contiguous(), want_forces=True)
        torch.cuda.synchronize()
        for key in KEYS:
            np.testing.assert_array_equal(_bits(single[key]), _bits(whole[key][b:b + 1]), err_msg=key)


def test_the_two_member_forms_give_the_same_bits():
    import torch
    names = ["bar-942_input_0", "bar-72_input_0"]
    _, db, loads = _resident(names, reorder="device")
    _, tdb, _ = _resident(names, table=True, reorder="device")
    assert tdb.table and not db.table
    a, b = db.member_loss(loads, want_forces=True), tdb.member_loss(loads, want_forces=True)
    torch.cuda.synchronize()
    _same(a, b, KEYS + ("u", "f_ext", "N"))


def test_repeated_calls_and_a_side_stream_give_the_same_bits():
    import torch
    names = ["bar-72_input_0", "cube-7_case_3"]
    _, db1, loads = _resident(names)
    _, db2, _ = _resident(names)
    first = _keep(db1.member_loss(loads, want_forces=True))
    again = db1.member_loss(loads, want_forces=True)
    torch.cuda.synchronize()
    _same(again, first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = db2.member_loss(loads, want_forces=True)
    torch.cuda.synchronize()
    _same(other, first)


# ---- 5. the intact state ------------------------------------------------------------------------------------------------
def test_the_intact_state_is_solve_cases_and_survives():
    import torch
    _, db, loads = _resident(["bar-942_input_0", "bar-47_input_0"], reorder="device")
    plain = _keep(db.solve_cases(loads))
    kept = db.cases_F.clone()
    before = db.generation
    out = db.member_loss(loads)
    torch.cuda.synchronize()
    assert "N_after" not in out and db.generation == before + 1
    _same(out, plain, ("u", "f_ext", "N"))
    np.testing.assert_array_equal(_bits(db.cases_F), _bits(kept))      # the chunk loop works on a buffer of its own
    grads = db.adjoint_cases(grad_u=torch.ones_like(loads), want=("A",))
    fresh = _keep(grads)
    db.solve_cases(loads)
    _same(db.adjoint_cases(grad_u=torch.ones_like(loads), want=("A",)), fresh, ("A",))
    # results go into a caller's dict, whose tensors are checked
    given = {"r": torch.zeros([db.B, db.nM_max], dtype=torch.float64, device=db.device)}
    assert db.member_loss(loads, out=given)["r"] is given["r"] and given["r"].any().item()
    with pytest.raises(ValueError):
        db.member_loss(loads, out={"critical": torch.zeros([db.B, db.nM_max], dtype=torch.int64, device=db.device)})


# ---- 6. errors and edges ------------------------------------------------------------------------------------------------
def test_no_factor_and_bad_arguments():
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    packed = batch.pack_json([H.load_json("bar-72_input_0")] * 2)
    db = batch.DeviceBatch(packed, "cuda:0", use_small=False)
    loads = torch.zeros([2, 1, packed.nJ_max, 3], dtype=torch.float64, device=db.device)
    with pytest.raises(ValueError, match="factor"):
        db.member_loss(loads)
    db.factor()
    for kw in (dict(r_tol=0.0), dict(r_tol=1.0), dict(chunk=0)):
        with pytest.raises(ValueError):
            db.member_loss(loads, **kw)
    with pytest.raises(ValueError):
        db.member_loss(loads.float())
    with pytest.raises(ValueError, match=str(2 * 72 * 72 * 8)):
        db.member_loss(loads, want_forces=True, max_result_bytes=1000)


def test_a_singular_truss_leaves_the_others_bits_unchanged():
    import torch
    good = "bar-72_input_0"
    from python_stable_3d_truss_analysis_amd import batch
    singular = H.edge_cases()["3d_mechanism_singular"]["input"]
    datas3 = [ref(good)[0], singular, ref(good)[0]]
    packed3 = batch.pack_json(datas3)
    packed2 = packed3.take([0, 2])
    loads3 = torch.from_numpy(batch_loads([good] * 3, packed3.nJ_max))
    loads3[1] = 0.0
    outs = []
    for packed, loads in ((packed3, loads3), (packed2, loads3[[0, 2]])):
        db = batch.DeviceBatch(packed, "cuda:0", use_small=False)
        db.factor()
        outs.append((db, db.member_loss(loads.contiguous().to(db.device), want_forces=True)))
    torch.cuda.synchronize()
    info = outs[0][0].info.cpu().numpy()
    assert info[0] == 0 and info[2] == 0 and info[1] > 0 and not outs[1][0].info.any().item()
    for key in KEYS:
        np.testing.assert_array_equal(_bits(outs[0][1][key][[0, 2]]), _bits(outs[1][1][key]), err_msg=key)


# ---- 7. the object model ------------------------------------------------------------------------------------------------
def test_truss_member_loss_on_bar72_and_bar47():
    from python_stable_3d_truss_analysis_amd import Truss
    data, loads, want, _closed, tol = ref("bar-72_input_0")
    truss = Truss(3).LoadFromJSON(data=data)
    before = truss.Serialize()
    cases = [{j: tuple(loads[k, j]) for j in range(len(data["joint"])) if loads[k, j].any()} for k in range(L)]
    got = truss.MemberLoss(cases, returnForces=True)
    assert len(got) == L and truss.Serialize() == before and not truss.isSolved
    _, res = alone("bar-72_input_0")
    for k in range(L):
        assert sorted(got[k]) == list(range(72))
        for e, rec in got[k].items():
            assert rec["redundancy"] == res.redundancy[0, e] and rec["critical"] is False
            assert rec["peakStress"] == res.peak_stress[0, k, e] and rec["peakStressMember"] == res.peak_member[0, k, e]
            assert rec["peakDisplacement"] == res.peak_displace[0, k, e]
            assert rec["peakDisplacementJoint"] == res.peak_joint[0, k, e]
            dense = np.zeros([72])
            for m, v in rec["forces"].items():
                dense[m] = v
            assert e not in rec["forces"] and all(abs(v) >= 1e-10 for v in rec["forces"].values())
            assert H.max_scaled_err(dense, want["N_after"][k, e]) <= tol
    # bar-47 (2D): its twelve critical members, with the truss's own forces as the one case
    data47, _loads, want47, _c, _t = ref("bar-47_input_0")
    only = Truss(2).LoadFromJSON(data=data47).MemberLoss()
    assert len(only) == 1 and "forces" not in only[0][0]
    critical = sorted(e for e, rec in only[0].items() if rec["critical"])
    assert critical == np.flatnonzero(want47["critical"]).tolist() and len(critical) == 12
    for e in critical:
        assert only[0][e]["peakStress"] == np.inf and only[0][e]["peakStressMember"] is None
        assert only[0][e]["peakDisplacement"] == np.inf and only[0][e]["peakDisplacementJoint"] is None
