"""Load cases with support settlements, member pre-strain and self-weight on the device (`solve_effect_cases`,
`DeviceBatch.solve_effect_cases`, `Truss.SolveEffectCases`; C ABI include/trs_effects.h) against the numpy restatement
of their definitions (`tests/effects_reference.py`), the physical identities, and the bit guarantees of the load cases."""
import numpy as np
import pytest

from oracle import truss_oracle as orc
from tests import effects_reference as R
from tests import helpers as H
from tests.test_effects import (NAMES, check_common_translation, check_uniform_strain, check_unit_gravity, res_mask)
from tests.test_gpu_load_cases import CONFIGS

pytestmark = pytest.mark.gpu
TOL = 1e-9
KEYS = ("u", "f_ext", "N", "body")


def draw(data, rng, nJ_max=None, nM_max=None):
    """One seeded case carrying all four inputs, padded: loads, ubar [nJ_max, 3], eps0 [nM_max], g [3] (z = 0 in 2D;
    ubar at the constrained DOFs only)."""
    dim, nJ, nM = orc.truss_dim(data), len(data["joint"]), len(data["member"])
    nJ_max, nM_max = nJ_max or nJ, nM_max or nM
    out = {"loads": np.zeros([nJ_max, 3]), "settlement": np.zeros([nJ_max, 3]), "prestrain": np.zeros([nM_max]),
           "accel": np.zeros([3])}
    out["loads"][:nJ, :dim] = rng.uniform(-3e4, 3e4, size=(nJ, dim))
    out["settlement"][:nJ, :dim] = rng.uniform(-0.02, 0.02, size=(nJ, dim)) * ~res_mask(data)
    out["prestrain"][:nM] = rng.uniform(-5e-4, 5e-4, size=nM)
    out["accel"][:dim] = rng.uniform(-2.0, 2.0, size=dim)
    return out


def reference(data, case):
    return R.solve(data, loads=case.get("loads"), prestrain=case.get("prestrain"), settlement=case.get("settlement"),
                   accel=case.get("accel"))


def stack(cases_of, B, L, key):
    """[B, L, ...] of `key` from cases_of(b, k)."""
    return np.stack([np.stack([cases_of(b, k)[key] for k in range(L)]) for b in range(B)])


def check(res, ref_of, B, L, nJ, nM, dims, tol=TOL):
    got_of = {"u": res.displace, "f_ext": res.external, "N": res.internal, "body": res.body}
    worst = 0.0
    for b in range(B):
        for k in range(L):
            ref = ref_of(b, k)
            for key in KEYS:
                got = got_of[key][b, k, :nM[b]] if key == "N" else got_of[key][b, k, :nJ[b], :dims[b]]
                err = H.max_scaled_err(got, ref[key])
                worst = max(worst, err)
                assert err <= tol, (b, k, key, err)
            # nothing beyond the truss's own joints, members and axes
            assert not got_of["N"][b, k, nM[b]:].any()
            for key in ("u", "f_ext", "body"):
                assert not got_of[key][b, k, nJ[b]:].any() and not got_of[key][b, k, :, dims[b]:].any()
    print(f"worst scaled error {worst:.3e}")


# ---- bar-942 x 64, eight seeded cases mixing all four inputs (each copy takes them in its own seeded order) ---------
_B942, _L942 = 64, 8


@pytest.fixture(scope="module")
def bar942():
    data = H.load_json("bar-942_input_0")
    rng = np.random.default_rng(942)
    cases = [draw(data, rng) for _ in range(_L942)]
    # cases 0 .. 3 carry ONE input each (the other arrays hold zeros there), 4 .. 7 all four
    for c, keep in enumerate(("loads", "prestrain", "settlement", "accel")):
        for key in cases[c]:
            if key != keep:
                cases[c][key] = np.zeros_like(cases[c][key])
    order = np.stack([rng.permutation(_L942) for _ in range(_B942)])
    refs = [reference(data, c) for c in cases]
    return data, cases, order, refs


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_bar942_effect_cases_against_the_reference(bar942, config):
    from python_stable_3d_truss_analysis_amd import batch
    data, cases, order, refs = bar942
    kw = dict(CONFIGS[config])
    packed = batch.pack_json([data] * _B942, members="auto" if kw.pop("table", False) else "general")
    assert packed.is_table == (config == "table")
    inputs = {key: stack(lambda b, k: cases[order[b, k]], _B942, _L942, key) for key in cases[0]}
    res = batch.solve_effect_cases(packed, **inputs, **kw)
    assert res.displace.shape == res.body.shape == (_B942, _L942, packed.nJ_max, 3)
    assert res.internal.shape == (_B942, _L942, packed.nM_max) and not res.info.any()
    check(res, lambda b, k: refs[order[b, k]], _B942, _L942, packed.nJ, packed.nM, packed.dim)


@pytest.mark.parametrize("config", ["plain", "reorder-device", "table"])
def test_ragged_batch_through_the_buckets(config):
    """bar-25, bar-47, bar-72, bar-942 and the cube-7 cases together: several size buckets, padded joints and members."""
    from python_stable_3d_truss_analysis_amd import batch
    kw = dict(CONFIGS[config])
    names = ["bar-25_input_0", "bar-47_input_0", "bar-72_input_0", "bar-942_input_0"] + H.cube7_case_names()
    datas = [H.load_json(n) for n in names]
    assert len(datas) >= 5
    packed = batch.pack_json(datas, members="auto" if kw.pop("table", False) else "general")
    B, L = packed.B, 3
    rng = np.random.default_rng(25)
    cases = [[draw(d, rng, packed.nJ_max, packed.nM_max) for _ in range(L)] for d in datas]
    inputs = {key: stack(lambda b, k: cases[b][k], B, L, key) for key in cases[0][0]}
    res = batch.solve_effect_cases(packed, **inputs, **kw)
    assert not res.info.any()
    refs = {}

    def ref_of(b, k):
        if (b, k) not in refs:
            c = cases[b][k]
            nj, nm = len(datas[b]["joint"]), len(datas[b]["member"])
            refs[b, k] = reference(datas[b], dict(loads=c["loads"][:nj], settlement=c["settlement"][:nj],
                                                  prestrain=c["prestrain"][:nm], accel=c["accel"]))
        return refs[b, k]
    check(res, ref_of, B, L, packed.nJ, packed.nM, packed.dim)


def test_the_2d_truss_with_two_component_vectors():
    from python_stable_3d_truss_analysis_amd import batch
    data = H.load_json("bar-10_input_0")
    assert orc.truss_dim(data) == 2
    B, L = 3, 4
    packed = batch.pack_json([data] * B)
    rng = np.random.default_rng(10)
    cases = [[draw(data, rng) for _ in range(L)] for _ in range(B)]
    inputs = {key: stack(lambda b, k: cases[b][k], B, L, key) for key in cases[0][0]}
    two = {key: (v if key == "prestrain" else v[..., :2]) for key, v in inputs.items()}
    res = batch.solve_effect_cases(packed, **two, reorder="device")
    assert not res.info.any()
    check(res, lambda b, k: reference(data, cases[b][k]), B, L, packed.nJ, packed.nM, packed.dim)
    again = batch.solve_effect_cases(packed, **inputs, reorder="device")
    for a, b in ((res.displace, again.displace), (res.external, again.external), (res.internal, again.internal),
                 (res.body, again.body)):
        np.testing.assert_array_equal(a, b)


# ---- the physical identities of tests/test_effects.py, on the device results ----------------------------------------
def device_solve(data, **case):
    from python_stable_3d_truss_analysis_amd import batch
    dim, nJ, nM = orc.truss_dim(data), len(data["joint"]), len(data["member"])
    res = batch.solve_effect_cases(batch.pack_json([data]), **{k: np.asarray(v, dtype=float)[None, None]
                                                                for k, v in case.items()})
    assert not res.info.any()
    return {"u": res.displace[0, 0, :nJ, :dim], "f_ext": res.external[0, 0, :nJ, :dim], "N": res.internal[0, 0, :nM],
            "body": res.body[0, 0, :nJ, :dim]}


@pytest.mark.parametrize("name", NAMES)
def test_device_common_translation(name):
    check_common_translation(H.load_json(name), device_solve)


@pytest.mark.parametrize("name", NAMES)
def test_device_uniform_strain(name):
    check_uniform_strain(H.load_json(name), device_solve)


@pytest.mark.parametrize("name", NAMES)
def test_device_unit_gravity(name):
    check_unit_gravity(H.load_json(name), device_solve)


# ---- against the plain load cases, and the bit guarantees -----------------------------------------------------------
def _resident(reorder="device", copies=4, table=False, datas=None):
    from python_stable_3d_truss_analysis_amd import batch
    datas = datas or [H.load_json("bar-942_input_0")] * copies
    packed = batch.pack_json(datas, members="auto" if table else "general")
    db = batch.DeviceBatch(packed, "cuda:0", use_small=False, reorder=reorder)
    db.factor()
    return packed, db


def _inputs(torch, packed, db, L, seed=3):
    """Seeded device tensors of all four inputs, different for every truss and case."""
    rng = np.random.default_rng(seed)
    held = packed.constrained()
    x = {"loads": rng.uniform(-3e4, 3e4, size=(db.B, L, db.nJ_max, 3)),
         "prestrain": rng.uniform(-5e-4, 5e-4, size=(db.B, L, db.nM_max)),
         "settlement": rng.uniform(-0.02, 0.02, size=(db.B, L, db.nJ_max, 3)) * held[:, None],
         "accel": rng.uniform(-2.0, 2.0, size=(db.B, L, 3))}
    return {k: torch.from_numpy(v).to(db.device) for k, v in x.items()}


def _bits(t):
    return t.cpu().numpy().view(np.uint64)


def _keep(out):
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("table", [False, True])
def test_loads_alone_are_solve_cases_bit_for_bit(table):
    import torch
    packed, db = _resident(table=table)
    x = _inputs(torch, packed, db, 6)
    plain = _keep(db.solve_cases(x["loads"]))
    got = db.solve_effect_cases(loads=x["loads"], want_body=True)
    torch.cuda.synchronize()
    for key in ("u", "f_ext", "N"):
        np.testing.assert_array_equal(_bits(got[key]), _bits(plain[key]))
    assert not got["body"].any().item()
    # explicit zero arrays for the three effects: the same numbers (a sum with zero may turn a -0 into +0, no more)
    zeros = {k: torch.zeros_like(x[k]) for k in ("prestrain", "settlement", "accel")}
    zero = db.solve_effect_cases(loads=x["loads"], want_body=True, **zeros)
    torch.cuda.synchronize()
    for key in ("u", "f_ext", "N"):
        assert H.max_scaled_err(zero[key].cpu().numpy(), plain[key].cpu().numpy()) <= 1e-12
    assert not zero["body"].any().item()


def test_a_case_does_not_depend_on_the_other_cases():
    """Case k alone and among eight (and among 17: two groups of the substitution) - bit for bit."""
    import torch
    packed, db = _resident()
    x = _inputs(torch, packed, db, 17)
    cut = lambda lo, hi: {k: v[:, lo:hi].contiguous() for k, v in x.items()}
    outs = {L: _keep(db.solve_effect_cases(**cut(0, L), want_body=True)) for L in (8, 17)}
    for k in (0, 5, 7):
        alone = db.solve_effect_cases(**cut(k, k + 1), want_body=True)
        torch.cuda.synchronize()
        for key in KEYS:
            np.testing.assert_array_equal(_bits(alone[key]), _bits(outs[8][key][:, k:k + 1]))
    for key in KEYS:
        np.testing.assert_array_equal(_bits(outs[17][key][:, :8]), _bits(outs[8][key]))


def test_a_truss_does_not_depend_on_the_batch():
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    datas = [H.load_json(n) for n in ("bar-942_input_0", "bar-72_input_0", "bar-942_input_0", "bar-25_input_0")]
    packed, db = _resident(datas=datas)
    x = _inputs(torch, packed, db, 8)
    whole = _keep(db.solve_effect_cases(**x, want_body=True))
    for b in (0, 2):
        one = batch.DeviceBatch(packed.take([b]), "cuda:0", use_small=False, reorder="device")
        one.factor()
        alone = one.solve_effect_cases(**{k: v[b:b + 1].contiguous() for k, v in x.items()}, want_body=True)
        torch.cuda.synchronize()
        for key in KEYS:
            np.testing.assert_array_equal(_bits(alone[key]), _bits(whole[key][b:b + 1]))


def test_the_two_member_forms_give_the_same_bits():
    import torch
    packed, db = _resident()
    tpacked, tdb = _resident(table=True)
    assert tdb.table and not db.table
    x = _inputs(torch, packed, db, 8)
    a, b = db.solve_effect_cases(**x, want_body=True), tdb.solve_effect_cases(**x, want_body=True)
    torch.cuda.synchronize()
    for key in KEYS:
        np.testing.assert_array_equal(_bits(a[key]), _bits(b[key]))


def test_repeated_calls_and_a_side_stream_give_the_same_bits():
    import torch
    packed, db1 = _resident()
    _, db2 = _resident()
    x = _inputs(torch, packed, db1, 8)
    ref = _keep(db1.solve_effect_cases(**x, want_body=True))
    again = db1.solve_effect_cases(**x, want_body=True)
    torch.cuda.synchronize()
    for key in KEYS:
        np.testing.assert_array_equal(_bits(again[key]), _bits(ref[key]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    outs = []
    for _ in range(3):
        o1 = db1.solve_effect_cases(**x, want_body=True)
        with torch.cuda.stream(side):
            o2 = db2.solve_effect_cases(**x, want_body=True)
        outs.append((o1, o2))
    torch.cuda.synchronize()
    for o1, o2 in outs:
        for key in KEYS:
            np.testing.assert_array_equal(_bits(o1[key]), _bits(ref[key]))
            np.testing.assert_array_equal(_bits(o2[key]), _bits(ref[key]))


# ---- behaviour around the factor ------------------------------------------------------------------------------------
def test_no_factor_and_the_adjoint_refusal():
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    packed = batch.pack_json([H.load_json("bar-942_input_0")] * 2)
    db = batch.DeviceBatch(packed, "cuda:0", use_small=False)
    x = _inputs(torch, packed, db, 2)
    with pytest.raises(ValueError):
        db.solve_effect_cases(**x)
    db.factor()
    with pytest.raises(ValueError):
        db.solve_effect_cases()
    with pytest.raises(ValueError):
        db.solve_effect_cases(loads=x["loads"], prestrain=x["prestrain"][:, :1].contiguous())
    with pytest.raises(ValueError):
        db.solve_effect_cases(accel=x["accel"].float())
    with pytest.raises(ValueError):
        db.solve_effect_cases(settlement=x["settlement"].cpu())
    db.solve_cases(x["loads"])
    gu = torch.ones_like(x["loads"])
    assert set(db.adjoint_cases(grad_u=gu, want=("A",))) == {"A"}      # (a plain forward state is differentiable)
    before = db.generation
    db.solve_effect_cases(**x)
    assert db.generation == before + 1
    with pytest.raises(ValueError):
        db.adjoint_cases(grad_u=gu, want=("A",))
    with pytest.raises(ValueError):
        db.adjoint_cases(grad_u=gu, want=("A",), generation=db.generation)
    db.solve_cases(x["loads"])                                           # and a plain solve makes it so again
    assert set(db.adjoint_cases(grad_u=gu, want=("A",))) == {"A"}


def test_a_singular_truss_leaves_the_others_bits_unchanged():
    import torch
    good = H.load_json("bar-942_input_0")
    singular = H.edge_cases()["3d_mechanism_singular"]["input"]
    packed3, db3 = _resident(reorder=False, datas=[good, singular, good])
    packed2, db2 = _resident(reorder=False, datas=[good, good])
    assert (packed3.nJ_max, packed3.nM_max) == (packed2.nJ_max, packed2.nM_max)
    x3 = _inputs(torch, packed3, db3, 4)
    x2 = {k: v[[0, 2]].contiguous() for k, v in x3.items()}
    r3, r2 = db3.solve_effect_cases(**x3, want_body=True), db2.solve_effect_cases(**x2, want_body=True)
    torch.cuda.synchronize()
    info = db3.info.cpu().numpy()
    assert info[0] == 0 and info[2] == 0 and info[1] > 0 and not db2.info.any().item()
    for key in KEYS:
        np.testing.assert_array_equal(_bits(r3[key][[0, 2]]), _bits(r2[key]))


# ---- the object model -----------------------------------------------------------------------------------------------
def test_truss_solve_effect_cases_on_bar72():
    from python_stable_3d_truss_analysis_amd import LoadCase, Truss
    data = H.load_json("bar-72_input_0")
    truss = Truss(3).LoadFromJSON(data=data)
    nJ, nM = truss.nJoint, truss.nMember
    support = next(j for j, (_p, s) in enumerate(data["joint"]) if s == "PIN")
    forces = {int(j): tuple(v) for j, v in data["force"]}
    cases = [LoadCase(forces=forces),
             LoadCase(forces=forces, settlements={support: (0.0, 0.004, -0.012)}, prestrains={17: 6.5e-6 * 80.0}),
             LoadCase(gravity=(0.0, 0.0, -1.0))]
    before = truss.Serialize()
    solved = truss.SolveEffectCases(cases)
    assert len(solved) == 3 and not truss.isSolved and truss.Serialize() == before
    loads = orc.densify(data["force"], nJ, 3)
    ubar, eps0 = np.zeros([nJ, 3]), np.zeros([nM])
    ubar[support], eps0[17] = (0.0, 0.004, -0.012), 6.5e-6 * 80.0
    refs = [R.solve(data, loads=loads), R.solve(data, loads=loads, prestrain=eps0, settlement=ubar),
            R.solve(data, accel=(0.0, 0.0, -1.0))]
    for t, ref in zip(solved, refs):
        assert t.isSolved
        dense = lambda d, n, w=None: orc.densify([[k, v] for k, v in d.items()], n, w)
        assert H.max_scaled_err(dense(t.GetDisplacements(), nJ, 3), ref["u"]) <= TOL
        assert H.max_scaled_err(dense(t.GetExternalForces(), nJ, 3), ref["f_ext"]) <= TOL
        assert H.max_scaled_err(dense(t.GetInternalForces(), nM), ref["N"]) <= TOL
        assert H.max_scaled_err(dense(t.bodyForces, nJ, 3), ref["body"]) <= TOL
    np.testing.assert_array_equal(solved[1].GetDisplacements()[support], [0.0, 0.004, -0.012])
    assert support not in solved[0].GetDisplacements()
    assert solved[1].GetForces() == solved[0].GetForces() and solved[2].GetForces() == {}
    assert abs(sum(v[2] for v in solved[2].GetResistances().values()) - truss.weight) <= TOL * truss.weight
    with pytest.raises(ValueError):     # a settlement along a free axis (the first unsupported joint)
        free = next(j for j, (_p, s) in enumerate(data["joint"]) if s == "NO")
        truss.SolveEffectCases([LoadCase(settlements={free: (0.0, 0.0, 0.01)})])
