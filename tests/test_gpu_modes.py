"""Natural frequencies and mode shapes from the resident factor (`solve_modes`, `DeviceBatch.modes`,
`Truss.NaturalFrequencies`; C ABI include/trs_modes.h) against numpy on the oracle's own matrices
(`tests/modes_reference.py`): eigenvalues against `eigvalsh`, shapes by what defines them."""
import numpy as np
import pytest

from oracle import truss_oracle as orc
from tests import helpers as H
from tests import modes_reference as R

pytestmark = pytest.mark.gpu
P = 8
LAM_TOL = 1e-9        # the project's asserted parity bound
PAIR_TOL = 1e-8       # |K phi - lam M phi|_2 / |K phi|_2
ORTHO_TOL = 1e-10     # |Phi^T M Phi - I|

FIXTURES = [n for n in H.data_case_names() if n.endswith("_input_0")] + H.cube7_case_names()
CONFIGS = {
    "general": dict(),
    "general-reorder": dict(reorder="device"),
    "table": dict(table=True),
    "table-reorder": dict(table=True, reorder="device"),
}
BIG_CONFIGS = {"dense": dict(use_envelope=False), "all-wide": dict(options={"all_wide": True})}

_reference = {}


def _ref(name, data=None, joint_mass=None, mass_scale=1.0):
    """(K_ff, m, mask, ascending eigenvalues) of a fixture, computed once."""
    if name not in _reference:
        K_ff, m, mask = R.matrices(H.load_json(name) if data is None else data, joint_mass, mass_scale)
        _reference[name] = (K_ff, m, mask, R.eigenvalues(K_ff, m))
    return _reference[name]


def _solve(datas, table=False, **kw):
    from python_stable_3d_truss_analysis_amd import batch
    packed = batch.pack_json(datas, members="auto" if table else "general")
    assert packed.is_table == table
    return batch.solve_modes(packed, p=P, **kw), packed


def _check_values(res, b, want, n_free, what):
    n_modes = int(res.n_modes[b])
    assert n_modes == min(P, n_free), what
    assert int(res.iters[b]) > 0 and int(res.info[b]) == 0, (what, res.iters[b], res.residual[b])
    lam = res.eigenvalue[b]
    err = (np.abs(lam[:n_modes] - want[:n_modes]) / want[:n_modes]).max()
    print(f"{what}: n_modes {n_modes} iters {int(res.iters[b])} eigenvalue error {err:.3e} "
          f"residual {np.nanmax(res.residual[b, :n_modes]):.3e}")
    assert err <= LAM_TOL, (what, err)
    assert np.isnan(lam[n_modes:]).all(), what
    np.testing.assert_array_equal(res.omega[b, :n_modes], np.sqrt(lam[:n_modes]))
    return n_modes


def _check_shapes(res, b, data, K_ff, m, mask, what):
    nJ, dim = len(data["joint"]), orc.truss_dim(data)
    n_modes = int(res.n_modes[b])
    shape = res.shape[b]
    free = np.zeros(shape.shape[1:], dtype=bool)
    free[:nJ, :dim] = mask.reshape(nJ, dim)
    assert not shape[:, ~free].any(), what                       # constrained DOFs, the z of a 2D truss, padding joints
    assert not shape[n_modes:].any(), what
    Phi = np.stack([shape[k, :nJ, :dim].ravel()[mask] for k in range(n_modes)], axis=1)
    lam = res.eigenvalue[b, :n_modes]
    KP = K_ff @ Phi
    pair = np.linalg.norm(KP - lam[None, :] * (m[:, None] * Phi), axis=0) / np.linalg.norm(KP, axis=0)
    ortho = np.abs(Phi.T @ (m[:, None] * Phi) - np.eye(n_modes)).max()
    print(f"{what}: pair residual {pair.max():.3e} orthonormality {ortho:.3e}")
    assert pair.max() <= PAIR_TOL and ortho <= ORTHO_TOL, (what, pair.max(), ortho)
    for k in range(n_modes):                                      # sign: the largest component, first on a tie, is positive
        v = shape[k].ravel()
        assert v[np.argmax(np.abs(v))] > 0, (what, k)


@pytest.fixture(scope="module")
def solved():
    """Every fixture in every configuration, solved once (batches of one: each fixture in its own shape)."""
    cache = {}

    def get(config, name):
        if (config, name) not in cache:
            kw = dict({**CONFIGS, **BIG_CONFIGS}[config])
            cache[config, name] = _solve([H.load_json(name)], **kw)[0]
        return cache[config, name]
    return get


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_eigenvalues_of_every_fixture(solved, config):
    for name in FIXTURES:
        K_ff, m, mask, want = _ref(name)
        _check_values(solved(config, name), 0, want, len(m), f"{name} [{config}]")


@pytest.mark.parametrize("config", sorted(BIG_CONFIGS))
def test_eigenvalues_bar942_dense_and_all_wide(solved, config):
    K_ff, m, mask, want = _ref("bar-942_input_0")
    res = solved(config, "bar-942_input_0")
    _check_values(res, 0, want, len(m), f"bar-942 [{config}]")
    _check_shapes(res, 0, H.load_json("bar-942_input_0"), K_ff, m, mask, f"bar-942 [{config}]")


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_shapes_of_every_fixture(solved, config):
    """With `reorder="device"` the shapes are checked against the UN-reordered matrices: caller's numbering."""
    for name in FIXTURES:
        K_ff, m, mask, _want = _ref(name)
        _check_shapes(solved(config, name), 0, H.load_json(name), K_ff, m, mask, f"{name} [{config}]")


def test_all_fixtures_in_one_ragged_batch():
    """The bucketed driver on a mixed batch (every fixture at once, device order): per truss as alone."""
    datas = [H.load_json(n) for n in FIXTURES]
    res, packed = _solve(datas, reorder="device")
    assert res.shape.shape == (len(datas), P, packed.nJ_max, 3)
    for b, name in enumerate(FIXTURES):
        K_ff, m, mask, want = _ref(name)
        _check_values(res, b, want, len(m), f"{name} [ragged]")
        _check_shapes(res, b, datas[b], K_ff, m, mask, f"{name} [ragged]")


# ---- bar-942 x 64: per-copy areas and joint masses, independence of the batch ---------------------------------------
_B = 64


@pytest.fixture(scope="module")
def bar942_copies():
    base = H.load_json("bar-942_input_0")
    rng = np.random.default_rng(942)
    scale = np.round(rng.uniform(0.5, 2.0, size=_B), 3)
    joint_mass = rng.uniform(0.0, 50.0, size=(_B, len(base["joint"])))
    datas = [dict(base, member=[[ends, [a * s, e, rho]] for ends, (a, e, rho) in base["member"]]) for s in scale]
    return datas, joint_mass


def _bits(res, b=slice(None)):
    return [np.ascontiguousarray(x[b]).view(np.uint64 if x.dtype == np.float64 else x.dtype)
            for x in (res.eigenvalue, res.shape, res.residual, res.iters)]


def test_bar942_batch_against_numpy_and_independent_of_the_batch(bar942_copies):
    from python_stable_3d_truss_analysis_amd import batch
    datas, joint_mass = bar942_copies
    kw = dict(p=P, joint_mass=joint_mass, reorder="device")
    packed = batch.pack_json(datas)
    res = batch.solve_modes(packed, **kw)
    for b in range(_B):
        K_ff, m, mask = R.matrices(datas[b], joint_mass[b])
        _check_values(res, b, R.eigenvalues(K_ff, m), len(m), f"copy {b}")
        if b % 8 == 0:
            _check_shapes(res, b, datas[b], K_ff, m, mask, f"copy {b}")
    again = batch.solve_modes(packed, **kw)
    for x, y in zip(_bits(res), _bits(again)):
        np.testing.assert_array_equal(x, y)
    for b in (0, 17, 42, 63):
        alone = batch.solve_modes(batch.pack_json([datas[b]]), p=P, joint_mass=joint_mass[b:b + 1], reorder="device")
        for x, y in zip(_bits(res, slice(b, b + 1)), _bits(alone)):
            np.testing.assert_array_equal(x, y, err_msg=f"copy {b} alone")
    table = batch.pack_json(datas, members="auto")
    assert table.is_table
    tab = batch.solve_modes(table, **kw)
    for x, y in zip(_bits(res), _bits(tab)):
        np.testing.assert_array_equal(x, y)


# ---- partly massless, mass_scale --------------------------------------------------------------------------------------
def test_partly_massless_truss_delivers_the_finite_pairs():
    from python_stable_3d_truss_analysis_amd import batch
    data = H.load_json("bar-25_input_0")
    data = dict(data, member=[[ends, [a, e, 0.0]] for ends, (a, e, _rho) in data["member"]])
    free_joints = [j for j, (_p, s) in enumerate(data["joint"]) if s == "NO"]
    joint_mass = np.zeros([1, len(data["joint"])])
    joint_mass[0, free_joints[:2]] = (3.0, 7.0)
    res = batch.solve_modes(batch.pack_json([data]), p=P, joint_mass=joint_mass)
    K_ff, m, mask = R.matrices(data, joint_mass[0])
    want = R.eigenvalues_semidefinite(K_ff, m)
    assert int(res.n_modes[0]) == 6 and len(want) == 6 and int(res.iters[0]) > 0
    err = (np.abs(res.eigenvalue[0, :6] - want) / want).max()
    print(f"partly massless: eigenvalue error {err:.3e}")
    assert err <= LAM_TOL
    assert np.isnan(res.eigenvalue[0, 6:]).all() and np.isnan(res.omega[0, 6:]).all()
    assert not res.shape[0, 6:].any() and res.shape[0, :6].any(axis=(1, 2)).all()


def test_mass_scale_scales_every_eigenvalue(solved):
    from python_stable_3d_truss_analysis_amd import batch
    for name in FIXTURES:
        plain = solved("general", name)
        scaled = batch.solve_modes(batch.pack_json([H.load_json(name)]), p=P, mass_scale=1.0 / 386.4)
        n_modes = int(plain.n_modes[0])
        assert int(scaled.n_modes[0]) == n_modes and int(scaled.iters[0]) > 0
        err = (np.abs(scaled.eigenvalue[0, :n_modes] / 386.4 - plain.eigenvalue[0, :n_modes])
               / plain.eigenvalue[0, :n_modes]).max()
        print(f"{name}: mass_scale error {err:.3e}")
        assert err <= 1e-12, (name, err)


# ---- the model's method, the small-truss route ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bar-72_input_0", "bar-942_input_0"])
def test_truss_natural_frequencies(name):
    import os
    from python_stable_3d_truss_analysis_amd import Truss, batch
    data = H.load_json(name)
    truss = Truss(orc.truss_dim(data)).LoadFromJSON(os.path.join(H.GOLDEN, "data", name + ".json"))
    before, solved_before = truss.Serialize(), truss.isSolved
    omega = truss.NaturalFrequencies()
    assert truss.Serialize() == before and truss.isSolved == solved_before and not solved_before
    res = batch.solve_modes([truss], p=6)
    assert omega.shape == (6,)
    np.testing.assert_array_equal(omega, res.omega[0])
    K_ff, m, mask, want = _ref(name)
    assert (np.abs(omega ** 2 - want[:6]) / want[:6]).max() <= LAM_TOL
    masses = {j: 2.0 + j for j in range(0, len(data["joint"]), 3)}
    omega2, shapes = truss.NaturalFrequencies(nModes=4, jointMasses=masses, massScale=0.5, returnShapes=True)
    dense = np.zeros([1, len(data["joint"])])
    for j, v in masses.items():
        dense[0, j] = v
    res2 = batch.solve_modes([truss], p=4, joint_mass=dense, mass_scale=0.5)
    np.testing.assert_array_equal(omega2, res2.omega[0])
    assert len(shapes) == 4 and sorted(shapes[0]) == list(range(len(data["joint"])))
    for k in range(4):
        got = np.stack([shapes[k][j] for j in range(len(data["joint"]))])
        np.testing.assert_array_equal(got, res2.shape[0, k, :len(data["joint"]), :truss.dim])
    truss.Solve()
    solved_state = truss.Serialize()
    truss.NaturalFrequencies(nModes=2)
    assert truss.isSolved and truss.Serialize() == solved_state


def test_small_trusses_go_through_the_staged_pipeline():
    """bar-25 and bar-120 together would take the fused small-system kernel in `solve_batch`, which keeps no factor."""
    from python_stable_3d_truss_analysis_amd import batch
    names = ["bar-25_input_0", "bar-120_input_0"]
    packed = batch.pack_json([H.load_json(n) for n in names])
    assert batch.DeviceBatch(packed, "cuda:0").small
    with pytest.raises(ValueError):
        batch.DeviceBatch(packed, "cuda:0").factor()
    res = batch.solve_modes(packed, p=P)
    for b, name in enumerate(names):
        K_ff, m, mask, want = _ref(name)
        _check_values(res, b, want, len(m), name)


# ---- the resident batch: what modes() does to the other users of the factor -----------------------------------------
def test_modes_between_the_other_users_of_the_factor():
    import torch
    from python_stable_3d_truss_analysis_amd import batch
    data = H.load_json("bar-942_input_0")
    nJ = len(data["joint"])
    packed = batch.pack_json([data] * 3)
    rng = np.random.default_rng(9)
    loads = rng.uniform(-30000.0, 30000.0, size=(3, 2, packed.nJ_max, 3))
    dev_loads = torch.from_numpy(loads).to("cuda:0")
    db = batch.DeviceBatch(packed, "cuda:0", use_small=False, reorder="device")
    with pytest.raises(ValueError):
        db.modes(P)                                   # no factor yet
    db.factor()
    with pytest.raises(ValueError):
        db.modes(9)
    db.solve_cases(dev_loads)
    seen = db.generation
    out = db.modes(P)
    assert db.generation > seen
    with pytest.raises(ValueError, match="stale"):
        db.adjoint_cases(grad_u=torch.ones_like(dev_loads))
    K_ff, m, mask, want = _ref("bar-942_input_0")
    lam = out["lam"].cpu().numpy()
    assert (out["iters"] > 0).all() and (np.abs(lam - want[None, :P]) / want[None, :P]).max() <= LAM_TOL
    # the factor was only read: the load cases still match the oracle
    res = db.solve_cases(dev_loads)
    torch.cuda.synchronize()
    for b in range(3):
        for k in range(2):
            force = [[j, [float(x) for x in loads[b, k, j]]] for j in range(nJ) if np.any(loads[b, k, j] != 0)]
            ref = orc.solve(dict(data, force=force))
            assert H.max_scaled_err(res["u"][b, k, :nJ].cpu().numpy(), ref["u"]) <= 1e-9
            assert H.max_scaled_err(res["N"][b, k, :len(data["member"])].cpu().numpy(), ref["N"]) <= 1e-9
    db.adjoint_cases(grad_u=torch.ones_like(dev_loads))   # and a fresh forward solution can be differentiated again
