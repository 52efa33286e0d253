"""Adjoint gradients without a GPU: the numpy reference of the formulas against central finite differences of the
oracle, the C ABI of the adjoint stages (declared, exported, argument checks before any launch) and the argument
errors of `DeviceBatch.adjoint_cases` / `solve_gradients` that need no device."""
import os

import numpy as np
import pytest

from oracle import truss_oracle as orc
from tests import adjoint_reference as R
from tests import helpers as H

TOL_FD = 1e-6   # the project's parity figure; the reference alone stays below 2.6e-8 on these inputs


def _seeded_cotangents(data, seed=1):
    """Random cotangents on u, f_ext and N at once, each scaled to its result (so every term of J weighs alike)."""
    nJ, nM, dim = len(data["joint"]), len(data["member"]), orc.truss_dim(data)
    rng = np.random.default_rng(seed)
    r0 = orc.solve(data)
    gu = rng.standard_normal((nJ, dim)) / np.abs(r0["u"]).max()
    gf = rng.standard_normal((nJ, dim)) / np.abs(r0["f_ext"]).max()
    gN = rng.standard_normal(nM) / np.abs(r0["N"]).max()
    return gu, gf, gN


@pytest.mark.parametrize("name,coordinates", [("bar-6", True), ("bar-10", True), ("bar-25", True), ("bar-72", True),
                                              ("bar-47", False)])
def test_reference_formulas_against_central_differences_of_the_oracle(name, coordinates):
    """bar-47's coordinate differences are truncation-dominated at this step (3.1e-6 measured when the formulas were
    derived), so it is checked for A, E and the loads only."""
    data = H.load_json(f"{name}_input_0")
    data = R.dense_forces(data, R.dense_loads(data))
    gu, gf, gN = _seeded_cotangents(data)
    got, _ = R.vjp(data, gu, gf, gN)
    fd = R.finite_differences(data, gu, gf, gN, h=1e-4, load_step=1e-2, coordinates=coordinates)
    errs = {k: H.max_scaled_err(got[k], fd[k]) for k in ("A", "E", "loads") + (("xyz",) if coordinates else ())}
    print(name, errs)
    for key, err in errs.items():
        assert err <= TOL_FD, (name, key, err)


def test_reference_of_several_cases_sums_the_parameter_gradients():
    data = H.load_json("bar-25_input_0")
    nJ, nM = len(data["joint"]), len(data["member"])
    rng = np.random.default_rng(4)
    loads = rng.uniform(-1e4, 1e4, size=(3, nJ, 3))
    gu, gf, gN = rng.standard_normal((3, nJ, 3)), rng.standard_normal((3, nJ, 3)), rng.standard_normal((3, nM))
    both, forward = R.vjp_cases(data, loads, gu, gf, gN)
    assert len(forward) == 3 and both["loads"].shape == (3, nJ, 3)
    parts = [R.vjp_cases(data, loads[k:k + 1], gu[k:k + 1], gf[k:k + 1], gN[k:k + 1])[0] for k in range(3)]
    for key in ("A", "E", "xyz"):
        np.testing.assert_allclose(both[key], sum(p[key] for p in parts), rtol=1e-12, atol=0)
    # the loads' gradient is zero at the supports and per case
    free = orc.free_mask(data).reshape(nJ, 3)
    assert not both["loads"][:, ~free].any()
    np.testing.assert_array_equal(both["loads"][1], parts[1]["loads"][0])


ADJOINT_SYMBOLS = {"trs_adjoint_fits", "trs_adjoint_rhs", "trs_adjoint_tab_rhs", "trs_adjoint_grad", "trs_adjoint_tab_grad"}


def test_every_adjoint_entry_point_is_declared_exported_and_bound():
    import ctypes
    from python_stable_3d_truss_analysis_amd import _capi
    from tests.test_capi_symbols import declared_symbols
    assert ADJOINT_SYMBOLS <= set(declared_symbols())
    assert ADJOINT_SYMBOLS <= set(_capi.SIGNATURES)
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in ADJOINT_SYMBOLS:
        assert hasattr(lib, name), name
    sig = _capi.SIGNATURES
    for stage in ("rhs", "grad"):
        assert len(sig[f"trs_adjoint_tab_{stage}"][1]) == len(sig[f"trs_adjoint_{stage}"][1])
    assert _capi.load().trs_abi_version() == 10


def test_the_public_names_are_importable_from_the_package():
    pytest.importorskip("torch")
    import python_stable_3d_truss_analysis_amd as pkg
    from python_stable_3d_truss_analysis_amd import DifferentiableTruss, GradientResult, solve_gradients
    assert callable(solve_gradients) and callable(DifferentiableTruss)
    assert [f for f in GradientResult.__dataclass_fields__] == ["dA", "dE", "dxyz", "dloads", "info"]
    assert {"solve_gradients", "GradientResult", "DifferentiableTruss"} <= set(pkg.__all__)
    assert hasattr(pkg.DeviceBatch, "adjoint_cases")


def test_adjoint_entry_points_check_their_arguments_before_any_launch():
    from python_stable_3d_truss_analysis_amd import _capi
    lib = _capi.load()
    nulls = [None] * 13
    # negative counts are refused, the table form without its tables too; nothing to do is not an error
    assert lib.trs_adjoint_rhs(-1, 1, 10, 10, *nulls, 64, None) != 0
    assert lib.trs_adjoint_rhs(1, -1, 10, 10, *nulls, 64, None) != 0
    assert lib.trs_adjoint_tab_rhs(1, 1, 10, 10, *nulls, 64, None) != 0
    assert lib.trs_adjoint_rhs(0, 4, 10, 10, *nulls, 64, None) == 0
    assert lib.trs_adjoint_rhs(4, 0, 10, 10, *nulls, 64, None) == 0
    assert lib.trs_adjoint_grad(-1, 1, 10, 10, *nulls[:11], 64, None, None, None, None, None, None) != 0
    assert lib.trs_adjoint_tab_grad(1, 1, 10, 10, *nulls[:11], 64, None, None, None, None, None, None) != 0
    assert lib.trs_adjoint_grad(0, 1, 10, 10, *nulls[:11], 64, None, None, None, None, None, None) == 0
    # the tables of one truss in 160 KB of LDS: two DOF vectors, the end lists of all joints, one double per member
    assert lib.trs_adjoint_fits(244, 942) == 1 and lib.trs_adjoint_fits(40000, 160000) == 0
    assert lib.trs_adjoint_fits(-1, 4) == 0
    bytes_of = lambda nj, nm: (6 * nj + nm) * 8 + (2 * nj + 1 + 2 * nm) * 4
    assert bytes_of(1500, 4500) <= 160 * 1024 < bytes_of(1600, 4800)
    assert lib.trs_adjoint_fits(1500, 4500) == 1 and lib.trs_adjoint_fits(1600, 4800) == 0


def _bare_device_batch(B=2, nJ_max=5, nM_max=7):
    """A `DeviceBatch` shell on the CPU device: enough for the argument checks, which come before any launch."""
    import torch
    from python_stable_3d_truss_analysis_amd import _capi, batch
    db = batch.DeviceBatch.__new__(batch.DeviceBatch)
    db.torch, db.device, db.lib = torch, torch.device("cpu"), _capi.load()
    db.B, db.nJ_max, db.nM_max, db.table = B, nJ_max, nM_max, False
    return db


def test_adjoint_cases_refuses_a_missing_or_stale_forward_state_and_bad_cotangents():
    torch = pytest.importorskip("torch")
    db = _bare_device_batch()
    with pytest.raises(ValueError, match="factor"):
        db.adjoint_cases()
    db._factored = True
    with pytest.raises(ValueError, match="solve_cases"):
        db.adjoint_cases()
    # a forward solution of L = 3, then another factorisation: stale
    db._generation = 2
    db._forward = (2, 3)
    z = lambda *shape, dtype=torch.float64: torch.zeros(list(shape), dtype=dtype)
    with pytest.raises(ValueError, match="L = 3"):
        db.adjoint_cases(grad_u=z(2, 2, 5, 3))            # L mismatch
    with pytest.raises(ValueError, match="grad_N"):
        db.adjoint_cases(grad_N=z(2, 3, 5))               # members, not joints
    with pytest.raises(ValueError, match="grad_f_ext"):
        db.adjoint_cases(grad_f_ext=z(2, 3, 5, 3, dtype=torch.float32))
    with pytest.raises(ValueError, match="want"):
        db.adjoint_cases(grad_u=z(2, 3, 5, 3), want=("A", "rho"))
    with pytest.raises(ValueError, match="out"):
        db.adjoint_cases(grad_u=z(2, 3, 5, 3), want=("A",), out={"A": z(2, 6)})
    with pytest.raises(ValueError, match="stale"):
        db.adjoint_cases(grad_u=z(2, 3, 5, 3), generation=1)
    db._bump_generation()                                 # what factor() and solve_cases() do
    with pytest.raises(ValueError, match="stale"):
        db.adjoint_cases(grad_u=z(2, 3, 5, 3))


def test_solve_gradients_refuses_section_variants_and_bad_shapes():
    pytest.importorskip("torch")
    from python_stable_3d_truss_analysis_amd import batch
    packed = batch.pack_json([H.load_json("bar-25_input_0")])
    nJ, nM = packed.nJ_max, packed.nM_max
    loads = np.zeros([1, 2, nJ, 3])
    with pytest.raises(ValueError, match="sections"):
        batch.solve_gradients(packed, loads, grad_u=np.zeros([1, 2, nJ, 3]), sections=[None])
    with pytest.raises(ValueError, match="loads"):
        batch.solve_gradients(packed, np.zeros([1, 2, nJ + 1, 3]), grad_u=np.zeros([1, 2, nJ, 3]))
    with pytest.raises(ValueError, match="grad_u"):
        batch.solve_gradients(packed, loads, grad_u=np.zeros([1, 3, nJ, 3]))      # L mismatch
    with pytest.raises(ValueError, match="grad_N"):
        batch.solve_gradients(packed, loads, grad_N=np.zeros([1, 2, nM + 1]))
    with pytest.raises(ValueError, match="nothing to differentiate"):
        batch.solve_gradients(packed, loads)
    with pytest.raises(ValueError, match="not both"):
        batch.solve_gradients(packed, loads, grad_u=np.zeros([1, 2, nJ, 3]), loss=lambda u, f, n: (u, None, None))
    with pytest.raises(ValueError, match="want"):
        batch.solve_gradients(packed, loads, grad_u=np.zeros([1, 2, nJ, 3]), want=("A", "rho"))
