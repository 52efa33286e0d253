"""Natural frequencies, the part that needs no device: the header `include/trs_modes.h` against its ctypes table and the
library's exports, the argument errors of `solve_modes`, and the numpy yardstick of the GPU tests
(`tests/modes_reference.py`) against `numpy.linalg.eigvalsh`."""
import ctypes
import os

import numpy as np
import pytest

from python_stable_3d_truss_analysis_amd import _capi
from tests import helpers as H
from tests import modes_reference as R
from tests.test_capi_symbols import declared_prototypes, declared_symbols


def test_modes_header_table_and_exports_agree():
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    names = declared_symbols("trs_modes.h")
    protos = declared_prototypes("trs_modes.h")
    assert sorted(protos) == names == sorted(_capi.MODES_SIGNATURES) and len(names) == 6
    for name in names:
        assert hasattr(lib, name), f"{name} declared in trs_modes.h but not exported"
        restype, argtypes = _capi.MODES_SIGNATURES[name]
        is_void, n_params = protos[name]
        assert len(argtypes) == n_params and not is_void and restype is ctypes.c_int, name
        assert not name.endswith("_tab")
    # the two tables are disjoint and trs_solver.h's own is what it was
    assert not set(_capi.MODES_SIGNATURES) & set(_capi.SIGNATURES)
    assert sorted(_capi.SIGNATURES) == declared_symbols() and len(_capi.SIGNATURES) == 44
    loaded = _capi.load()
    assert loaded.trs_modes_abi_version() == _capi.MODES_ABI_VERSION == 1 and loaded.trs_abi_version() == 10
    header = open(os.path.join(H.ROOT, "include", "trs_modes.h")).read()
    assert "#define TRS_MODES_ABI_VERSION 1" in header and f"#define TRS_MODES_BLOCK {_capi.MODES_BLOCK} " in header
    # host-side answers: a bar-942-sized truss fits the mass kernel, a shape beyond a CU's LDS does not, and the step
    # refuses a block it cannot deliver before any launch
    assert loaded.trs_modes_fits(244, 942) == 1 and loaded.trs_modes_fits(10, 1 << 20) == 0
    assert loaded.trs_modes_step(1, 17, None, None, None, None, None, 64, None, None, None, 0, 0, 1, 1e-10, None) != 0
    assert loaded.trs_modes_step(0, 8, None, None, None, None, None, 64, None, None, None, 0, 0, 1, 1e-10, None) == 0


def test_solve_modes_argument_errors_need_no_gpu():
    import python_stable_3d_truss_analysis_amd as pkg
    from python_stable_3d_truss_analysis_amd import batch
    assert {"solve_modes", "ModeResult"} <= set(pkg.__all__)
    assert pkg.solve_modes is batch.solve_modes and pkg.ModeResult is batch.ModeResult
    packed = batch.pack_json([H.load_json("bar-25_input_0")] * 2)
    ok_mass = np.zeros([2, packed.nJ_max])
    for kw in (dict(p=0), dict(p=9), dict(p=2.5), dict(joint_mass=np.zeros([2, packed.nJ_max + 1])),
               dict(joint_mass=np.zeros([1, packed.nJ_max])), dict(joint_mass=ok_mass - 1.0),
               dict(joint_mass=ok_mass * np.nan), dict(mass_scale=-1.0), dict(tol=0.0), dict(max_iters=0)):
        with pytest.raises(ValueError):
            batch.solve_modes(packed, **kw)
    assert hasattr(pkg.Truss, "NaturalFrequencies")


@pytest.mark.parametrize("name", [n for n in H.data_case_names() if n.endswith("_input_0")] + H.cube7_case_names())
def test_numpy_block_iteration_agrees_with_eigvalsh(name):
    data = H.load_json(name)
    K_ff, m, _mask = R.matrices(data)
    want = R.eigenvalues(K_ff, m)
    lam, Phi, resid, n_modes, iters = R.block_iteration(K_ff, m, p=8)
    assert n_modes == min(8, len(m)) and iters > 0
    assert (np.abs(lam[:n_modes] - want[:n_modes]) / want[:n_modes]).max() <= 1e-9
    assert np.isnan(lam[n_modes:]).all() and (resid[:n_modes] <= 1e-10).all()
    G = Phi[:, :n_modes].T @ (m[:, None] * Phi[:, :n_modes])
    assert np.abs(G - np.eye(n_modes)).max() <= 1e-10


def test_partly_massless_reference():
    """Six DOFs with mass out of eighteen: the iteration delivers the six finite eigenvalues, exact after one step."""
    data = H.load_json("bar-25_input_0")
    data = dict(data, member=[[ends, [a, e, 0.0]] for ends, (a, e, _rho) in data["member"]])
    free_joints = [j for j, (_p, s) in enumerate(data["joint"]) if s == "NO"]
    joint_mass = np.zeros(len(data["joint"]))
    joint_mass[free_joints[:2]] = (3.0, 7.0)
    K_ff, m, _mask = R.matrices(data, joint_mass)
    assert (m > 0).sum() == 6
    lam, _Phi, _resid, n_modes, iters = R.block_iteration(K_ff, m, p=8)
    want = R.eigenvalues_semidefinite(K_ff, m)
    assert n_modes == 6 and iters == 8 and len(want) == 6
    assert (np.abs(lam[:6] - want) / want).max() <= 1e-9 and np.isnan(lam[6:]).all()
