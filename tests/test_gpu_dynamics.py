"""Transient response on the GPU (`DeviceBatch.factor_dynamic` / `transient`, `solve_transient`,
`Truss.TransientResponse`; C ABI include/trs_dynamics.h) against the numpy yardstick `tests/dynamics_reference.py`.

The parity tolerance is not a constant: per truss it is 100 x the relative difference between the yardstick in float64
and in longdouble on the same inputs (floor 1e-12) - what float64 itself loses on that truss, times a factor for a
different elimination order and fused multiply-adds.  Measured over 32 steps that difference is 6e-15 .. 1.1e-13 on the
default batch and 3.4e-11 / 9.1e-11 (undamped / damped) on bar-942, whose value is stored with its inputs' seed in
tests/golden/dynamics_tol.json."""
import json
import os

import numpy as np
import pytest

from oracle import truss_oracle as orc
from tests import dynamics_reference as dref
from tests.helpers import GOLDEN, load_json

pytestmark = pytest.mark.gpu
STEPS = 32
FLOOR = 1e-12
ENVELOPES = (("u_peak", "u_step"), ("N_max", "N_max_step"), ("N_min", "N_min_step"))
KEYS = ("u", "v", "a", "u_peak", "u_step", "N_max", "N_max_step", "N_min", "N_min_step", "hist_u", "hist_N")

_cache = {}


def _datas(names=dref.BATCH):
    return [load_json(n) for n in names]


def _reference(names, damped, dtype=np.float64):
    key = (names, damped, dtype)
    if key not in _cache:
        _cache[key] = dref.reference(_datas(names), 3, STEPS, damped, dtype)
    return _cache[key]


def _tolerances(names, damped):
    """Per truss: max(FLOOR, 100 x the float64 - longdouble difference of the yardstick); bar-942's from the golden file."""
    if names == (dref.BIG,):
        with open(os.path.join(GOLDEN, "dynamics_tol.json")) as fh:
            stored = json.load(fh)
        assert stored["truss"] == dref.BIG and stored["seed"] == dref.SEED and stored["steps"] == STEPS
        return [max(FLOOR, 100.0 * stored["relative_difference"]["damped" if damped else "undamped"])]
    r64, rld = _reference(names, damped), _reference(names, damped, np.longdouble)
    return [max(FLOOR, 100.0 * dref.relative_difference(a, b)) for a, b in zip(r64, rld)]


def _monitors(datas):
    """Per truss three joints and three members (first, last, middle) and one empty slot, caller's ids."""
    mj = np.array([[0, len(d["joint"]) - 1, len(d["joint"]) // 2, -1] for d in datas], dtype=np.int32)
    mm = np.array([[0, len(d["member"]) - 1, -1, len(d["member"]) // 2] for d in datas], dtype=np.int32)
    return mj, mm


def _inputs(datas, L, damped, steps=STEPS, setting=None):
    dt, omega, alpha, beta_r = setting or dref.setting(datas, damped)
    pattern, scale, accel = dref.excitation(datas, L, steps, dt, omega, dref.SEED)
    return dict(dt=dt, alpha=alpha, beta_r=beta_r, pattern=pattern, scale=scale, accel=accel)


def _device_batch(datas, table=False, **kw):
    from python_stable_3d_truss_analysis_amd import batch
    packed = batch.pack_json(datas, members="auto" if table else "general")
    assert packed.is_table == table
    return batch.DeviceBatch(packed, use_small=False, **kw)


def _numpy(out):
    return {k: out[k].cpu().numpy() for k in KEYS}


def _run(datas, inp, table=False, cases=None, state=None, db=None, span=None, **kw):
    """factor_dynamic + transient on ONE DeviceBatch over all of `datas`; `cases`: the case indices to run (default
    all), `span`: (first, last) time points of the inputs.  Returns (numpy results, DeviceBatch, transient's dict)."""
    import torch
    if db is None:
        db = _device_batch(datas, table, **kw)
        db.factor_dynamic(inp["dt"], damp_mass=inp["alpha"], damp_stiff=inp["beta_r"])
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(db.device)
    sel = slice(None) if cases is None else list(cases)
    lo, hi = span or (0, inp["scale"].shape[2] - 1)
    mj, mm = _monitors(datas)
    out = db.transient(up(inp["pattern"][:, sel]), hi - lo, scale=up(inp["scale"][:, sel, lo:hi + 1]),
                       accel=up(inp["accel"][:, sel, lo:hi + 1]), monitor_joints=up(mj), monitor_members=up(mm),
                       state=state)
    torch.cuda.synchronize(db.device)
    assert not db.info.any().item()
    return _numpy(out), db, out


def _compare(got, ref, b, data, tol, what):
    """Truss b of device results `got` against its yardstick `ref` (L cases, STEPS steps); returns (ties, entries) of the
    peak steps."""
    nJ, nM, dim = len(data["joint"]), len(data["member"]), orc.truss_dim(data)
    mj, mm = _monitors([data])
    scale = {k: float(np.abs(ref[k]).max()) for k in ("u", "v", "a", "N")}
    worst = {}

    def close(name, x, y, s):
        worst[name] = float(np.abs(x - y).max()) / s
        assert worst[name] <= tol, (what, name, worst[name], tol)

    for k in ("u", "v", "a"):
        close(k, got[k][b, :, :nJ, :dim], ref[k][:, -1], scale[k])
        assert not got[k][b, :, nJ:].any() and not got[k][b, :, :, dim:].any(), (what, k)
    close("u_peak", got["u_peak"][b, :, :nJ, :dim], ref["u_peak"], scale["u"])
    close("N_max", got["N_max"][b, :, :nM], ref["N_max"], scale["N"])
    close("N_min", got["N_min"][b, :, :nM], ref["N_min"], scale["N"])
    for p, j in enumerate(mj[0]):
        want = ref["u"][:, :, j] if j >= 0 else np.zeros_like(ref["u"][:, :, 0])
        close(f"hist_u[{p}]", got["hist_u"][b, :, :, p, :dim], want, scale["u"])
        assert not got["hist_u"][b, :, :, p, dim:].any()
    for p, m in enumerate(mm[0]):
        close(f"hist_N[{p}]", got["hist_N"][b, :, :, p], ref["N"][:, :, m] if m >= 0 else 0.0, scale["N"])
    ties = entries = 0
    series = {"u_step": (np.abs(ref["u"]), scale["u"], (slice(None, nJ), slice(None, dim))),
              "N_max_step": (ref["N"], scale["N"], (slice(None, nM),)), "N_min_step": (ref["N"], scale["N"], (slice(None, nM),))}
    for key, (hist, s, cut) in series.items():
        mine = got[key][(b, slice(None)) + cut]
        outside = got[key][b].copy()
        outside[(slice(None),) + cut] = 0
        assert not outside.any(), (what, key)                        # padding and the z of a 2D truss: step 0
        theirs = ref[key]
        entries += theirs.size
        for idx in zip(*np.nonzero(mine != theirs)):
            series_at = hist[(idx[0], slice(None)) + tuple(idx[1:])]
            gap = abs(series_at[mine[idx]] - series_at[theirs[idx]]) / s
            assert gap <= tol, (what, key, idx, int(mine[idx]), int(theirs[idx]), gap)
            ties += 1
    print(f"{what}: tol {tol:.2e} worst {max(worst.values()):.2e} ({max(worst, key=worst.get)}) ties {ties}/{entries}")
    return ties, entries


def _check_batch(got, names, damped, what):
    datas, refs, tols = _datas(names), _reference(names, damped), _tolerances(names, damped)
    ties = entries = 0
    for b, data in enumerate(datas):
        t, e = _compare(got, refs[b], b, data, tols[b], f"{what} {names[b]}")
        ties, entries = ties + t, entries + e
    assert ties <= 0.02 * entries, (what, ties, entries)


# ---- 1. the shift -----------------------------------------------------------------------------------------------------
def test_shift_touches_the_diagonal_only():
    """Dense slab, no envelope: assemble, then shift.  Everything off the diagonal keeps its bits (the unwritten entries
    their poison), the diagonal is K_cc + sigma m_c within one unit in the last place, the identity padding stays."""
    import torch
    from python_stable_3d_truss_analysis_amd import _capi, batch
    datas = _datas()
    db = _device_batch(datas, use_envelope=False)
    sigma = batch.newmark_constants(dref.setting(datas, False)[0])["sigma"]
    db.dofmap()
    db.assemble()
    Mf, _ = db._lumped_mass(None, 1.0)
    before = db.S.clone()
    _capi.check(db.lib.trs_dyn_shift(db.B, db.n_free.data_ptr(), db.ld, db.rows, db.S.data_ptr(), Mf.data_ptr(), db.rows,
                                     sigma, db._stream()), "trs_dyn_shift")
    torch.cuda.synchronize(db.device)
    S0, S1, m, n_free = before.cpu().numpy(), db.S.cpu().numpy(), Mf.cpu().numpy(), db.n_free.cpu().numpy()
    rows = np.arange(db.rows)
    off = np.ones(S0.shape[1:], dtype=bool)
    off[rows, rows] = False
    np.testing.assert_array_equal(S0[:, off].view(np.uint64), S1[:, off].view(np.uint64))
    for b, data in enumerate(datas):
        n = int(n_free[b])
        K_ff, m_ref, _ = dref.mref.matrices(data)
        assert n == len(m_ref)
        d0, d1 = S0[b, rows, rows], S1[b, rows, rows]
        want = d0[:n] + sigma * m[b, :n]
        assert np.all(np.abs(d1[:n] - want) <= np.spacing(want)), dref.BATCH[b]
        np.testing.assert_array_equal(d1[n:], d0[n:])
        # (and it is the matrix that is meant: without a joint order the reduced numbering is the oracle's)
        np.testing.assert_allclose(d1[:n], np.diag(K_ff) + sigma * m_ref, rtol=1e-12)


# ---- 2. parity with the yardstick ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("reorder", [False, True], ids=["as-given", "reorder"])
@pytest.mark.parametrize("damped", [False, True], ids=["undamped", "rayleigh"])
def test_parity_on_the_ragged_batch(damped, reorder):
    datas = _datas()
    got, db, _ = _run(datas, _inputs(datas, 3, damped), reorder=reorder)
    assert db.env is not None                                         # the envelope is on, through the factor
    _check_batch(got, dref.BATCH, damped, f"damped={damped} reorder={reorder}")


@pytest.mark.parametrize("damped", [False, True], ids=["undamped", "rayleigh"])
def test_parity_on_the_large_truss(damped):
    """bar-942: members and joints beyond one 256-thread pass, more than one slab row block."""
    datas = _datas((dref.BIG,))
    got, db, _ = _run(datas, _inputs(datas, 3, damped), reorder=damped)
    assert db.rows > 256 and db.nM_max > 256
    _check_batch(got, (dref.BIG,), damped, f"damped={damped}")


def test_parity_through_solve_transient_and_the_buckets():
    from python_stable_3d_truss_analysis_amd import batch
    datas = _datas()
    inp = _inputs(datas, 3, True)
    mj, mm = _monitors(datas)
    res = batch.solve_transient(batch.pack_json(datas), inp["pattern"], inp["dt"], STEPS, scale=inp["scale"],
                                accel=inp["accel"], damp_mass=inp["alpha"], damp_stiff=inp["beta_r"], monitor_joints=mj,
                                monitor_members=mm, reorder=True, max_slab_bytes=1 << 20)
    assert isinstance(res, batch.TransientResult) and not res.info.any()
    got = {key: getattr(res, field) for field, (key, *_rest) in batch.TransientResult.FIELDS.items()}
    _check_batch(got, dref.BATCH, True, "solve_transient")


def test_truss_transient_response_returns_the_yardsticks_histories():
    from python_stable_3d_truss_analysis_amd.truss import Truss
    data = load_json("bar-25_input_0")
    truss = Truss(3).LoadFromJSON(data=data)
    omega = dref.first_frequency(data)
    dt, nJ, nM = 2.0 * np.pi / omega / 20, len(data["joint"]), len(data["member"])
    scale = np.sin(np.sqrt(2.0) * omega * dt * np.arange(STEPS + 1))
    got = truss.TransientResponse(dt, STEPS, scale=scale, dampMass=0.05 * omega, dampStiff=0.02 / omega,
                                  monitorJoints=range(nJ), monitorMembers=range(nM))
    pattern = orc.force_vector(data).reshape(1, nJ, 3)
    args = dict(scale=scale[None], damp_mass=0.05 * omega, damp_stiff=0.02 / omega)
    ref = dref.newmark(data, pattern, dt, STEPS, **args)
    tol = max(FLOOR, 100.0 * dref.relative_difference(ref, dref.newmark(data, pattern, dt, STEPS, dtype=np.longdouble, **args)))
    assert got["historyDisplace"].shape == (1, STEPS + 1, nJ, 3) and got["historyForce"].shape == (1, STEPS + 1, nM)
    assert np.abs(got["historyDisplace"] - ref["u"]).max() <= tol * np.abs(ref["u"]).max()
    assert np.abs(got["historyForce"] - ref["N"]).max() <= tol * np.abs(ref["N"]).max()
    assert np.abs(got["forceMax"] - ref["N_max"]).max() <= tol * np.abs(ref["N"]).max()
    assert np.abs(got["velocity"] - ref["v"][:, -1]).max() <= tol * np.abs(ref["v"]).max()


# ---- 3. bit-for-bit invariants ------------------------------------------------------------------------------------------
def _same(x, y, what, cases=slice(None), other=slice(None), trusses=slice(None), nJ=None, nM=None):
    """x[trusses, cases] against y[:, other], bit for bit (joint and member axes cut to nJ, nM where given)."""
    for key in KEYS:
        a, b = x[key][trusses, cases], y[key][:, other]
        if nJ is not None and key in ("u", "v", "a", "u_peak", "u_step"):
            a, b = a[:, :, :nJ], b[:, :, :nJ]
        if nM is not None and key in ("N_max", "N_max_step", "N_min", "N_min_step"):
            a, b = a[:, :, :nM], b[:, :, :nM]
        np.testing.assert_array_equal(a, b, err_msg=f"{what} {key}")


@pytest.fixture(scope="module")
def base():
    """The damped run of the default batch with 17 cases (one more than a case group): (inputs, results)."""
    datas = _datas()
    inp = _inputs(datas, 17, True)
    return inp, _run(datas, inp)[0]


def test_a_case_depends_neither_on_L_nor_on_the_other_cases_nor_on_its_place(base):
    inp, full = base
    datas = _datas()
    three = _run(datas, inp, cases=[0, 1, 2])[0]
    _same(full, three, "L=17 / L=3", cases=slice(0, 3))
    one = _run(datas, inp, cases=[16])[0]
    _same(full, one, "L=17 / L=1", cases=slice(16, 17))
    moved = _run(datas, inp, cases=[5, 16, 0])[0]
    _same(full, moved, "places", cases=[5, 16, 0])


def test_a_truss_depends_neither_on_B_nor_on_the_other_trusses(base):
    inp, full = base
    datas = _datas()
    for b in (0, 2):
        data = datas[b]
        nJ, nM = len(data["joint"]), len(data["member"])
        alone = {k: inp[k] for k in ("dt", "alpha", "beta_r")}
        alone.update({k: inp[k][b:b + 1, :3, :nJ] if k == "pattern" else inp[k][b:b + 1, :3] for k in ("pattern", "scale", "accel")})
        got = _run([data], alone)[0]
        _same(full, got, f"truss {b}", cases=slice(0, 3), trusses=slice(b, b + 1), nJ=nJ, nM=nM)


def test_member_forms_and_streams_give_the_same_bits(base):
    import torch
    inp, full = base
    datas = _datas()
    _same(full, _run(datas, inp, table=True)[0], "table form")
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = []
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            outs.append(_run(datas, inp)[0])
    for k, got in enumerate(outs):
        _same(full, got, f"stream {k}")


def test_two_batches_on_two_streams_at_once(base):
    """Enqueued side by side, synchronised once: the bits of the single run."""
    import torch
    inp, full = base
    datas = _datas()
    up = lambda x, dev: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    mj, mm = _monitors(datas)
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            db = _device_batch(datas)
            db.factor_dynamic(inp["dt"], damp_mass=inp["alpha"], damp_stiff=inp["beta_r"])
            outs.append(db.transient(up(inp["pattern"], db.device), STEPS, scale=up(inp["scale"], db.device),
                                     accel=up(inp["accel"], db.device), monitor_joints=up(mj, db.device),
                                     monitor_members=up(mm, db.device)))
    torch.cuda.synchronize()
    for k, out in enumerate(outs):
        _same(full, _numpy(out), f"concurrent {k}")


def test_thirty_two_steps_equal_sixteen_and_sixteen_with_the_state_carried(base):
    inp, full = base
    datas = _datas()
    first, db, out = _run(datas, inp, span=(0, 16))
    assert out["state"]["step"] == 16
    second, _, out2 = _run(datas, inp, span=(16, 32), db=db, state=out["state"])
    assert out2["state"]["step"] == 32
    for key in ("u", "v", "a"):
        np.testing.assert_array_equal(second[key], full[key], err_msg=key)
    for key in ("hist_u", "hist_N"):
        np.testing.assert_array_equal(first[key], full[key][:, :, :17], err_msg=key)
        np.testing.assert_array_equal(second[key], full[key][:, :, 16:], err_msg=key)
    for (value, step), better in zip(ENVELOPES, (np.greater, np.greater, np.less)):
        take = better(second[value], first[value])                   # strict: an equal later value keeps the first step
        np.testing.assert_array_equal(np.where(take, second[value], first[value]), full[value], err_msg=value)
        np.testing.assert_array_equal(np.where(take, second[step] + 16, first[step]), full[step], err_msg=step)


def test_damp_stiff_zero_given_or_omitted():
    datas = _datas()
    inp = _inputs(datas, 3, False)
    results = []
    for kw in (dict(), dict(damp_stiff=0.0), dict(damp_mass=0.0, damp_stiff=0.0)):
        db = _device_batch(datas)
        db.factor_dynamic(inp["dt"], **kw)
        results.append(_run(datas, inp, db=db)[0])
    _same(results[0], results[1], "damp_stiff=0.0")
    _same(results[0], results[2], "damp_mass=0.0, damp_stiff=0.0")


# ---- 4. meaning ---------------------------------------------------------------------------------------------------------
def test_zero_excitation_gives_zeros_and_step_zero():
    datas = _datas()
    inp = _inputs(datas, 3, True)
    inp["pattern"] = np.zeros_like(inp["pattern"])
    inp["accel"] = np.zeros_like(inp["accel"])
    got = _run(datas, inp)[0]
    for key in KEYS:
        assert not got[key].any(), key


def test_monitored_histories_close_on_the_envelopes(base):
    """The maximum and minimum of a monitored member's history are N_max and N_min at the first step that attains them;
    the same for a monitored joint and u_peak."""
    _, full = base
    datas = _datas()
    mj, mm = _monitors(datas)
    for b in range(len(datas)):
        for p, m in enumerate(mm[b]):
            if m < 0:
                continue
            series = full["hist_N"][b, :, :, p]
            np.testing.assert_array_equal(series.max(1), full["N_max"][b, :, m])
            np.testing.assert_array_equal(series.argmax(1), full["N_max_step"][b, :, m])
            np.testing.assert_array_equal(series.min(1), full["N_min"][b, :, m])
            np.testing.assert_array_equal(series.argmin(1), full["N_min_step"][b, :, m])
        for p, j in enumerate(mj[b]):
            if j < 0:
                continue
            series = np.abs(full["hist_u"][b, :, :, p])
            np.testing.assert_array_equal(series.max(1), full["u_peak"][b, :, j])
            np.testing.assert_array_equal(series.argmax(1), full["u_step"][b, :, j])


def test_a_huge_step_under_a_constant_load_is_the_static_solution():
    """dt = 1e6 / omega_1 (omega_1 the lowest fundamental frequency of the batch): sigma -> 0 leaves K_ff.  A load that is
    constant from the first step on, on a truss at rest in equilibrium (scale 0 at the start, so a_0 = 0), gives
    `solve_cases`' static u at point 1 within the tolerance of the parity tests.  The same load present at the start too
    (a_0 = f / M) gives TWICE that: the average-acceleration rule at an infinite step maps the undamped step response
    u_st (1 - cos omega t) onto its extremes 0, 2 u_st, 0, ... - asserted as well."""
    import torch
    datas = _datas()
    omega = min(dref.first_frequency(d) for d in datas)
    inp = _inputs(datas, 2, False, steps=1, setting=(1e6 / omega, omega, 0.0, 0.0))
    inp["pattern"][:, 1], inp["scale"][:, 1], inp["accel"][:, 1] = inp["pattern"][:, 0], 1.0, 0.0
    inp["scale"][:, 0, 0] = 0.0                       # case 0: applied after the start; case 1: there from the start
    got, db, _ = _run(datas, inp)
    db.factor()
    static = db.solve_cases(torch.from_numpy(inp["pattern"][:, :1].copy()).to(db.device))["u"].cpu().numpy()[:, 0]
    tols = _tolerances(dref.BATCH, False)
    errs = []
    for b in range(len(datas)):
        size = np.abs(static[b]).max()
        at_rest = np.abs(got["u"][b, 0] - static[b]).max() / size
        sudden = np.abs(got["u"][b, 1] - 2.0 * static[b]).max() / (2.0 * size)
        errs.append(max(at_rest, sudden))
        print(f"{dref.BATCH[b]}: static {at_rest:.2e}, twice static {sudden:.2e} (tol {tols[b]:.2e})")
    for b, err in enumerate(errs):
        assert err <= tols[b], (dref.BATCH[b], err, tols[b])


# ---- 5. state handling --------------------------------------------------------------------------------------------------
def test_static_and_dynamic_factors_exclude_each_other():
    import torch
    datas = _datas()
    inp = _inputs(datas, 2, False, steps=2)
    db = _device_batch(datas)
    loads = torch.from_numpy(inp["pattern"]).to(db.device)
    with pytest.raises(ValueError, match="factor_dynamic"):
        db.transient(loads, 2)
    db.factor()
    with pytest.raises(ValueError, match="factor_dynamic"):
        db.transient(loads, 2)
    generation = db.generation
    db.factor_dynamic(inp["dt"])
    assert db.generation > generation
    for call in (lambda: db.solve_cases(loads), lambda: db.member_loss(loads), lambda: db.modes(2)):
        with pytest.raises(ValueError, match="no factor"):
            call()
    out = db.transient(loads, 2)
    with pytest.raises(ValueError, match="state"):
        db.transient(loads[:, :1].contiguous(), 2, state=out["state"])          # another L
    other = _device_batch(datas)
    other.factor_dynamic(inp["dt"])
    with pytest.raises(ValueError, match="state"):
        other.transient(loads, 2, state=out["state"])                             # another object
    db.factor_dynamic(inp["dt"])
    with pytest.raises(ValueError, match="state"):
        db.transient(loads, 2, state=out["state"])                                # another generation
    with pytest.raises(ValueError, match="compact"):
        _device_batch(datas, options={"compact": True}).factor_dynamic(inp["dt"])
    db.factor()                                                                   # the static analyses are back
    fresh = _device_batch(datas)
    fresh.factor()
    a, b = db.solve_cases(loads), fresh.solve_cases(loads)
    for key in ("u", "f_ext", "N"):
        np.testing.assert_array_equal(a[key].cpu().numpy(), b[key].cpu().numpy(), err_msg=key)
