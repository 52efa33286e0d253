"""The preconditions of `tests/test_gpu_routes.py`, pinned on the CPU: the shapes of `tests/route_shapes.py` hold the
sizes, reaches and windows the GPU tests are about, the restated envelope tables agree with the host library, and the
float64 oracle is a reference a factor of 100 finer than the 1e-8 those tests assert."""
import numpy as np
import pytest

from oracle import truss_oracle as orc
from tests import helpers as H
from tests import route_shapes as R


@pytest.fixture(scope="module")
def batch():
    from python_stable_3d_truss_analysis_amd import batch
    return batch


def test_sweep_holds_every_size(batch):
    cases = R.sweep_cases()
    assert cases is R.sweep_cases()                       # one shared list
    n_free = batch.pack_json(cases).n_free.tolist()
    dims = [orc.truss_dim(d) for d in cases]
    want3 = list(range(2, 202)) + list(range(254, 259)) + list(range(318, 323))
    assert sorted(n for n, dim in zip(n_free, dims) if dim == 3) == want3      # each size once
    assert [n for n, dim in zip(n_free, dims) if dim == 2] == list(range(1, 71))
    assert dims == sorted(dims, reverse=True) and len(cases) == 280    # the towers first, then the strips
    assert max(len(d["member"]) for d in cases) <= 400 and max(len(d["joint"]) for d in cases) <= 111
    # the shapes of the existing 3D sweep, seed for seed
    from tests.test_gpu_parity import _strip_truss_json
    assert cases[:3] == [_strip_truss_json(4, seed=12 + r, dim=3, rollers=r) for r in (0, 1)] + \
        [_strip_truss_json(5, seed=15, dim=3, rollers=0)]
    # every residue of the tile and of the panel, and one below / at / one above each panel edge up to the fifth
    assert {n % 64 for n in want3} == set(range(64))
    assert {64 * k + d for k in range(1, 6) for d in (-1, 0, 1)} <= set(want3)
    assert {1, 15, 16, 17, 63, 64, 65} <= set(range(1, 71))


def test_restated_envelope_agrees_with_the_host_library(batch):
    """`route_shapes.envelope_tables` against `batch.envelope_reach` (csrc/reorder.c) on every shape."""
    for cases in (R.sweep_cases(), R.reach_cases(), R.window_cases()):
        host = batch.envelope_reach(batch.pack_json(cases))
        tables = [R.envelope_tables(d) for d in cases]
        assert [t["reach"] for t in tables] == host.tolist()
        assert [t["n"] for t in tables] == batch.pack_json(cases).n_free.tolist()
    # the sweep's towers and strips: reach 1 at the most - the wave-per-matrix kernel by themselves
    assert max(R.envelope_tables(d)["reach"] for d in R.sweep_cases()) == 1


def test_reach_batch_sits_on_the_routing_threshold(batch):
    cases = R.reach_cases()
    reach = batch.envelope_reach(batch.pack_json(cases)).tolist()
    assert reach == [23, 23, 24, 24, 25, 25, 26, 26]
    assert batch.NARROW_MAX_BELOW == R.NARROW_MAX_BELOW == 24
    assert len({d["joint"][5][0][0] for d in cases[:2]}) == 2       # two different towers per value
    for data, (nj, _seed, a, span) in zip(cases, R.REACH_SHAPES):
        assert len(data["joint"]) == nj and data["member"][-1][0] == [a, a + span]
        assert [s for _, s in data["joint"]].count("ROLLER_Z") == 1
    # a narrow matrix stores at most 24 + 4 tiles per chunk (the compact tile table's cap, the bits of a kmask word);
    # the reach-24 towers fill that
    rows = [int((t["cend"] - np.arange(t["nch"])).max()) for t in map(R.envelope_tables, cases)]
    assert rows[:4] == [24, 27, 25, 28] and max(rows[:4]) == R.NARROW_MAX_BELOW + 4


def test_window_batch_sits_on_the_ring(batch):
    cases = R.window_cases()
    tables = [R.envelope_tables(d) for d in cases]
    assert [t["window"] for t in tables] == [15, 15, 16, 16, 17, 17]
    assert R.CASES_WINDOW == 16
    for t in tables:
        assert t["nch"] >= 24 and t["reach"] <= R.NARROW_MAX_BELOW     # the ring wraps; the narrow route's cend
        # the restatement of tests/test_gpu_parity.py::test_stages_against_oracle, literally
        lastc = [max(q for q in range(t["nch"]) if t["ft"][q] <= c) for c in range(t["nch"])]
        assert t["cend"].tolist() == [min(t["nch"], max(lastc[c] + 1, (c | 3) + 1)) for c in range(t["nch"])]


def test_identity_padding_needs_the_64_of_the_entry_capacity(batch):
    """n % 64 == 1 pads 63 rows.  In the sweep the members' and joints' share of `ecap` = 18 nM + 9 nJ + 64 leaves room
    for that anyway (a support takes entries away, a member across a tile edge has no mirror); the two-joint truss
    alone in its batch is the shape that needs the "+ 64"."""
    lone = R.lone_padding_case()
    packed = batch.pack_json([lone])
    assert packed.n_free.tolist() == [1] and (packed.nJ_max, packed.nM_max) == (2, 1)
    assert R.compact_entries(lone) == 64 and 18 * packed.nM_max + 9 * packed.nJ_max < 64 <= 18 * packed.nM_max + 9 * packed.nJ_max + 64
    assert R.oracle_loss(lone) <= 1e-10
    for data in R.sweep_cases():         # (why the sweep alone would not notice: even a bucket of its own has room)
        assert R.compact_entries(data) <= 18 * len(data["member"]) + 9 * len(data["joint"])


def test_multi_rhs_reference_is_the_oracle():
    """One solve with L right-hand sides = L solves of the oracle; the longdouble variant agrees with both."""
    data = R.sweep_cases()[100]
    loads = R.case_loads([data], 3, seed=1)[0]
    many = R.multi_rhs_reference(data, loads)
    exact = R.multi_rhs_reference(data, loads, dtype=np.longdouble)
    assert many.dtype == np.float64 and exact.dtype == np.longdouble
    for k in range(3):
        ref = orc.solve(R.with_forces(data, loads[k]))
        assert H.max_scaled_err(many[k], ref["u"]) <= 1e-12
        assert H.max_scaled_err(many[k], exact[k].astype(float)) <= 1e-11
    strip = R.sweep_cases()[-1]
    assert R.multi_rhs_reference(strip, R.case_loads([strip], 2, seed=1)[0]).shape == (2, len(strip["joint"]), 2)


def test_the_float64_oracle_loses_no_more_than_1e_10():
    """`orc.solve` against the longdouble Cholesky solve of the same K_ff, u scaled by its largest entry, on EVERY
    truss of the three shape sets: <= 1e-10, a factor of 100 under the 1e-8 the GPU tests assert.
    Measured: 5.0e-12 over the sweep (2.7e-13 over its 2D strips), 3.5e-11 over the reach towers (n = 590 / 632),
    1.2e-11 over the window towers (n = 410 / 440)."""
    for name, cases in (("sweep", R.sweep_cases()), ("reach", R.reach_cases()), ("window", R.window_cases())):
        loss = [R.oracle_loss(d) for d in cases]
        print(f"oracle loss, {name}: worst {max(loss):.2e} (truss {int(np.argmax(loss))})")
        assert max(loss) <= 1e-10, (name, int(np.argmax(loss)), max(loss))
