"""Every system size and envelope reach through every solver route (`DEFAULT_OPTIONS`: "none of them changes a
result"): the shapes of `tests/route_shapes.py` - n_free = 1 ... 201, the 4th and 5th panel edge, envelope reaches
23 ... 26 around the routing threshold, substitution windows 15 ... 17 around the LDS ring of `trs_potrs_cases_kernel` -
through the wave-per-matrix and the work-group factorisation, the compact form, the separate substitution, the dense
mode and the unstaged recoveries, each truss against the CPU oracle at 1e-8 (the bound for generated trusses, DESIGN
section 4; `tests/test_route_shapes.py` pins that the oracle itself loses <= 1e-10 on these shapes) and with the route
actually taken read back from the device's routing word.  The worst errors are printed (run with -s)."""
import functools

import numpy as np
import pytest

from oracle import truss_oracle as orc
from tests import helpers as H
from tests import route_shapes as R

pytestmark = pytest.mark.gpu
TOL = 1e-8
L = 17        # one full group of 16 cases plus a group with one live lane

ROUTES = {
    "default": {},
    "all-wide": {"options": {"all_wide": True}},
    "all-wide-ordered": {"options": {"all_wide": True}, "reorder": "device"},
    "compact": {"options": {"compact": True}},
    "compact-ordered": {"options": {"compact": True}, "reorder": "device"},
    "separate-substitution": {"options": {"fused_substitution": False}},
    "dense": {"use_envelope": False},
    "unstaged": {"options": {"recover_unstaged": True}},
    "unstaged-scan": {"options": {"recover_unstaged": True, "recover_scan": True}},
}
CASE_ROUTES = ("default", "all-wide", "compact-ordered", "separate-substitution", "dense")
# the threshold batch: the routes, and whether the host's `all_narrow` hint is forced on
THRESHOLD_ROUTES = {
    "default": ("default", False), "compact": ("compact", False),
    "separate-substitution": ("separate-substitution", False), "all-wide": ("all-wide", False),
    "forced-narrow": ("default", True), "compact-forced-narrow": ("compact", True),
}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from python_stable_3d_truss_analysis_amd import batch
    return batch


class _ShapeSet:
    """One batch of shapes with everything the routes are compared against, computed once: the oracle's solve of every
    truss, L seeded load cases, their u from one dense solve per truss, and the oracle's solve of cases 0 and L - 1."""

    def __init__(self, cases, seed):
        from python_stable_3d_truss_analysis_amd import batch
        self.cases = cases
        self.packed = batch.pack_json(cases)
        self.dims = [orc.truss_dim(d) for d in cases]
        self.reach = batch.envelope_reach(self.packed)
        self.refs = [orc.solve(d) for d in cases]
        self.loads = R.case_loads(cases, L, seed, self.packed.nJ_max)
        self.multi = [R.multi_rhs_reference(d, self.loads[b]) for b, d in enumerate(cases)]
        self.case_refs = {k: [orc.solve(R.with_forces(d, self.loads[b, k])) for b, d in enumerate(cases)]
                          for k in (0, L - 1)}


@functools.lru_cache(maxsize=None)
def _shapes(name):
    return {"sweep": lambda: _ShapeSet(R.sweep_cases(), 11), "reach": lambda: _ShapeSet(R.reach_cases(), 12),
            "window": lambda: _ShapeSet(R.window_cases(), 13)}[name]()


def _device_batch(gpu, shapes, route, **kw):
    args = dict(ROUTES[route], **kw)
    args["options"] = dict(args.get("options", {}))
    return gpu.DeviceBatch(shapes.packed, use_small=False, **args)


def _check(shapes, refs, u, f_ext, N, tag):
    """u, f_ext [B, nJ_max, 3] and N [B, nM_max] against `refs` (the oracle's dicts; None entries are not compared);
    the padding joints and members and the z column of the 2D trusses must be exactly zero.  Returns the worst scaled
    error of each part."""
    worst = np.zeros(3)
    for b, (data, dim) in enumerate(zip(shapes.cases, shapes.dims)):
        nJ, nM = len(data["joint"]), len(data["member"])
        got = (u[b, :nJ, :dim], f_ext[b, :nJ, :dim] if f_ext is not None else None, N[b, :nM] if N is not None else None)
        for i, (g, key) in enumerate(zip(got, ("u", "f_ext", "N"))):
            if g is None or refs[b].get(key) is None:
                continue
            err = H.max_scaled_err(g, refs[b][key])
            assert err <= TOL, (tag, b, key, int(shapes.packed.n_free[b]), err)     # (NaN fails here too)
            worst[i] = max(worst[i], err)
        for x in (u, f_ext):
            if x is not None:
                assert not x[b, nJ:].any() and not x[b, :, dim:].any(), (tag, b, "padding")
        if N is not None:
            assert not N[b, nM:].any(), (tag, b, "padding")
    return worst


def _words(db):
    """The routing word of every truss (csrc/trs_common.h `slack`), as `test_launch_hints_and_forced_narrow_routing`
    reads it."""
    db.torch.cuda.synchronize()
    return db.env.cpu().numpy()[:, db.rows // 16 + db.rows // 64].astype(np.int64)


def _check_words(db, shapes, route, forced_narrow=False, tag=""):
    """The route actually taken: low byte 1 = wave-per-matrix kernel (by reach, or forced), 3 = work-group kernel;
    0x100 = compact form (narrow by its OWN reach only); 0x400 = substituted by the factorising wave."""
    if db.env is None:
        assert ROUTES[route].get("use_envelope") is False
        return
    options = ROUTES[route].get("options", {})
    words = _words(db)
    own = shapes.reach <= R.NARROW_MAX_BELOW
    narrow = np.zeros_like(own) if options.get("all_wide") else (own | forced_narrow)
    np.testing.assert_array_equal(words & 0xff, np.where(narrow, 1, 3), err_msg=f"{tag}: kernel")
    np.testing.assert_array_equal((words & 0x100) != 0, narrow & own & bool(options.get("compact")),
                                  err_msg=f"{tag}: compact form")
    fused = narrow & bool(options.get("fused_substitution", True)) & (db.rows <= 1024)
    np.testing.assert_array_equal((words & 0x400) != 0, fused, err_msg=f"{tag}: fused substitution")
    assert not (words & ~0x7ff).any()


def _solve_and_check(db, shapes, tag):
    db.solve()
    res = db.result()
    assert not res.info.any(), (tag, np.flatnonzero(res.info))
    return _check(shapes, shapes.refs, res.displace, res.external, res.internal, tag)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _cases_and_check(db, shapes, tag):
    """`factor()` + `solve_cases` with the L seeded cases: u of all of them against the one dense solve, f_ext and N
    of the first and the last against the oracle, and the last case run alone (L = 1: another slot of its group, no
    neighbours) bit for bit."""
    torch = db.torch
    loads = torch.from_numpy(shapes.loads).to(db.device)
    db.factor()
    out = {k: v.cpu().numpy() for k, v in db.solve_cases(loads).items()}
    assert not db.info.cpu().numpy().any(), tag
    worst = np.zeros(3)
    for k in range(L):
        full = k in shapes.case_refs
        refs = [{"u": m[k], "f_ext": shapes.case_refs[k][b]["f_ext"] if full else None,
                 "N": shapes.case_refs[k][b]["N"] if full else None} for b, m in enumerate(shapes.multi)]
        if full:    # (the two references agree far inside the bound: the same K_ff, one or L right-hand sides)
            for b, m in enumerate(shapes.multi):
                assert H.max_scaled_err(m[k], shapes.case_refs[k][b]["u"]) <= 1e-10
        worst = np.maximum(worst, _check(shapes, refs, out["u"][:, k], out["f_ext"][:, k] if full else None,
                                         out["N"][:, k] if full else None, (tag, "case", k)))
        for key in ("f_ext", "N"):   # padding of the cases that have no oracle run of their own
            for b, data in enumerate(shapes.cases):
                n = len(data["joint"] if key == "f_ext" else data["member"])
                assert not out[key][b, k, n:].any(), (tag, key, b, k)
    alone = {k: v.cpu().numpy() for k, v in db.solve_cases(loads[:, L - 1:].contiguous()).items()}
    for key in ("u", "f_ext", "N"):
        np.testing.assert_array_equal(_bits(alone[key]), _bits(out[key][:, L - 1:]), err_msg=f"{tag}: {key} of case {L - 1} alone")
    return worst


def _report(part, route, worst):
    print(f"\nroutes {part} [{route}]: worst scaled error u {worst[0]:.1e}  f_ext {worst[1]:.1e}  N {worst[2]:.1e}")


# ---- a. every size through every route -------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
def test_every_size_through_the_route(gpu, route):
    """The 280 trusses of `sweep_cases()` as ONE padded batch through `solve()`, each against the oracle, the
    routing word of each as the route dictates; for the work-group kernel and the compact form once more through
    `solve_batch`, whose size buckets give each size other `rows` / `ld` (and the fused small-system kernel up to 128)."""
    shapes = _shapes("sweep")
    db = _device_batch(gpu, shapes, route)
    assert not db.small and db.rows == 384
    worst = _solve_and_check(db, shapes, route)
    _check_words(db, shapes, route, tag=route)
    if route in ("all-wide", "compact"):
        for reorder in (False, True):
            res = gpu.solve_batch(shapes.packed, reorder=reorder, options=ROUTES[route]["options"])
            assert not res.info.any()
            tag = (route, "solve_batch", reorder)
            worst = np.maximum(worst, _check(shapes, shapes.refs, res.displace, res.external, res.internal, tag))
    _report("a. sizes", route, worst)


def test_identity_padding_fills_the_compact_entry_lists(gpu):
    """`ecap` = 18 nM + 9 nJ + 64 (csrc/trs_common.h): the "+ 64" is for the identity padding, 63 rows at n % 64 == 1.
    The sweep has those sizes but room to spare in the members' share; the two-joint truss (n_free = 1) alone in its
    batch holds 64 entries where the lists would hold 36 without it (`tests/test_route_shapes.py`).  Three copies, so
    that an overrun would land in a neighbour's lists: compact form = slab form bit for bit = the oracle."""
    data = R.lone_padding_case()
    ref = orc.solve(data)
    packed = gpu.pack_json([data] * 3)
    got = {}
    for compact in (False, True):
        db = gpu.DeviceBatch(packed, use_small=False, options={"compact": compact})
        assert not db.small
        db.solve()
        res = got[compact] = db.result()
        assert not res.info.any()
        words = _words(db)
        assert (words & 0xff == 1).all() and ((words & 0x100 != 0) == compact).all()
        for b in range(3):
            assert H.max_scaled_err(res.displace[b, :, :2], ref["u"]) <= TOL
            assert H.max_scaled_err(res.external[b, :, :2], ref["f_ext"]) <= TOL
            assert H.max_scaled_err(res.internal[b], ref["N"]) <= TOL
            assert not res.displace[b, :, 2].any() and not res.external[b, :, 2].any()
    for key in ("displace", "external", "internal"):
        np.testing.assert_array_equal(getattr(got[True], key), getattr(got[False], key))


# ---- b. every size through the multi-case substitution ---------------------------------------------------------------
@pytest.mark.parametrize("route", CASE_ROUTES)
def test_every_size_through_the_multi_case_substitution(gpu, route):
    shapes = _shapes("sweep")
    db = _device_batch(gpu, shapes, route)
    worst = _cases_and_check(db, shapes, route)
    _check_words(db, shapes, route, tag=route)     # (factor() routes and substitutes as solve() does)
    _report("b. load cases", route, worst)


# ---- c. the routing threshold ----------------------------------------------------------------------------------------
def _kmask_words(db, b):
    """(cend, kmask) of truss b over its own chunks, from the device's envelope metadata."""
    env = db.env.cpu().numpy()[b]
    nchm, npan = db.rows // 16, db.rows // 64
    nch = (int(db.packed.n_free[b]) + 63) // 64 * 4
    return env[nchm + npan + 8: nchm + npan + 8 + nch].astype(int), \
        env[2 * nchm + npan + 8: 2 * nchm + npan + 8 + nch].astype(np.int64) & 0xffffffff


@pytest.mark.parametrize("variant", list(THRESHOLD_ROUTES))
def test_routing_threshold_in_one_batch(gpu, variant):
    """Reaches 23, 24 | 25, 26 in ONE batch, given numbering: the host's `envelope_reach` against the device's routing
    (<= 24: wave-per-matrix kernel, compact form if asked; >= 25: work-group kernel, slab), both kernels in one launch
    sequence, then solve() and the load cases against the oracle.  Forced narrow (`all_narrow`), every matrix takes
    the wave-per-matrix kernel and the reach-25 / 26 towers keep the slab.  The narrow towers run with a real
    `kmask` (the long member leaves most tiles of its rows without an entry: "worth skipping" in assemble.hip): every
    tile that holds an entry of the oracle's K_ff has its bit, the highest of them bit 27 of the word (reach 24 below
    a joint in the first chunk of its panel)."""
    route, forced = THRESHOLD_ROUTES[variant]
    shapes = _shapes("reach")
    assert shapes.reach.tolist() == [23, 23, 24, 24, 25, 25, 26, 26]
    db = _device_batch(gpu, shapes, route, reorder=False)
    assert not db.all_narrow            # the host saw the wide envelopes: both kernels are launched
    db.all_narrow = forced
    worst = _solve_and_check(db, shapes, variant)
    _check_words(db, shapes, route, forced_narrow=forced, tag=variant)
    if route != "all-wide":
        masked, top = 0, 0
        for b in np.flatnonzero(shapes.reach <= R.NARROW_MAX_BELOW):
            cend, kmask = _kmask_words(db, b)
            np.testing.assert_array_equal(cend, R.envelope_tables(shapes.cases[b])["cend"])
            if (kmask == 0xffffffff).all():
                continue
            masked += 1
            n, nch = int(shapes.packed.n_free[b]), len(cend)
            K = np.eye(16 * nch)
            K[:n, :n] = shapes.refs[b]["K_ff"]
            tiles = np.abs(K).reshape(nch, 16, nch, 16).max(axis=(1, 3)) > 0
            for t in range(nch):
                want = sum(1 << (q - t) for q in range(t, nch) if tiles[t, q])
                assert want < 1 << (cend[t] - t) and int(kmask[t]) & want == want, (variant, b, t)
                top = max(top, want.bit_length() - 1)
        assert masked >= 1 and top == R.NARROW_MAX_BELOW + 3
    _report("c. threshold, solve", variant, worst)
    worst = _cases_and_check(db, shapes, variant)
    _check_words(db, shapes, route, forced_narrow=forced, tag=variant)
    _report("c. threshold, load cases", variant, worst)


# ---- d. the substitution's ring --------------------------------------------------------------------------------------
def test_substitution_window_around_the_lds_ring(gpu):
    """Windows of 15, 16 and 17 chunks in towers of 28 chunks, one batch, given numbering, default route: the ring of
    `TRS_CASES_WINDOW` = 16 chunks wraps with a slot to spare, with every slot live (`in_lds = w <= wc`), and is
    overrun (the global-memory path) - the window read from the device's own `cend`."""
    shapes = _shapes("window")
    db = _device_batch(gpu, shapes, "default", reorder=False)
    assert db.rows // 16 >= R.CASES_WINDOW        # (the launch sizes the ring min(n_pad_max / 16, 16) chunks)
    worst = _cases_and_check(db, shapes, "window")
    windows = []
    for b in range(db.B):
        cend, _ = _kmask_words(db, b)
        assert len(cend) >= 24
        windows.append(R.window_of(cend))
    assert windows == [15, 15, 16, 16, 17, 17]
    _check_words(db, shapes, "default", tag="window")
    _report("d. ring", "default", worst)
