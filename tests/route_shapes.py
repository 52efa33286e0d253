"""Shapes for the route tests (`tests/test_route_shapes.py`, `tests/test_gpu_routes.py`), built on the CPU: every
system size around the tile (16) and panel (64) edges, towers whose envelope reach sits on the routing threshold
`TRS_NARROW_MAX_BELOW` = 24, towers whose substitution window sits on the LDS ring `TRS_CASES_WINDOW` = 16 of
`trs_potrs_cases_kernel`, and a multi-right-hand-side reference from one dense solve of the oracle's K_ff.

The envelope tables (`envelope_tables`) restate `trs_assemble`'s metadata (csrc/trs_common.h "envelope") from the
joint coupling alone, so that the spans below can be tuned - and the preconditions of the GPU tests pinned - without
a GPU.  Test infrastructure: never imported by the product package."""
import functools

import numpy as np

from oracle import truss_oracle as orc
from tests.test_gpu_parity import _strip_truss_json

NARROW_MAX_BELOW = 24     # csrc/trs_common.h TRS_NARROW_MAX_BELOW (batch.NARROW_MAX_BELOW)
CASES_WINDOW = 16         # csrc/cases.hip TRS_CASES_WINDOW


# ---- the sweep: every size -------------------------------------------------------------------------------------------
def _tower(nj, rollers, seed=None):
    return _strip_truss_json(nj, seed=3 * nj + rollers if seed is None else seed, dim=3, rollers=rollers)


def _one_free_dof():
    """n_free = 1 (2D only: a 3D joint frees 3, 2 or 0): the three-joint strip with both ends pinned and the apex on
    a roller that holds x - its y displacement is the one unknown."""
    data = _strip_truss_json(3, seed=3, extra_pin=True)
    data["joint"][1][1] = "ROLLER_X"
    data["force"] = [[1, [0.0, -500.0]]]
    return data


def lone_padding_case():
    """The smallest truss there is - a pin, one member, a joint on a roller that holds x: n_free = 1, so 63 of the 64
    entries of its compact form are identity padding.  As the ONLY shape of a batch (nJ_max = 2, nM_max = 1) the
    entry lists hold 18 nM + 9 nJ + 64 = 100 entries: without the "+ 64" (csrc/trs_common.h `ecap`) they would hold 36."""
    return {"joint": [[[0.0, 0.0], "PIN"], [[30.0, 80.0], "ROLLER_X"]], "force": [[1, [0.0, -700.0]]],
            "member": [[[0, 1], [1.5, 1e7, 0.1]]]}


def compact_entries(data):
    """How many entries the compact form of this truss holds (csrc/assemble.hip phase 1c): every structural entry
    (row c, column q) of K_ff with q >= 16 floor(c / 16) - the upper part by 16-row tiles, diagonal tiles whole -
    plus one per padding row.  Counted on the oracle's K_ff (no exact zeros in these jittered shapes)."""
    K = orc.solve(data)["K_ff"]
    n = len(K)
    c, q = np.nonzero(K)
    return int((q >= c // 16 * 16).sum()) + (-n % 64)


def _strip(n_free):
    """The 2D strip of `n_free` free DOFs: n_free = 2 nj - 3, or 2 nj - 4 with the second pin."""
    if n_free == 1:
        return _one_free_dof()
    if n_free % 2:
        return _strip_truss_json((n_free + 3) // 2, seed=n_free)
    return _strip_truss_json((n_free + 4) // 2, seed=n_free, extra_pin=True)


@functools.lru_cache(maxsize=None)
def sweep_cases():
    """3D towers n_free = 2 ... 201 (the shapes of the existing 3D sweep), 3D towers n_free = 254 ... 258 and
    318 ... 322 (the 4th and 5th panel edge; n_free = 3 (nj - 3) - rollers), then 2D strips n_free = 1 ... 70.
    280 trusses, at most 324 members each.  Cached: the tests share one list and leave it unchanged."""
    cases = [_tower(nj, r) for nj in range(4, 71) for r in (0, 1, 2) if not (nj == 4 and r == 2)]
    for n_free in list(range(254, 259)) + list(range(318, 323)):
        rollers = -n_free % 3
        cases.append(_tower((n_free + rollers) // 3 + 3, rollers))
    cases += [_strip(n_free) for n_free in range(1, 71)]
    return cases


# ---- one long member: reach and window -------------------------------------------------------------------------------
def tower_with_long_member(nj, seed, a, span):
    """The 3D tower of `nj` joints (one roller) plus ONE member between joints `a` and `a + span`: every row chunk
    between the two joints then reaches back to a's chunk (the envelope is made monotone), which sets the reach
    below a's diagonal block and the substitution's window, and leaves most tiles of those rows without an entry."""
    data = _strip_truss_json(nj, seed=seed, dim=3, rollers=1)
    assert 3 <= a and a + span < nj - 1
    data["member"].append([[a, a + span], [1.0, 1e7, 0.1]])
    return data


# (joints, seed, a, span) -> the reach in the comment; tuned with `envelope_tables` and checked against the host
# library's `envelope_reach` in tests/test_route_shapes.py
# library's `envelope_reach` in tests/test_route_shapes.py.  Joint 20's rows lie in the LAST chunk of their panel
# (chunk 3: its row of tiles is reach + 1 wide), joint 26's in the FIRST of theirs (chunk 4: reach + 4 wide - at
# reach 24 the 28 tiles per chunk that the compact tile table and the bits of a kmask word are sized for).
REACH_SHAPES = (
    (200, 1, 20, 126), (214, 2, 26, 141),     # 23
    (200, 1, 20, 131), (214, 2, 26, 146),     # 24: the longest span that stays narrow
    (200, 1, 20, 132), (214, 2, 26, 147),     # 25: one joint further
    (200, 1, 20, 137), (214, 2, 26, 153),     # 26
)
# (joints, seed, a, span) -> the window in the comment
WINDOW_SHAPES = (
    (140, 5, 20, 78), (150, 6, 40, 74),       # 15
    (140, 5, 20, 83), (150, 6, 40, 79),       # 16: the longest span that stays in the ring
    (140, 5, 20, 84), (150, 6, 40, 80),       # 17: one joint further
)


@functools.lru_cache(maxsize=None)
def reach_cases():
    """Towers whose `envelope_reach` is 23, 24, 25 and 26 (two each): one chunk either side of the routing threshold
    and the threshold itself."""
    return [tower_with_long_member(*shape) for shape in REACH_SHAPES]


@functools.lru_cache(maxsize=None)
def window_cases():
    """Towers (n_pad >= 24 chunks, narrow route) whose substitution window is 15, 16 and 17 chunks (two each): the
    LDS ring of 16 chunks with a slot to spare, with every slot live, and overrun (the global-memory path)."""
    return [tower_with_long_member(*shape) for shape in WINDOW_SHAPES]


def envelope_tables(data, narrow=None):
    """`trs_assemble`'s envelope metadata restated from the joint coupling (csrc/assemble.hip phase "envelope
    metadata", csrc/reorder.c `trs_envelope_reach`), in units of 16-row chunks: n, nch, ft, lastc, reach, cend (of
    the route the reach selects, or of the one `narrow` forces) and the substitution's window
    w = max_t (max_{t' <= t} cend[t'] - t) (csrc/cases.hip)."""
    dim = orc.truss_dim(data)
    mask = orc.free_mask(data).reshape(-1, dim)
    index = np.where(mask, np.cumsum(mask.ravel()).reshape(mask.shape) - 1, -1)
    n = int(mask.sum())
    nch = (n + 63) // 64 * 4
    first = [int(row[row >= 0].min()) if (row >= 0).any() else -1 for row in index]
    mincol = [f if f >= 0 else 1 << 30 for f in first]
    for (a, b), _ in data["member"]:
        if first[b] >= 0:
            mincol[a] = min(mincol[a], first[b])
        if first[a] >= 0:
            mincol[b] = min(mincol[b], first[a])
    ft = np.arange(nch)                                   # padding rows: diagonal only
    for j, row in enumerate(index):
        for r in row[row >= 0]:
            ft[r // 16] = min(ft[r // 16], mincol[j] // 16)
    ft = np.minimum.accumulate(ft[::-1])[::-1]
    lastc = np.array([max(q for q in range(nch) if ft[q] <= t) for t in range(nch)], dtype=int)
    reach = max([int(lastc[4 * j + 3]) - (4 * j + 3) for j in range(nch // 4)], default=0)
    if narrow is None:
        narrow = reach <= NARROW_MAX_BELOW
    t = np.arange(nch)
    if narrow:
        cend = np.minimum(nch, np.maximum(lastc + 1, (t | 3) + 1))
    else:
        cend = np.minimum(nch, lastc[t | 3] + 1 + 3) if nch else t
    return {"n": n, "nch": nch, "ft": ft, "lastc": lastc, "reach": reach, "cend": cend, "window": window_of(cend)}


def window_of(cend):
    """The widest live window of `trs_potrs_cases_kernel` over one truss's `cend` table (its own chunks only)."""
    cend = np.asarray(cend, dtype=int)
    if not len(cend):
        return 0
    return int((np.maximum.accumulate(cend) - np.arange(len(cend))).max())


# ---- references ------------------------------------------------------------------------------------------------------
def with_forces(data, loads):
    """`data` with its "force" block replaced by the dense loads [nJ, >= dim] (dim columns used)."""
    dim = orc.truss_dim(data)
    force = [[j, [float(x) for x in loads[j, :dim]]] for j in range(len(data["joint"])) if np.any(loads[j, :dim] != 0)]
    return dict(data, force=force)


def _cholesky_solve(K, F):
    """K X = F by a plain Cholesky factorisation and two substitutions in K's own dtype (numpy's element loops for
    longdouble: no LAPACK, no BLAS)."""
    n = len(K)
    L = np.zeros_like(K)
    for j in range(n):
        d = K[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Y = np.zeros_like(F)
    for j in range(n):
        Y[j] = (F[j] - L[j, :j] @ Y[:j]) / L[j, j]
    X = np.zeros_like(F)
    for j in range(n - 1, -1, -1):
        X[j] = (Y[j] - L[j + 1:, j] @ X[j + 1:]) / L[j, j]
    return X


def multi_rhs_reference(data, loads, dtype=np.float64):
    """u [L, nJ, dim] of the L load cases `loads` [L, >= nJ, >= dim] (dense, zero rows allowed) from ONE dense solve
    of the oracle's K_ff with L right-hand sides, in float64 (`np.linalg.solve`); `dtype=np.longdouble`: the same by
    `_cholesky_solve` in extended precision - the measure of what the float64 oracle itself loses."""
    dim, nJ = orc.truss_dim(data), len(data["joint"])
    loads = np.asarray(loads)
    L = len(loads)
    K, mask = orc.global_K(data), orc.free_mask(data)
    F = loads[:, :nJ, :dim].reshape(L, nJ * dim)[:, mask].T
    K_ff = K[mask][:, mask]
    if np.dtype(dtype) == np.float64:
        X = np.linalg.solve(K_ff, F) if mask.any() else F
    else:
        X = _cholesky_solve(K_ff.astype(dtype), F.astype(dtype))
    u = np.zeros([L, nJ * dim], dtype=dtype)
    u[:, mask] = X.T
    return u.reshape(L, nJ, dim)


def own_loads(data):
    """The truss's own "force" block as dense loads [1, nJ, dim] (what `orc.solve(data)` solves for)."""
    return orc.force_vector(data).reshape(1, len(data["joint"]), orc.truss_dim(data))


def oracle_loss(data):
    """What the float64 oracle loses on this truss: `orc.solve`'s u against the longdouble solve, scaled by u's
    largest entry."""
    exact = multi_rhs_reference(data, own_loads(data), dtype=np.longdouble)[0]
    got = orc.solve(data)["u"]
    scale = np.abs(exact).max()        # (a small strip may carry no load at all: u = 0 on both sides)
    return float(np.abs(got - exact).max() / (scale if scale > 0 else 1.0))


def case_loads(cases, L, seed, nJ_max=None):
    """Seeded loads [B, L, nJ_max, 3] for a batch of `cases`: zero on the padding joints and on z of a 2D truss."""
    nJ_max = max(len(d["joint"]) for d in cases) if nJ_max is None else nJ_max
    rng = np.random.default_rng(seed)
    loads = np.zeros([len(cases), L, nJ_max, 3])
    for b, data in enumerate(cases):
        nJ, dim = len(data["joint"]), orc.truss_dim(data)
        loads[b, :, :nJ, :dim] = rng.uniform(-3e4, 3e4, size=(L, nJ, dim))
    return loads
