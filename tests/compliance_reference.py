"""Numpy yardstick of the compliance sizing (test infrastructure, never imported by the package): the stiffest design
at a given weight, the optimality-criteria method of include/trs_compliance.h stated on the dense stiffness matrix of
`tests/sizing_reference.Geometry`, in any floating-point type - `numpy.float64`, or `numpy.longdouble` to measure what
float64 itself loses.  The linear systems are solved by `sizing_reference.analyse`, so both types run the same algorithm.

The method (the header, the kernel and this file state it in the same words).  Inputs: L load cases (joint forces),
weights alpha[L], each >= 0 and not all zero; the measure: "weight" gives w_m = rho_m L0_m, "volume" gives w_m = L0_m;
the target W > 0 (None: the initial design's own measure); eta in (0, 1]; move in (0, 1]; per member a_min > 0 and
a_max >= a_min (equal bounds fix a member); tol >= 0 and max_iters >= 0.  The initial design is the truss's own A (> 0).
Analysis k (k = 0, 1, ...) of design A = A_k:
  - proj_ml = c_m.(u_l,j1 - u_l,j0);
  - C_l = sum_m (E_m A_m / L0_m) proj_ml^2: the compliance as twice the strain energy (f_l.u_l but for rounding);
  - J = sum_l alpha_l C_l, summed in ascending l;
  - s_m = sum_l alpha_l (E_m / L0_m) proj_ml^2, summed in ascending l: -dJ/dA_m;
  - lo_m = clamp((1 - move) A_m, a_min_m, a_max_m) and hi_m = clamp((1 + move) A_m, a_min_m, a_max_m);
  - a member with w_m <= 0 keeps lo_m = hi_m = clamp(A_m, a_min_m, a_max_m);
  - p_m = A_m (s_m / w_m)^eta (0 for a member with w_m <= 0);
  - t_m(x) = min(max(p_m x, lo_m), hi_m);
  - V(x) = sum_m w_m t_m(x), non-decreasing in x; eta enters only through p_m: the search below needs no pow;
  - the new design A', with x0 = min and x1 = max over the members with p_m > 0 of lo_m / p_m and hi_m / p_m:
      sum w lo >= W                A' = lo       multiplier 0
      sum w hi <= W                A' = hi       multiplier 0
      no member has p_m > 0        A' = lo       multiplier 0
      V(x1) <= W                   A' = t(x1)    multiplier x1^(-1/eta)
      otherwise                    A' = t(x0) after the bisection below, multiplier x0^(-1/eta)
    (the first line that applies);
  - the bisection runs 64 times: xm = sqrt(x0 x1); if V(xm) <= W then x0 = xm, else x1 = xm;
  - change = max_m |A'_m - A_m| / A_m over the truss's live members;
  - if change <= tol the truss is converged (status 0) and keeps A_k;
  - otherwise, if k = max_iters, the truss gets status 1 and keeps A_k;
  - otherwise A_{k+1} = A' and the truss's `iterations` becomes k + 1;
  - if the factorisation of A_k reports info != 0 the truss gets status 2, its design goes back to A_{k-1}, and its
    outputs (iterations among them) stay those of analysis k - 1; for k = 0 the outputs are zero (nothing was analysed),
    the areas are the initial ones and `iterations` is 0."""
import numpy as np

from tests import sizing_reference as sref
from tests.sizing_reference import BATCH, BIG, DEPTH, Geometry, cases  # noqa: F401  (the inputs the tests share)

ACTIVE, CONVERGED, ITER_LIMIT, NOT_PD = -1, 0, 1, 2
BISECTIONS = 64
COMPARED = ("areas", "measure", "compliance", "objective", "objective_history", "sensitivity", "multiplier")
CONFIGS = {"single": (1.0, 0.0), "weighted": (0.6, 0.4)}
FULL = {"tol": 1e-4, "max_iters": 60}
#: bays of the girder of more than 1024 members (`generated(WIDE_NX)`: 1128): five members per thread of the step kernel
WIDE_NX = 260
#: a full run whose last `change` lies within this (relative) of `tol` leaves its count to the rounding
DECIDED = 0.01


def measure_weights(geo, measure):
    """w [nM]: rho L0 ("weight") or L0 ("volume")."""
    if measure == "weight":
        return geo.rho * geo.L0
    if measure == "volume":
        return geo.L0.copy()
    raise ValueError(measure)


def analysis(geo, A, loads, alpha, solve=None):
    """One analysis of the design A under `loads` [L, nJ, dim]: None when the reduced stiffness matrix is not positive
    definite, else (compliance [L], J, s [nM], u [L, nJ, dim])."""
    an = sref.analyse(geo, A, loads, 1.0, 1.0, solve=solve)
    if an is None:
        return None
    dtype = geo.dtype
    u = an["u"]
    proj = ((u[:, geo.j1] - u[:, geo.j0]) * geo.c[None]).sum(axis=2)            # [L, nM]
    pp = proj * proj
    C = ((geo.E * A / geo.L0)[None] * pp).sum(axis=1)
    J, s = dtype(0), np.zeros(len(A), dtype=dtype)
    for l in range(len(loads)):                                                  # ascending l
        J = J + dtype(alpha[l]) * C[l]
        s = s + dtype(alpha[l]) * ((geo.E / geo.L0) * pp[l])
    return C, J, s, u


def resize(A, s, w, W, eta, move, lo_bound, hi_bound):
    """(A', multiplier) of one resizing, in A's floating-point type."""
    dtype = A.dtype.type
    one, mv, et = dtype(1), dtype(move), dtype(eta)
    clamp = lambda x: np.minimum(np.maximum(x, lo_bound), hi_bound)
    live = w > 0
    lo = np.where(live, clamp((one - mv) * A), clamp(A))
    hi = np.where(live, clamp((one + mv) * A), clamp(A))
    p = np.where(live, A * np.power(np.where(live, s / np.where(live, w, one), 0), et), 0)
    t = lambda x: np.minimum(np.maximum(p * x, lo), hi)
    V = lambda x: (w * t(x)).sum()
    if (w * lo).sum() >= W:
        return lo, dtype(0)
    if (w * hi).sum() <= W:
        return hi, dtype(0)
    pos = p > 0
    if not pos.any():
        return lo, dtype(0)
    x0, x1 = (lo[pos] / p[pos]).min(), (hi[pos] / p[pos]).max()
    if V(x1) <= W:
        return t(x1), np.power(x1, -one / et)
    for _ in range(BISECTIONS):
        xm = np.sqrt(x0 * x1)
        if V(xm) <= W:
            x0 = xm
        else:
            x1 = xm
    return t(x0), np.power(x0, -one / et)


def minimise(data, loads, alpha, target=None, measure="weight", eta=0.5, move=0.2, area_min=None, area_max=None, tol=1e-4,
             max_iters=60, dtype=np.float64, solve=None, areas=None):
    """The compliance sizing of one truss.  loads [L, nJ, dim]; area_min, area_max scalars or [nM]; `areas`: another
    initial design than the truss's own.  Returns a dict: areas, sensitivity [nM], measure, compliance [L], objective,
    multiplier, iterations, status, info (0, or 1 for a design that could not be factored), objective_history
    [max_iters + 1], target, and per analysis of the loop: changes, measures (lists)."""
    geo = Geometry(data, dtype)
    nM, L = len(geo.A0), len(loads)
    lo = np.broadcast_to(np.asarray(area_min, dtype=dtype), [nM])
    hi = np.broadcast_to(np.asarray(area_max, dtype=dtype), [nM])
    A = geo.A0.copy() if areas is None else np.asarray(areas, dtype=dtype).copy()
    w = measure_weights(geo, measure)
    W = (w * A).sum() if target is None else dtype(target)
    out = {"areas": A.copy(), "sensitivity": np.zeros(nM, dtype=dtype), "measure": dtype(0),
           "compliance": np.zeros(L, dtype=dtype), "objective": dtype(0), "multiplier": dtype(0), "iterations": 0,
           "status": ACTIVE, "info": 0, "objective_history": np.zeros(max_iters + 1, dtype=dtype), "target": W,
           "changes": [], "measures": []}
    k = 0
    while True:
        an = analysis(geo, A, loads, alpha, solve=solve)
        if an is None:                      # the outputs stay those of analysis k - 1
            out["status"], out["info"] = NOT_PD, 1
            out["iterations"] = max(k - 1, 0)
            break
        C, J, s, _ = an
        new, mult = resize(A, s, w, W, eta, move, lo, hi)
        out.update(areas=A.copy(), sensitivity=s, measure=(w * A).sum(), compliance=C, objective=J, multiplier=mult)
        out["objective_history"][k] = J
        out["measures"].append(out["measure"])
        change = (np.abs(new - A) / A).max() if nM else dtype(0)
        out["changes"].append(change)
        if change <= dtype(tol):
            out["status"] = CONVERGED
            break
        if k == max_iters:
            out["status"] = ITER_LIMIT
            break
        A = new
        k += 1
        out["iterations"] = k
    return out


def relative_difference(x, y):
    """The largest max-scaled difference between two `minimise` results over COMPARED."""
    worst = 0.0
    for key in COMPARED:
        a, b = np.asarray(x[key], dtype=np.longdouble), np.asarray(y[key], dtype=np.longdouble)
        scale = float(np.abs(b).max())
        if scale > 0:
            worst = max(worst, float(np.abs(a - b).max()) / scale)
    return worst


def config(data, which):
    """The keyword arguments of `minimise` (and, renamed, of the device) for one of CONFIGS on a fixture: both cases of
    `sizing_reference.cases`, the target the initial weight (None), area_min 1e-3 of the smallest initial area, area_max
    1000 x the largest."""
    geo = Geometry(data, np.float64)
    return {"loads": cases(data), "alpha": CONFIGS[which], "target": None, "measure": "weight",
            "area_min": 1e-3 * float(geo.A0.min()), "area_max": 1000.0 * float(geo.A0.max())}


def generated(nx=70, seed=5):
    """A generated plane truss for the second stride of the step kernel (257 to 512 members): a Pratt-like girder of
    `nx` bays - two chords, posts, alternating diagonals and a second diagonal in every third bay - pinned at one end, on a roller at the other, loaded at
    every lower joint; areas, moduli and densities vary from member to member."""
    rng = np.random.default_rng(seed)
    joints = []
    for i in range(nx + 1):
        joints.append([[float(i), 0.0], "PIN" if i == 0 else "ROLLER_Y" if i == nx else "NO"])
        joints.append([[float(i), 1.0 + 0.1 * np.sin(0.3 * i)], "NO"])
    members = []
    add = lambda a, b: members.append([[a, b], [float(rng.uniform(0.5, 2.0)), float(rng.uniform(1.0e7, 3.0e7)),
                                               float(rng.uniform(0.1, 0.3))]])
    for i in range(nx):
        add(2 * i, 2 * i + 2)
        add(2 * i + 1, 2 * i + 3)
        add(2 * i, 2 * i + 3) if i % 2 == 0 else add(2 * i + 1, 2 * i + 2)
        if i % 3 == 0:                      # (every third bay is cross-braced: the girder is redundant)
            add(2 * i + 1, 2 * i + 2) if i % 2 == 0 else add(2 * i, 2 * i + 3)
    for i in range(nx + 1):
        add(2 * i, 2 * i + 1)
    forces = [[2 * i, [float(100.0 * np.cos(0.2 * i)), -1000.0 - 50.0 * (i % 3)]] for i in range(1, nx)]
    return {"joint": joints, "force": forces, "member": members}


GENERATED, WIDE = "generated", "wide"


def fixture(name):
    """The truss `name`: a fixture of tests/golden/data, or GENERATED / WIDE."""
    from tests.helpers import load_json
    return generated() if name == GENERATED else generated(WIDE_NX) if name == WIDE else load_json(name)


def batch_arguments(names, which):
    """(PackedBatch, keyword arguments of `solve_min_compliance` as host arrays) for the trusses `names`, each with its own
    configuration `which`: the area bounds one row per truss, the target None."""
    from python_stable_3d_truss_analysis_amd import batch
    datas = [fixture(n) for n in names]
    packed = batch.pack_json(datas)
    B, nJ, nM = packed.B, packed.nJ_max, packed.nM_max
    kw = {"loads": np.zeros([B, 2, nJ, 3]), "alpha": CONFIGS[which], "area_min": np.ones([B, nM]),
          "area_max": np.ones([B, nM])}
    for b, data in enumerate(datas):
        one = config(data, which)
        dim = one["loads"].shape[2]
        kw["loads"][b, :, :one["loads"].shape[1], :dim] = one["loads"]
        kw["area_min"][b], kw["area_max"][b] = one["area_min"], one["area_max"]
    return packed, kw


def floor(data, which, run, solve=None):
    """(relative difference of the float64 and the longdouble run, the float64 run, the longdouble run)."""
    kw = config(data, which)
    f64 = minimise(data, **kw, **run, solve=solve)
    f80 = minimise(data, dtype=np.longdouble, **kw, **run)
    return relative_difference(f64, f80), f64, f80


def decided(run, tol):
    """Whether no `change` of a full run lies within DECIDED (relative) of `tol`: its count is not the rounding's."""
    return all(abs(float(c) - tol) > DECIDED * tol for c in run["changes"])


def record(load, big=True):
    """What tests/golden/compliance_tol.json holds (`load`: name -> fixture; `big`: measure bar-942 and the wide girder too, several
    minutes in longdouble): python -c "from tests import compliance_reference as c; from tests.helpers import load_json;
    import json; print(json.dumps(c.record(load_json), indent=1))"."""
    depth = {"tol": 0.0, "max_iters": DEPTH}
    rec = {"what": "largest max-scaled difference between tests/compliance_reference.minimise in float64 and in longdouble "
                   "over areas, measure, compliance, objective, objective_history, sensitivity and multiplier "
                   "(compliance_reference.relative_difference); the device is allowed 100 x these",
           "inputs": "compliance_reference.config: both cases of sizing_reference.cases (case 0 the fixture's own forces f0, "
                     "case 1 [j, a] = 0.3 f0[j, a] - 0.5 f0[j, dim - 1 - a]); single: alpha (1, 0); weighted: alpha (0.6, "
                     "0.4); measure weight, target the initial weight, eta 0.5, move 0.2, area_min 1e-3 x the smallest "
                     "initial area, area_max 1000 x the largest; generated: compliance_reference.generated(); wide: "
                     "compliance_reference.generated(WIDE_NX); bar-942 and wide: the float64 run solves with "
                     "numpy.linalg.solve",
           "trusses": list(BATCH), "big_truss": BIG, "generated_members": len(generated()["member"]),
           "decided": DECIDED, "depth": dict(depth, configs={}), "full": dict(FULL, configs={}),
           "generated": dict(depth, configs={}), "big": dict(depth, configs={}),
           "wide": dict(depth, nx=WIDE_NX, members=len(generated(WIDE_NX)["member"]), configs={})}
    for which in CONFIGS:
        per = [floor(load(name), which, depth)[0] for name in BATCH]
        rec["depth"]["configs"][which] = {"per_truss": per, "relative_difference": max(per)}
        runs = [floor(load(name), which, FULL) for name in BATCH]
        assert all(a["status"] == b["status"] and a["iterations"] == b["iterations"] for _, a, b in runs)
        rec["full"]["configs"][which] = {
            "per_truss": [d for d, _, _ in runs], "relative_difference": max(d for d, _, _ in runs),
            "status": [int(a["status"]) for _, a, _ in runs], "iterations": [int(a["iterations"]) for _, a, _ in runs],
            "last_change": [float(a["changes"][-1]) for _, a, _ in runs],
            "decided": [bool(decided(a, FULL["tol"]) and decided(b, FULL["tol"])) for _, a, b in runs]}
        rec["generated"]["configs"][which] = {"relative_difference": floor(generated(), which, depth)[0]}
        if big:
            rec["big"]["configs"][which] = {"relative_difference": floor(load(BIG), which, depth, solve=np.linalg.solve)[0]}
            rec["wide"]["configs"][which] = {
                "relative_difference": floor(generated(WIDE_NX), which, depth, solve=np.linalg.solve)[0]}
    return rec
