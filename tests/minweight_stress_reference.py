"""Numpy yardstick of the minimum-weight sizing under stress AND displacement limits (test infrastructure, never imported
by the package): `tests/minweight_reference.py` with the stress floor of include/trs_minweight_stress.h (trs_mw_step_stress) on
top.  `Geometry`, `analysis`, `resize`, `measure_weights` and the constants are the ones of `minweight_reference`, unchanged;
this file adds only the floor, the three outputs and the status rule.  Any floating-point type, as there.

The method (the header, the kernel and this file state it in the same words).  Everything in `minweight_reference` stays
as it is.  Further inputs: allow_tension > 0 and allow_compression > 0 (+inf switches a side off) and euler_kappa >= 0 as
in `sizing_reference` (it models I = kappa A^2; 0 means no member buckling term).  Analysis k of design A:
  - for every REAL case l < L, N_ml = ((E_m / L0_m) A_m) proj_m(u_l);
  - the required area in case l is N / allow_tension for N > 0; for P = -N > 0 it is
    max(P / allow_compression, sqrt(P L0^2 / (pi^2 E kappa))), the second term only when kappa > 0;
  - req_m is the maximum over the cases in ascending l; on a tie the lowest l governs; governing_m is that l, or -1 where
    req_m = 0;
  - the floor: lo_m = min(max(lo_m, req_m), hi_m), lo_m and hi_m the move-and-bound interval of `resize`: a member that
    needs more than (1 + move) A_m grows at the move limit, and a member with w_m <= 0 keeps lo_m = hi_m;
  - the subproblem, the cut, the dual solve, the bisection, A'(mu) and `change` are unchanged: only lo differs;
  - utilisation_m = req_m / A_m, and stress_worst = its maximum over the members; `worst` and worst_history stay the
    displacement figure; stress_history[k] = stress_worst;
  - if change <= tol: status 0 if max(worst, stress_worst) <= 1 + limit_tol, else status 3; statuses 1 and 2 and the
    roll-back are those of `minweight_reference`.

How the floor reaches `resize` without a change to it: `resize` forms lo = clamp((1 - move) A) and hi = clamp((1 + move) A)
(clamp(A) twice where w <= 0) with clamp(x) = min(max(x, lo_bound), hi_bound).  Handing it lo_bound' = min(max(lo, req), hi)
- the floored lower end itself, which lies in [lo, hi] - gives lo' = lo_bound' and hi' = hi in every case of the two
clamps (each is a selection, no arithmetic: (1 - move) A <= lo <= lo_bound' <= hi <= hi_bound wherever (1 - move) A <=
hi_bound, and lo = hi = hi_bound beyond; (1 + move) A, lo_bound and hi_bound select hi as before because lo_bound' <= hi).
With req = 0 (both allowables inf, kappa 0) lo_bound' = lo and the run is `minweight_reference.minimise` bit for bit."""
import numpy as np

from tests import minweight_reference as mref
from tests import sizing_reference as sref
from tests.minweight_reference import (ACTIVE, BATCH, BIG, CONVERGED, DECIDED, DEPTH, FLOOR_LEAST,  # noqa: F401
                                       GENERATED, INFEASIBLE, ITER_LIMIT, MAX_LIMITS, MOVE, NOT_PD, Geometry, analysis,
                                       fixture, generated, measure_weights, resize)

COMPARED = mref.COMPARED + ("stress_history", "utilisation")
#: name -> (the configuration of `minweight_reference.CONFIGS` that gives loads, limits and bounds, euler_kappa)
CONFIGS = {"single": ("single", 0.0), "pair": ("pair", 0.0), "euler": ("pair", 1.0 / (4.0 * np.pi))}
#: limit_tol 0.05 for the reason `minweight_reference.FULL` gives - a converged truss has worst = 1 or stress_worst = 1,
#: clear of the band around 1.05; max_iters 200: bar-25 and bar-47 take 122 and 145 resizings under "single"
FULL = {"tol": 1e-4, "max_iters": 200, "limit_tol": 0.05}
#: the classical 10-bar truss: bays of 360, E = 1e7, rho = 0.1, 100 000 down at the two lower free joints, +-25 000
#: stress, 2.0 on the downward displacement of the four free joints, area_min 0.1; the literature's optimum weight
TEN_BAR = {"bay": 360.0, "E": 1e7, "rho": 0.1, "load": 1e5, "stress": 25000.0, "deflection": 2.0, "area_min": 0.1,
           "area_max": 100.0, "area": 10.0, "move": 0.1, "optimum": 5060.85}


def requirement(geo, A, u, allow_tension, allow_compression, euler_kappa=0.0):
    """required [L, nM]: the area every member needs in every real case of the design A with displacements u
    [L, nJ, dim] - `sizing_reference.analyse`'s expressions, the force formed as ((E / L0) A) proj."""
    dtype = geo.dtype
    proj = ((u[:, geo.j1] - u[:, geo.j0]) * geo.c[None]).sum(axis=2)
    N = ((geo.E / geo.L0) * A)[None] * proj
    at, ac, kappa = dtype(allow_tension), dtype(allow_compression), dtype(euler_kappa)
    comp = np.maximum(-N, 0)
    required = np.where(N > 0, N / at, comp / ac)
    if euler_kappa > 0:
        pi = dtype(np.pi) if dtype is np.float64 else np.arctan(dtype(1)) * 4
        euler = np.sqrt(comp * ((geo.L0 * geo.L0) / ((pi * pi * geo.E) * kappa))[None])
        required = np.where(N < 0, np.maximum(required, euler), required)
    return required


def minimise(data, loads, limits, allow_tension, allow_compression, euler_kappa=0.0, measure="weight", move=MOVE,
             area_min=None, area_max=None, tol=1e-4, max_iters=100, sweeps=2, limit_tol=1e-2, dtype=np.float64, solve=None,
             areas=None):
    """`minweight_reference.minimise` with the stress floor.  Returns its dict, and utilisation [nM], governing (int32
    [nM]), stress_history [max_iters + 1], `required` [L, nM] of the analysis the outputs describe, and per analysis of
    the loop: stress_worsts (a list)."""
    geo = Geometry(data, dtype)
    nM, J = len(geo.A0), len(limits)
    assert 1 <= J <= MAX_LIMITS
    lo = np.broadcast_to(np.asarray(area_min, dtype=dtype), [nM])
    hi = np.broadcast_to(np.asarray(area_max, dtype=dtype), [nM])
    A = geo.A0.copy() if areas is None else np.asarray(areas, dtype=dtype).copy()
    w = measure_weights(geo, measure)
    on = mref.enabled(limits)
    unit = [(case, joint, np.asarray(d, dtype=dtype) / np.sqrt((np.asarray(d, dtype=dtype) ** 2).sum()), value)
            for case, joint, d, value in limits]
    ubar = np.array([dtype(value) if on[j] else dtype(np.inf) for j, (_, _, _, value) in enumerate(limits)], dtype=dtype)
    mu = np.zeros(J, dtype=dtype)
    out = {"areas": A.copy(), "sensitivity": np.zeros([J, nM], dtype=dtype), "measure": dtype(0),
           "displacement": np.zeros(J, dtype=dtype), "ratio": np.zeros(J, dtype=dtype), "multipliers": mu.copy(),
           "iterations": 0, "status": ACTIVE, "info": 0, "measure_history": np.zeros(max_iters + 1, dtype=dtype),
           "worst_history": np.zeros(max_iters + 1, dtype=dtype), "changes": [], "worsts": [],
           "utilisation": np.zeros(nM, dtype=dtype), "governing": np.full(nM, -1, dtype=np.int32),
           "stress_history": np.zeros(max_iters + 1, dtype=dtype), "required": np.zeros([len(loads), nM], dtype=dtype),
           "stress_worsts": []}
    one, mv = dtype(1), dtype(move)
    clamp = lambda x: np.minimum(np.maximum(x, lo), hi)
    live = w > 0
    k = 0
    while True:
        an = analysis(geo, A, loads, unit, solve=solve)
        if an is None:                      # the outputs stay those of analysis k - 1
            out["status"], out["info"] = NOT_PD, 1
            out["iterations"] = max(k - 1, 0)
            break
        c, g, u = an
        required = requirement(geo, A, u, allow_tension, allow_compression, euler_kappa)
        req = required.max(axis=0)
        case = required.argmax(axis=0)          # (the first of equal maxima: the lowest l)
        governing = np.where(req > 0, case, -1).astype(np.int32)
        lo_k = np.where(live, clamp((one - mv) * A), clamp(A))      # the move-and-bound interval of `resize`
        hi_k = np.where(live, clamp((one + mv) * A), clamp(A))
        floor = np.minimum(np.maximum(lo_k, req), hi_k)
        new, mu = resize(A, c, w, ubar, on, mu, move, floor, hi, sweeps)
        ratio = np.where(on, g / np.where(on, ubar, dtype(1)), dtype(0))
        worst = ratio[on].max() if on.any() else dtype(0)
        util = req / A
        stress_worst = util.max() if nM else dtype(0)
        out.update(areas=A.copy(), sensitivity=c, measure=(w * A).sum(), displacement=g, ratio=ratio, multipliers=mu.copy(),
                   utilisation=util, governing=governing, required=required)
        out["measure_history"][k], out["worst_history"][k] = out["measure"], worst
        out["stress_history"][k] = stress_worst
        change = (np.abs(new - A) / A).max() if nM else dtype(0)
        out["changes"].append(change)
        out["worsts"].append(worst)
        out["stress_worsts"].append(stress_worst)
        if change <= dtype(tol):
            out["status"] = CONVERGED if max(worst, stress_worst) <= dtype(1) + dtype(limit_tol) else INFEASIBLE
            break
        if k == max_iters:
            out["status"] = ITER_LIMIT
            break
        A = new
        k += 1
        out["iterations"] = k
    return out


def differences(x, y):
    """key -> the max-scaled difference between two `minimise` results, for every key of COMPARED."""
    out = {}
    for key in COMPARED:
        a, b = np.asarray(x[key], dtype=np.longdouble), np.asarray(y[key], dtype=np.longdouble)
        scale = float(np.abs(b).max())
        out[key] = float(np.abs(a - b).max()) / scale if scale > 0 else 0.0
    return out


def relative_difference(x, y):
    return max(differences(x, y).values())


def config(data, which, solve=None):
    """The keyword arguments of `minimise` for one of CONFIGS on a fixture: loads, limits, move and area bounds of
    `minweight_reference.config`, the "stress" allowables of `sizing_reference.config` and the configuration's kappa."""
    base, kappa = CONFIGS[which]
    kw = mref.config(data, base, solve=solve)
    allow = sref.config(data, "stress", solve=solve)
    return dict(kw, allow_tension=allow["allow_tension"], allow_compression=allow["allow_compression"], euler_kappa=kappa)


def batch_arguments(names, which):
    """(PackedBatch, keyword arguments of `solve_min_weight` as host arrays) for the trusses `names`, each with its own
    configuration `which`: `minweight_reference.batch_arguments` and the allowables one per truss."""
    base, kappa = CONFIGS[which]
    packed, kw = mref.batch_arguments(names, base)
    at, ac = np.zeros(len(names)), np.zeros(len(names))
    for b, name in enumerate(names):
        data = fixture(name)
        one = sref.config(data, "stress", solve=np.linalg.solve if len(data["member"]) > 500 else None)
        at[b], ac[b] = one["allow_tension"], one["allow_compression"]
    return packed, dict(kw, allow_tension=at, allow_compression=ac, euler_kappa=kappa)


def floor(data, which, run, solve=None):
    """(key -> max-scaled difference of the float64 and the longdouble run, the float64 run, the longdouble run)."""
    kw = config(data, which, solve=solve)
    f64 = minimise(data, **kw, **run, solve=solve)
    f80 = minimise(data, dtype=np.longdouble, **kw, **run)
    return differences(f64, f80), f64, f80


def decided(run, tol, limit_tol):
    """`minweight_reference.decided` (no `change` within DECIDED of `tol`, no `worst` within DECIDED of 1 + limit_tol), and
    the stress_worst of the LAST analysis not within DECIDED (relative) of 1 + limit_tol either.  (The status rule reads
    stress_worst only where change <= tol, that is at the last analysis of a converged run; the changes that could end
    the run elsewhere are already kept clear of `tol`.)"""
    edge = 1.0 + limit_tol
    return mref.decided(run, tol, limit_tol) and abs(float(run["stress_worsts"][-1]) - edge) > DECIDED * edge


def ten_bar():
    """(data, keyword arguments of `minimise`) of the classical 10-bar truss (TEN_BAR): joints 0, 1 held at x = 0 (top,
    bottom), 2, 3 at x = 360, 4, 5 at x = 720; the loads at the lower joints 3 and 5; one limit of 2.0 on the downward
    displacement of each of the four free joints."""
    t = TEN_BAR
    b = t["bay"]
    joints = [[0.0, b], [0.0, 0.0], [b, b], [b, 0.0], [2 * b, b], [2 * b, 0.0]]
    members = [(0, 2), (2, 4), (1, 3), (3, 5), (2, 3), (4, 5), (0, 3), (1, 2), (2, 5), (3, 4)]
    data = {"joint": [[p, "PIN" if j < 2 else "NO"] for j, p in enumerate(joints)],
            "force": [[3, [0.0, -t["load"]]], [5, [0.0, -t["load"]]]],
            "member": [[list(m), [t["area"], t["E"], t["rho"]]] for m in members]}
    geo = Geometry(data, np.float64)
    loads = np.zeros([1, geo.nJ, geo.dim])
    loads[0, 3, 1] = loads[0, 5, 1] = -t["load"]
    down = np.zeros(geo.dim)
    down[1] = -1.0
    limits = [(0, j, down.copy(), t["deflection"]) for j in (2, 3, 4, 5)]
    return data, {"loads": loads, "limits": limits, "allow_tension": t["stress"], "allow_compression": t["stress"],
                  "euler_kappa": 0.0, "measure": "weight", "move": t["move"], "area_min": t["area_min"],
                  "area_max": t["area_max"]}


def record(load, big=True):
    """What tests/golden/minweight_stress_tol.json holds (`load`: name -> fixture; `big`: measure bar-942 too, minutes in
    longdouble): python -c "from tests import minweight_stress_reference as c; from tests.helpers import load_json; import
    json; print(json.dumps(c.record(load_json), indent=1))"."""
    depth = {"tol": 0.0, "max_iters": DEPTH}
    rec = {"what": "largest max-scaled difference between tests/minweight_stress_reference.minimise in float64 and in "
                   "longdouble over areas, measure, measure_history, worst_history, displacement, ratio, multipliers, "
                   "sensitivity, stress_history and utilisation (minweight_stress_reference.differences), kept per truss "
                   "and result; relative_difference is the largest of a part and configuration; the device is allowed "
                   "100 x the largest of a truss's own figures (floor_least at least)",
           "inputs": "minweight_stress_reference.config: loads, limits, move 0.3 and area bounds of "
                     "minweight_reference.config (single, pair), the stress allowables of sizing_reference.config, euler: "
                     "pair with euler_kappa 1 / (4 pi); generated: compliance_reference.generated(); bar-942 and its "
                     "float64 run solve with numpy.linalg.solve; ten_bar: minweight_stress_reference.ten_bar()",
           "trusses": list(BATCH), "big_truss": BIG, "generated_members": len(generated()["member"]),
           "decided": DECIDED, "floor_least": FLOOR_LEAST, "kappa": {k: v[1] for k, v in CONFIGS.items()},
           "depth": dict(depth, configs={}), "full": dict(FULL, configs={}), "generated": dict(depth, configs={}),
           "big": dict(depth, configs={}), "ten_bar": {}}
    args = (FULL["tol"], FULL["limit_tol"])
    one = lambda d: {"per_truss": [d], "relative_difference": max(d.values())}
    for which in CONFIGS:
        per = [floor(load(name), which, depth)[0] for name in BATCH]
        rec["depth"]["configs"][which] = {"per_truss": per, "relative_difference": max(max(d.values()) for d in per)}
        runs = [floor(load(name), which, FULL) for name in BATCH]
        rec["full"]["configs"][which] = {
            "per_truss": [d for d, _, _ in runs], "relative_difference": max(max(d.values()) for d, _, _ in runs),
            "status": [int(a["status"]) for _, a, _ in runs], "iterations": [int(a["iterations"]) for _, a, _ in runs],
            "last_change": [float(a["changes"][-1]) for _, a, _ in runs],
            "last_worst": [float(a["worsts"][-1]) for _, a, _ in runs],
            "last_stress_worst": [float(a["stress_worsts"][-1]) for _, a, _ in runs],
            "measure": [float(a["measure"]) for _, a, _ in runs],
            "decided": [bool(decided(a, *args) and decided(b, *args) and a["status"] == b["status"]
                             and a["iterations"] == b["iterations"]) for _, a, b in runs]}
        rec["generated"]["configs"][which] = one(floor(generated(), which, depth)[0])
        if big:
            rec["big"]["configs"][which] = one(floor(load(BIG), which, depth, solve=np.linalg.solve)[0])
    data, kw = ten_bar()
    f64 = minimise(data, **kw, **FULL)
    f80 = minimise(data, dtype=np.longdouble, **kw, **FULL)
    rec["ten_bar"] = dict(one(differences(f64, f80)), status=int(f64["status"]), iterations=int(f64["iterations"]),
                          weight=float(f64["measure"]), last_worst=float(f64["worsts"][-1]),
                          last_stress_worst=float(f64["stress_worsts"][-1]),
                          decided=bool(decided(f64, *args) and decided(f80, *args) and f64["status"] == f80["status"]
                                       and f64["iterations"] == f80["iterations"]))
    return rec
