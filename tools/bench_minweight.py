#!/usr/bin/env python3
"""Minimum weight under displacement limits: what one iteration of the optimality-criteria method costs, launch by
launch, for 1, 2 and 8 limits.

    python tools/bench_minweight.py [--copies 4096] [--reps 25] [--warmup 3] [--rounds 3] [--json out.json]

The batch (bar-942 x `--copies`) is resident and ordered on the device; the two load cases are the fixture's own forces
and a rotation of them; limit j is on case j % 2, at the joint with the (j // 2 + 1)-th largest displacement under that
case, along that displacement, at half of it; move 0.3, the bounds 1e-3 of the smallest and 1000 x the largest initial
area.  Warmed up and timed with events `--reps` times, median reported, per J in (1, 2, 8):
  assemble_ms, potrf_ms, gather_ms, potrs_cases_ms, step_ms   the five launches of ONE iteration, each alone, on the
                              buffers of the first analysis of a run (every truss is active; the case block has 2 + J
                              columns)
  iteration_ms                the same launches back to back, as `min_weight` issues them
  limits_with_a_multiplier    how many of the J limits of truss 0 that step left with a multiplier > 0 (a limit without
                              one costs one evaluation per sweep, one with one up to 66)
  cm_step_ms                  `trs_cm_step` on the same batch and the same case block (its 2 + J columns as cases with
                              equal weights): the step of the compliance sizing, one 64-round bisection
  min_weight_ms, iterations, status   a whole `min_weight(...)` call (tol 1e-4, 60 iterations at most) and how it ended
The stress leg: the same run with stress limits - allow_tension 0.5 and allow_compression 0.4 of the largest |N| / A of
the initial design over both cases, euler_kappa 1 / (4 pi) - through `trs_mw_step_stress`:
  step_ms_rounds, stress_step_ms_rounds   the two step kernels alone, alternating, `--rounds` medians each (their spread
                              is the run-to-run spread); step_ms and stress_step_ms are the medians of those.  The floor
                              changes which searches the dual solve runs, so the two do different work
  stress_off_step_ms(_rounds) `trs_mw_step_stress` with both allowables infinite and kappa 0: the floor is the lower end
                              itself, the dual solve walks the path of `trs_mw_step`, and what it costs more is the
                              stress work alone (every real case projected, the requirement, one more reduction)
  stress_min_weight_ms, stress_iterations, stress_status, stress_utilisation_max   a whole call with stress limits
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from python_stable_3d_truss_analysis_amd import _capi, batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--copies", type=int, default=4096)
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--limits", type=int, nargs="+", default=[1, 2, 8])
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()


def timed(fn, reps=None):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps or args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


with open(os.path.join(ROOT, "tests", "golden", "data", "bar-942_input_0.json")) as fh:
    packed = batch.pack_json([json.load(fh)]).replicate(args.copies)
dev = torch.device("cuda:0")
L = 2
own = torch.from_numpy(packed.loads).to(dev)
loads = torch.stack([math.cos(l) * own + 0.5 * math.sin(l) * own.flip(-1) for l in range(L)], dim=1).contiguous()
db = batch.DeviceBatch(packed, dev, use_small=False, reorder="device")
db.factor()
u0 = db.solve_cases(loads)["u"][0].cpu().numpy()                    # [L, nJ, 3], the caller's numbering
A0 = db.A.clone()
kw_bounds = dict(area_min=1e-3 * float(A0.min().item()), area_max=1000.0 * float(A0.max().item()))
kw = dict(move=0.3, **kw_bounds)
bounds = [(None, kw["area_min"]), (None, kw["area_max"])]
# the largest |N| / A of the initial design: `sizing` with allowables of 1 and no resizing reports it as the utilisation
s0 = float(db.sizing(loads, allow_tension=1.0, allow_compression=1.0, max_iters=0, **kw_bounds)["utilisation"].max().item())
stress = dict(allow_tension=0.5 * s0, allow_compression=0.4 * s0, euler_kappa=1.0 / (4.0 * math.pi))
norm = np.sqrt((u0 ** 2).sum(axis=2))
order = np.argsort(-norm, axis=1)
results = []
for J in args.limits:
    case = [j % L for j in range(J)]
    joint = [int(order[j % L, j // L]) for j in range(J)]
    lim = dict(limit_case=case, limit_joint=joint, limit_direction=[u0[l, k] for l, k in zip(case, joint)],
               limit_value=[0.5 * float(norm[l, k]) for l, k in zip(case, joint)])

    def run():
        db.A.copy_(A0)
        return db.min_weight(loads, **lim, **kw)

    out = run()
    torch.cuda.synchronize()
    iterations = int(out["iterations"].max().item())
    status = sorted(set(out["status"].cpu().numpy().ravel().tolist()))
    weight = float((out["measure"] / out["measure_history"][:, 0]).max().item())
    worst = float(out["ratio"].max().item())
    t_copy = timed(lambda: db.A.copy_(A0))
    t_run = timed(run, reps=max(3, args.reps // 5)) - t_copy

    def run_stress():
        db.A.copy_(A0)
        return db.min_weight(loads, **lim, **kw, **stress)

    out_s = run_stress()
    torch.cuda.synchronize()
    s_iterations = int(out_s["iterations"].max().item())
    s_status = sorted(set(out_s["status"].cpu().numpy().ravel().tolist()))
    s_util = float(out_s["utilisation"].max().item())
    t_run_s = timed(run_stress, reps=max(3, args.reps // 5)) - t_copy

    # the buffers of the first analysis
    val = batch._check_min_weight_scalars("bench", move=kw["move"])
    checked = batch._check_limits("bench", **lim, B=db.B, nJ_max=db.nJ_max, L=L)
    ws = db._mw_workspace(val, bounds, loads, checked, out)
    ws_s = db._mw_workspace(val, bounds, loads, checked, out_s, batch._check_stress_limits("bench", B=db.B, **stress))
    ws_s["F"] = ws["F"]
    off = batch._check_stress_limits("bench", math.inf, math.inf, 0.0, db.B)
    ws_off = db._mw_workspace(val, bounds, loads, checked, out_s, off)
    ws_off["F"] = ws["F"]
    C = L + J
    cm_val = batch._check_min_compliance_scalars("bench", None, L=C)
    cm_out = {k: torch.zeros(shape, dtype=dtype, device=dev) for k, (shape, dtype) in batch._field_shapes(
        batch.MinComplianceResult.FIELDS, db.B, db._sizes(H=cm_val["max_iters"] + 1, L=C)).items()}
    cm_ws = db._cm_workspace(cm_val, bounds, ws["loads"], torch.zeros([db.B], dtype=torch.float64, device=dev), cm_out)
    cm_ws["F"] = ws["F"]
    jo, stream, _ = db._case_launch()
    db.A.copy_(A0)
    db.dofmap()

    def gather():
        _capi.check(db.lib.trs_gather_cases(db.B, C, db.nJ_max, ws["loads"].data_ptr(), db.free_index.data_ptr(),
                                            db.n_free.data_ptr(), db.nJ.data_ptr(), jo, ws["F"].data_ptr(), db.rows, stream),
                    "trs_gather_cases")

    def reset():
        db.A.copy_(A0)          # (every repeat is analysis 0 of a run that has just begun: nothing freezes)
        ws["st"].zero_()
        ws["active"].zero_()

    def cm_reset():
        reset()
        cm_ws["st"].zero_()
        cm_ws["active"].zero_()
        cm_ws["target"].zero_()

    def iteration():
        reset()
        db._analyse_cases(ws)
        db._mw_step(ws, 0, 0)

    t_assemble = timed(db.assemble)
    t_potrf = timed(lambda: (db.assemble(), db.potrf())) - t_assemble
    t_gather = timed(gather)
    db.assemble()
    db.potrf()
    t_potrs = timed(lambda: (gather(), db._potrs_cases(ws["F"], C))) - t_gather
    gather()
    db._potrs_cases(ws["F"], C)
    t_reset = timed(reset)

    def reset_stress():
        db.A.copy_(A0)
        for w in (ws_s, ws_off):
            w["st"].zero_()
            w["active"].zero_()

    t_reset_s = timed(reset_stress)
    rounds = {"plain": [], "stress": [], "off": []}
    for _ in range(max(args.rounds, 1)):   # (alternating: what differs between rounds of one kernel is the spread)
        rounds["plain"].append(timed(lambda: (reset(), db._mw_step(ws, 0, 0))) - t_reset)
        rounds["stress"].append(timed(lambda: (reset_stress(), db._mw_step(ws_s, 0, 0))) - t_reset_s)
        rounds["off"].append(timed(lambda: (reset_stress(), db._mw_step(ws_off, 0, 0))) - t_reset_s)
    t_step, t_step_s = statistics.median(rounds["plain"]), statistics.median(rounds["stress"])
    reset()
    db._mw_step(ws, 0, 0)
    torch.cuda.synchronize()
    active = int((ws["mu"][0] > 0).sum().item())
    t_cm_reset = timed(cm_reset)
    t_cm_step = timed(lambda: (cm_reset(), db._cm_step(cm_ws, 0, 0))) - t_cm_reset
    t_iteration = timed(iteration) - t_reset
    results.append({"J": J, "columns": C, "iterations": iterations, "status": status, "weight_ratio_max": round(weight, 4),
                    "worst_ratio": round(worst, 6), "assemble_ms": round(t_assemble, 4), "potrf_ms": round(t_potrf, 4),
                    "gather_ms": round(t_gather, 4), "potrs_cases_ms": round(t_potrs, 4), "step_ms": round(t_step, 4),
                    "limits_with_a_multiplier": active, "cm_step_ms": round(t_cm_step, 4),
                    "iteration_ms": round(t_iteration, 4), "min_weight_ms": round(t_run, 3),
                    "step_ms_rounds": [round(t, 4) for t in rounds["plain"]], "stress_step_ms": round(t_step_s, 4),
                    "stress_step_ms_rounds": [round(t, 4) for t in rounds["stress"]],
                    "stress_off_step_ms": round(statistics.median(rounds["off"]), 4),
                    "stress_off_step_ms_rounds": [round(t, 4) for t in rounds["off"]],
                    "stress_min_weight_ms": round(t_run_s, 3), "stress_iterations": s_iterations,
                    "stress_status": s_status, "stress_utilisation_max": round(s_util, 6)})
summary = {"shape": f"bar-942 x {args.copies}", "B": int(db.B), "L": L, "rows": int(db.rows), "reps": args.reps,
           "statistic": "median of event-timed repeats", "sweeps": 2, "runs": results}
print(json.dumps(summary))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(summary, fh, indent=1)
