#!/usr/bin/env python3
"""Tension-only and compression-only members: what one analysis of the active-set iteration costs, launch by launch.

    python tools/bench_unilateral.py [--copies 4096] [--slack 1e-3] [--reps 25] [--warmup 3] [--json out.json]

The batch (bar-942 x `--copies`) is resident and ordered on the device; the load case is the fixture's own forces.  From
the linear solution every fourth member whose |N| is at least 5 % of the largest is made tension-only (the rule "q" of
tests/unilateral_reference.py); a slack member keeps `--slack` of its area.  Warmed up and timed with events `--reps`
times, median reported:
  assemble_ms, potrf_ms, rhs_ms, potrs_cases_ms, step_ms   the five launches of ONE analysis, each alone, on the buffers of
                              the first analysis of a run (every truss is active, every member too)
  analysis_ms                 the same launches back to back, as `unilateral` issues them
  sz_step_ms                  `trs_sz_step` with L = 1 on the same batch and case block: the step of the member sizing,
                              which does more per member (requirement areas, weight, per-member LDS tables); the two
                              steps are timed in three alternating rounds (step_rounds_ms), the median round reported
  recover_ms                  `trs_effects_recover` (L = 1) of the final structure, once per run
  unilateral_ms, iterations   a whole `unilateral(...)` call (20 rounds at most) and how far it got
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from python_stable_3d_truss_analysis_amd import _capi, batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--copies", type=int, default=4096)
ap.add_argument("--slack", type=float, default=1e-3)
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--warmup", type=int, default=3)
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
loads = torch.from_numpy(packed.loads).to(dev)              # the caller's joint numbering
db = batch.DeviceBatch(packed, dev, use_small=False, reorder="device")
db.factor()
first = db.solve_cases(loads.unsqueeze(1).contiguous())
N = first["N"][:, 0]
chosen = (N.abs() >= 0.05 * N.abs().amax(dim=1, keepdim=True)) & (torch.arange(db.nM_max, device=dev)[None, :] % 4 == 0)
kind = chosen.to(torch.int8)
A0 = db.A.clone()
kw = dict(slack_factor=args.slack, max_iters=20)


def unilateral():
    db.A.copy_(A0)
    return db.unilateral(kind, loads, **kw)


out = unilateral()
torch.cuda.synchronize()
iterations = int(out["iterations"].max().item())
status = sorted(set(out["status"].cpu().numpy().ravel().tolist()))
flips = out["flips_history"][0, :iterations + 1].cpu().numpy().tolist()
t_copy = timed(lambda: db.A.copy_(A0))
t_unilateral = timed(unilateral, reps=max(3, args.reps // 5)) - t_copy

# the buffers of the first analysis
db.A.copy_(A0)
on = {"kind": kind, "loads": loads, "prestrain": None, "state": None}
ws = db._un_workspace(on, args.slack, kw["max_iters"], out)
jo, stream, _ = db._case_launch()
db.dofmap()
members = db._members() + (db.rho.data_ptr(),)


def rhs():
    _capi.check(db.lib.trs_effects_rhs(
        db.B, 1, db.nJ_max, db.nM_max, db.xyz.data_ptr(), *members, loads.data_ptr(), None, None, None,
        db.free_index.data_ptr(), db.n_free.data_ptr(), db.nJ.data_ptr(), db.nM.data_ptr(), jo, ws["F"].data_ptr(), db.rows,
        stream), "trs_effects_rhs")


def recover():
    _capi.check(db.lib.trs_effects_recover(
        db.B, 1, db.nJ_max, db.nM_max, db.xyz.data_ptr(), *members, loads.data_ptr(), None, None, None,
        db.free_index.data_ptr(), db.nJ.data_ptr(), db.nM.data_ptr(), ws["F"].data_ptr(), db.rows, out["u"].data_ptr(),
        out["f_ext"].data_ptr(), out["N"].data_ptr(), None, jo, stream), "trs_effects_recover")


def reset():
    db.A.copy_(A0)          # (every repeat is analysis 0 of a run that has just begun: nothing freezes)
    ws["st"].zero_()
    ws["active"].zero_()


def step():
    reset()
    db._un_step(ws, 0, 0)


def analysis():
    reset()
    db._un_analyse(ws)
    db._un_step(ws, 0, 0)


# the member sizing's step on the same case block, L = 1
s0 = float((N.abs() / A0).max().item())
val = batch._check_sizing_scalars("bench", 0.5 * s0, 0.4 * s0)
keys = [k for k, *_ in batch.SizingResult.FIELDS.values() if k != "catalog_index"]
sz_out = db._out_tensors("sizing", batch._field_shapes(batch.SizingResult.FIELDS, db.B, db._sizes(H=val["max_iters"] + 1),
                                                       keys), None)
bounds = [(None, 0.1 * float(A0.min().item())), (None, 1000.0 * float(A0.max().item()))]
sz = db._sz_workspace(val, bounds, loads.unsqueeze(1).contiguous(), sz_out)
sz["F"] = ws["F"]


def sz_reset():
    db.A.copy_(A0)
    sz["st"].zero_()
    sz["active"].zero_()


def sz_step():
    sz_reset()
    db._sz_step(sz, 0, 0)


t_assemble = timed(db.assemble)
t_potrf = timed(lambda: (db.assemble(), db.potrf())) - t_assemble
t_rhs = timed(rhs)
db.assemble()
db.potrf()
t_potrs = timed(lambda: (rhs(), db._potrs_cases(ws["F"], 1))) - t_rhs
rhs()
db._potrs_cases(ws["F"], 1)
t_reset = timed(reset)
t_sz_reset = timed(sz_reset)
rounds = []     # the two steps alternate, so that a drift of the machine shows in both
for _ in range(3):
    rounds.append((timed(step) - t_reset, timed(sz_step) - t_sz_reset))
t_step, t_sz_step = (statistics.median(r[i] for r in rounds) for i in range(2))
t_recover = timed(recover)
t_analysis = timed(analysis) - t_reset
summary = {"shape": f"bar-942 x {args.copies}", "B": int(db.B), "rows": int(db.rows), "reps": args.reps,
           "statistic": "median of event-timed repeats", "slack_factor": args.slack,
           "unilateral_members": int(chosen[0].sum().item()), "iterations": iterations, "status": status, "flips": flips,
           "assemble_ms": round(t_assemble, 4), "potrf_ms": round(t_potrf, 4), "rhs_ms": round(t_rhs, 4),
           "potrs_cases_ms": round(t_potrs, 4), "step_ms": round(t_step, 4), "sz_step_ms": round(t_sz_step, 4),
           "recover_ms": round(t_recover, 4), "analysis_ms": round(t_analysis, 4), "unilateral_ms": round(t_unilateral, 3),
           "reset_ms": round(t_reset, 4), "sz_reset_ms": round(t_sz_reset, 4),
           "step_rounds_ms": [[round(a, 4), round(b, 4)] for a, b in rounds]}
print(json.dumps(summary))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(summary, fh, indent=1)
