#!/usr/bin/env python3
"""Member sizing: what one iteration of the stress-ratio method costs, launch by launch.

    python tools/bench_sizing.py [--copies 4096] [--cases 8] [--reps 25] [--warmup 3] [--json out.json]

The batch (bar-942 x `--copies`) is resident and ordered on the device; the `--cases` load cases are rotations of the
fixture's own forces, the allowables 0.5 / 0.4 of the largest initial stress.  Warmed up and timed with events `--reps`
times, median reported:
  assemble_ms, potrf_ms, gather_ms, potrs_cases_ms, step_ms   the five launches of ONE iteration, each alone, on the
                              buffers of the first analysis of a run (every truss is active)
  iteration_ms                the same launches back to back, as `sizing` issues them
  recover_cases_ms            `trs_recover_cases` on the same batch, case block and L: the kernel that `trs_sz_step`
                              replaces (it reads the same solutions and writes u, f_ext and N of every case)
  sizing_ms, iterations       a whole `sizing(...)` call (tol 1e-4, 40 iterations at most) and how far it got
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from python_stable_3d_truss_analysis_amd import _capi, batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--copies", type=int, default=4096)
ap.add_argument("--cases", type=int, default=8)
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
L = args.cases
own = torch.from_numpy(packed.loads).to(dev)
loads = torch.stack([math.cos(l) * own + 0.5 * math.sin(l) * own.flip(-1) for l in range(L)], dim=1).contiguous()
db = batch.DeviceBatch(packed, dev, use_small=False, reorder="device")
db.factor()
first = db.solve_cases(loads)
s0 = float((first["N"].abs() / db.A.unsqueeze(1)).max().item())
A0 = db.A.clone()
kw = dict(allow_tension=0.5 * s0, allow_compression=0.4 * s0, area_min=0.1 * float(A0.min().item()),
          area_max=1000.0 * float(A0.max().item()))


def sizing():
    db.A.copy_(A0)
    return db.sizing(loads, **kw)


out = sizing()
torch.cuda.synchronize()
iterations = int(out["iterations"].max().item())
status = sorted(set(out["status"].cpu().numpy().ravel().tolist()))
t_copy = timed(lambda: db.A.copy_(A0))
t_sizing = timed(sizing, reps=max(3, args.reps // 5)) - t_copy

# the buffers of the first analysis
val = batch._check_sizing_scalars("bench", kw["allow_tension"], kw["allow_compression"])
ws = db._sz_workspace(val, [(None, kw["area_min"]), (None, kw["area_max"])], loads, out)
jo, stream, _ = db._case_launch()
db.A.copy_(A0)
db.dofmap()


def gather():
    _capi.check(db.lib.trs_gather_cases(db.B, L, db.nJ_max, loads.data_ptr(), db.free_index.data_ptr(), db.n_free.data_ptr(),
                                        db.nJ.data_ptr(), jo, ws["F"].data_ptr(), db.rows, stream), "trs_gather_cases")


def reset():
    db.A.copy_(A0)          # (every repeat is analysis 0 of a run that has just begun: nothing freezes)
    ws["st"].zero_()
    ws["active"].zero_()


def step():
    reset()
    db._sz_step(ws, 0, 0)


def recover():
    _capi.check(db.lib.trs_recover_cases(
        db.B, L, db.nJ_max, db.nM_max, db.xyz.data_ptr(), *db._members(), loads.data_ptr(), db.free_index.data_ptr(),
        db.nJ.data_ptr(), db.nM.data_ptr(), ws["F"].data_ptr(), db.rows, first["u"].data_ptr(), first["f_ext"].data_ptr(),
        first["N"].data_ptr(), jo, stream), "trs_recover_cases")


def iteration():
    reset()
    db._analyse_cases(ws)
    db._sz_step(ws, 0, 0)


t_assemble = timed(db.assemble)
t_potrf = timed(lambda: (db.assemble(), db.potrf())) - t_assemble
t_gather = timed(gather)
db.assemble()
db.potrf()
t_potrs = timed(lambda: (gather(), db._potrs_cases(ws["F"], L))) - t_gather
gather()
db._potrs_cases(ws["F"], L)
t_reset = timed(reset)
t_step = timed(step) - t_reset
t_recover = timed(recover)
t_iteration = timed(iteration) - t_reset
case_block = db.B * L * db.rows * 8
summary = {"shape": f"bar-942 x {args.copies}", "B": int(db.B), "L": L, "rows": int(db.rows), "reps": args.reps,
           "statistic": "median of event-timed repeats", "iterations": iterations, "status": status,
           "assemble_ms": round(t_assemble, 4), "potrf_ms": round(t_potrf, 4), "gather_ms": round(t_gather, 4),
           "potrs_cases_ms": round(t_potrs, 4), "step_ms": round(t_step, 4), "recover_cases_ms": round(t_recover, 4),
           "iteration_ms": round(t_iteration, 4), "sizing_ms": round(t_sizing, 3),
           "case_block_bytes": case_block, "step_case_block_GBps": round(case_block / (t_step * 1e-3) / 1e9, 1)}
print(json.dumps(summary))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(summary, fh, indent=1)
