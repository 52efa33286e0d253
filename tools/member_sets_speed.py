#!/usr/bin/env python3
"""Member-set scenarios from the resident factor: what a scenario costs, beside one whole-pipeline step.

    python tools/member_sets_speed.py [--copies 4096] [--scenarios 64] [--reps 5] [--cases 1 8] [--chunks 64 128]
                                      [--json out.json]

The batch (bar-942 x `--copies`) is resident and ordered on the device and factored once.  Two scenario lists, the same
for every truss: `--scenarios` seeded random TRIPLES of members and as many random 8-SETS, every member removed
(gamma = 0).  Warmed up and timed with events `--reps` times, median reported, for every L of `--cases` and every
`--chunks` value:
  sets_ms            one `member_sets(loads, sets, chunk=...)` call: the intact `solve_cases`, the host's plan and its
                     uploads, then per range of scenarios `trs_sets_rhs`, `trs_potrs_cases`, `trs_sets_apply`
  ranges, columns    how the plan cut the scenario axis, and the substitution columns it used (distinct members)
  ms_per_scenario    sets_ms / S: the whole batch, one scenario of every truss
beside
  solve_ms           one whole-pipeline `solve()` of the same resident batch: what ONE scenario costs today, by
                     assembling, factoring and solving the changed batch again (`solve_ms` does not depend on this
                     feature: that pipeline is untouched, so on the same tree it is the plain step of the commit before)
`ratio` = solve_ms / ms_per_scenario.  There is no pass mark.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from python_stable_3d_truss_analysis_amd import batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--copies", type=int, default=4096)
ap.add_argument("--scenarios", type=int, default=64)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--cases", type=int, nargs="+", default=[1, 8])
ap.add_argument("--chunks", type=int, nargs="+", default=[64, 128])
ap.add_argument("--json", default=None)
args = ap.parse_args()


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
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
db = batch.DeviceBatch(packed, dev, use_small=False, reorder="device")
nM, S = int(packed.nM_max), args.scenarios
solve_ms = timed(db.solve, max(args.reps, 20), 3)
factor_ms = timed(db.factor, max(args.reps, 20), 3)
rng = np.random.default_rng(942)
lists = {}
for kind, k in (("triples", 3), ("8-sets", 8)):
    one = np.full([S, 8], -1, dtype=np.int64)
    for s in range(S):
        one[s, :k] = rng.choice(nM, size=k, replace=False)
    lists[kind] = np.ascontiguousarray(np.broadcast_to(one, (db.B, S, 8)))
rows = []
for L in args.cases:
    loads = torch.from_numpy(rng.uniform(-3e4, 3e4, size=(1, L, packed.nJ_max, 3))).to(dev).expand(db.B, -1, -1, -1)
    loads = loads.contiguous()
    for kind, sets in lists.items():
        for chunk in args.chunks:
            plan = batch.plan_member_sets(sets[:1], chunk, nM)
            out = db.member_sets(loads, sets, chunk=chunk)
            ms = timed(lambda: db.member_sets(loads, sets, chunk=chunk, out=out), args.reps, args.warmup)
            rows.append({"L": L, "sets": kind, "chunk": chunk, "sets_ms": round(ms, 2), "ranges": len(plan),
                         "columns": int(sum((cols[0] >= 0).sum() for _s0, _s1, cols, _slot in plan)),
                         "ms_per_scenario": round(ms / S, 3), "ratio": round(solve_ms / (ms / S), 2),
                         "unstable": int(out["unstable"][0].sum().item())})
summary = {"shape": f"bar-942 x {args.copies}", "B": int(db.B), "nM": nM, "S": S, "reps": args.reps,
           "statistic": "median of event-timed repeats", "solve_ms": round(solve_ms, 4),
           "factor_ms": round(factor_ms, 4), "runs": rows}
print(json.dumps(summary))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(summary, fh, indent=1)
