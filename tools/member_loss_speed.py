#!/usr/bin/env python3
"""Member-loss analysis from the resident factor: what a call costs, and what the same answers cost without it.

    python tools/member_loss_speed.py [--copies 4096] [--reps 5] [--cases 1 8] [--chunks 64 128] [--json out.json]

The batch (bar-942 x `--copies`) is resident and ordered on the device and factored once.  Warmed up and timed with
events `--reps` times, median reported, for every L of `--cases` and every `--chunks` value:
  loss_ms            one `member_loss(loads, chunk=...)` call: the intact `solve_cases`, then per chunk of members
                     `trs_loss_rhs`, `trs_potrs_cases`, `trs_loss_apply`
  removals_per_s     B * nM * L / loss_ms: (truss, removed member, load case) states per second
and the baseline: without this analysis one removal is one more solve of a rebuilt batch, so all of them cost
  baseline_ms = nM * solve_ms,   solve_ms = one whole-pipeline `solve()` of the same resident batch
(`solve_ms` does not depend on this feature: it is the plain step of the commit before it; for L > 1 the baseline is
generous to the old way, which would also have to substitute the other L - 1 cases per removal).  `ratio` =
baseline_ms / loss_ms.  The split between the three kernels comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool.
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
nM = int(packed.nM_max)
solve_ms = timed(db.solve, max(args.reps, 20), 3)
factor_ms = timed(db.factor, max(args.reps, 20), 3)
rng = np.random.default_rng(942)
rows = []
for L in args.cases:
    loads = torch.from_numpy(rng.uniform(-3e4, 3e4, size=(1, L, packed.nJ_max, 3))).to(dev).expand(db.B, -1, -1, -1)
    loads = loads.contiguous()
    for chunk in args.chunks:
        out = db.member_loss(loads, chunk=chunk)
        ms = timed(lambda: db.member_loss(loads, chunk=chunk, out=out), args.reps, args.warmup)
        baseline = nM * solve_ms
        rows.append({"L": L, "chunk": chunk, "loss_ms": round(ms, 2),
                     "removals_per_s": round(db.B * nM * L / (ms * 1e-3)), "baseline_ms": round(baseline, 1),
                     "ratio": round(baseline / ms, 2), "critical": int(out["critical"][0].sum().item())})
summary = {"shape": f"bar-942 x {args.copies}", "B": int(db.B), "nM": nM, "reps": args.reps,
           "statistic": "median of event-timed repeats", "solve_ms": round(solve_ms, 4),
           "factor_ms": round(factor_ms, 4), "solves_per_s": round(db.B / (solve_ms * 1e-3)), "runs": rows}
print(json.dumps(summary))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(summary, fh, indent=1)
