#!/usr/bin/env python3
"""The adjoint (backward) pass against the forward pass it differentiates, on the headline shape (bar-942 x 4096).

    python tools/adjoint_speed.py [--copies 4096] [--reps 25] [--cases 1,8] [--json out.json]

The batch is resident, ordered and factored once (DeviceBatch(reorder=True)).  For every L, on the same factor, in the
same process, each warmed up and timed with events `--reps` times (median reported):
  factor_ms    `factor()`: dofmap, assembly, Cholesky factorisation
  cases_ms     `solve_cases()`: gather + substitution + recovery of L cases (the forward pass)
  adjoint_ms   `adjoint_cases()` with cotangents on u, f_ext and N and all four gradients wanted:
               right-hand sides + substitution + contraction (the backward pass)
  rhs_ms / grad_ms   the two new kernels alone (`trs_adjoint_rhs`, `trs_adjoint_grad`)
and the ratios adjoint / cases and adjoint / factor.
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
from python_stable_3d_truss_analysis_amd import _capi, batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--copies", type=int, default=4096)
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--cases", default="1,8")
ap.add_argument("--json", default=None)
args = ap.parse_args()


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
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
db = batch.DeviceBatch(packed, dev, use_small=False, reorder=True)
lib = _capi.load()
rng = np.random.default_rng(0)
dense = lambda *shape, scale=1.0: torch.from_numpy(rng.uniform(-scale, scale, size=shape)).to(dev)

rows = []
for L in (int(x) for x in args.cases.split(",")):
    loads = dense(db.B, L, db.nJ_max, 3, scale=3e4)
    cots = {"grad_u": dense(db.B, L, db.nJ_max, 3, scale=1e2), "grad_f_ext": dense(db.B, L, db.nJ_max, 3, scale=1e-4),
            "grad_N": dense(db.B, L, db.nM_max, scale=1e-4)}
    fwd = {"u": torch.empty([db.B, L, db.nJ_max, 3], dtype=torch.float64, device=dev),
           "f_ext": torch.empty([db.B, L, db.nJ_max, 3], dtype=torch.float64, device=dev),
           "N": torch.empty([db.B, L, db.nM_max], dtype=torch.float64, device=dev)}
    out = {k: torch.empty(shape, dtype=dtype, device=dev) for k, (shape, dtype) in
           batch._field_shapes(batch.GradientResult.FIELDS, db.B, db._sizes(L=L), db.GRADIENTS).items()}
    t_factor = timed(db.factor)
    t_cases = timed(lambda: db.solve_cases(loads, fwd))
    t_adjoint = timed(lambda: db.adjoint_cases(**cots, out=out))
    Lam, stream = db.cases_Lam, torch.cuda.current_stream(dev).cuda_stream
    jo = db.joint_out.data_ptr() if db.joint_out is not None else None
    scratch = torch.empty_like(Lam)
    t_rhs = timed(lambda: _capi.check(lib.trs_adjoint_rhs(
        db.B, L, db.nJ_max, db.nM_max, db.xyz.data_ptr(), *db._members(), cots["grad_u"].data_ptr(),
        cots["grad_f_ext"].data_ptr(), cots["grad_N"].data_ptr(), db.free_index.data_ptr(), db.n_free.data_ptr(),
        db.nJ.data_ptr(), db.nM.data_ptr(), jo, scratch.data_ptr(), db.rows, stream), "trs_adjoint_rhs"))
    t_grad = timed(lambda: _capi.check(lib.trs_adjoint_grad(
        db.B, L, db.nJ_max, db.nM_max, db.xyz.data_ptr(), *db._members(), cots["grad_f_ext"].data_ptr(),
        cots["grad_N"].data_ptr(), db.free_index.data_ptr(), db.nJ.data_ptr(), db.nM.data_ptr(), db.cases_F.data_ptr(),
        Lam.data_ptr(), db.rows, out["A"].data_ptr(), out["E"].data_ptr(), out["xyz"].data_ptr(),
        out["loads"].data_ptr(), jo, stream), "trs_adjoint_grad"))
    rows.append({"L": L, "factor_ms": round(t_factor, 4), "cases_ms": round(t_cases, 4),
                 "adjoint_ms": round(t_adjoint, 4), "rhs_ms": round(t_rhs, 4), "grad_ms": round(t_grad, 4),
                 "adjoint_over_cases": round(t_adjoint / t_cases, 4), "adjoint_over_factor": round(t_adjoint / t_factor, 4)})
    print(json.dumps(rows[-1]), flush=True)

summary = {"shape": f"bar-942 x {args.copies}", "reps": args.reps, "statistic": "median of event-timed repeats",
           "adjoint_lds_bytes_per_work_group": (6 * db.nJ_max + db.nM_max) * 8 + (2 * db.nJ_max + 1 + 2 * db.nM_max) * 4,
           "rows": rows}
print(json.dumps(summary))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(summary, fh, indent=1)
