#!/usr/bin/env python3
"""Transient response on the resident factor of K + sigma M: what a time step costs, and what the factor costs.

    python tools/bench_dynamics.py [--copies 4096] [--reps 25] [--warmup 3] [--cases 8,16] [--json out.json]

The batch (bar-942 x `--copies`) is resident and ordered on the device.  Warmed up and timed with events `--reps` times,
median reported, for every L of `--cases`, undamped (beta_R = 0) and with Rayleigh damping (beta_R > 0):
  factor_ms           `factor()`: dofmap, assembly, Cholesky factorisation
  factor_dynamic_ms   `factor_dynamic()`: the same plus the lumped mass and the diagonal shift
  potrs_ms            ONE `trs_potrs_cases` launch on the L right-hand sides (the yardstick of the step kernel)
  step_ms             ONE `trs_dyn_step` launch beside it (a middle time point: state, envelopes, next right-hand side)
  per_step_ms         both, as a time step of `transient` costs them
  transient_ms        a whole `transient(steps=--steps)` call, with four monitored joints and members
`step_bytes` is what the step kernel has to move at least: F, U, V, Acc read and written, Pr and Mf read, the three
envelopes read.
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
ap.add_argument("--cases", default="8,16")
ap.add_argument("--steps", type=int, default=16)
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
db = batch.DeviceBatch(packed, dev, use_small=False, reorder="device")
lib = _capi.load()
rng = np.random.default_rng(0)
omega = 30.0     # (the times do not depend on the values; any positive frequency scale does)
dt = 2.0 * np.pi / omega / 20
t_factor = timed(db.factor)
rows = []
for damped in (False, True):
    damping = dict(damp_mass=0.05 * omega, damp_stiff=0.02 / omega) if damped else {}
    t_dynamic = timed(lambda: db.factor_dynamic(dt, **damping))
    for L in (int(x) for x in args.cases.split(",")):
        f64 = lambda *shape: torch.from_numpy(rng.uniform(-1.0, 1.0, size=shape)).to(dev)
        pattern = f64(db.B, L, db.nJ_max, 3)
        T1 = args.steps + 1
        scale, accel = f64(db.B, L, T1), f64(db.B, L, T1, 3)
        monitors = torch.arange(4, dtype=torch.int32, device=dev).expand(db.B, 4).contiguous()
        run = lambda: db.transient(pattern, args.steps, scale=scale, accel=accel, monitor_joints=monitors,
                                   monitor_members=monitors)
        out = run()
        t_transient = timed(run, reps=max(3, args.reps // 5))
        # the two launches of one time step, on the buffers as the run left them
        dyn, state, F, Pr = db._dynamic, out["state"], db._dyn_F, db._dyn_Pr
        stream = torch.cuda.current_stream(dev).cuda_stream
        fn = getattr(lib, "trs_dyn_tab_step" if db.table else "trs_dyn_step")
        G = F.clone()   # (the substitution timed alone works on a copy: F stays the loop's)

        def potrs(X=F):
            _capi.check(lib.trs_potrs_cases(db.B, L, db.n_free.data_ptr(), db.ld, db.rows, db.S.data_ptr(), X.data_ptr(),
                                            db.rows, db._env_ptr(), stream), "trs_potrs_cases")

        def step():
            _capi.check(fn(db.B, L, db.nJ_max, db.nM_max, db.xyz.data_ptr(), *db._members(), db.free_index.data_ptr(),
                           db.n_free.data_ptr(), db.nJ.data_ptr(), db.nM.data_ptr(), dyn["Mf"].data_ptr(), Pr.data_ptr(),
                           scale.data_ptr(), accel.data_ptr(), T1, args.steps // 2, 0, dyn["dt"], dyn["beta"],
                           dyn["gamma"], dyn["damp_mass"], dyn["damp_stiff"], F.data_ptr(), state["U"].data_ptr(),
                           state["V"].data_ptr(), state["Acc"].data_ptr(), db.rows, out["u_peak"].data_ptr(),
                           out["u_step"].data_ptr(), out["N_max"].data_ptr(), out["N_max_step"].data_ptr(),
                           out["N_min"].data_ptr(), out["N_min_step"].data_ptr(), monitors.data_ptr(), 4,
                           monitors.data_ptr(), 4, out["hist_u"].data_ptr(), out["hist_N"].data_ptr(),
                           batch._ptr(db.joint_out), stream), "trs_dyn_step")

        def both():
            # (the repeats ARE a time integration - the middle time point over and over - so the state stays bounded)
            potrs()
            step()

        step()           # F holds a right-hand side again, as inside the loop
        t_both = timed(both)
        t_potrs = timed(lambda: potrs(G))   # (its time does not depend on the values)
        n_pad = (db.n_free.cpu().numpy().astype(np.int64) + 63) // 64 * 64
        rows.append({"damped": damped, "L": L, "factor_dynamic_ms": round(t_dynamic, 4), "potrs_ms": round(t_potrs, 4),
                     "step_ms": round(t_both - t_potrs, 4), "per_step_ms": round(t_both, 4),
                     "transient_ms": round(t_transient, 3), "steps": args.steps,
                     "step_bytes": int(8 * L * 9 * n_pad.sum() + 8 * n_pad.sum()
                                       + 8 * L * db.B * (3 * db.nJ_max + 2 * db.nM_max))})
summary = {"shape": f"bar-942 x {args.copies}", "B": int(db.B), "rows": int(db.rows), "reps": args.reps,
           "statistic": "median of event-timed repeats", "factor_ms": round(t_factor, 4), "runs": rows}
print(json.dumps(summary))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(summary, fh, indent=1)
