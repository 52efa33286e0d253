#!/usr/bin/env python3
"""Harmonic response from the resident mode block: what the call and its three parts cost.

    python tools/harmonic_speed.py [--copies 4096] [--reps 15] [--p 8] [--cases 8] [--freqs 256] [--json out.json]

The batch (bar-942 x `--copies`) is resident and ordered on the device, factored, and `modes(p)` has converged.  Warmed
up and timed with events `--reps` times, median reported:
  modes_ms      the whole `modes(p)` call, and `potrs_ms`: ONE `trs_potrs_cases` launch on the block of 16 vectors -
                the two yardsticks the harmonic call stands beside
  harmonic_ms   the whole `harmonic()` call: L = `--cases` ground accelerations, S = `--freqs` frequencies from 0 to twice
                the p-th natural frequency, zeta = 0.02, residual on, no monitors
  modal_ms, residual_potrs_ms, sweep_ms   its three launches, each alone, on the buffers the call left
  no_residual_ms, monitors_ms             the call again with residual off, and with 8 + 8 monitors
and the sweep kernel's FP64 rate: (2 p + 3) x 2 flops per item and frequency over all items (members, three displacement
components per joint, three reaction components per joint with a held DOF) over `sweep_ms`, as a fraction of
`--peak-tflops` (the datasheet's 78.6 TFLOP/s of vector FP64, the figure of DESIGN.md's roofline).
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
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--p", type=int, default=8)
ap.add_argument("--cases", type=int, default=8)
ap.add_argument("--freqs", type=int, default=256)
ap.add_argument("--peak-tflops", type=float, default=78.6)
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
db.factor()
modes = db.modes(args.p)
torch.cuda.synchronize()
t_modes = timed(lambda: db.modes(args.p, out=modes), reps=max(3, args.reps // 5))
lam = modes["lam"][0].cpu().numpy()
L, S, p = args.cases, args.freqs, args.p
W = np.linspace(0.0, 2.0 * float(np.sqrt(np.nanmax(lam))), S)
rng = np.random.default_rng(0)
accel = rng.uniform(-1.0, 1.0, size=[L, 3])
out = db.harmonic(W, accel=accel)
torch.cuda.synchronize()
assert all(bool(v.isfinite().all()) for v in out.values())
t_call = timed(lambda: db.harmonic(W, accel=accel, out=out))
t_plain = timed(lambda: db.harmonic(W, accel=accel, residual=False, out=out))
mon_j = torch.arange(8, dtype=torch.int32, device=dev).expand(db.B, -1).contiguous()
mon_m = torch.arange(8, dtype=torch.int32, device=dev).expand(db.B, -1).contiguous()
with_mon = db.harmonic(W, accel=accel, monitor_joints=mon_j, monitor_members=mon_m)
t_mon = timed(lambda: db.harmonic(W, accel=accel, monitor_joints=mon_j, monitor_members=mon_m, out=with_mon))

# the three launches alone, on the buffers the call left (the times do not depend on the values)
ws, F, stream = db._modes_ws, db.cases_F, torch.cuda.current_stream(dev).cuda_stream
ag = torch.from_numpy(np.broadcast_to(accel, (db.B, L, 3)).copy()).to(dev)
W_d = torch.from_numpy(W).to(dev)
jo, _, tab = db._case_launch()


def modal():
    _capi.check(lib.trs_hr_modal(db.B, L, db.nJ_max, db.free_index.data_ptr(), db.n_free.data_ptr(), db.nJ.data_ptr(),
                                 ws["X"].data_ptr(), db.rows, ws["lam"].data_ptr(), ws["Mf"].data_ptr(),
                                 ws["n_mass"].data_ptr(), p, None, ag.data_ptr(), 1, out["g"].data_ptr(), F.data_ptr(),
                                 stream), "trs_hr_modal")


def potrs():
    _capi.check(lib.trs_potrs_cases(db.B, 16, db.n_free.data_ptr(), db.ld, db.rows, db.S.data_ptr(), F.data_ptr(),
                                    db.rows, db._env_ptr(), stream), "trs_potrs_cases")


def sweep():
    _capi.check(getattr(lib, f"trs_hr_sweep{tab}")(
        db.B, L, db.nJ_max, db.nM_max, db.xyz.data_ptr(), *db._members(), db.free_index.data_ptr(), db.n_free.data_ptr(),
        db.nJ.data_ptr(), db.nM.data_ptr(), jo, ws["X"].data_ptr(), db.rows, ws["lam"].data_ptr(), ws["n_mass"].data_ptr(),
        p, out["g"].data_ptr(), F.data_ptr(), S, W_d.data_ptr(), 0.02, 0.0, 0.0, out["u_amp"].data_ptr(),
        out["u_at"].data_ptr(), out["R_amp"].data_ptr(), out["R_at"].data_ptr(), out["N_amp"].data_ptr(),
        out["N_at"].data_ptr(), None, 0, None, 0, None, None, stream), f"trs_hr_sweep{tab}")


t_modal, t_potrs, t_sweep = timed(modal), timed(potrs), timed(sweep)
nJ, nM = packed.nJ.astype(np.int64), packed.nM.astype(np.int64)
held = np.array([int(((packed.cbits[b, :nJ[b]] & 7) != 0).sum()) for b in range(packed.B)], dtype=np.int64)
items = int((nM + 3 * nJ + 3 * held).sum()) * L
flops = (2 * p + 3) * 2 * items * S
summary = {
    "shape": f"bar-942 x {args.copies}", "B": int(db.B), "p": p, "L": L, "S": S, "reps": args.reps,
    "statistic": "median of event-timed repeats",
    "modes_ms": round(t_modes, 3), "potrs_ms": round(t_potrs, 4), "harmonic_ms": round(t_call, 4),
    "modal_ms": round(t_modal, 4), "residual_potrs_ms": round(t_potrs, 4), "sweep_ms": round(t_sweep, 4),
    "no_residual_ms": round(t_plain, 4), "monitors_ms": round(t_mon, 4),
    "sweep_items": items, "sweep_flops": flops, "sweep_tflops": round(flops / (t_sweep * 1e-3) / 1e12, 3),
    "sweep_fraction_of_vector_fp64_peak": round(flops / (t_sweep * 1e-3) / 1e12 / args.peak_tflops, 4),
    "peak_tflops": args.peak_tflops,
    "harmonic_us_per_truss_case_frequency": round(t_call * 1e3 / (db.B * L * S), 5),
}
print(json.dumps(summary))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(summary, fh, indent=1)
