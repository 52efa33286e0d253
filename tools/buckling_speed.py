#!/usr/bin/env python3
"""Linear buckling from shifted factors: what the pieces cost.

    python tools/buckling_speed.py [--copies 4096] [--reps 25] [--p 4] [--json out.json]

The batch (bar-942 x `--copies`) is resident and ordered on the device.  Warmed up and timed with events `--reps` times,
median reported:
  factor_ms          `factor()`: dofmap, assembly, Cholesky factorisation
  potrs_ms           ONE `trs_potrs_cases` launch on the block of 16 vectors
  product_ms         ONE `trs_bk_product` launch (G = H Y)
  step_ms            ONE `trs_bk_step` launch (check = 0), and `step_check_ms` with the residuals formed
  modes_step_ms      ONE `trs_modes_step` launch beside the same substitution (check = 0): the modes iteration
  members_ms, assemble_ms, amend_ms, potrf_ms   the launches of a shift round (`trs_bk_members`, `trs_assemble`,
                     `trs_nl_tangent` with W(theta), `trs_potrf_batched`) at half the critical factor
  buckling_ms        `factor()` and the whole `buckling(p)` call, with the iterations and rounds it took
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
ap.add_argument("--p", type=int, default=4)
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
stream = torch.cuda.current_stream(dev).cuda_stream
t_factor = timed(db.factor)


def whole():
    db.factor()
    return db.buckling(args.p)


out = whole()
torch.cuda.synchronize()
iters, rounds = out["iters"].cpu().numpy(), out["rounds"].cpu().numpy()
critical = float(out["critical"][0])
t_whole = timed(whole, reps=max(3, args.reps // 5))

# the launches of one iteration, on buffers in the state the iteration leaves them in (a converged block that goes on)
db.factor()
ws, F = db._bk_ws, db.cases_F
F.copy_(ws["Fk"])
ws["state"].zero_()
ws["theta"].zero_()


def potrs():
    _capi.check(lib.trs_potrs_cases(db.B, 16, db.n_free.data_ptr(), db.ld, db.rows, db.S.data_ptr(), F.data_ptr(),
                                    db.rows, db._env_ptr(), stream), "trs_potrs_cases")


def product():
    _capi.check(lib.trs_bk_product(db.B, db.nJ_max, db.nM_max, ws["ends"].data_ptr(), ws["Mt"].data_ptr(),
                                   db.free_index.data_ptr(), db.n_free.data_ptr(), db.nJ.data_ptr(), db.nM.data_ptr(),
                                   F.data_ptr(), ws["G"].data_ptr(), db.rows, stream), "trs_bk_product")


def step(check):
    # tol = 0: nothing freezes, every repeat does the same work
    _capi.check(lib.trs_bk_step(db.B, args.p, db.n_free.data_ptr(), ws["theta"].data_ptr(), F.data_ptr(),
                                ws["G"].data_ptr(), ws["Fk"].data_ptr(), ws["X"].data_ptr(), db.rows,
                                ws["lam"].data_ptr(), ws["resid"].data_ptr(), ws["rank"].data_ptr(),
                                ws["state"].data_ptr(), 0, check, 1, 0.0, stream), "trs_bk_step")


def iteration(check):
    potrs()
    product()
    step(check)


t_iter = timed(lambda: iteration(0))
t_iter_check = timed(lambda: iteration(1))
rank = ws["rank"].cpu().numpy()
potrs()
t_product = timed(product)    # (Y stays as it is: the same work every time)
t_potrs = timed(potrs)        # (on whatever the previous solves left: the substitution's time does not depend on the values)

# the modes iteration beside it: the same substitution and `trs_modes_step`
db.modes(args.p)
mw = db._modes_ws
F.copy_(mw["X"] * mw["Mf"][:, None, :])
mw["state"].zero_()


def modes_iteration():
    potrs()
    _capi.check(lib.trs_modes_step(db.B, args.p, db.n_free.data_ptr(), mw["n_mass"].data_ptr(), mw["Mf"].data_ptr(),
                                   F.data_ptr(), mw["X"].data_ptr(), db.rows, mw["lam"].data_ptr(),
                                   mw["resid"].data_ptr(), mw["state"].data_ptr(), 0, 0, 1, 0.0, stream),
                "trs_modes_step")


t_modes_iter = timed(modes_iteration)

# a shift round at half the critical factor
ws["theta"].fill_(0.5 * critical)
tab = "_tab" if db.table else ""


def members():
    _capi.check(getattr(lib, "trs_bk_members" + tab)(
        db.B, db.nJ_max, db.nM_max, db.xyz.data_ptr(), *db._members(), db.free_index.data_ptr(), db.n_free.data_ptr(),
        db.nJ.data_ptr(), db.nM.data_ptr(), ws["u0"].data_ptr(), db.rows, ws["theta"].data_ptr(), ws["N"].data_ptr(),
        ws["ends"].data_ptr(), ws["Mt"].data_ptr(), ws["W"].data_ptr(), stream), "trs_bk_members" + tab)


def shift_round():
    members()
    db.assemble()
    db._nl_tangent(ws)
    db.potrf()


t_members = timed(members)
t_assemble = timed(db.assemble)
t_round = timed(shift_round)
db.assemble()
t_amend = timed(lambda: db._nl_tangent(ws))   # (amends the slab again and again: the same work, other values)
db.assemble()
db._nl_tangent(ws)
t_round_info = int((db.info != 0).sum().item())
n_pad = (db.n_free.cpu().numpy().astype(np.int64) + 63) // 64 * 64

summary = {
    "shape": f"bar-942 x {args.copies}", "B": int(db.B), "rows": int(db.rows), "p": args.p, "reps": args.reps,
    "statistic": "median of event-timed repeats",
    "factor_ms": round(t_factor, 4), "potrs_ms": round(t_potrs, 4), "product_ms": round(t_product, 4),
    "step_ms": round(t_iter - t_potrs - t_product, 4), "step_check_ms": round(t_iter_check - t_potrs - t_product, 4),
    "iteration_ms": round(t_iter, 4), "iteration_check_ms": round(t_iter_check, 4),
    "modes_iteration_ms": round(t_modes_iter, 4), "modes_step_ms": round(t_modes_iter - t_potrs, 4),
    "members_ms": round(t_members, 4), "assemble_ms": round(t_assemble, 4), "amend_ms": round(t_amend, 4),
    "potrf_ms": round(t_round - t_members - t_assemble - t_amend, 4), "shift_round_ms": round(t_round, 4),
    "shift_round_not_pd": t_round_info,
    "factor_and_buckling_ms": round(t_whole, 3), "iters_max": int(iters.max()), "iters_min": int(iters.min()),
    "rounds_max": int(rounds.max()), "rank_min": int(rank.min()), "critical": critical,
    "product_bytes": int(2 * 16 * 8 * n_pad.sum() + db.B * db.nM_max * 40),
    "product_GBps": round((2 * 16 * 8 * n_pad.sum() + db.B * db.nM_max * 40) / t_product / 1e6, 1),
    "step_bytes": int(6 * 16 * 8 * n_pad.sum()),
}
print(json.dumps(summary))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(summary, fh, indent=1)
