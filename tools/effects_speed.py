#!/usr/bin/env python3
"""Load cases with settlements, pre-strain and self-weight: what they cost beside plain load cases.

    python tools/effects_speed.py [--copies 4096] [--cases 8] [--reps 25] [--table] [--json out.json]

The batch (bar-942 x `--copies`) is resident and ordered on the device.  In ONE process, warmed up and timed with events
`--reps` times, median reported:
  factor_ms          `factor()`: dofmap, assembly, Cholesky factorisation
  plain_ms           factor + `solve_cases(loads)` with `--cases` cases (the shape of EXPERIMENTS R7.1)
  effects_ms         factor + `solve_effect_cases(loads, prestrain, settlement, accel, want_body=True)`, as many cases
  plain_step_ms, effects_step_ms    the two without the factorisation
  effects_step_no_accel_ms, effects_step_loads_only_ms    the effect step without self-weight / with loads alone
and the launches of either step (gather / rhs, `trs_potrs_cases`, recover) as differences of chains timed one launch
longer each, so that no launch is timed on its own output.  `*_bytes`: the algorithmic HBM
traffic of the two steps without the factor's tiles (the same for both) - the per-case streams and, once per kernel, the
truss's own tables - so that the extra time can be set against the extra streams.
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
ap.add_argument("--cases", type=int, default=8)
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--table", action="store_true", help="the table member form")
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
    packed = batch.pack_json([json.load(fh)], members="auto" if args.table else "general").replicate(args.copies)
dev = torch.device("cuda:0")
db = batch.DeviceBatch(packed, dev, use_small=False, reorder="device")
lib = _capi.load()
B, L, nJ, nM = db.B, args.cases, db.nJ_max, db.nM_max

rng = np.random.default_rng(12)
held = packed.constrained()[0]
up = lambda a: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))).to(dev)
loads = up(rng.uniform(-3e4, 3e4, size=(L, nJ, 3)))
eps0 = up(rng.uniform(-5e-4, 5e-4, size=(L, nM)))
ubar = up(rng.uniform(-0.02, 0.02, size=(L, nJ, 3)) * held)
accel = up(rng.uniform(-2.0, 2.0, size=(L, 3)))
f64 = lambda *shape: torch.zeros(list(shape), dtype=torch.float64, device=dev)
plain_out = {"u": f64(B, L, nJ, 3), "f_ext": f64(B, L, nJ, 3), "N": f64(B, L, nM)}
eff_out = dict({k: torch.zeros_like(v) for k, v in plain_out.items()}, body=f64(B, L, nJ, 3))

plain_step = lambda: db.solve_cases(loads, out=plain_out)
effects_step = lambda: db.solve_effect_cases(loads, eps0, ubar, accel, want_body=True, out=eff_out)


def both(step):
    db.factor()
    step()


t_factor = timed(db.factor)
t_plain, t_effects = timed(lambda: both(plain_step)), timed(lambda: both(effects_step))
t_plain_step, t_effects_step = timed(plain_step), timed(effects_step)
t_plain_2, t_effects_2 = timed(lambda: both(plain_step)), timed(lambda: both(effects_step))   # (again: the box's drift)
# the effect step with fewer effects: what each of them adds
t_no_accel = timed(lambda: db.solve_effect_cases(loads, eps0, ubar, None, want_body=False, out=plain_out))
t_loads_only = timed(lambda: db.solve_effect_cases(loads, out=plain_out))

# the launches of either step: each chain is timed one launch longer, and a launch's time is the difference - so every
# substitution works on a freshly built right-hand side and every recovery on a solution, never on its own output
F, stream = db.cases_F, torch.cuda.current_stream(dev).cuda_stream
ptr = lambda x: None if x is None else x.data_ptr()
jo = ptr(db.joint_out)
tab = "_tab" if db.table else ""
members = db._members() if db.table else db._members() + (ptr(db.rho),)
shape4 = (B, L, nJ, nM)
effects = (loads.data_ptr(), eps0.data_ptr(), ubar.data_ptr(), accel.data_ptr())
tables = (db.free_index.data_ptr(), db.n_free.data_ptr(), db.nJ.data_ptr(), db.nM.data_ptr())


def gather():
    _capi.check(lib.trs_gather_cases(B, L, nJ, loads.data_ptr(), *tables[:3], jo, F.data_ptr(), db.rows, stream),
                "trs_gather_cases")


def potrs():
    _capi.check(lib.trs_potrs_cases(B, L, db.n_free.data_ptr(), db.ld, db.rows, db.S.data_ptr(), F.data_ptr(), db.rows,
                                    db._env_ptr(), stream), "trs_potrs_cases")


def recover_plain():
    fn = lib.trs_recover_tab_cases if db.table else lib.trs_recover_cases
    _capi.check(fn(*shape4, db.xyz.data_ptr(), *db._members(), loads.data_ptr(), tables[0], tables[2], tables[3],
                   F.data_ptr(), db.rows, plain_out["u"].data_ptr(), plain_out["f_ext"].data_ptr(),
                   plain_out["N"].data_ptr(), jo, stream), "trs_recover_cases")


def rhs():
    _capi.check(getattr(lib, f"trs_effects{tab}_rhs")(*shape4, db.xyz.data_ptr(), *members, *effects, *tables, jo,
                                                     F.data_ptr(), db.rows, stream), "trs_effects_rhs")


def recover_effects():
    _capi.check(getattr(lib, f"trs_effects{tab}_recover")(
        *shape4, db.xyz.data_ptr(), *members, *effects, tables[0], tables[2], tables[3], F.data_ptr(), db.rows,
        eff_out["u"].data_ptr(), eff_out["f_ext"].data_ptr(), eff_out["N"].data_ptr(), eff_out["body"].data_ptr(), jo,
        stream), "trs_effects_recover")


def chain(*fns):
    def run():
        for fn in fns:
            fn()
    return timed(run)


split = {}
for first, last, names in ((gather, recover_plain, ("gather", "potrs_plain", "recover_plain")),
                           (rhs, recover_effects, ("rhs", "potrs_effects", "recover_effects"))):
    t1, t2, t3 = chain(first), chain(first, potrs), chain(first, potrs, last)
    split.update(zip(names, (t1, t2 - t1, t3 - t2)))

# algorithmic bytes per truss (without the factor's tiles, which both steps read alike in trs_potrs_cases)
n_pad = (int(packed.n_free[0]) + 63) // 64 * 64
joint_arr, member_arr, red = 8 * L * 3 * nJ, 8 * L * nM, 8 * L * n_pad
member_tab = nM * (5 if db.table else 8 + 16)             # end joints + what E A is made of
dof_tab = 8 * 3 * nJ + 4 * 3 * nJ + (4 * nJ if jo else 0)  # xyz, free_index, joint order
plain_bytes = (joint_arr + 4 * 3 * nJ + red) + 4 * red + (red + joint_arr + member_tab + dof_tab + 2 * joint_arr + member_arr)
effects_bytes = (2 * joint_arr + member_arr + member_tab + dof_tab + (0 if db.table else 8 * nM) + red) + 4 * red + \
    (red + 2 * joint_arr + member_arr + member_tab + dof_tab + (0 if db.table else 8 * nM) + 3 * joint_arr + member_arr)

extra_ms = t_effects_step - t_plain_step
summary = {
    "shape": f"bar-942 x {B}", "B": B, "L": L, "rows": int(db.rows), "member_form": "table" if db.table else "general",
    "reps": args.reps, "statistic": "median of event-timed repeats, one process",
    "factor_ms": round(t_factor, 4), "plain_ms": round(t_plain, 4), "effects_ms": round(t_effects, 4),
    "plain_ms_again": round(t_plain_2, 4), "effects_ms_again": round(t_effects_2, 4),
    "effects_over_plain": round(t_effects / t_plain, 4),
    "plain_step_ms": round(t_plain_step, 4), "effects_step_ms": round(t_effects_step, 4),
    "step_ratio": round(t_effects_step / t_plain_step, 4),
    "effects_step_no_accel_ms": round(t_no_accel, 4), "effects_step_loads_only_ms": round(t_loads_only, 4),
    "split_ms": {k: round(v, 4) for k, v in split.items()},
    "plain_step_bytes_per_truss": int(plain_bytes), "effects_step_bytes_per_truss": int(effects_bytes),
    "bytes_ratio": round(effects_bytes / plain_bytes, 4),
    "extra_ms": round(extra_ms, 4), "extra_bytes": int((effects_bytes - plain_bytes) * B),
    "extra_GBps": round((effects_bytes - plain_bytes) * B / max(extra_ms, 1e-9) / 1e6, 1),
}
print(json.dumps(summary))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(summary, fh, indent=1)
