#!/usr/bin/env python3
"""Influence lines and moving-load envelopes from the resident factor: what a call costs beside the member-loss analysis.

    python tools/influence_speed.py [--copies 4096] [--reps 25] [--chunk 64] [--joints 32] [--only influence|loss]
                                    [--json out.json]

The batch (bar-942 x `--copies`) is resident and ordered on the device and factored once.  The path climbs one leg of
the tower: from a support, always along a member to the higher joint that strays least sideways (27 joints reach the
top; the rest go down the next leg the same way), `--joints` joints;
the load is horizontal (1, 0, 0), the train three axles.  Warmed up and timed with events `--reps` times, median:
  influence_ms   one `influence(...)` call: per chunk of members `trs_loss_rhs`, `trs_potrs_cases`, `trs_influence_apply`
  loss_ms        one `member_loss(loads, chunk=...)` call with L = 1: the intact `solve_cases`, then per chunk the same
                 right-hand sides and the same substitution, and `trs_loss_apply` - the yardstick: the difference is the
                 new kernel against `trs_loss_apply` (and the one `solve_cases`)
`--only` runs one of the two (for a `rocprofv3 --kernel-trace --stats` run of its own, which gives the split between the
three kernels of a chunk).
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
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--chunk", type=int, default=64)
ap.add_argument("--joints", type=int, default=32)
ap.add_argument("--only", choices=["influence", "loss"], default=None)
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
    return statistics.median(ts), min(ts), max(ts)


def leg_path(data, count):
    """Joint ids climbing one leg: from the lowest support along members, each time to the higher neighbour whose
    horizontal distance from the current joint is smallest; at the top, on downwards in the same way."""
    xyz = np.array([j[0] for j in data["joint"]], dtype=float)
    near = [[] for _ in xyz]
    for (j0, j1), _section in data["member"]:
        near[j0].append(j1)
        near[j1].append(j0)
    at = min((j for j, (_x, s) in enumerate(data["joint"]) if s != "NO"), key=lambda j: tuple(xyz[j][::-1]))
    path, sign = [at], 1.0
    while len(path) < count:
        ahead = [j for j in near[at] if sign * (xyz[j, 2] - xyz[at, 2]) > 1e-9 and j not in path[-2:]]
        if not ahead and sign > 0:
            sign = -1.0          # over the top: down the next leg
            continue
        if not ahead:
            break
        at = min(ahead, key=lambda j: (np.hypot(*(xyz[j, :2] - xyz[at, :2])), j))
        path.append(at)
    return path


with open(os.path.join(ROOT, "tests", "golden", "data", "bar-942_input_0.json")) as fh:
    data = json.load(fh)
packed = batch.pack_json([data]).replicate(args.copies)
dev = torch.device("cuda:0")
db = batch.DeviceBatch(packed, dev, use_small=False, reorder="device")
db.factor()
B, nM = int(db.B), int(packed.nM_max)
path = leg_path(data, args.joints)
train = [(1.0, 0.0), (1.0, 150.0), (0.5, 400.0)]
summary = {"shape": f"bar-942 x {args.copies}", "B": B, "nM": nM, "chunk": args.chunk, "path_joints": len(path),
           "axles": len(train), "reps": args.reps, "statistic": "median (min, max) of event-timed repeats"}
if args.only != "loss":
    call = (torch.tensor([path], dtype=torch.int32, device=dev).expand(B, -1).contiguous(),
            torch.full([B], len(path), dtype=torch.int32, device=dev),
            torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float64, device=dev).expand(B, -1).contiguous(),
            torch.tensor([w for w, _o in train], dtype=torch.float64, device=dev),
            torch.tensor([o for _w, o in train], dtype=torch.float64, device=dev))
    out = db.influence(*call, chunk=args.chunk)
    ms = timed(lambda: db.influence(*call, chunk=args.chunk, out=out), args.reps, args.warmup)
    summary.update(influence_ms=[round(x, 2) for x in ms], lines_per_s=round(B * nM / (ms[0] * 1e-3)),
                   N_max_of_member_0=float(out["N_max"][0, 0].item()), info_any=bool(db.info.any().item()))
if args.only != "influence":
    loads = torch.from_numpy(np.random.default_rng(942).uniform(-3e4, 3e4, size=(1, 1, packed.nJ_max, 3))).to(dev)
    loads = loads.expand(B, -1, -1, -1).contiguous()
    kept = db.member_loss(loads, chunk=args.chunk)
    ms = timed(lambda: db.member_loss(loads, chunk=args.chunk, out=kept), args.reps, args.warmup)
    summary.update(loss_ms=[round(x, 2) for x in ms])
print(json.dumps(summary))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(summary, fh, indent=1)
