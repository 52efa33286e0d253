#!/usr/bin/env python3
"""Sizing by gradient: projected gradient descent on the member areas of bar-25 at constant weight, the compliance
p . u as the objective, through `DifferentiableTruss` (forward: factor + substitution, backward: one more substitution
against the same factor - no finite differences).

    python tools/adjoint_sizing_demo.py [--steps 30] [--step 0.05] [--json]

Every step moves the areas against the gradient inside the plane of constant weight (sum rho A L), by at most `--step`
of the mean area (shrinking by 10 % per step), keeps them above a tenth of the smallest starting area and rescales them
to the starting weight.  Prints the compliance and the weight before the first and after every step.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from python_stable_3d_truss_analysis_amd import DifferentiableTruss, batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--step", type=float, default=0.05)
ap.add_argument("--json", action="store_true", help="one JSON line with the whole history instead of a table")
args = ap.parse_args()

with open(os.path.join(ROOT, "tests", "golden", "data", "bar-25_input_0.json")) as fh:
    packed = batch.pack_json([json.load(fh)])
dt = DifferentiableTruss(packed, "cuda:0")
loads = torch.from_numpy(packed.loads[:, None].copy()).to(dt.device)          # one load case: the truss's own
ends = packed.xyz[0][packed.conn[0, :, 1]] - packed.xyz[0][packed.conn[0, :, 0]]
w = torch.from_numpy(packed.rho * np.sqrt((ends * ends).sum(1))[None, :]).to(dt.device)   # weight per unit area
A = dt.A.clone()
weight0, floor = float((w * A).sum()), 0.1 * float(A.min())


def compliance_and_gradient(A):
    A = A.clone().requires_grad_()
    u, _, _ = dt.solve(dt.xyz, A, dt.E, loads)
    c = (u * loads).sum()
    c.backward()
    return float(c), A.grad


history = {"compliance": [], "weight": []}
for it in range(args.steps + 1):
    c, g = compliance_and_gradient(A)
    history["compliance"].append(c)
    history["weight"].append(float((w * A).sum()))
    if it == args.steps:
        break
    d = -(g - (g * w).sum() / (w * w).sum() * w)                # descent direction inside the plane of constant weight
    A = A + args.step * 0.9 ** it * float(A.mean()) / float(d.abs().max()) * d
    A = A.clamp_min(floor)
    A = A * (weight0 / float((w * A).sum()))
if args.json:
    print(json.dumps(history))
else:
    for it, (c, wt) in enumerate(zip(history["compliance"], history["weight"])):
        print(f"step {it:3d}  compliance {c:.6e}  weight {wt:.6e}")
