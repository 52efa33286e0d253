#!/usr/bin/env python3
"""Wave-cycle shares per phase of trs_joint_order_kernel on bar-942 x 4096, effort 3, from a -DTRS_ORDER_STAMPS build:
python tools/order_stamps_bar.py <tag>   (variants/libtrs_<tag>.so)"""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from python_stable_3d_truss_analysis_amd import _capi
_capi.LIB_PATH = os.path.join(ROOT, "python_stable_3d_truss_analysis_amd", "variants", f"libtrs_{sys.argv[1]}.so")
from python_stable_3d_truss_analysis_amd import batch

lib = _capi.load()
names = ("A0 adjacency", "A1 Cuthill-McKee", "A2 barrier", "B sort", "B price pair", "B tail", "C wait at barrier",
         "C perm+reach", "C apply")
with open(os.path.join(ROOT, "tests", "golden", "data", "bar-942_input_0.json")) as fh:
    bar = batch.pack_json([json.load(fh)]).replicate(4096)
tensors = {f: torch.from_numpy(np.ascontiguousarray(getattr(bar, f))).cuda() for f in ("xyz", "conn", "cbits", "loads", "nJ", "nM")}
for _ in range(3):
    out = batch.joint_order_device(torch, tensors, effort=3)
torch.cuda.synchronize()
buf = (ctypes.c_ulonglong * 16)()
lib.trs_order_debug_stamps(buf, 1)
for _ in range(10):
    batch.joint_order_device(torch, tensors, effort=3, out=out)
torch.cuda.synchronize()
lib.trs_order_debug_stamps(buf, 1)
tot = float(sum(buf)) or 1.0
waves = 10 * 4096 * 4
print(f"{sys.argv[1]}: bar-942 x 4096 effort 3, 10 launches; clocks per wave (memtime ticks), share")
for i, n in enumerate(names):
    print(f"  {n:22s} {buf[i] / waves:10.0f}  {buf[i] / tot:.3f}")
print(f"  total {tot / waves:.0f} ticks per wave")
