#!/usr/bin/env python3
"""trs_joint_order on bar-942 x 4096, effort 3: variant builds of the library interleaved in one process (kernel alone).
20 launches back to back per round, 10 rounds each, every output compared bit for bit with the first variant's.
    python tools/order_kernel_ab.py [tag ...]     variants/libtrs_<tag>.so; default: parent new
(a variant that differs in order.hip only: compile that file and link it with the product build's other objects)"""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from python_stable_3d_truss_analysis_amd import _capi, batch

VAR = os.path.join(ROOT, "python_stable_3d_truss_analysis_amd", "variants")
libs = {}
TAGS = tuple(sys.argv[1:]) or ("parent", "new")
for tag in TAGS:
    lib = ctypes.CDLL(os.path.join(VAR, f"libtrs_{tag}.so"))
    for name, (restype, argtypes) in _capi.SIGNATURES.items():
        fn = getattr(lib, name); fn.restype, fn.argtypes = restype, argtypes
    libs[tag] = lib
_capi.load()
with open(os.path.join(ROOT, "tests", "golden", "data", "bar-942_input_0.json")) as fh:
    bar = batch.pack_json([json.load(fh)]).replicate(4096)
raw = {f: torch.from_numpy(np.ascontiguousarray(getattr(bar, f))).cuda() for f in batch.DeviceBatch.INPUT_FIELDS}
outs = {tag: None for tag in libs}


def run(tag, n):
    keep, _capi._lib = _capi._lib, libs[tag]
    try:
        for _ in range(n):
            outs[tag] = batch.joint_order_device(torch, raw, effort=3, out=outs[tag])
    finally:
        _capi._lib = keep


for tag in libs:
    run(tag, 3)
torch.cuda.synchronize()
for tag in TAGS[1:]:
    same = all(torch.equal(outs[TAGS[0]][k].view(torch.uint8), outs[tag][k].view(torch.uint8))
               for k in ("perm", "reach", "xyz", "conn", "cbits", "loads"))
    print(f"{tag} against {TAGS[0]}: outputs bitwise equal: {same}")
times = {tag: [] for tag in libs}
for rnd in range(10):
    for tag in libs:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(tag, 20); e1.record(); torch.cuda.synchronize()
        times[tag].append(e0.elapsed_time(e1) / 20)
for tag, ts in times.items():
    print(f"{tag:8s} median {np.median(ts):.4f} ms  min {min(ts):.4f}  max {max(ts):.4f}  (20 launches back to back, 10 rounds interleaved)")
    print("   rounds: " + " ".join(f"{t:.4f}" for t in ts))
