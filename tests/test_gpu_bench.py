"""`bench.py` on one GPU without `--full`, `-m gpu`: the plain run measures the headline only, and `--dump-outputs`
writes what its last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(400)
def test_bench_plain_run_prints_the_headline_and_dumps_its_outputs(tmp_path):
    from oracle import truss_oracle as orc
    out_dir = tmp_path / "outputs"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--batch", "64", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    line = json.loads(lines[0])
    assert line["metric"] == "truss solves/sec (batched Solve)" and line["unit"] == "solves/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64" and line["steps"] == 3
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["info_nonzero"] == 0
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - 64) < 1e-6 * 64
    assert not {"repeats", "roofline", "stages_ms", "cube_batch", "dataset", "cpu_baseline"} & set(line)
    got = {n: np.load(out_dir / (n + ".npy")) for n in ("truss_index", "displace", "external", "internal", "info")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["truss_index"], np.arange(64.0)) and not got["info"].any()
    data = H.load_json("bar-942_input_0")
    ref = orc.solve(data)
    nJ, nM = len(data["joint"]), len(data["member"])
    for a, want in ((got["displace"][:, :nJ], ref["u"]), (got["external"][:, :nJ], ref["f_ext"]),
                    (got["internal"][:, :nM], ref["N"])):
        assert np.abs(a - want[None]).max() / np.abs(want).max() <= 1e-9
