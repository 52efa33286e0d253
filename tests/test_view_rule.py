"""The rule of csrc/trs_view.h - whatever the counts and ids of a batch hold, `TrsBatch::truss(b)` trims every count to
the arrays and hands out no index outside them - on plain host arrays: tests/view_rule.cpp is a stand-alone program
(its own `main`, no GPU call) over a well-formed batch in both member forms and over one with nJ, nM and n_free negative
and past the maxima, end joints of -1 and nJ_max, joint_out and free_index entries outside the arrays, and nJ_max == 0.
Compiled here with hipcc (the header includes the HIP runtime's); skipped where there is none."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python_stable_3d_truss_analysis_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_the_view_trims_and_clamps_on_host_arrays(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip(f"no hipcc at {HIPCC}")
    exe = str(tmp_path / "view_rule")
    built = subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", CSRC,
                            os.path.join(ROOT, "tests", "view_rule.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0 and ran.stdout.strip().endswith("view rule ok"), ran.stdout + ran.stderr
