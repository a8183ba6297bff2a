"""The banded Cholesky sweeps and substitutions of the path QP and the smoothing QP, on their own: tools/qp_rows_test.hip (R rows
per lane, emp_qp_rows.h, half bandwidth 3 and 2) and tools/qp_group_test.hip (one row per lane, emp_qp_wave.h, the two-problem
form included) solve random SPD band systems - problems of 0, 1, 2, KD rows and a full group side by side in one wavefront - and
compare with the scalar band_chol / band_solve of emp_qp_core.h: relative error below 1e-11, no NaN in a factor entry outside a
problem.  A copy of the sweep that drifts shows in no parity test until two problems of unlike size share a wavefront.
tools/qp_box_test.hip calls the interior-point fallback of the smoothing QP (box_qp_lanes<32> and smooth_pair_lanes), which no scene
reaches behind the active-set solver, and holds it against the scalar solver on the host (its header lists cases and checks)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flags(source):
    """the hipcc line of the tool's header comment, without the compiler, the source and the output"""
    with open(source) as f:
        line = next(l for l in f if re.match(r"//\s+hipcc ", l))
    words = line.split()[2:]
    words = words[:words.index("-o")]
    words.remove(os.path.relpath(source, ROOT))
    return [("-I" + os.path.join(ROOT, w[2:])) if w.startswith("-I") else w for w in words]


@pytest.mark.gpu
@pytest.mark.parametrize("tool", ["qp_rows_test", "qp_group_test", "qp_box_test"])
def test_band_solver_tool(tool, tmp_path):
    source = os.path.join(ROOT, "tools", tool + ".hip")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / tool)
    build = subprocess.run([hipcc] + _flags(source) + [source, "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and "all ok" in run.stdout, run.stdout + run.stderr
