"""CPU suite of the controller completion (Longitudinal_PID_controller, Vehicle_control, the feed-forward MPC): the PID step
and the actuation of csrc/emp_control_core.h compiled with g++ and checked bit for bit against the reference's recorded
sequences (tests/golden/control/control.npz) and Python's own min / max; the drop-in module imports, and the ``sys.modules`` swap of
INTEGRATION.md lets an unmodified driver line import Vehicle_control without cvxopt."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(ROOT, "tests", "host_check", "control_check.cpp")


@pytest.fixture(scope="module")
def cc(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("control_check") / "libcontrolcheck.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", SRC, "-o", out], check=True)
    lib = C.CDLL(out)
    d, i, p = C.c_double, C.c_int, C.c_void_p
    lib.cc_pid_step.restype = d
    lib.cc_pid_step.argtypes = [p, d, d, p, i, p, p]
    lib.cc_actuate.restype = None
    lib.cc_actuate.argtypes = [d, d, p]
    lib.cc_pid_buffer.restype = i
    return lib


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "control", "control.npz"))


def _speed_kmh(v):
    return 3.6 * math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])        # reference controller.py:647-649


def _pid_run(cc, gains, vel, target, alias):
    prm = np.array(list(gains) + [1.0], np.float64)
    buf, n = np.zeros(60), 0
    cmds, bufs, ns = [], [], []
    for k in range(len(vel)):
        out = buf if alias else np.full(60, np.nan)
        no = C.c_int(-1)
        cmds.append(cc.cc_pid_step(prm.ctypes.data, _speed_kmh(vel[k]), float(target[k]), buf.ctypes.data, n, out.ctypes.data,
                                   C.byref(no)))
        buf, n = out.copy(), no.value
        bufs.append(buf.copy())
        ns.append(n)
    return np.array(cmds), np.array(bufs), np.array(ns)


@pytest.mark.parametrize("alias", [False, True])
def test_pid_core_matches_the_reference_sequences_bit_for_bit(cc, g, alias):
    assert cc.cc_pid_buffer() == 60
    assert g["pid_gains"].shape[0] >= 4 and g["pid_command"].shape[1] >= 150
    for s in range(g["pid_gains"].shape[0]):
        cmd, buf, n = _pid_run(cc, g["pid_gains"][s], g["pid_vel"][s], g["pid_target"][s], alias)
        np.testing.assert_array_equal(n, g["pid_n_err"][s])
        np.testing.assert_array_equal(cmd, g["pid_command"][s])
        np.testing.assert_array_equal(buf, g["pid_err"][s])


def test_pid_fixture_covers_eviction_and_separation(g):
    n = g["pid_n_err"]
    assert (n == 60).sum(axis=1).min() > 5                       # full deque for a while: appends evict
    assert (np.diff(n, axis=1) < 0).any(axis=1).all()            # every sequence crosses the threshold at least once
    assert len({tuple(r) for r in g["pid_gains"]}) == g["pid_gains"].shape[0]
    assert (g["pid_gains"][:, 1] != 0).any() and (g["pid_gains"][:, 2] != 0).any() and (g["pid_gains"][:, 3] != 0.01).any()


def _py_actuation(s, acc):
    """Vehicle_control.run_step (reference :705-718) with its limits, Python's own min / max."""
    steering = min(1, s) if s >= 0 else max(-1, s)
    if acc >= 0:
        return float(min(1, acc)), float(steering), 0.0
    return 0.0, float(steering), float(max(1, acc))


def test_actuation_table_matches_python_min_max(cc):
    vals = [float("nan"), 0.0, -0.0, 1e-300, -1e-300, 0.5, -0.5, 1.0, -1.0, 1.0000000000000002, -1.0000000000000002, 3.7,
            -3.7, float("inf"), float("-inf")]
    out = np.zeros(3)
    for s in vals:
        for acc in vals:
            cc.cc_actuate(s, acc, out.ctypes.data)
            want = _py_actuation(s, acc)
            got = tuple(out)
            for w, v in zip(want, got):
                assert (math.isnan(w) and math.isnan(v)) or (w == v and math.copysign(1, w) == math.copysign(1, v)), (s, acc, want, got)
    cc.cc_actuate(float("nan"), float("nan"), out.ctypes.data)
    assert tuple(out) == (0.0, -1.0, 1.0)
    cc.cc_actuate(-0.0, -2.0, out.ctypes.data)
    assert out[0] == 0.0 and out[1] == 0.0 and math.copysign(1, out[1]) < 0 and out[2] == 1.0


def test_dropin_module_defines_the_reference_classes():
    from emplanner_carla_amd.controller import controller as c
    for name in ("Lateral_MPC_controller", "Lateral_LQR_controller", "Longitudinal_PID_controller", "Vehicle_control",
                 "Lateral_MPC__with_feedforward_controller"):
        assert isinstance(getattr(c, name), type), name
    pid = c.Longitudinal_PID_controller(None)
    assert (pid.K_P, pid.K_I, pid.K_D, pid.dt, pid.error_threshold, pid.target_speed) == (1.15, 0, 0, 0.01, 1, None)
    assert pid.error_buffer.maxlen == 60 and len(pid.error_buffer) == 0
    with pytest.raises(AttributeError):                 # the constructor reads the vehicle (reference :755-756)
        c.Lateral_MPC__with_feedforward_controller(object(), (1, 1, 1, 1, 1, 1), [])


def test_sys_modules_swap_imports_vehicle_control_without_cvxopt():
    """a driver's unmodified `from controller.controller import Vehicle_control` resolves to the drop-in."""
    code = ("import sys\n"
            "import emplanner_carla_amd.controller as ctl\n"
            "import emplanner_carla_amd.controller.controller as cc\n"
            "sys.modules['controller'] = ctl\n"
            "sys.modules['controller.controller'] = cc\n"
            "from controller.controller import Vehicle_control, Longitudinal_PID_controller\n"
            "assert Vehicle_control is cc.Vehicle_control\n"
            "assert 'cvxopt' not in sys.modules and 'carla' not in sys.modules\n"
            "vc = Vehicle_control(None, (1.015, 1.895, 1412, -148970, -82204, 1537), [(0.0, 0.0, 0.0, 0.0)], 'unknown')\n"
            "try:\n    vc.run_step(30)\nexcept AttributeError:\n    print('OK')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT,
                         env=dict(os.environ, EMP_SKIP_TORCH_PRELOAD="1"))
    assert out.stdout.strip() == "OK", out.stdout + out.stderr


def test_control_fixture_regenerates_from_the_reference_bit_for_bit(tmp_path):
    """As tests/test_reference_live.py for the fixture this file reads (that file's generator list is a yardstick)."""
    sys.path.insert(0, GOLDEN)
    import ref_loader
    if not ref_loader.reference_available():
        pytest.skip("the reference tree is not present (fixture regeneration runs only where it is)")
    env = dict(os.environ, EMP_GOLDEN_OUT=str(tmp_path), OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1")
    p = subprocess.run([sys.executable, "-B", os.path.join(GOLDEN, "make_golden_control.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    want = np.load(os.path.join(GOLDEN, "control", "control.npz"))
    got = np.load(os.path.join(str(tmp_path), "control.npz"))
    assert sorted(want.files) == sorted(got.files)
    for k in want.files:
        assert want[k].dtype == got[k].dtype and want[k].shape == got[k].shape, k
        assert np.array_equal(want[k], got[k], equal_nan=True), k
