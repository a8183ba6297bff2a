"""CPU suite of the closed-loop rollout (emp_vehicle_step, emp_rollout): the header declares both calls and emp_vehicle_params,
the ctypes VehicleParams has the C layout (a g++ probe prints sizeof / offsetof), the binding lists both prototypes, and the
vehicle model of csrc/emp_control_core.h - compiled with g++ - agrees with tests/vehicle_port.py: bit for bit where only
+ - * / are involved (Vy, fi_dot, Vx), to 1e-12 relative where libm's sin / cos enter (the pose).  The invariants at the end
follow from the model's definition alone."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "emplanner.h")
SRC = os.path.join(ROOT, "tests", "host_check", "vehicle_check.cpp")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vehicle_port as vp  # noqa: E402

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is needed to compile the host programs")


def test_header_declares_the_vehicle_model_and_the_rollout():
    text = open(HEADER).read()
    assert re.search(r"#define EMP_ABI_VERSION 13\b", text)                      # additions do not bump the version
    assert "typedef struct emp_vehicle_params" in text and "} emp_vehicle_params;" in text
    assert re.search(r"void emp_vehicle_params_default\(", text)
    assert re.search(r"int emp_vehicle_step\(", text) and re.search(r"int emp_rollout\(", text)
    assert "THE MODEL IS THIS PROJECT'S DEFINITION, NOT THE REFERENCE'S" in text
    from emplanner_carla_amd import _lib
    assert _lib.ABI_VERSION == 13
    for name in ("emp_vehicle_params_default", "emp_vehicle_step", "emp_rollout"):
        assert name in _lib.PROTOTYPES, name
    assert len(_lib.PROTOTYPES["emp_rollout"][1]) == 27 and len(_lib.PROTOTYPES["emp_vehicle_step"][1]) == 10


@needs_gxx
def test_vehicle_params_ctypes_layout_matches_the_c_struct(tmp_path):
    from emplanner_carla_amd import _lib
    fields = [name for name, _ in _lib.VehicleParams._fields_]
    assert fields == ["a", "b", "Cf", "Cr", "m", "Iz", "dt", "steer_gain", "throttle_accel", "brake_decel", "drag", "reserved"]
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "emplanner.h"\nint main() {\n'
                   '    std::printf("sizeof %zu\\n", sizeof(emp_vehicle_params));\n'
                   + "".join(f'    std::printf("{f} %zu\\n", offsetof(emp_vehicle_params, {f}));\n' for f in fields)
                   + "    return 0;\n}\n")
    exe = tmp_path / "probe"
    r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
               if line)
    assert int(got["sizeof"]) == C.sizeof(_lib.VehicleParams)
    for f in fields:
        assert int(got[f]) == getattr(_lib.VehicleParams, f).offset, f


def test_python_defaults_are_the_issue_s():
    from emplanner_carla_amd import api
    p = api.vehicle_params()
    assert (p.a, p.b, p.Cf, p.Cr, p.m, p.Iz) == (1.015, 2.910 - 1.015, 1412.0, -148970.0, -82204.0, 1537.0)
    assert (p.dt, p.steer_gain, p.throttle_accel, p.brake_decel, p.drag, p.reserved) == (0.01, 1.0, 3.0, 6.0, 0.0, 0)
    assert vp.params() == (p.a, p.b, p.Cf, p.Cr, p.m, p.Iz, p.dt, p.steer_gain, p.throttle_accel, p.brake_decel, p.drag)
    for name in ("vehicle_step", "rollout"):
        assert callable(getattr(api.Planner, name))
    assert [f for f in api.RolloutResult.__dataclass_fields__] == ["state", "min_index", "err", "n_err", "status", "fail_tick",
                                                                   "log_state", "log_control", "log_err", "log_index"]


@pytest.fixture(scope="module")
def vc(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is needed to compile the host programs")
    out = str(tmp_path_factory.mktemp("vehicle_check") / "libvehiclecheck.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", SRC, "-o", out], check=True)
    lib = C.CDLL(out)
    lib.vc_step.restype = None
    lib.vc_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def core_step(vc, prm, state, control, ctl=False):
    prm = np.ascontiguousarray(prm, np.float64)
    state = np.ascontiguousarray(np.atleast_2d(state), np.float64)
    control = np.ascontiguousarray(np.atleast_2d(control), np.float64)
    out = np.full_like(state, np.nan)
    co = np.full((len(state), 3), np.nan)
    vc.vc_step(prm.ctypes.data, len(state), state.ctypes.data, control.ctypes.data, out.ctypes.data, co.ctypes.data if ctl else None)
    return (out, co) if ctl else out


def random_states(n, seed):
    """Speeds from standstill through the clamp to motorway pace; every control within its range."""
    rng = np.random.default_rng(seed)
    vx = rng.choice([0.0, 0.001, 0.004, 0.5, 5.0, 20.0, 35.0], n) * rng.uniform(0.5, 1.0, n)
    st = np.column_stack([rng.uniform(-100, 100, n), rng.uniform(-100, 100, n), rng.uniform(-4, 4, n), rng.normal(0, 0.5, n),
                          rng.normal(0, 0.3, n), vx])
    ct = np.column_stack([rng.uniform(0, 1, n), rng.uniform(-1, 1, n), rng.choice([0.0, 1.0], n)])
    return st, ct


def test_vehicle_core_matches_the_port_on_1000_random_states(vc):
    st, ct = random_states(1000, 7)
    for prm in (vp.params(), vp.params(drag=0.05, steer_gain=0.6, dt=0.02)):
        got, gc = core_step(vc, prm, st, ct, ctl=True)
        want = np.array([vp.step(prm, st[i], ct[i]) for i in range(len(st))])
        assert np.isfinite(got).all()
        assert np.array_equal(got[:, 3:], want[:, 3:])                        # Vy+, fi_dot+, Vx+: bit for bit
        assert np.all(np.abs(got[:, :3] - want[:, :3]) <= 1e-12 * np.maximum(1.0, np.abs(want[:, :3])))   # the pose: libm
        assert np.array_equal(gc[:, 0], [vp.clamp_vx(v) for v in want[:, 5]])
        assert np.array_equal(gc[:, 1], [vp.speed_kmh(want[i, 5], want[i, 3]) for i in range(len(st))])
    alias = st.copy()
    vc.vc_step(np.array(vp.params()).ctypes.data, len(st), alias.ctypes.data, ct.ctypes.data, alias.ctypes.data, None)
    assert np.array_equal(alias, core_step(vc, vp.params(), st, ct))


def test_zero_steer_on_the_axis_stays_on_the_axis(vc):
    s = np.array([[3.0, 0.0, 0.0, 0.0, 0.0, 12.0]])
    for _ in range(500):
        s = core_step(vc, vp.params(), s, [[0.4, 0.0, 0.0]])
        assert s[0, 1] == 0.0 and s[0, 2] == 0.0 and s[0, 3] == 0.0 and s[0, 4] == 0.0
    assert s[0, 0] > 3.0


def test_full_throttle_is_the_repeated_sum(vc):
    prm = vp.params()
    s = np.array([[0.0, 0.0, 0.3, 0.0, 0.0, 2.0]])
    v = 2.0
    for _ in range(400):
        s = core_step(vc, prm, s, [[1.0, 0.0, 0.0]])
        v = v + 0.01 * ((3.0 * 1.0 - 6.0 * 0.0) - 0.0 * v)
        assert s[0, 5] == v


def test_full_brake_never_reverses_and_standstill_is_finite(vc):
    s = np.array([[0.0, 0.0, -1.0, 0.2, 0.1, 1.0]])
    seen_zero = False
    for _ in range(60):
        s = core_step(vc, vp.params(), s, [[0.0, 0.5, 1.0]])
        assert s[0, 5] >= 0.0 and np.isfinite(s).all()
        seen_zero |= s[0, 5] == 0.0
    assert seen_zero
    still = core_step(vc, vp.params(), [[1.0, 2.0, 0.5, 0.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    assert np.isfinite(still).all() and still[0, 5] == 0.0
    assert np.isfinite(core_step(vc, vp.params(), [[1.0, 2.0, 0.5, 0.3, -0.2, 0.0]], [[0.0, -1.0, 1.0]])).all()
