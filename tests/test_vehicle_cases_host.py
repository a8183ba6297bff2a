"""CPU suite of the vehicle model on hard input (tests/vehicle_cases.py): the g++ build of ctl::vehicle_step
(tests/host_check/vehicle_check.cpp, the program tests/test_rollout_host.py drives) against tests/vehicle_port.py on every case
under every parameter set, BIT FOR BIT with NaN matching NaN - the pose included: both sides call the host's libm - and the
properties the header states: the model does not reverse, a NaN speed steps to 0, and v = 0 exactly gives +0.0."""
from __future__ import annotations

import ctypes as C
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_check", "vehicle_check.cpp")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vehicle_cases as V  # noqa: E402
import vehicle_port as vp  # noqa: E402


@pytest.fixture(scope="module")
def vc(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is needed to compile the host programs")
    out = str(tmp_path_factory.mktemp("vehicle_cases") / "libvehiclecheck.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", SRC, "-o", out], check=True)
    lib = C.CDLL(out)
    lib.vc_step.restype = None
    lib.vc_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def core_step(vc, prm, state, control):
    prm = np.ascontiguousarray(prm, np.float64)
    state, control = np.ascontiguousarray(state, np.float64), np.ascontiguousarray(control, np.float64)
    out, co = np.full_like(state, 7.0), np.full((len(state), 3), 7.0)
    vc.vc_step(prm.ctypes.data, len(state), state.ctypes.data, control.ctypes.data, out.ctypes.data, co.ctypes.data)
    return out, co


def port_step(prm, state, control):
    want = np.array([vp.step(prm, state[i], control[i]) for i in range(len(state))])
    ctl = np.array([(vp.clamp_vx(w[5]), vp.speed_kmh(w[5], w[3])) for w in want])
    return want, ctl


def test_the_table_holds_what_it_says():
    t = V.table()
    names = [c["name"] for c in t]
    assert len(set(names)) == len(t) and 80 <= len(t) <= 200
    vx = [c["state"][5] for c in t]
    for v in (0.005, math.nextafter(0.005, 1.0), math.nextafter(0.005, 0.0), -0.005, -3.0, 1e-300, 60.0, math.inf):
        assert v in vx
    assert any(v == 0 and math.copysign(1, v) < 0 for v in vx) and any(v == 0 and math.copysign(1, v) > 0 for v in vx)
    assert any(math.isnan(v) for v in vx)
    for j in range(3):
        col = [c["control"][j] for c in t]
        assert any(math.isnan(v) for v in col) and math.inf in col and -math.inf in col
    assert any(c["control"][0] > 1 for c in t) and any(c["control"][0] < 0 for c in t) and any(abs(c["control"][1]) > 1 for c in t)
    assert any(c["control"][2] > 1 for c in t) and any(c["control"][2] < 0 for c in t)
    for j in range(6):
        assert any(math.isnan(c["state"][j]) for c in t), j
    assert 1e6 in [c["state"][2] for c in t]
    assert all(names[i].startswith("plain_") for i in range(1, len(t), 2))                     # ordinary neighbours everywhere


@pytest.mark.parametrize("pset", list(V.PARAM_SETS))
def test_vehicle_core_equals_the_port_bit_for_bit(vc, pset):
    prm = vp.params(**V.PARAM_SETS[pset])
    state, control = V.arrays()
    got, gc = core_step(vc, prm, state, control)
    want, wc = port_step(prm, state, control)
    for b, c in enumerate(V.table()):
        assert V.eq_nan(got[b], want[b]), (pset, c["name"], got[b], want[b])
        assert V.eq_nan(gc[b, :2], wc[b]) and gc[b, 2] == 0.0, (pset, c["name"], gc[b], wc[b])
    alias = state.copy()
    vc.vc_step(np.array(prm).ctypes.data, len(state), alias.ctypes.data, control.ctypes.data, alias.ctypes.data, None)
    assert V.eq_nan(alias, got)


def test_what_the_model_returns_at_rest_in_reverse_and_on_nan(vc):
    by = {c["name"]: b for b, c in enumerate(V.table())}
    state, control = V.arrays()
    for pset, kw in V.PARAM_SETS.items():
        got, gc = core_step(vc, vp.params(**kw), state, control)
        vx = got[:, 5]
        assert not np.isnan(vx).any() and (vx >= 0.0).all() and not np.signbit(vx[vx == 0.0]).any(), pset     # never reverses, never -0.0, never NaN
        assert vx[by["vx_nan"]] == 0.0 and vx[by["vx_nan_braking"]] == 0.0                    # a NaN speed steps to 0
        assert np.isnan(got[by["vx_nan"], :2]).all() and np.isfinite(got[by["vx_nan"], 2])     # ... its pose step is NaN, fi is not
        assert vx[by["vx_reversing"]] == 0.0 and vx[by["reversing_coasting"]] == 0.0 and vx[by["vx_n0_braking"]] == 0.0
        assert vx[by["brakes_through_zero"]] == 0.0
        assert vx[by["vx_inf"]] == 0.0                  # drag * inf is NaN (drag = 0) or ax = -inf and inf - inf: an infinite speed steps to 0 too
        assert (gc[vx == 0.0, 0] == 0.005).all()                                              # the next tick's clamped Vx
        for name in ("throttle_nan", "brake_nan"):                                            # NaN in ax: Vx+ = 0, nothing else
            assert vx[by[name]] == 0.0 and np.isfinite(got[by[name]]).all()
        assert np.isnan(got[by["steer_nan"], 3:5]).all() and np.isfinite(got[by["steer_nan"], [0, 1, 2, 5]]).all()
        if pset == "stop":
            b = by["v_exactly_zero"]
            assert state[b, 5] + 0.125 * ((3.0 * 0.0 - 4.0 * 1.0) - 0.0 * state[b, 5]) == 0.0
            assert vx[b] == 0.0 and not np.signbit(vx[b])
        if pset == "drag":
            assert (-3.0) + 0.01 * ((0.0 - 0.0) - 0.05 * -3.0) < 0.0 and vx[by["reversing_coasting"]] == 0.0
