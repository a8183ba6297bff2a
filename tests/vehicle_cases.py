"""Case table of the hard-input tests of the vehicle model (ctl::vehicle_step: emp_vehicle_step, emp_rollout):
tests/test_vehicle_cases_host.py runs it through the g++ build of the core, tests/test_gpu_vehicle_cases.py through the device
build, both against tests/vehicle_port.py.  A plain helper module: no fixtures, no hooks.  Each case is one vehicle: state[6] = x, y,
fi, Vy, fi_dot, Vx and control[3] = throttle, steer, brake; every case runs under every parameter set of PARAM_SETS.

What the cases hold: Vx at +0, -0.0, on the clamp 0.005 and one ulp to either side, -0.005, reversing, 1e-300, 60 m/s, inf and NaN; a
vehicle that brakes through zero and one whose v = Vx + dt * ax is EXACTLY 0 under the `stop` parameters (0.5 + 0.125 * -4: the
result is +0.0); controls outside [0, 1] and [-1, 1]; NaN and +-inf in each control; NaN in each state field; fi = 1e6; drag on a
reversing vehicle (the `drag` parameters); and random ordinary vehicles between them."""
from __future__ import annotations

import functools
import math

import numpy as np

NAN, INF = math.nan, math.inf
PARAM_SETS = {"default": {}, "stop": dict(dt=0.125, brake_decel=4.0), "drag": dict(drag=0.05, steer_gain=0.6)}
BASE_STATE = (3.0, -2.0, 0.4, 0.2, 0.05, 8.0)
BASE_CONTROL = (0.3, 0.1, 0.0)
CLAMP = 0.005
VX_VALUES = (("p0", 0.0), ("n0", -0.0), ("clamp", CLAMP), ("clamp_up", math.nextafter(CLAMP, INF)), ("clamp_down", math.nextafter(CLAMP, 0.0)),
             ("minus_clamp", -CLAMP), ("reversing", -3.0), ("1e-300", 1e-300), ("60", 60.0), ("inf", INF), ("nan", NAN))


def _case(name, state, control):
    return dict(name=name, state=np.array(state, np.float64), control=np.array(control, np.float64))


def _with(seq, i, v):
    out = list(seq)
    out[i] = v
    return out


@functools.lru_cache(maxsize=None)
def table():
    out = []
    for tag, v in VX_VALUES:
        out.append(_case(f"vx_{tag}", _with(BASE_STATE, 5, v), BASE_CONTROL))
        out.append(_case(f"vx_{tag}_braking", _with(BASE_STATE, 5, v), (0.0, -0.4, 1.0)))
    out.append(_case("brakes_through_zero", _with(BASE_STATE, 5, 0.02), (0.0, 0.2, 1.0)))
    out.append(_case("v_exactly_zero", _with(BASE_STATE, 5, 0.5), (0.0, 0.0, 1.0)))            # under `stop`: 0.5 + 0.125 * -4 = +0.0
    for j, c in enumerate(((1.7, 2.5, 0.0), (-0.4, -3.0, 0.0), (0.0, 0.0, -0.5), (0.2, 0.0, 1.8))):
        out.append(_case(f"controls_outside_{j}", BASE_STATE, c))
    for tag, v in (("nan", NAN), ("pinf", INF), ("ninf", -INF)):
        for j, cname in enumerate(("throttle", "steer", "brake")):
            out.append(_case(f"{cname}_{tag}", BASE_STATE, _with(BASE_CONTROL, j, v)))
    for j, sname in enumerate(("x", "y", "fi", "Vy", "fi_dot", "Vx")):
        if sname != "Vx":
            out.append(_case(f"state_{sname}_nan", _with(BASE_STATE, j, NAN), BASE_CONTROL))
    out.append(_case("fi_1e6", _with(BASE_STATE, 2, 1e6), BASE_CONTROL))
    out.append(_case("reversing_coasting", _with(BASE_STATE, 5, -3.0), (0.0, 0.0, 0.0)))         # under `drag`: ax = +0.15, still no reversing
    rng = np.random.default_rng(31)
    special, mixed = out, []
    for i, c in enumerate(special):                                                            # an ordinary vehicle after each special one
        mixed.append(c)
        mixed.append(_case(f"plain_{i}", (rng.uniform(-100, 100), rng.uniform(-100, 100), rng.uniform(-4, 4), rng.normal(0, 0.5),
                                          rng.normal(0, 0.3), rng.uniform(0.5, 35.0)),
                           (rng.uniform(0, 1), rng.uniform(-1, 1), float(rng.integers(0, 2)))))
    return tuple(mixed)


def arrays():
    t = table()
    return np.array([c["state"] for c in t]), np.array([c["control"] for c in t])


def eq_nan(a, b):
    """Bit-equal, NaN matching NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))
