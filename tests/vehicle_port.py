"""Python-float port of the project's vehicle model (csrc/emp_control_core.h: ctl::vehicle_step, the arithmetic of
emp_vehicle_step and emp_rollout), operation by operation in the header's order, and the closed loop around it: the PID rule of
include/emplanner.h, the actuation of Vehicle_control.run_step and oracle/mpc_lateral.py as the lateral law.  The model is the
project's own definition (the reference's plant is CARLA); this port is what the GPU is compared with.  Test tool only: the
package never imports it."""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VEHICLE_PARA = (1.015, 2.910 - 1.015, 1412.0, -148970.0, -82204.0, 1537.0)
DEFAULTS = dict(dt=0.01, steer_gain=1.0, throttle_accel=3.0, brake_decel=6.0, drag=0.0)


def params(vehicle_para=VEHICLE_PARA, **kw):
    """The eleven doubles of emp_vehicle_params, in its order."""
    d = dict(DEFAULTS, **kw)
    return tuple(float(v) for v in vehicle_para) + tuple(float(d[k]) for k in ("dt", "steer_gain", "throttle_accel", "brake_decel",
                                                                             "drag"))


def clamp_vx(Vx):
    """cal_vehicle_info's clamp (reference controller.py:106-109)."""
    if Vx < 0:
        return -max(abs(Vx), 0.005)
    return max(Vx, 0.005)


def speed_kmh(Vx, Vy):
    return 3.6 * math.sqrt(Vx * Vx + Vy * Vy)


def step(prm, state, control):
    """One tick of one vehicle: state (x, y, fi, Vy, fi_dot, Vx), control (throttle, steer, brake) -> the next state."""
    a, b, Cf, Cr, m, Iz, dt, steer_gain, throttle_accel, brake_decel, drag = (float(v) for v in prm)
    x, y, fi, Vy, fi_dot, Vx = (float(v) for v in state)
    throttle, steer, brake = (float(v) for v in control)
    delta = steer_gain * steer
    ax = (throttle_accel * throttle - brake_decel * brake) - drag * Vx
    Vxc = clamp_vx(Vx)
    a11 = (Cf + Cr) / (m * Vxc)
    a12 = (a * Cf - b * Cr) / (m * Vxc) - Vxc
    a21 = (a * Cf - b * Cr) / (Iz * Vxc)
    a22 = (a * a * Cf + b * b * Cr) / (Iz * Vxc)
    bv1, bv2 = -Cf / m, -a * Cf / Iz
    h = dt / 2.0
    m11, m12, m21, m22 = h * a11, h * a12, h * a21, h * a22
    l11, l12, l21, l22 = 1.0 - m11, -m12, -m21, 1.0 - m22
    r1 = ((1.0 + m11) * Vy + m12 * fi_dot) + (dt * bv1) * delta
    r2 = (m21 * Vy + (1.0 + m22) * fi_dot) + (dt * bv2) * delta
    det = l11 * l22 - l12 * l21
    Vy_n = (r1 * l22 - l12 * r2) / det
    fd_n = (l11 * r2 - l21 * r1) / det
    c, sn = math.cos(fi), math.sin(fi)
    x_n = x + dt * (Vx * c - Vy * sn)
    y_n = y + dt * (Vx * sn + Vy * c)
    fi_n = fi + dt * fi_dot
    v = Vx + dt * ax
    Vx_n = v if v > 0.0 else 0.0
    return (x_n, y_n, fi_n, Vy_n, fd_n, Vx_n)


def pid_step(gains, speed, target, buf):
    """The rule include/emplanner.h states for emp_pid_longitudinal on a Python list `buf` (oldest first): (command, buffer)."""
    K_P, K_I, K_D, dt, thr = gains
    e = target - speed
    buf = (buf + [e])[-60:]
    integral = differential = 0.0
    if len(buf) >= 2:
        s = 0.0
        for v in buf:
            s = s + v
        integral = s * dt
        differential = (buf[-1] - buf[-2]) / dt
    if abs(e) > thr:
        integral = 0.0
        buf = []
    return (K_P * e + K_I * integral) + K_D * differential, buf


def actuate(s, acc):
    """Vehicle_control.run_step (reference controller.py:705-718): (throttle, steer, brake)."""
    steering = min(1, s) if s >= 0 else max(-1, s)
    if acc >= 0:
        return float(min(1, acc)), float(steering), 0.0
    return 0.0, float(steering), float(max(1, acc))


def closed_loop_mpc(prm, path, state, min_index, target_speed, T, gains=(1.15, 0.0, 0.0, 0.01, 1.0)):
    """T ticks of one vehicle: oracle/mpc_lateral.py's chain + the PID rule + the actuation, then `step`.  Returns per-tick
    arrays: states seen by the controller (T, 6), controls (T, 3), e_rr (T, 4), the match index (T,), and the final state."""
    from oracle import mpc_lateral as mpc
    para = tuple(float(v) for v in prm[:6])
    state = tuple(float(v) for v in state)
    buf = []
    S, U, E, I = [], [], [], []
    for _ in range(T):
        r = mpc.lateral_mpc(path, state[:5], clamp_vx(state[5]), int(min_index), para)
        min_index = r["min_index"]
        acc, buf = pid_step(gains, speed_kmh(state[5], state[3]), target_speed, buf)
        u = actuate(r["steering"], acc)
        S.append(state)
        U.append(u)
        E.append(r["e_rr"])
        I.append(min_index)
        state = step(prm, state, u)
    return np.array(S), np.array(U), np.array(E), np.array(I), np.array(state)
