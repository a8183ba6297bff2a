"""Python-float port of the agents' law (csrc/emp_agent_core.h: agt::tick, agt::pid10, agt::observe - the arithmetic of
emp_agent_observe, emp_agent_control and emp_agent_rollout), operation by operation in the order include/emplanner.h states it.
The law is the reference's LocalPlanner.run_step + VehiclePIDController.run_step (agents/navigation/) without a hazard in sight;
tests/golden/agents/ holds what those classes do on the same inputs.  Test tool only: the package never imports it.

Non-finite input goes through like any other: NaN compares false, Python's min / max keep their first argument against a NaN."""
from __future__ import annotations

import math

import numpy as np

from tests import vehicle_port

BUFFER = 10
DONE = 1
DEFAULTS = dict(lat_K_P=1.95, lat_K_I=0.05, lat_K_D=0.2, lon_K_P=1.0, lon_K_I=0.05, lon_K_D=0.0, dt=0.05, max_throttle=0.75,
                max_brake=0.3, max_steer=0.8, base_min_distance=3.0)
#: (a, b, Cf, Cr, m, Iz) in physical order: the plant the agents are driven on (api.agent_vehicle_params)
VEHICLE_PARA = (1.015, 2.910 - 1.015, -148970.0, -82204.0, 1412.0, 1537.0)


def params(**kw):
    return dict(DEFAULTS, **kw)


def vehicle_params(**kw):
    return vehicle_port.params(VEHICLE_PARA, **dict(dict(dt=0.05), **kw))


def clip1(v):
    """np.clip(v, -1.0, 1.0): a NaN passes through."""
    if v != v:
        return v
    return -1.0 if v < -1.0 else (1.0 if v > 1.0 else v)


def sqrt(v):
    """IEEE sqrt: NaN below zero, where math.sqrt raises."""
    return math.sqrt(v) if v >= 0 or v != v else math.nan


def cos(v):
    return math.cos(v) if math.isfinite(v) else math.nan


def sin(v):
    return math.sin(v) if math.isfinite(v) else math.nan


def pid(kp, ki, kd, dt, e, buf):
    """_pid_control on the list `buf` (oldest first): (clipped command, the deque after the call)."""
    buf = (buf + [e])[-BUFFER:]
    de = ie = 0.0
    if len(buf) >= 2:
        s = 0.0
        for v in buf:
            s = s + v
        de = (buf[-1] - buf[-2]) / dt
        ie = s * dt
    return clip1((kp * e + kd * de) + ki * ie), buf


def observe(state):
    """emp_agent_observe of one vehicle: ((c, s), speed_kmh, (x, y, wx, wy))."""
    x, y, fi, Vy, _, Vx = (float(v) for v in state)
    c, s = cos(fi), sin(fi)
    wx, wy = Vx * c - Vy * s, Vx * s + Vy * c
    return (c, s), 3.6 * sqrt((wx * wx + wy * wy) + 0.0), (x, y, wx, wy)


class Agent:
    """The state the law keeps for one agent."""

    def __init__(self, head=0, past_steer=0.0, lon=(), lat=()):
        self.head, self.past_steer = int(head), float(past_steer)
        self.lon, self.lat = [float(v) for v in lon][:BUFFER], [float(v) for v in lat][:BUFFER]


def tick(prm, path, n_path, x, y, c, s, speed_kmh, target_speed, ag):
    """One tick of one agent: -> dict(control=(throttle, steer, brake), status, lat_error, lon_command); `ag` is updated."""
    x, y, c, s, speed_kmh, target_speed = (float(v) for v in (x, y, c, s, speed_kmh, target_speed))
    n_path = min(max(int(n_path), 0), len(path))
    ag.head = min(max(ag.head, 0), n_path)
    min_distance = prm["base_min_distance"] + 0.5 * (speed_kmh / 3.6)
    while ag.head < n_path:
        px, py = float(path[ag.head][0]), float(path[ag.head][1])
        md = 1.0 if n_path - ag.head == 1 else min_distance
        if sqrt((x - px) * (x - px) + (y - py) * (y - py)) < md:
            ag.head += 1
        else:
            break
    if ag.head >= n_path:
        return dict(control=(0.0, 0.0, 1.0), status=DONE, lat_error=0.0, lon_command=0.0)
    acc, ag.lon = pid(prm["lon_K_P"], prm["lon_K_I"], prm["lon_K_D"], prm["dt"], target_speed - speed_kmh, ag.lon)
    px, py = float(path[ag.head][0]), float(path[ag.head][1])
    wx, wy = px - x, py - y
    nn = sqrt(wx * wx + wy * wy) * sqrt((c * c + s * s) + 0.0)
    if nn == 0.0:
        dot = 1.0
    else:
        dot = math.acos(clip1(((wx * c + wy * s) + 0.0) / nn))
    if c * wy - s * wx < 0.0:
        dot = -dot
    cs, ag.lat = pid(prm["lat_K_P"], prm["lat_K_I"], prm["lat_K_D"], prm["dt"], dot, ag.lat)
    if cs > ag.past_steer + 0.1:
        cs = ag.past_steer + 0.1
    elif cs < ag.past_steer - 0.1:
        cs = ag.past_steer - 0.1
    if cs >= 0:
        steer = min(prm["max_steer"], cs)
    else:
        steer = max(-prm["max_steer"], cs)
    if acc >= 0.0:
        throttle, brake = min(acc, prm["max_throttle"]), 0.0
    else:
        throttle, brake = 0.0, min(abs(acc), prm["max_brake"])
    ag.past_steer = steer
    return dict(control=(throttle, steer, brake), status=0, lat_error=dot, lon_command=acc)


# ---- batches: the arrays of emp_agent_control / emp_agent_rollout -----------------------------------------------------------------
def agents_of(head, past_steer, lon_err, n_lon, lat_err, n_lat):
    c = lambda n: min(max(int(n), 0), BUFFER)
    return [Agent(head[a], past_steer[a], lon_err[a][:c(n_lon[a])], lat_err[a][:c(n_lat[a])]) for a in range(len(head))]


def pack(agents, lon_err, lat_err):
    """The agent state as arrays; deque entries at and past the count are those of lon_err / lat_err (they pass through)."""
    A = len(agents)
    out = dict(head=np.array([g.head for g in agents], np.int32).reshape(A), past_steer=np.array([g.past_steer for g in agents], np.float64).reshape(A),
               lon_err=np.array(lon_err, np.float64, copy=True).reshape(A, BUFFER), lat_err=np.array(lat_err, np.float64, copy=True).reshape(A, BUFFER),
               n_lon=np.array([len(g.lon) for g in agents], np.int32).reshape(A), n_lat=np.array([len(g.lat) for g in agents], np.int32).reshape(A))
    for a, g in enumerate(agents):
        out["lon_err"][a, :len(g.lon)] = g.lon
        out["lat_err"][a, :len(g.lat)] = g.lat
    return out


def control_batch(prm, path, n_path, state, forward, speed_kmh, target_speed, head, past_steer, lon_err, n_lon, lat_err, n_lat):
    """emp_agent_control: a dict of its outputs."""
    A = len(head)
    agents = agents_of(head, past_steer, lon_err, n_lon, lat_err, n_lat)
    rows = [tick(prm, path[a], n_path[a], state[a][0], state[a][1], forward[a][0], forward[a][1], speed_kmh[a], target_speed[a], agents[a])
            for a in range(A)]
    out = pack(agents, lon_err, lat_err)
    out.update(control=np.array([r["control"] for r in rows], np.float64).reshape(A, 3), status=np.array([r["status"] for r in rows], np.int32).reshape(A),
               lat_error=np.array([r["lat_error"] for r in rows], np.float64).reshape(A),
               lon_command=np.array([r["lon_command"] for r in rows], np.float64).reshape(A))
    return out


def observe_batch(state):
    rows = [observe(s) for s in state]
    A = len(rows)
    return dict(forward=np.array([r[0] for r in rows], np.float64).reshape(A, 2), speed_kmh=np.array([r[1] for r in rows], np.float64).reshape(A),
                actors=np.array([r[2] for r in rows], np.float64).reshape(A, 4))


def rollout(prm, vp, path, n_path, state, target_speed, ag, T):
    """T ticks of one agent on vehicle_port.step: per-tick states seen (T, 6), controls (T, 3), heads (T,), statuses (T,) and the
    final state; `ag` is updated."""
    state = tuple(float(v) for v in state)
    S, U, H, ST = [], [], [], []
    for _ in range(T):
        (c, s), kmh, _ = observe(state)
        r = tick(prm, path, n_path, state[0], state[1], c, s, kmh, target_speed, ag)
        S.append(state)
        U.append(r["control"])
        H.append(ag.head)
        ST.append(r["status"])
        state = vehicle_port.step(vp, state, r["control"])
    return np.array(S).reshape(T, 6), np.array(U).reshape(T, 3), np.array(H, np.int32), np.array(ST, np.int32), np.array(state)


def polyline_distance(xy, pts):
    """Distance of each point of pts (N, 2) to the polyline xy (M, 2)."""
    xy, pts = np.asarray(xy, np.float64), np.asarray(pts, np.float64)
    a, b = xy[:-1], xy[1:]
    ab = b - a
    den = np.maximum((ab * ab).sum(1), 1e-300)
    t = np.clip(((pts[:, None, :] - a[None]) * ab[None]).sum(2) / den[None], 0.0, 1.0)
    proj = a[None] + t[..., None] * ab[None]
    return np.sqrt(((pts[:, None, :] - proj) ** 2).sum(2)).min(1)
