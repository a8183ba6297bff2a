"""Python-float port of emp_drive_request (csrc/emp_drive_kernels.h: drive_request_kernel), written from the formulas of
include/emplanner.h in their order: the driver's perception (which actors matter, static or dynamic, nearest first), the planner's
30 m gate, predict_block and the pass-through fields.  One vehicle at a time, plain floats, every operation rounded separately.
This is what the GPU is compared with; tests/golden/drive/drive_request.npz holds what the reference's own functions return for the
same inputs.  Test tool only: the package never imports it.

One known difference to the reference's text: it squares with ``** 2``, which CPython hands to libm's pow; pow(x, 2) is not always
the correctly rounded product x * x (about 0.08 % of doubles differ in the last bit).  The library and this port multiply.

Non-finite input goes through like any other (IEEE: NaN compares false, sin / cos of an infinity are NaN - math.sin raises there,
hence `sin` and `cos` below); tests/drive_request_cases.py holds such vehicles."""
from __future__ import annotations

import math

import numpy as np

DEFAULTS = dict(dis_limitation=50.0, lateral_band=5.0, behind=-10.0, dynamic_speed=1.0, static_gate=30.0, pred_ts=0.2, advance_s=0.0)
TRUNCATED = 1


def params(**kw):
    return dict(DEFAULTS, **kw)


def cos(v):
    """IEEE cos: NaN for an infinite argument, where math.cos raises."""
    return math.cos(v) if math.isfinite(v) else math.nan


def sin(v):
    return math.sin(v) if math.isfinite(v) else math.nan


def world_velocity(fi, Vy, Vx):
    """Body-frame (Vx, Vy) at heading fi -> world-frame (wx, wy)."""
    c, s = cos(fi), sin(fi)
    return Vx * c - Vy * s, Vx * s + Vy * c


def measure(state, actor):
    """dis, lat, along, speed of one actor (x, y, vx, vy) seen from one vehicle: the four decision variables."""
    x, y, fi, Vy, _, Vx = (float(v) for v in state)
    ax, ay, avx, avy = (float(v) for v in actor)
    c, s = cos(fi), sin(fi)
    wx, wy = world_velocity(fi, Vy, Vx)
    dx, dy = x - ax, y - ay
    dis = math.sqrt((dx * dx + dy * dy) + 0.0)
    v1x, v1y = ax - x, ay - y
    lat = v1x * (-s) + v1y * c
    along = v1x * wx + v1y * wy
    speed = math.sqrt((avx * avx + avy * avy) + 0.0)
    return dis, lat, along, speed


def perceive(state, actors, n_act, prm=None):
    """-> (statics, dynamics): lists of (actor index, dis) and (actor index, dis, speed), nearest first, ties in index order;
    uncapped, as the reference's get_actor_from_world returns them."""
    prm = prm or DEFAULTS
    n = min(max(int(n_act), 0), len(actors))
    statics, dynamics = [], []
    for i in range(n):
        dis, lat, along, speed = measure(state, actors[i])
        if dis < prm["dis_limitation"] and -prm["lateral_band"] < lat < prm["lateral_band"] and along > prm["behind"]:
            if speed > prm["dynamic_speed"]:
                dynamics.append((i, dis, speed))
            else:
                statics.append((i, dis))
    statics.sort(key=lambda t: t[1])          # stable: equal dis keeps index order
    dynamics.sort(key=lambda t: t[1])
    return statics, dynamics


def predict(state, ts):
    """predict_block: (x, y, fi) ts seconds ahead."""
    x, y, fi, Vy, fi_dot, Vx = (float(v) for v in state)
    wx, wy = world_velocity(fi, Vy, Vx)
    V = math.sqrt((wx * wx + wy * wy) + 0.0)
    beta = math.atan2(wy, wx) - fi
    V_y = V * sin(beta)
    V_x = V * cos(beta)
    px = x + V_x * ts * cos(fi) - V_y * ts * sin(fi)
    py = y + V_y * ts * cos(fi) + V_x * ts * sin(fi)
    return px, py, fi + fi_dot * ts


def advance(actors, n_act, advance_s):
    """The actors advance_s later: the product rounded, then the sum; slots at or beyond n_act unchanged."""
    out = np.array(actors, np.float64, copy=True)
    n = min(max(int(n_act), 0), len(out))
    for i in range(n):
        out[i, 0] = float(out[i, 0]) + float(out[i, 2]) * advance_s
        out[i, 1] = float(out[i, 1]) + float(out[i, 3]) * advance_s
    return out


def request(state, accel, actors, n_act, max_obs, max_dyn, prm=None):
    """One vehicle's emp_drive_request as a dict of arrays shaped like one row of the call's outputs."""
    prm = prm or DEFAULTS
    actors = np.asarray(actors, np.float64)
    statics, dynamics = perceive(state, actors, n_act, prm)
    out = dict(static_xy=np.zeros((max_obs, 2)), static_dis=np.zeros(max_obs), dyn=np.zeros((max_dyn, 4)))
    for r, (i, dis) in enumerate(statics[:max_obs]):
        out["static_xy"][r] = actors[i, :2]
        out["static_dis"][r] = dis
    for r, (i, dis, speed) in enumerate(dynamics[:max_dyn]):
        out["dyn"][r] = (actors[i, 0], actors[i, 1], dis, speed)
    ns, nd = min(len(statics), max_obs), min(len(dynamics), max_dyn)
    out["n_static"], out["n_dyn"] = ns, nd
    out["static_idx"] = [i for i, _ in statics[:max_obs]]
    out["dyn_idx"] = [i for i, _, _ in dynamics[:max_dyn]]
    out["dyn_dis_speed"] = np.array(dynamics[0][1:] if dynamics else (math.nan, math.nan))
    out["n_obs"] = ns if ns > 0 and statics[0][1] <= prm["static_gate"] else 0
    x, y, fi, Vy, _, Vx = (float(v) for v in state)
    px, py, pfi = predict(state, prm["pred_ts"])
    out["origin_xy"] = np.array((x, y))
    out["start_xy"] = np.array((px, py))
    out["pred_fi"] = pfi
    out["start_v"] = np.array(world_velocity(fi, Vy, Vx))
    out["start_a"] = np.zeros(2) if accel is None else np.asarray(accel, np.float64).copy()
    out["req_status"] = TRUNCATED if len(statics) > max_obs or len(dynamics) > max_dyn else 0
    out["actors_next"] = advance(actors, n_act, prm["advance_s"])
    return out


def request_batch(state, accel, actors, n_act, max_obs, max_dyn, prm=None):
    """The batch form: a dict of stacked arrays (static_idx / dyn_idx stay lists of lists)."""
    rows = [request(state[b], None if accel is None else accel[b], actors[b], n_act[b], max_obs, max_dyn, prm) for b in range(len(state))]
    out = {}
    for k in rows[0]:
        out[k] = [r[k] for r in rows] if k.endswith("_idx") else np.array([r[k] for r in rows])
    return out
