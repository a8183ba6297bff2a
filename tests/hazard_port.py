"""Python-float port of the hazard rule (csrc/emp_hazard_core.h: hz::behave - the arithmetic of emp_agent_behave_hazards and
emp_traffic_rollout_hazards), operation by operation in the order include/emplanner.h states it: red lights with the sticky
_last_traffic_light, walkers with the 10 m filter and the 60 degree cone, then tests/behavior_port.behave unchanged.
tests/golden/hazards/ holds what the reference's class did on the same inputs.  Test tool only: the package never imports it."""
from __future__ import annotations

import math

import numpy as np

from tests import agent_port as ap
from tests import behavior_port as bp
from tests import vehicle_port

HZ_NONE, HZ_LIGHT, HZ_WALKER, HZ_VEHICLE = range(4)              # EMP_HZ_*
MAX_HAZARD = 64
INF = math.inf
PARAMS = dict(tlight_threshold=5.0, tlight_up_angle=90.0, walker_radius=10.0, walker_up_angle=60.0)
FIELDS = ("tlight_threshold", "tlight_up_angle", "walker_radius", "walker_up_angle")


def params(**kw):
    return dict(PARAMS, **kw)


def is_red(cycle, k):
    period, red_from, red_to = (int(v) for v in cycle)
    return period >= 1 and red_from <= int(k) % period < red_to


def within(up_angle, th, c, s, tvx, tvy, margins=None):
    """bhv::within with the cone as an argument."""
    return bp.within(dict(up_angle=up_angle), th, c, s, tvx, tvy, margins)


def _emergency(prb, limit):
    return dict(control=(0.0, 0.0, prb["emergency_brake"]), status=0, lat_error=0.0, lon_command=0.0, mode=bp.EMERGENCY, blocker=-1,
                distance=INF, ttc=INF, target=limit)


def light_scan(hp, path, lane, n_path, head, x, y, c, s, lights, k, last_light, margins=None, notes=None, ego=None):
    """-> (hit, last_light).  lights: rows of (x, y, dx, dy, key, period, red_from, red_to).  ego: (key, vex, vey) of another lane
    waypoint than the rule's stand-ins (the fixtures' generator compares the two)."""
    if not 0 <= last_light < len(lights):
        last_light = -1
    if last_light >= 0:
        if is_red(lights[last_light][5:8], k):
            if notes is not None:
                notes.append("sticky")
            return last_light, last_light
        last_light = -1
    at = max(head - 1, 0)
    key_cur = int(lane[at])
    vex = vey = 0.0
    if n_path >= 2:
        i0 = min(at, n_path - 2)
        vex = float(path[i0 + 1][0]) - float(path[i0][0])
        vey = float(path[i0 + 1][1]) - float(path[i0][1])
    if ego is not None:
        key_cur, vex, vey = ego
    hit = -1
    for q, row in enumerate(lights):
        lx, ly, dx, dy = (float(v) for v in row[:4])
        key = int(row[4])
        if hit >= 0 or key < 0 or key != key_cur:
            continue
        dot = vex * dx + vey * dy
        if margins is not None and dot != 0.0:
            margins.append(abs(dot))
        if dot < 0.0:
            continue
        if not is_red(row[5:8], k):
            continue
        if within(hp["tlight_up_angle"], hp["tlight_threshold"], c, s, lx - x, ly - y, margins):
            hit = q
    return hit, (hit if hit >= 0 else last_light)


def walker_scan(hp, prb, path, lane, n_path, head, x, y, c, s, limit, extent, walkers, tau, margins=None, notes=None, ego=None):
    """-> (hit, d).  walkers: rows of (x, y, vx, vy, extent, key).  ego: (key_cur, px, py) of another lane waypoint than the rule's."""
    at = max(head - 1, 0)
    px, py = float(path[at][0]), float(path[at][1])
    th = bp.pymax(prb["min_proximity_threshold"], limit / 3.0)
    key_cur = int(lane[at])
    key_next = int(lane[max(min(head + int(prb["look_steps"]), n_path - 1), 0)])
    if ego is not None:
        key_cur, px, py = ego
    hit, hrow = -1, None
    for q, row in enumerate(walkers):
        wx0, wy0, vx, vy, ext = (float(v) for v in row[:5])
        key = int(row[5])
        wx, wy = wx0 + vx * tau, wy0 + vy * tau
        ex, ey = wx - px, wy - py
        if hit >= 0:
            continue
        r = ap.sqrt((ex * ex + ey * ey) + 0.0)
        if margins is not None:
            margins.append(abs(r - hp["walker_radius"]))
        if not r < hp["walker_radius"]:
            if notes is not None and key >= 0 and key in (key_cur, key_next) and \
                    within(hp["walker_up_angle"], th, c, s, wx - x, wy - y):
                notes.append("filter")
            continue
        if key < 0 or (key != key_cur and key != key_next):
            continue
        if within(hp["walker_up_angle"], th, c, s, wx - x, wy - y, margins):
            hit, hrow = q, (wx, wy, ext)
    if hit < 0:
        return -1, INF
    dx, dy = x - hrow[0], y - hrow[1]
    return hit, ((ap.sqrt((dx * dx + dy * dy) + 0.0) + bp.EPS) - hrow[2]) - extent


def behave(prm, prb, hp, path, lane, n_path, x, y, c, s, kmh, limit, extent, cands, lights, walkers, k, ag, last_light, margins=None,
           notes=None, geo=None):
    """One tick of one agent at tick index k.  -> behavior_port.behave's dict plus cause, light_hit, walker_hit, walker_distance,
    last_light; `ag` is updated.  notes: a list that takes "sticky", "ignored", "filter" as the branches are met.  geo: (key, x, y,
    forward x, forward y) of another lane waypoint for the ego than the rule's stand-ins (the fixtures' generator compares the rule
    with a geometric lookup)."""
    x, y, c, s, kmh, limit, extent = (float(v) for v in (x, y, c, s, kmh, limit, extent))
    n_path = min(max(int(n_path), 0), len(path))
    ag.head = min(max(ag.head, 0), n_path)
    extra = dict(cause=HZ_NONE, light_hit=-1, walker_hit=-1, walker_distance=INF, last_light=int(last_light))
    if ag.head < n_path:
        tau = float(k) * prm["dt"]
        hit, last = light_scan(hp, path, lane, n_path, ag.head, x, y, c, s, lights, k, int(last_light), margins, notes,
                               None if geo is None else (geo[0], geo[3], geo[4]))
        extra.update(light_hit=hit, last_light=last)
        if hit >= 0:
            return dict(_emergency(prb, limit), **dict(extra, cause=HZ_LIGHT))
        wh, d = walker_scan(hp, prb, path, lane, n_path, ag.head, x, y, c, s, limit, extent, walkers, tau, margins, notes,
                            None if geo is None else geo[:3])
        extra.update(walker_hit=wh, walker_distance=d)
        if wh >= 0:
            if margins is not None:
                margins.append(abs(d - prb["braking_distance"]))
            if d < prb["braking_distance"]:
                return dict(_emergency(prb, limit), **dict(extra, cause=HZ_WALKER))
            if notes is not None:
                notes.append("ignored")
    r = bp.behave(prm, prb, path, lane, n_path, x, y, c, s, kmh, limit, extent, cands, ag, margins, None if geo is None else geo[0])
    if r["mode"] == bp.EMERGENCY:
        extra["cause"] = HZ_VEHICLE
    return dict(r, **extra)


def light_rows(w):
    n = min(max(int(w.get("n_light", 0)), 0), len(w["light"]))
    return [tuple(w["light"][q]) + (int(w["light_lane"][q]),) + tuple(int(v) for v in w["light_cycle"][q]) for q in range(n)]


def walker_rows(w):
    n = min(max(int(w.get("n_walker", 0)), 0), len(w["walker"]))
    return [tuple(w["walker"][q]) + (int(w["walker_lane"][q]),) for q in range(n)]


def world_tick(prm, prb, hp, w, agents, last_light, tick, margins=None, notes=None):
    """One synchronous tick of one world: behavior_port.world_tick's dict plus light (L, 4), light_lane, light_cycle (L, 3), n_light,
    walker (K, 5), walker_lane, n_walker.  last_light: a list, updated."""
    n = len(agents)
    tau = float(tick) * prm["dt"]
    pub = [(float(w["state"][j][0]), float(w["state"][j][1]), float(w["speed_kmh"][j]), float(w["extent"][j]),
            bp.lane_key(w["lane"][j], w["n_path"][j], agents[j].head)) for j in range(n)]
    oth = [bp.other_at(w["other"][o], tau) + (int(w["other_lane"][o]),) for o in range(len(w["other"]))]
    lights, walkers = light_rows(w), walker_rows(w)
    rows = []
    for i in range(n):
        r = behave(prm, prb, hp, w["path"][i], w["lane"][i], w["n_path"][i], w["state"][i][0], w["state"][i][1], w["forward"][i][0],
                   w["forward"][i][1], w["speed_kmh"][i], w["speed_limit"][i], w["extent"][i], pub[:i] + pub[i + 1:] + oth, lights, walkers,
                   int(tick), agents[i], last_light[i], margins[i] if margins is not None else None,
                   notes[i] if notes is not None else None)
        last_light[i] = r["last_light"]
        rows.append(r)
    return rows


def rollout(prm, prb, hp, vp, w, agents, last_light, T, tick0=0):
    """T ticks of [observe, world_tick, vehicle_port.step] of one world from w["state"]: per-tick arrays and the final state (n, 6);
    the agents and last_light are updated."""
    n = len(agents)
    state = [tuple(float(v) for v in s) for s in w["state"]]
    keys = ("control", "mode", "target", "distance", "status", "cause", "light_hit", "walker_hit", "walker_distance", "last_light")
    log = {k: [] for k in ("state", "head") + keys}
    for t in range(T):
        obs = [ap.observe(s) for s in state]
        wt = dict(w, state=state, forward=[o[0] for o in obs], speed_kmh=[o[1] for o in obs])
        rows = world_tick(prm, prb, hp, wt, agents, last_light, tick0 + t)
        log["state"].append(state)
        log["head"].append([g.head for g in agents])
        for k in keys:
            log[k].append([r[k] for r in rows])
        state = [vehicle_port.step(vp, state[i], rows[i]["control"]) for i in range(n)]
    ints = ("head", "mode", "status", "cause", "light_hit", "walker_hit", "last_light")
    out = {k: np.array(v, np.int32 if k in ints else np.float64) for k, v in log.items()}
    out["state"] = out["state"].reshape(T, n, 6)
    out["control"] = out["control"].reshape(T, n, 3)
    out["end"] = np.array(state, np.float64).reshape(n, 6)
    return out
