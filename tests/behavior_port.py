"""Python-float port of the car-following law (csrc/emp_behavior_core.h: bhv::behave - the arithmetic of emp_agent_behave and
emp_traffic_rollout), operation by operation in the order include/emplanner.h states it.  The law is the part of the reference's
BehaviorAgent.run_step (agents/navigation/behavior_agent.py) that looks at other vehicles: the speed-limit target, the
vehicle-ahead detector, the time-to-collision rule and the emergency stop, on top of tests/agent_port.tick.
tests/golden/behavior/ holds what the reference's class did on the same inputs.  Test tool only: the package never imports it."""
from __future__ import annotations

import math

import numpy as np

from tests import agent_port as ap
from tests import vehicle_port

NORMAL, SLOW, FOLLOW, CLEAR, EMERGENCY, DONE = range(6)          # EMP_BHV_*
MAX_WORLD = 64
EPS = 2.0 ** -52
RAD_TO_DEG = 180.0 / math.pi
INF = math.inf
#: behavior_types.py plus BehaviorAgent._min_speed, BasicAgent._max_brake, the detector's cone and its look-ahead
KINDS = dict(
    cautious=dict(max_speed=40.0, speed_lim_dist=6.0, speed_decrease=12.0, safety_time=3.0, min_proximity_threshold=12.0, braking_distance=6.0),
    normal=dict(max_speed=50.0, speed_lim_dist=3.0, speed_decrease=10.0, safety_time=3.0, min_proximity_threshold=10.0, braking_distance=5.0),
    aggressive=dict(max_speed=70.0, speed_lim_dist=1.0, speed_decrease=8.0, safety_time=3.0, min_proximity_threshold=8.0, braking_distance=4.0))
COMMON = dict(min_speed=5.0, emergency_brake=0.5, up_angle=30.0, look_steps=5)
FIELDS = ("max_speed", "speed_lim_dist", "speed_decrease", "safety_time", "min_proximity_threshold", "braking_distance", "min_speed",
          "emergency_brake", "up_angle", "look_steps")


def params(kind="normal", **kw):
    return dict(dict(KINDS[kind], **COMMON), **kw)


def pymin(a, b):
    """Python's min(a, b): a unless b is strictly smaller."""
    return b if b < a else a


def pymax(a, b):
    return b if b > a else a


def lane_key(lane, n_path, head):
    """The stand-in for map.get_waypoint(location): the key of the waypoint behind the queue's head; -1 without a plan."""
    n_path = min(max(int(n_path), 0), len(lane))
    if n_path == 0:
        return -1
    head = min(max(int(head), 0), n_path)
    return int(lane[max(head - 1, 0)])


def within(bp, th, c, s, tvx, tvy, margins=None):
    """is_within_distance(target, ego, th, [0, up_angle])."""
    norm = ap.sqrt(tvx * tvx + tvy * tvy)
    if margins is not None:
        margins += [abs(norm - 0.001), abs(norm - th)]
    if norm < 0.001:
        return True
    if norm > th:
        return False
    q = ap.clip1((c * tvx + s * tvy) / norm)
    angle = (math.acos(q) if q == q else math.nan) * RAD_TO_DEG
    if margins is not None:
        margins += [abs(angle) if angle != 0.0 else INF, abs(angle - bp["up_angle"])]        # exactly 0 is no rounding matter
    return 0.0 < angle < bp["up_angle"]


def behave(prm, bp, path, lane, n_path, x, y, c, s, kmh, limit, extent, cands, ag, margins=None, key_cur=None):
    """One tick of one agent.  cands: the scan list of (x, y, km/h, extent, key).  -> dict(control, status, lat_error, lon_command,
    mode, blocker, distance, ttc, target); `ag` is updated.  margins: a list that takes |value - threshold| of every comparison made;
    key_cur: another key for the ego than the rule's (the fixtures' generator compares the rule with a geometric lookup)."""
    x, y, c, s, kmh, limit, extent = (float(v) for v in (x, y, c, s, kmh, limit, extent))
    n_path = min(max(int(n_path), 0), len(path))
    ag.head = min(max(ag.head, 0), n_path)
    none = dict(blocker=-1, distance=INF, ttc=INF)
    if ag.head == n_path:
        return dict(none, control=(0.0, 0.0, 1.0), status=ap.DONE, lat_error=0.0, lon_command=0.0, mode=DONE, target=limit)
    th = pymax(bp["min_proximity_threshold"], limit / 3.0)
    key_cur = int(lane[max(ag.head - 1, 0)]) if key_cur is None else int(key_cur)
    key_next = int(lane[max(min(ag.head + int(bp["look_steps"]), n_path - 1), 0)])
    blocker = -1
    for k, (xj, yj, _, _, key) in enumerate(cands):
        if blocker >= 0 or key < 0 or (key != key_cur and key != key_next):
            continue
        if within(bp, th, c, s, float(xj) - x, float(yj) - y, margins):
            blocker = k
    normal = pymin(bp["max_speed"], limit - bp["speed_lim_dist"])
    if blocker < 0:
        r = ap.tick(prm, path, n_path, x, y, c, s, kmh, normal, ag)
        return dict(r, **none, mode=NORMAL, target=normal)
    xj, yj, vs, ext_j, _ = (float(v) for v in cands[blocker])
    dx, dy = x - xj, y - yj
    d = ((ap.sqrt((dx * dx + dy * dy) + 0.0) + EPS) - ext_j) - extent
    if margins is not None:
        margins.append(abs(d - bp["braking_distance"]))
    if d < bp["braking_distance"]:
        return dict(control=(0.0, 0.0, bp["emergency_brake"]), status=0, lat_error=0.0, lon_command=0.0, mode=EMERGENCY, blocker=blocker,
                    distance=d, ttc=INF, target=limit)
    dv = pymax(1.0, (kmh - vs) / 3.6)
    ttc = d / dv
    if margins is not None:
        margins += [abs(ttc - bp["safety_time"]), abs(ttc - 2.0 * bp["safety_time"]), abs(ttc)]
    if bp["safety_time"] > ttc > 0.0:
        v = vs - bp["speed_decrease"]
        mode, target = SLOW, pymin(pymin(v if v > 0.0 else 0.0, bp["max_speed"]), limit - bp["speed_lim_dist"])
    elif 2.0 * bp["safety_time"] > ttc >= bp["safety_time"]:
        mode, target = FOLLOW, pymin(pymin(pymax(bp["min_speed"], vs), bp["max_speed"]), limit - bp["speed_lim_dist"])
    else:
        mode, target = CLEAR, normal
    # the reference steps its local planner in car_following_manager AND once more at the end of run_step (behavior_agent.py:275 /
    # :284 / :292, then :360): two ticks on the same observation, the second one's control is returned
    ap.tick(prm, path, n_path, x, y, c, s, kmh, target, ag)
    r = ap.tick(prm, path, n_path, x, y, c, s, kmh, target, ag)
    return dict(r, mode=mode, blocker=blocker, distance=d, ttc=ttc, target=target)


def other_at(row, tau):
    """An other (x, y, vx, vy, extent) at time tau: (x, y, km/h, extent)."""
    x, y, vx, vy, ext = (float(v) for v in row)
    return x + vx * tau, y + vy * tau, 3.6 * ap.sqrt((vx * vx + vy * vy) + 0.0), ext


def world_tick(prm, bp, w, agents, tick, margins=None):
    """One synchronous tick of one world.  w: dict(path (n, M, 4), n_path, lane (n, M), state (n, 6), forward (n, 2), speed_kmh (n,),
    speed_limit, extent, other (m, 5), other_lane (m,)) for the world's n live agents; agents: their ap.Agent.  -> list of behave's
    dicts; the agents are updated."""
    n = len(agents)
    tau = float(tick) * prm["dt"]
    pub = [(float(w["state"][j][0]), float(w["state"][j][1]), float(w["speed_kmh"][j]), float(w["extent"][j]),
            lane_key(w["lane"][j], w["n_path"][j], agents[j].head)) for j in range(n)]
    oth = [other_at(w["other"][o], tau) + (int(w["other_lane"][o]),) for o in range(len(w["other"]))]
    return [behave(prm, bp, w["path"][i], w["lane"][i], w["n_path"][i], w["state"][i][0], w["state"][i][1], w["forward"][i][0],
                   w["forward"][i][1], w["speed_kmh"][i], w["speed_limit"][i], w["extent"][i], pub[:i] + pub[i + 1:] + oth, agents[i],
                   margins[i] if margins is not None else None) for i in range(n)]


def rollout(prm, bp, vp, w, agents, T, tick0=0):
    """T ticks of [observe, world_tick, vehicle_port.step] of one world from w["state"]: dict of per-tick arrays (state seen
    (T, n, 6), control (T, n, 3), head, mode, target, distance, status) and the final state (n, 6); the agents are updated."""
    n = len(agents)
    state = [tuple(float(v) for v in s) for s in w["state"]]
    log = dict(state=[], control=[], head=[], mode=[], target=[], distance=[], status=[])
    for t in range(T):
        obs = [ap.observe(s) for s in state]
        wt = dict(w, state=state, forward=[o[0] for o in obs], speed_kmh=[o[1] for o in obs])
        rows = world_tick(prm, bp, wt, agents, tick0 + t)
        log["state"].append(state)
        log["head"].append([g.head for g in agents])
        for k, f in (("control", "control"), ("mode", "mode"), ("target", "target"), ("distance", "distance"), ("status", "status")):
            log[k].append([r[f] for r in rows])
        state = [vehicle_port.step(vp, state[i], rows[i]["control"]) for i in range(n)]
    out = {k: np.array(v, np.int32 if k in ("head", "mode", "status") else np.float64) for k, v in log.items()}
    out["state"] = out["state"].reshape(T, n, 6)
    out["control"] = out["control"].reshape(T, n, 3)
    out["end"] = np.array(state, np.float64).reshape(n, 6)
    return out
