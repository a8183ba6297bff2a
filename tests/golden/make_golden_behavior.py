"""Behaviour fixtures: the reference's ``BehaviorAgent`` ("normal", agents/navigation/behavior_agent.py), loaded through duck-typed
stubs, driving several vehicles tick by tick in closed loop on the project's vehicle model, recorded as arrays under
tests/golden/behavior/.

    python tests/golden/make_golden_behavior.py        (EMP_GOLDEN_OUT=<dir>: write to <dir>/behavior/ instead)

The scenario half of this file needs nothing but NumPy: tests rebuild a scenario from ``scenario(name)``.  The recording half
extends the stubs of make_golden_agents.py: a ``carla`` module with LaneChange / LaneType / TrafficLightState, a world with an
actor list, vehicles with an id, a speed limit and a bounding box, a stub ``GlobalRoutePlanner`` (BasicAgent builds one; nothing
here asks it for a route), and a map whose ``get_waypoint`` answers GEOMETRICALLY: the nearest waypoint of the scenario's lane
table, with its lane key as ``road_id``, lane markings that allow no lane change and no junction.  The agents are stepped one after
another between two steps of the plant, as the reference's drivers do; the plant is tests/vehicle_port.step.

Per scenario ``<name>.npz`` holds, for V vehicles (slot order = the order of the world's actor list) and T ticks,
  xy [V][M][2], lane [V][M], n_path [V], state0 [V][6], speed_limit [V], extent [V]     the plans and the vehicles
  brake_from [V]   the tick from which the vehicle is no longer driven by its agent but held at control (0, 0, 1); -1: never
  seen [T][V][5]     x, y, forward x, forward y, get_speed: what the vehicle showed in tick t
  control [T][V][3]  throttle, steer, brake
  queue [T][V]       len(_waypoints_queue) after the tick
  target [T][V]      _local_planner._target_speed after the tick
  mode [T][V]        the port's mode on the recorded inputs (tests/behavior_port.py), -1 where the vehicle is not driven
  margin [T][V]      the smallest |value - threshold| of any comparison the port made in that tick (+inf without one)
  mode_ticks [V][6]  how often each mode occurred
  state_end [V][6]
The generator refuses a scenario in which a margin is below 1e-6, or in which the geometric lane lookup and the law's own rule (the
key of the waypoint behind the queue's head) would decide a tick differently.
"""
from __future__ import annotations

import importlib
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import make_golden_agents as mk  # noqa: E402

NAMES = ("follow", "cruise", "closing", "stopped_leader", "collinear", "other_lane", "merge", "platoon4")
EXTENT = 2.4
MIN_MARGIN = 1e-6


# ---- scenarios ----------------------------------------------------------------------------------------------------------------------
def _arc(radius=100.0, length=470.0):
    return mk.polyline([("a", radius, length / radius)])


def _vehicle(xy, at, speed, limit, key=1, keys=None, lateral=0.0):
    """A vehicle standing on waypoint `at` of xy, heading along it, with the rest of xy as its plan."""
    th = math.atan2(xy[at + 1][1] - xy[at][1], xy[at + 1][0] - xy[at][0])
    plan = np.array(xy[at:], np.float64)
    lane = np.full(len(plan), key, np.int32) if keys is None else np.asarray(keys[at:], np.int32)
    return dict(xy=plan, lane=lane, state0=(float(xy[at][0]) - lateral * math.sin(th), float(xy[at][1]) + lateral * math.cos(th), th, 0.0, 0.0, float(speed)),
                speed_limit=float(limit), extent=EXTENT, brake_from=-1)


def scenario(name):
    """-> dict(vehicles=[dict(xy, lane, state0, speed_limit, extent, brake_from)], T).  Slot 0 is the follower."""
    arc = _arc()
    if name == "follow":          # 30 m behind a leader limited to 23 km/h: every branch fires
        return dict(vehicles=[_vehicle(arc, 0, 10.0, 60.0), _vehicle(arc, 15, 5.5, 23.0)], T=600)
    if name == "cruise":          # 8 m behind a leader limited to 43 km/h: the follower settles at the leader's 40 km/h
        return dict(vehicles=[_vehicle(arc, 0, 8.0, 60.0), _vehicle(arc, 4, 8.0, 43.0)], T=600)
    if name == "closing":
        return dict(vehicles=[_vehicle(arc, 0, 13.8, 60.0), _vehicle(arc, 20, 5.5, 23.0)], T=400)
    if name == "stopped_leader":  # the leader brakes for good from tick 200: the follower ends up passing through it
        v = [_vehicle(arc, 0, 10.0, 60.0), _vehicle(arc, 15, 5.5, 23.0)]
        v[1]["brake_from"] = 200
        return dict(vehicles=v, T=600)
    if name == "collinear":       # an axis-aligned straight: acos(1) = 0 and the leader is never seen
        line = mk.polyline([("s", 200)])
        return dict(vehicles=[_vehicle(line, 0, 10.0, 60.0), _vehicle(line, 15, 5.5, 23.0)], T=400)
    if name == "other_lane":      # the leader on the lane to the left, keyed otherwise
        inner = mk.polyline([("a", 96.5, 470.0 / 100.0)])
        inner = inner + np.array([0.0, 3.5])
        return dict(vehicles=[_vehicle(arc, 0, 10.0, 60.0), _vehicle(inner, 15, 5.5, 23.0, key=2)], T=400)
    if name == "merge":           # the key changes 24 m ahead of the follower, the leader stands beyond: seen once head + 5 crosses
        keys = np.where(np.arange(len(arc)) < 12, 1, 2)
        return dict(vehicles=[_vehicle(arc, 0, 3.0, 90.0, keys=keys), _vehicle(arc, 14, 3.0, 23.0, keys=keys)], T=300)
    if name == "platoon4":        # slot 1 is the FARTHER of the two vehicles the rear one sees: the first hit wins
        return dict(vehicles=[_vehicle(arc, 0, 6.0, 90.0), _vehicle(arc, 12, 6.0, 43.0), _vehicle(arc, 6, 6.0, 60.0),
                              _vehicle(arc, 18, 6.0, 33.0)], T=600)
    raise KeyError(name)


def arrays(sc):
    """The padded arrays of a scenario: xy (V, M, 2), lane (V, M), n_path, state0, speed_limit, extent, brake_from."""
    vs = sc["vehicles"]
    V, M = len(vs), max(len(v["xy"]) for v in vs)
    xy, lane = np.zeros((V, M, 2)), np.full((V, M), -1, np.int32)
    for i, v in enumerate(vs):
        xy[i, :len(v["xy"])], lane[i, :len(v["xy"])] = v["xy"], v["lane"]
    return dict(xy=xy, lane=lane, n_path=np.array([len(v["xy"]) for v in vs], np.int32), state0=np.array([v["state0"] for v in vs], np.float64),
                speed_limit=np.array([v["speed_limit"] for v in vs], np.float64), extent=np.array([v["extent"] for v in vs], np.float64),
                brake_from=np.array([v["brake_from"] for v in vs], np.int32))


# ---- the stubs and the recording ------------------------------------------------------------------------------------------------------
class _Names:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class MapWaypoint(mk.Waypoint):
    """A waypoint of a plan or of the map: the lane key is its road_id."""

    def __init__(self, location, key):
        super().__init__(location)
        self.road_id, self.lane_id, self.section_id = int(key), 1, 0
        self.is_junction = False
        self.left_lane_marking = self.right_lane_marking = _Names(lane_change="none")
        self.lane_type = "driving"

    def get_left_lane(self):
        return None

    def get_right_lane(self):
        return None


class LaneMap:
    """get_waypoint(location): the nearest waypoint of the lane table (ties: the first)."""

    def __init__(self, xy, key):
        self.xy, self.key = np.asarray(xy, np.float64).reshape(-1, 2), np.asarray(key, np.int64).reshape(-1)

    def key_at(self, x, y):
        d = (self.xy[:, 0] - x) ** 2 + (self.xy[:, 1] - y) ** 2
        return int(np.argmin(d))

    def get_waypoint(self, location):
        k = self.key_at(location.x, location.y)
        return MapWaypoint(mk.Location(self.xy[k, 0], self.xy[k, 1], 0.0), self.key[k])


class ActorList(list):
    def filter(self, pattern):
        return ActorList(a for a in self if "vehicle" in pattern)


class World:
    def __init__(self, lane_map):
        self.map, self.actors = lane_map, ActorList()

    def get_map(self):
        return self.map

    def get_actors(self):
        return self.actors


class Actor(mk.Vehicle):
    def __init__(self, world, ident, state, speed_limit, extent):
        super().__init__(state)
        self.world, self.id, self.speed_limit = world, ident, float(speed_limit)
        self.bounding_box = _Names(extent=_Names(x=float(extent), y=float(extent) / 2.4, z=0.75))

    def get_world(self):
        return self.world

    def get_speed_limit(self):
        return self.speed_limit


def load_behavior():
    """The reference's (behavior_agent, local_planner, misc) modules with this file's ``carla`` and a stub GlobalRoutePlanner."""
    import ref_loader
    if not ref_loader.reference_available():
        raise RuntimeError("reference tree not present at " + ref_loader.REFERENCE_ROOT)
    sys.dont_write_bytecode = True
    carla = types.ModuleType("carla")
    carla.Location, carla.Vector3D, carla.VehicleControl, carla.Transform = mk.Location, mk.Vector3D, mk.VehicleControl, mk.Transform
    carla.LaneChange = _Names(NONE="none", Right="right", Left="left", Both="both")
    carla.LaneType = _Names(Driving="driving")
    carla.TrafficLightState = _Names(Red="red")
    grp = types.ModuleType("agents.navigation.global_route_planner")

    class GlobalRoutePlanner:
        def __init__(self, wmap, sampling_resolution):
            self.map, self.sampling_resolution = wmap, sampling_resolution

    grp.GlobalRoutePlanner = GlobalRoutePlanner
    names = ("agents", "agents.tools", "agents.tools.misc", "agents.navigation", "agents.navigation.controller", "agents.navigation.local_planner",
             "agents.navigation.behavior_types", "agents.navigation.basic_agent", "agents.navigation.behavior_agent")
    saved = {k: sys.modules.get(k) for k in names + ("carla", grp.__name__)}
    sys.modules["carla"] = carla
    sys.path.insert(0, ref_loader.REFERENCE_ROOT)
    try:
        for k in names:
            sys.modules.pop(k, None)
        importlib.import_module("agents.navigation")
        sys.modules[grp.__name__] = grp
        mods = tuple(importlib.import_module(k) for k in ("agents.navigation.behavior_agent", "agents.navigation.local_planner", "agents.tools.misc"))
    finally:
        sys.path.remove(ref_loader.REFERENCE_ROOT)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mods


def record(name, mods=None):
    """Drive scenario `name` with the reference's BehaviorAgent: the dict of arrays its fixture holds."""
    from tests import agent_port as ap
    from tests import behavior_port as bp_
    from tests import vehicle_port
    ba, lp, misc = mods or load_behavior()
    sc = scenario(name)
    arr = arrays(sc)
    V, T = len(sc["vehicles"]), sc["T"]
    lane_map = LaneMap(np.concatenate([v["xy"] for v in sc["vehicles"]]), np.concatenate([v["lane"] for v in sc["vehicles"]]))
    world = World(lane_map)
    actors = [Actor(world, 100 + i, v["state0"], v["speed_limit"], v["extent"]) for i, v in enumerate(sc["vehicles"])]
    world.actors.extend(actors)
    agents = []
    for v, actor in zip(sc["vehicles"], actors):
        agent = ba.BehaviorAgent(actor, "normal")
        agent.set_global_plan([(MapWaypoint(mk.Location(x, y, 0.0), k), lp.RoadOption.LANEFOLLOW) for (x, y), k in zip(v["xy"], v["lane"])])
        agents.append(agent)
    prm, bp, vp = ap.params(), bp_.params(), ap.vehicle_params()
    port = [ap.Agent() for _ in range(V)]
    paths = [np.c_[v["xy"], np.zeros((len(v["xy"]), 2))] for v in sc["vehicles"]]
    seen, control, queue, target, mode, margin = [], [], [], [], [], []
    for t in range(T):
        row = []
        for a in actors:
            fw = a.get_transform().get_forward_vector()
            row.append((a.state[0], a.state[1], fw.x, fw.y, misc.get_speed(a)))
        seen.append(row)
        driven = [v["brake_from"] < 0 or t < v["brake_from"] for v in sc["vehicles"]]
        heads = [len(v["xy"]) - len(ag._local_planner._waypoints_queue) for v, ag in zip(sc["vehicles"], agents)]
        ctl = []
        for i, agent in enumerate(agents):                     # one after another, nobody moves in between
            if driven[i]:
                c = agent.run_step()
                ctl.append((float(c.throttle), float(c.steer), float(c.brake)))
            else:
                ctl.append((0.0, 0.0, 1.0))
        # the port on the same inputs: its mode and margins, and the law's lane rule against the geometric lookup
        m_row, g_row = [], []
        for i, v in enumerate(sc["vehicles"]):
            if not driven[i]:
                m_row.append(-1)
                g_row.append(math.inf)
                port[i].head = heads[i]
                continue
            assert port[i].head == heads[i], f"{name} tick {t} vehicle {i}: the port's head {port[i].head} left the reference's {heads[i]}"
            others = [j for j in range(V) if j != i]
            rule = [(row[j][0], row[j][1], row[j][4], sc["vehicles"][j]["extent"], bp_.lane_key(sc["vehicles"][j]["lane"], len(paths[j]), heads[j]))
                    for j in others]
            geo = [c[:4] + (int(lane_map.key[lane_map.key_at(c[0], c[1])]),) for c in rule]
            x, y, fx, fy, kmh = row[i]
            twin = ap.Agent(port[i].head, port[i].past_steer, port[i].lon, port[i].lat)
            g = bp_.behave(prm, bp, paths[i], v["lane"], len(paths[i]), x, y, fx, fy, kmh, v["speed_limit"], v["extent"], geo, twin,
                           key_cur=int(lane_map.key[lane_map.key_at(x, y)]))
            mg = []
            r = bp_.behave(prm, bp, paths[i], v["lane"], len(paths[i]), x, y, fx, fy, kmh, v["speed_limit"], v["extent"], rule, port[i], mg)
            if (r["mode"], r["blocker"]) != (g["mode"], g["blocker"]):
                raise RuntimeError(f"{name} tick {t} vehicle {i}: the head - 1 rule gives mode {r['mode']}, the geometric lookup {g['mode']}")
            m_row.append(r["mode"])
            g_row.append(min(mg) if mg else math.inf)
        mode.append(m_row)
        margin.append(g_row)
        control.append(ctl)
        queue.append([len(ag._local_planner._waypoints_queue) for ag in agents])
        target.append([float(ag._local_planner._target_speed) for ag in agents])
        for a, c in zip(actors, ctl):
            a.state = vehicle_port.step(vp, a.state, c)
    margin = np.array(margin, np.float64).reshape(T, V)
    if margin.min() < MIN_MARGIN:
        t, i = np.unravel_index(np.argmin(margin), margin.shape)
        raise RuntimeError(f"{name}: a threshold comparison at tick {t}, vehicle {i} is decided by {margin.min():.3g}")
    mode = np.array(mode, np.int32).reshape(T, V)
    return dict(arr, seen=np.array(seen, np.float64).reshape(T, V, 5), control=np.array(control, np.float64).reshape(T, V, 3),
                queue=np.array(queue, np.int32).reshape(T, V), target=np.array(target, np.float64).reshape(T, V), mode=mode, margin=margin,
                mode_ticks=np.array([[int((mode[:, i] == m).sum()) for m in range(6)] for i in range(V)], np.int32),
                state_end=np.array([a.state for a in actors], np.float64))


def main():
    out = os.path.join(os.environ.get("EMP_GOLDEN_OUT", HERE), "behavior")
    os.makedirs(out, exist_ok=True)
    mods = load_behavior()
    for name in NAMES:
        rec = record(name, mods)
        np.savez_compressed(os.path.join(out, name + ".npz"), **rec)
        gaps = np.sqrt(((rec["seen"][:, 0, :2] - rec["seen"][:, 1, :2]) ** 2).sum(1))
        print(f"{name}: follower mode ticks (normal, slow, follow, clear, emergency, done) {rec['mode_ticks'][0].tolist()}, smallest centre "
              f"distance {gaps.min():.2f} m, smallest margin {rec['margin'].min():.3g}")


if __name__ == "__main__":
    main()
