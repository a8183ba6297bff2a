"""Hazard fixtures: the reference's ``BehaviorAgent`` ("normal") meeting red lights and pedestrians, recorded as arrays under
tests/golden/hazards/.

    python tests/golden/make_golden_hazards.py        (EMP_GOLDEN_OUT=<dir>: write to <dir>/hazards/ instead)

The scenario half needs nothing but NumPy.  The recording half extends the stubs of make_golden_behavior.py (imported, not edited):
  - a traffic-light actor with ``state`` (red by the clock rule of include/emplanner.h: period, red_from, red_to in ticks),
    ``get_transform`` and a ``trigger_volume`` chosen so that the reference's get_trafficlight_trigger_location lands on the
    intended lane waypoint;
  - a walker actor with a location, a transform and a bounding box, moved by the clock rule x + vx * (k * dt);
  - an actor list whose ``filter`` tells ``*vehicle*``, ``*traffic_light*`` and ``*walker.pedestrian*`` apart by ``type_id``;
  - map waypoints whose forward vector is the lane tangent (the chord to the next waypoint of the lane table, normalised).
Per scenario ``<name>.npz`` holds what a behaviour fixture holds (make_golden_behavior.py) and
  light [L][4], light_lane [L], light_cycle [L][3], walker [K][5], walker_lane [K]     the rows of emp_hazard_io
  emergency [T][V]   the reference returned emergency_stop()'s control
  last_light [T][V]  the index of the reference's _last_traffic_light after the tick, -1 for none
  cause, light_hit, walker_hit [T][V], walker_distance [T][V]   the port's on the recorded inputs (tests/hazard_port.py)
  sticky, ignored, filtered [T][V]   the tick was decided by the sticky light / saw a walker and ignored it / lost a walker to the
                     10 m filter that the cone and the range would have taken
  cause_ticks [V][3]
The generator refuses a scenario in which a margin is below 1e-6 (the chord's dot product, the 10 m filter and the 5 m threshold
among them), or in which the geometric map lookup and the rule's stand-ins (the chord, path[max(head - 1, 0)], the head - 1 key)
would decide a tick differently, or which does not show what it is there to show.
"""
from __future__ import annotations

import fnmatch
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import make_golden_behavior as mkb  # noqa: E402

mk = mkb.mk
NAMES = ("red_light", "sticky", "green_light", "opposite_light", "other_key_light", "walker_crossing", "walker_outside_radius",
         "walker_and_leader", "queue_at_light")
MIN_MARGIN = 1e-6
DT = 0.05
WALKER_EXTENT = 0.4


# ---- scenarios ----------------------------------------------------------------------------------------------------------------------
def _tangent(xy, k):
    k = min(k, len(xy) - 2)
    dx, dy = xy[k + 1][0] - xy[k][0], xy[k + 1][1] - xy[k][1]
    n = math.hypot(dx, dy)
    return dx / n, dy / n


def _light(xy, at, cycle, key=1, flip=False):
    """A light whose trigger volume lies on waypoint `at` of the lane xy."""
    tx, ty = _tangent(xy, at)
    if flip:
        tx, ty = -tx, -ty
    return dict(row=(float(xy[at][0]), float(xy[at][1]), tx, ty), key=key, cycle=tuple(int(v) for v in cycle))


def _walker(xy, at, lateral, speed, key=1, ahead=0.0):
    """A walker `lateral` m to the left of waypoint `at` at tick 0, walking across the lane to the right at `speed` m/s."""
    tx, ty = _tangent(xy, at)
    x, y = xy[at][0] + ahead * tx - lateral * ty, xy[at][1] + ahead * ty + lateral * tx
    return dict(row=(float(x), float(y), speed * ty, -speed * tx, WALKER_EXTENT), key=key)


def scenario(name):
    """-> dict(vehicles=[...] as make_golden_behavior.scenario, lights=[dict(row, key, cycle)], walkers=[dict(row, key)],
    lanes=[dict(xy, key, flip)] map lanes beside the vehicles' plans, T)."""
    arc = mkb._arc()
    v = mkb._vehicle
    if name == "red_light":           # slow enough to stop short of the trigger waypoint: drive, stop, go on green
        return dict(vehicles=[v(arc, 0, 2.0, 12.0)], lights=[_light(arc, 8, (100000, 0, 330))], walkers=[], lanes=[], T=600)
    if name == "sticky":              # 27 km/h: the vehicle rolls past the trigger waypoint while braking and is held by last_light
        return dict(vehicles=[v(arc, 0, 7.5, 30.0)], lights=[_light(arc, 20, (100000, 0, 300))], walkers=[], lanes=[], T=600)
    if name == "green_light":         # red only before the vehicle arrives and after it has passed
        return dict(vehicles=[v(arc, 0, 7.5, 30.0)], lights=[_light(arc, 20, (300, 0, 60))], walkers=[], lanes=[], T=400)
    inner = mk.polyline([("a", 96.5, 470.0 / 100.0)]) + np.array([0.0, 3.5])         # the lane 3.5 m to the left
    if name == "opposite_light":      # the same road key, the oncoming lane: dot < 0
        return dict(vehicles=[v(arc, 0, 7.5, 30.0)], lights=[_light(inner, 20, (100000, 0, 100000), flip=True)], walkers=[],
                    lanes=[dict(xy=inner, key=1, flip=True)], T=400)
    if name == "other_key_light":     # a road beside the vehicle's, keyed otherwise
        return dict(vehicles=[v(arc, 0, 7.5, 30.0)], lights=[_light(inner, 20, (100000, 0, 100000), key=2)], walkers=[],
                    lanes=[dict(xy=inner, key=2, flip=False)], T=400)
    if name == "walker_crossing":     # seen and ignored while d >= braking_distance, then the emergency, then the walker is across
        return dict(vehicles=[v(arc, 0, 7.5, 30.0)], lights=[], walkers=[_walker(arc, 30, 4.0, 0.5)], lanes=[], T=600)
    if name == "walker_outside_radius":   # limit 60: th = 20 m, so cone and range take the walker long before the 10 m filter does
        return dict(vehicles=[v(arc, 0, 10.0, 60.0)], lights=[], walkers=[_walker(arc, 40, 3.0, 0.3)], lanes=[], T=500)
    if name == "walker_and_leader":   # a walker 7 m beside the lane is seen and ignored while the leader ahead is followed
        return dict(vehicles=[v(arc, 0, 8.0, 60.0), v(arc, 6, 6.0, 23.0)], lights=[], walkers=[_walker(arc, 25, 7.0, 0.0)], lanes=[], T=500)
    if name == "queue_at_light":      # the leader stops at the light, the follower behind it by the vehicle rule; both leave on green
        return dict(vehicles=[v(arc, 0, 2.0, 12.0), v(arc, 8, 2.0, 12.0)], lights=[_light(arc, 20, (100000, 0, 450))], walkers=[], lanes=[], T=600)
    raise KeyError(name)


def arrays(sc):
    """The padded arrays of a scenario: make_golden_behavior.arrays plus the rows of emp_hazard_io."""
    arr = mkb.arrays(sc)
    L, K = len(sc["lights"]), len(sc["walkers"])
    arr.update(light=np.array([l["row"] for l in sc["lights"]], np.float64).reshape(L, 4),
               light_lane=np.array([l["key"] for l in sc["lights"]], np.int32).reshape(L),
               light_cycle=np.array([l["cycle"] for l in sc["lights"]], np.int32).reshape(L, 3),
               walker=np.array([w["row"] for w in sc["walkers"]], np.float64).reshape(K, 5),
               walker_lane=np.array([w["key"] for w in sc["walkers"]], np.int32).reshape(K))
    return arr


# ---- the stubs and the recording ------------------------------------------------------------------------------------------------------
class Location(mk.Location):
    def __add__(self, other):
        return Location(self.x + other.x, self.y + other.y, self.z + other.z)


class TangentMap(mkb.LaneMap):
    """The lane table with a forward vector per waypoint: the lane tangent."""

    def __init__(self, xy, key, forward):
        super().__init__(xy, key)
        self.forward = np.asarray(forward, np.float64).reshape(-1, 2)

    def get_waypoint(self, location):
        k = self.key_at(location.x, location.y)
        w = mkb.MapWaypoint(mk.Location(self.xy[k, 0], self.xy[k, 1], 0.0), self.key[k])
        w.transform = mk.Transform(w.transform.location, mk.Vector3D(self.forward[k, 0], self.forward[k, 1], 0.0))
        return w


class ActorList(list):
    def filter(self, pattern):
        return ActorList(a for a in self if fnmatch.fnmatchcase(a.type_id, pattern))


class World(mkb.World):
    def __init__(self, lane_map):
        super().__init__(lane_map)
        self.actors, self.tick = ActorList(), 0


class Car(mkb.Actor):
    type_id = "vehicle.stub.car"


class LightTransform:
    """A transform at the light's pole without rotation: transform(p) is a translation."""

    def __init__(self, location):
        self.location, self.rotation = location, mkb._Names(yaw=0.0, pitch=0.0, roll=0.0)

    def transform(self, p):
        return Location(self.location.x + p.x, self.location.y + p.y, self.location.z + p.z)


class TrafficLight:
    type_id = "traffic.traffic_light"

    def __init__(self, world, ident, row, cycle):
        self.world, self.id, self.cycle = world, ident, tuple(int(v) for v in cycle)
        pole = Location(row[0] + 6.0 * row[3], row[1] - 6.0 * row[2], 0.0)         # 6 m to the right of the lane
        self._transform = LightTransform(pole)
        self.trigger_volume = mkb._Names(location=Location(row[0] - pole.x, row[1] - pole.y, 0.0), extent=mkb._Names(x=1.5, y=1.5, z=1.0))

    def get_transform(self):
        return self._transform

    @property
    def state(self):
        period, red_from, red_to = self.cycle
        return "red" if period >= 1 and red_from <= self.world.tick % period < red_to else "green"


class Walker:
    type_id = "walker.pedestrian.0001"

    def __init__(self, world, ident, row):
        self.world, self.id, self.row = world, ident, tuple(float(v) for v in row)
        self.bounding_box = mkb._Names(extent=mkb._Names(x=self.row[4], y=self.row[4] / 2.0, z=0.9))

    def get_location(self):
        tau = float(self.world.tick) * DT
        return Location(self.row[0] + self.row[2] * tau, self.row[1] + self.row[3] * tau, 0.0)

    def get_transform(self):
        return mk.Transform(self.get_location(), mk.Vector3D(1.0, 0.0, 0.0))


def lane_table(sc):
    """The map: every vehicle's plan (as make_golden_behavior's) and the scenario's further lanes, with the tangent of each waypoint."""
    rows = [(v["xy"], v["lane"], 1.0) for v in sc["vehicles"]]
    rows += [(l["xy"], np.full(len(l["xy"]), l["key"]), -1.0 if l["flip"] else 1.0) for l in sc["lanes"]]
    xy = np.concatenate([r[0] for r in rows])
    key = np.concatenate([r[1] for r in rows])
    fw = np.concatenate([[tuple(r[2] * c for c in _tangent(r[0], k)) for k in range(len(r[0]))] for r in rows])
    return xy, key, fw


def record(name, mods=None):
    """Drive scenario `name` with the reference's BehaviorAgent: the dict of arrays its fixture holds."""
    from tests import agent_port as ap
    from tests import behavior_port as bp_
    from tests import hazard_port as hp_
    from tests import vehicle_port
    ba, lp, misc = mods or mkb.load_behavior()
    misc.carla.Location = Location                                 # get_trafficlight_trigger_location adds two locations
    sc = scenario(name)
    arr = arrays(sc)
    V, T = len(sc["vehicles"]), sc["T"]
    lane_map = TangentMap(*lane_table(sc))
    world = World(lane_map)
    cars = [Car(world, 100 + i, v["state0"], v["speed_limit"], v["extent"]) for i, v in enumerate(sc["vehicles"])]
    light_actors = [TrafficLight(world, 200 + i, l["row"], l["cycle"]) for i, l in enumerate(sc["lights"])]
    walker_actors = [Walker(world, 300 + i, w["row"]) for i, w in enumerate(sc["walkers"])]
    world.actors.extend(cars + light_actors + walker_actors)
    rule_lights = [l["row"] + (l["key"],) + l["cycle"] for l in sc["lights"]]
    # the light as the reference finds it: the map waypoint under its trigger location
    geo_lights = []
    for actor, l in zip(light_actors, sc["lights"]):
        loc = misc.get_trafficlight_trigger_location(actor)
        k = lane_map.key_at(loc.x, loc.y)
        geo_lights.append((lane_map.xy[k, 0], lane_map.xy[k, 1], lane_map.forward[k, 0], lane_map.forward[k, 1], int(lane_map.key[k])) + l["cycle"])
        if max(abs(a - b) for a, b in zip(geo_lights[-1][:5], l["row"] + (l["key"],))) > 1e-12:
            raise RuntimeError(f"{name}: a light's trigger location does not land on its waypoint")
    agents = []
    for v, car in zip(sc["vehicles"], cars):
        agent = ba.BehaviorAgent(car, "normal")
        agent.set_global_plan([(mkb.MapWaypoint(mk.Location(x, y, 0.0), k), lp.RoadOption.LANEFOLLOW) for (x, y), k in zip(v["xy"], v["lane"])])
        agents.append(agent)
    prm, bp, hp, vp = ap.params(), bp_.params(), hp_.params(), ap.vehicle_params()
    port = [ap.Agent() for _ in range(V)]
    last = [-1] * V
    paths = [np.c_[v["xy"], np.zeros((len(v["xy"]), 2))] for v in sc["vehicles"]]
    keys = ("seen", "control", "queue", "target", "mode", "margin", "emergency", "last_light", "cause", "light_hit", "walker_hit",
            "walker_distance", "sticky", "ignored", "filtered")
    log = {k: [] for k in keys}
    sticky_beyond_scan = 0
    for t in range(T):
        world.tick = t
        row = []
        for a in cars:
            fw = a.get_transform().get_forward_vector()
            row.append((a.state[0], a.state[1], fw.x, fw.y, misc.get_speed(a)))
        heads = [len(v["xy"]) - len(ag._local_planner._waypoints_queue) for v, ag in zip(sc["vehicles"], agents)]
        ctl = []
        for agent in agents:                                       # one after another, nobody moves in between
            c = agent.run_step()
            ctl.append((float(c.throttle), float(c.steer), float(c.brake)))
        ref_last = [light_actors.index(ag._last_traffic_light) if ag._last_traffic_light is not None else -1 for ag in agents]
        tau = float(t) * DT
        rule_walkers = [w["row"] + (w["key"],) for w in sc["walkers"]]
        geo_walkers = []
        for w in sc["walkers"]:
            wx, wy = w["row"][0] + w["row"][2] * tau, w["row"][1] + w["row"][3] * tau
            geo_walkers.append(w["row"] + (int(lane_map.key[lane_map.key_at(wx, wy)]),))
        cur = {k: [] for k in keys if k not in ("seen", "control", "queue", "target")}
        for i, v in enumerate(sc["vehicles"]):
            assert port[i].head == heads[i], f"{name} tick {t} vehicle {i}: the port's head {port[i].head} left the reference's {heads[i]}"
            others = [j for j in range(V) if j != i]
            rule = [(row[j][0], row[j][1], row[j][4], sc["vehicles"][j]["extent"], bp_.lane_key(sc["vehicles"][j]["lane"], len(paths[j]), heads[j]))
                    for j in others]
            geo = [c[:4] + (int(lane_map.key[lane_map.key_at(c[0], c[1])]),) for c in rule]
            x, y, fx, fy, kmh = row[i]
            k = lane_map.key_at(x, y)
            ego = (int(lane_map.key[k]), lane_map.xy[k, 0], lane_map.xy[k, 1], lane_map.forward[k, 0], lane_map.forward[k, 1])
            twin = ap.Agent(port[i].head, port[i].past_steer, port[i].lon, port[i].lat)
            g = hp_.behave(prm, bp, hp, paths[i], v["lane"], len(paths[i]), x, y, fx, fy, kmh, v["speed_limit"], v["extent"], geo, geo_lights,
                           geo_walkers, t, twin, last[i], geo=ego)
            mg, notes = [], []
            if last[i] >= 0 and hp_.is_red(sc["lights"][last[i]]["cycle"], t):
                if hp_.light_scan(hp, paths[i], v["lane"], len(paths[i]), port[i].head, x, y, fx, fy, rule_lights, t, -1)[0] < 0:
                    sticky_beyond_scan += 1
            r = hp_.behave(prm, bp, hp, paths[i], v["lane"], len(paths[i]), x, y, fx, fy, kmh, v["speed_limit"], v["extent"], rule, rule_lights,
                           rule_walkers, t, port[i], last[i], mg, notes)
            what = lambda d: (d["mode"], d["cause"], d["blocker"], d["light_hit"], d["last_light"])
            if what(r) != what(g):
                raise RuntimeError(f"{name} tick {t} vehicle {i}: the stand-ins give {what(r)}, the geometric lookup {what(g)}")
            last[i] = r["last_light"]
            if last[i] != ref_last[i]:
                raise RuntimeError(f"{name} tick {t} vehicle {i}: the port holds light {last[i]}, the reference {ref_last[i]}")
            cur["mode"].append(r["mode"])
            cur["margin"].append(min(mg) if mg else math.inf)
            cur["emergency"].append(int(ctl[i] == (0.0, 0.0, 0.5)))
            cur["last_light"].append(ref_last[i])
            for f in ("cause", "light_hit", "walker_hit", "walker_distance"):
                cur[f].append(r[f])
            cur["sticky"].append(int("sticky" in notes))
            cur["ignored"].append(int("ignored" in notes))
            cur["filtered"].append(int("filter" in notes))
        for k_, v_ in cur.items():
            log[k_].append(v_)
        log["seen"].append(row)
        log["control"].append(ctl)
        log["queue"].append([len(ag._local_planner._waypoints_queue) for ag in agents])
        log["target"].append([float(ag._local_planner._target_speed) for ag in agents])
        for a, c in zip(cars, ctl):
            a.state = vehicle_port.step(vp, a.state, c)
    ints = ("queue", "mode", "emergency", "last_light", "cause", "light_hit", "walker_hit", "sticky", "ignored", "filtered")
    rec = {k: np.array(v, np.int32 if k in ints else np.float64) for k, v in log.items()}
    rec["seen"], rec["control"] = rec["seen"].reshape(T, V, 5), rec["control"].reshape(T, V, 3)
    for k in keys[2:]:
        rec[k] = rec[k].reshape(T, V)
    if rec["margin"].min() < MIN_MARGIN:
        t, i = np.unravel_index(np.argmin(rec["margin"]), rec["margin"].shape)
        raise RuntimeError(f"{name}: a threshold comparison at tick {t}, vehicle {i} is decided by {rec['margin'].min():.3g}")
    mode, cause = rec["mode"], rec["cause"]
    rec.update(arr, mode_ticks=np.array([[int((mode[:, i] == m).sum()) for m in range(6)] for i in range(V)], np.int32),
               cause_ticks=np.array([[int((cause[:, i] == m).sum()) for m in (1, 2, 3)] for i in range(V)], np.int32),
               state_end=np.array([a.state for a in cars], np.float64))
    _shows(name, rec, sticky_beyond_scan)
    return rec


def _shows(name, rec, sticky_beyond_scan):
    """What each scenario is there to show."""
    ct, T = rec["cause_ticks"], len(rec["mode"])
    moved = lambda i: float(np.hypot(*(rec["state_end"][i, :2] - rec["seen"][-100, i, :2])))
    ok = True
    if name in ("red_light", "sticky"):
        ok = ct[0, 0] > 0 and rec["cause"][-1, 0] == 0 and rec["last_light"][-1, 0] == -1 and moved(0) > 2.0
        if name == "red_light":
            ok = ok and sticky_beyond_scan == 0
        else:
            ok = ok and sticky_beyond_scan >= 1
    elif name in ("green_light", "opposite_light", "other_key_light"):
        ok = ct.sum() == 0 and (rec["light_hit"] < 0).all()
    elif name == "walker_crossing":
        first = int(np.argmax(rec["cause"][:, 0] == 2))
        ok = ct[0, 1] > 0 and rec["ignored"][:first, 0].sum() > 0 and rec["cause"][-1, 0] == 0 and moved(0) > 2.0
    elif name == "walker_outside_radius":
        ok = rec["filtered"][:, 0].sum() > 0 and (rec["walker_hit"][:, 0] >= 0).sum() > 0
    elif name == "walker_and_leader":
        both = (rec["ignored"][:, 0] == 1) & np.isin(rec["mode"][:, 0], (1, 2, 3))
        ok = both.sum() > 0 and ct[0, 1] == 0
    elif name == "queue_at_light":
        ok = ct[1, 0] > 0 and ct[0, 2] > 0 and ct[0, 0] == 0 and moved(0) > 2.0 and moved(1) > 2.0
    if not ok:
        raise RuntimeError(f"{name}: the scenario does not show what it is there to show (cause ticks {ct.tolist()}, sticky beyond the scan "
                           f"{sticky_beyond_scan}, ignored {rec['ignored'].sum(0).tolist()}, filtered {rec['filtered'].sum(0).tolist()})")


def main():
    out = os.path.join(os.environ.get("EMP_GOLDEN_OUT", HERE), "hazards")
    os.makedirs(out, exist_ok=True)
    mods = mkb.load_behavior()
    for name in NAMES:
        rec = record(name, mods)
        np.savez_compressed(os.path.join(out, name + ".npz"), **rec)
        print(f"{name}: cause ticks (light, walker, vehicle) {rec['cause_ticks'].tolist()}, sticky {rec['sticky'].sum(0).tolist()}, ignored "
              f"{rec['ignored'].sum(0).tolist()}, filtered {rec['filtered'].sum(0).tolist()}, smallest margin {rec['margin'].min():.3g}")


if __name__ == "__main__":
    main()
