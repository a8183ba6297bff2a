"""Agent fixtures: the reference's ``LocalPlanner`` and ``VehiclePIDController`` (agents/navigation/), loaded through duck-typed
stubs, driven tick by tick in closed loop on the project's vehicle model, recorded as arrays under tests/golden/agents/.

    python tests/golden/make_golden_agents.py        (EMP_GOLDEN_OUT=<dir>: write to <dir>/agents/ instead)

The scenario half of this file needs nothing but NumPy: tests rebuild a scenario's path and start from ``scenario(name)``.  The
recording half imports the reference's two modules with a ``carla`` module of its own (Location, Vector3D, VehicleControl,
Transform), a vehicle with get_world / get_control / get_location / get_transform / get_velocity, and a map whose get_waypoint
echoes the location.  The plant is tests/vehicle_port.step with the vehicle tuple in physical order (tests/agent_port.VEHICLE_PARA)
at the agents' tick, 0.05 s.

Per scenario ``<name>.npz`` holds
  xy [M][2], n_path, state0 [6], target_speed             the plan handed to set_global_plan, the start, set_speed's km/h
  seen [T][5]     x, y, forward x, forward y, get_speed   what LocalPlanner.run_step read from the vehicle in tick t
  control [T][3]  throttle, steer, brake                  what it returned
  queue [T]       len(_waypoints_queue) after the tick    (head = n_path - queue; DONE where 0)
  state_end [6]                                           the vehicle after the last tick
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

NAMES = ("corner", "straight", "s_bend", "one_waypoint", "empty", "beside", "behind")


# ---- scenarios ----------------------------------------------------------------------------------------------------------------------
def polyline(pieces, step=2.0):
    """Points `step` apart along straight ('s', count) and arc ('a', radius, angle: > 0 turns left) pieces, from (0, 0) heading +x."""
    x, y, th = 0.0, 0.0, 0.0
    pts = [(x, y)]
    for piece in pieces:
        if piece[0] == "s":
            for _ in range(piece[1]):
                x, y = x + step * math.cos(th), y + step * math.sin(th)
                pts.append((x, y))
        else:
            _, radius, angle = piece
            n = max(1, int(round(abs(angle) * radius / step)))
            sgn = 1.0 if angle > 0 else -1.0
            cx, cy = x - sgn * radius * math.sin(th), y + sgn * radius * math.cos(th)
            for k in range(1, n + 1):
                t = th + angle * k / n
                pts.append((cx + sgn * radius * math.sin(t), cy - sgn * radius * math.cos(t)))
            x, y = pts[-1]
            th += angle
    return np.array(pts, np.float64)


def scenario(name):
    """-> dict(xy (M, 2), state0 (6,), target_speed, T)."""
    half = math.pi / 2
    if name == "corner":          # 30 points straight, a 12 m-radius right angle, 29 points straight, at 20 km/h
        return dict(xy=polyline([("s", 29), ("a", 12.0, half), ("s", 29)]), state0=(0.0, 0.0, 0.0, 0.0, 0.0, 0.0), target_speed=20.0, T=700)
    if name == "straight":
        return dict(xy=polyline([("s", 39)]), state0=(-1.0, 0.4, 0.05, 0.0, 0.0, 3.0), target_speed=30.0, T=400)
    if name == "s_bend":
        return dict(xy=polyline([("s", 8), ("a", 15.0, 0.9), ("a", 15.0, -0.9), ("s", 8)]), state0=(0.0, 0.0, 0.0, 0.0, 0.0, 4.0), target_speed=25.0,
                    T=500)
    if name == "one_waypoint":
        return dict(xy=np.array([[6.0, 0.5]]), state0=(0.0, 0.0, 0.0, 0.0, 0.0, 2.0), target_speed=10.0, T=160)
    if name == "empty":
        return dict(xy=np.zeros((0, 2)), state0=(1.0, 2.0, 0.3, 0.0, 0.0, 5.0), target_speed=20.0, T=30)
    if name == "beside":          # 2.5 m to the left of the path's middle, heading along it
        return dict(xy=polyline([("s", 30)]), state0=(20.0, 2.5, 0.0, 0.0, 0.0, 5.0), target_speed=20.0, T=500)
    if name == "behind":          # 8 m behind the first waypoint, heading half a radian off
        return dict(xy=polyline([("s", 20)]), state0=(-8.0, -1.0, 0.5, 0.0, 0.0, 1.0), target_speed=20.0, T=500)
    raise KeyError(name)


# ---- the stubs and the recording ------------------------------------------------------------------------------------------------------
class Vector3D:
    def __init__(self, x=0.0, y=0.0, z=0.0):
        self.x, self.y, self.z = float(x), float(y), float(z)


class Location(Vector3D):
    def distance(self, other):
        dx, dy = self.x - other.x, self.y - other.y
        return math.sqrt(dx * dx + dy * dy)


class Transform:
    def __init__(self, location, forward):
        self.location, self._forward = location, forward

    def get_forward_vector(self):
        return self._forward


class VehicleControl:
    def __init__(self):
        self.throttle = self.steer = self.brake = 0.0
        self.hand_brake = self.manual_gear_shift = False


class Waypoint:
    def __init__(self, location):
        self.transform = Transform(location, Vector3D(1.0, 0.0, 0.0))


class Vehicle:
    """The project's vehicle model behind CARLA's getters: tests/agent_port.observe says what they return."""

    def __init__(self, state):
        self.state = tuple(float(v) for v in state)

    def _seen(self):
        from tests import agent_port
        return agent_port.observe(self.state)

    def get_world(self):
        return self

    def get_map(self):
        return self

    def get_waypoint(self, location):
        return Waypoint(location)

    def get_control(self):
        return VehicleControl()

    def get_location(self):
        return Location(self.state[0], self.state[1], 0.0)

    def get_transform(self):
        (c, s), _, _ = self._seen()
        return Transform(self.get_location(), Vector3D(c, s, 0.0))

    def get_velocity(self):
        _, _, (_, _, wx, wy) = self._seen()
        return Vector3D(wx, wy, 0.0)


def load_agents():
    """The reference's (local_planner, controller, misc) modules with this file's ``carla``."""
    import ref_loader
    if not ref_loader.reference_available():
        raise RuntimeError("reference tree not present at " + ref_loader.REFERENCE_ROOT)
    sys.dont_write_bytecode = True
    carla = types.ModuleType("carla")
    carla.Location, carla.Vector3D, carla.VehicleControl, carla.Transform = Location, Vector3D, VehicleControl, Transform
    names = ("agents", "agents.tools", "agents.tools.misc", "agents.navigation", "agents.navigation.controller", "agents.navigation.local_planner")
    saved = {k: sys.modules.get(k) for k in names + ("carla",)}
    sys.modules["carla"] = carla
    sys.path.insert(0, ref_loader.REFERENCE_ROOT)
    try:
        for k in names:
            sys.modules.pop(k, None)
        mods = tuple(importlib.import_module(k) for k in ("agents.navigation.local_planner", "agents.navigation.controller", "agents.tools.misc"))
    finally:
        sys.path.remove(ref_loader.REFERENCE_ROOT)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mods


def record(name, mods=None):
    """Drive scenario `name` with the reference's classes: the dict of arrays its fixture holds."""
    from tests import agent_port, vehicle_port
    lp, _, misc = mods or load_agents()
    sc = scenario(name)
    vehicle = Vehicle(sc["state0"])
    planner = lp.LocalPlanner(vehicle)
    planner.set_speed(sc["target_speed"])
    planner.set_global_plan([(Waypoint(Location(x, y, 0.0)), lp.RoadOption.LANEFOLLOW) for x, y in sc["xy"]])
    vp = agent_port.vehicle_params()
    seen, control, queue = [], [], []
    for _ in range(sc["T"]):
        fw = vehicle.get_transform().get_forward_vector()
        seen.append((vehicle.state[0], vehicle.state[1], fw.x, fw.y, misc.get_speed(vehicle)))
        c = planner.run_step()
        control.append((float(c.throttle), float(c.steer), float(c.brake)))
        queue.append(len(planner._waypoints_queue))
        assert planner.done() == (queue[-1] == 0)
        vehicle.state = vehicle_port.step(vp, vehicle.state, control[-1])
    T = sc["T"]
    return dict(xy=np.asarray(sc["xy"], np.float64).reshape(-1, 2), n_path=np.int32(len(sc["xy"])), state0=np.array(sc["state0"], np.float64),
                target_speed=np.float64(sc["target_speed"]), seen=np.array(seen, np.float64).reshape(T, 5),
                control=np.array(control, np.float64).reshape(T, 3), queue=np.array(queue, np.int32).reshape(T),
                state_end=np.array(vehicle.state, np.float64))


def main():
    out = os.path.join(os.environ.get("EMP_GOLDEN_OUT", HERE), "agents")
    os.makedirs(out, exist_ok=True)
    mods = load_agents()
    for name in NAMES:
        rec = record(name, mods)
        np.savez_compressed(os.path.join(out, name + ".npz"), **rec)
        q = rec["queue"]
        print(f"{name}: {len(q)} ticks, {int(rec['n_path'])} waypoints, DONE from tick {int(np.argmax(q == 0)) if (q == 0).any() else -1}")


if __name__ == "__main__":
    main()
