"""Fixture of the fleet loop's request (emp_drive_request): what the REFERENCE's own driver functions return for a set of
scenes - ``test_9.get_actor_from_world`` (test_9.py:48-89) and ``planning_utils.predict_block`` (planning_utils.py:591-614), called on
duck-typed fake vehicles (the reference only calls get_world / get_actors().filter / get_location / get_velocity / get_transform /
get_angular_velocity / id on them).  The fixture holds inputs and recorded results only: per scene the vehicle state, the actors,
the kept actor indices in the reference's order with their ``dis`` (and ``speed``), and the predicted x, y, fi.

The decision thresholds see np.dot and libm on one side and device code on the other, so every decision variable stays at
least MARGIN from its threshold (dis against 50 and 30, lat against +-5, along against -10, speed against 1): an actor that does
not is drawn again, and the finished set is asserted.  Ties on dis appear only as exact duplicates (same position).  The
reference squares with ``** 2`` (libm's pow, not always the correctly rounded product); the library multiplies, so an actor
whose four squares are not the same bits either way is drawn again as well - about one in 300.

Run:  python tests/golden/make_golden_drive.py      (writes tests/golden/drive/drive_request.npz)
"""
from __future__ import annotations

import math
import os
import sys
from types import SimpleNamespace as NS

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
#: tests/golden/drive/ (a directory of its own: tests/test_reference_live.py pins the .npz files directly under tests/golden/),
#: or a scratch directory for tests/test_drive_host.py (regenerate and compare)
OUT = os.environ.get("EMP_GOLDEN_OUT", os.path.join(HERE, "drive"))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import drive_port as port  # noqa: E402
import ref_loader  # noqa: E402

MAX_ACT = 64
MARGIN = 1e-6
DIS_LIMITATION, PRED_TS = 50, 0.2          # test_9.py:377, :335
DEG = math.pi / 180                         # the reference's factor (test_9.py:75, planning_utils.py:601)


class FakeVehicle:
    """What the reference asks of a carla.Vehicle, from plain numbers (yaw and yaw rate in degrees, as CARLA reports them)."""

    def __init__(self, vid, x, y, vx, vy, yaw_deg=0.0, yaw_rate_deg=0.0, world=None):
        self.id = vid
        self._loc, self._vel = NS(x=x, y=y, z=0.0), NS(x=vx, y=vy, z=0.0)
        self._tf = NS(rotation=NS(yaw=yaw_deg))
        self._w = NS(x=0.0, y=0.0, z=yaw_rate_deg)
        self._world = world

    def get_world(self):
        return self._world

    def get_location(self):
        return self._loc

    def get_velocity(self):
        return self._vel

    def get_transform(self):
        return self._tf

    def get_angular_velocity(self):
        return self._w


class FakeWorld:
    def __init__(self):
        self.vehicles = []

    def get_actors(self):
        return NS(filter=lambda pattern: list(self.vehicles))


def squares_agree(*values):
    return all(v ** 2 == v * v for v in values)


def actor_ok(state, actor):
    """Every decision variable at least MARGIN from its threshold, and squares that do not depend on how they are taken."""
    dis, lat, along, speed = port.measure(state, actor)
    far = lambda v, t: abs(v - t) >= MARGIN
    return (far(dis, 50.0) and far(dis, 30.0) and far(lat, 5.0) and far(lat, -5.0) and far(along, -10.0) and far(speed, 1.0)
            and squares_agree(state[0] - actor[0], state[1] - actor[1], actor[2], actor[3]))


def make_state(rng, speed=None, yaw_deg=None):
    yaw = float(rng.uniform(-180, 180)) if yaw_deg is None else yaw_deg
    yaw_rate = float(rng.uniform(-20, 20))
    Vx = float(rng.uniform(1.0, 15.0)) if speed is None else speed
    Vy = float(rng.normal(0, 0.3)) if Vx > 0 else 0.0
    return [float(rng.uniform(-200, 200)), float(rng.uniform(-200, 200)), yaw * DEG, Vy, yaw_rate * DEG, Vx], yaw, yaw_rate


def place(state, ahead, side):
    """World position `ahead` metres along the heading and `side` metres to its left."""
    c, s = math.cos(state[2]), math.sin(state[2])
    return state[0] + ahead * c - side * s, state[1] + ahead * s + side * c


def draw_actor(rng, state, kind):
    """One actor of a kind; drawn again until actor_ok."""
    for _ in range(1000):
        ahead, side = float(rng.uniform(-5, 45)), float(rng.uniform(-4.5, 4.5))
        moving = bool(rng.integers(0, 2))
        if kind == "static":
            moving = False
        elif kind == "dynamic":
            moving = True
        elif kind == "behind":           # more than 10 m (m/s) behind
            ahead = float(rng.uniform(-40, -15))
        elif kind == "outside":
            side = float(rng.choice([-1, 1]) * rng.uniform(5.5, 12))
        elif kind == "beyond":
            ahead = float(rng.uniform(52, 90))
        elif kind == "far_static":       # kept, static, beyond the 30 m gate
            ahead, moving = float(rng.uniform(33, 47)), False
        elif kind == "wide":             # anywhere
            ahead, side = float(rng.uniform(-30, 70)), float(rng.uniform(-9, 9))
        x, y = place(state, ahead, side)
        if moving:
            v, d = float(rng.uniform(1.5, 12)), float(rng.uniform(-math.pi, math.pi))
            vx, vy = v * math.cos(d), v * math.sin(d)
        else:
            v, d = float(rng.choice([0.0, 0.0, 0.3, 0.9])), float(rng.uniform(-math.pi, math.pi))
            vx, vy = v * math.cos(d), v * math.sin(d)
        actor = [x, y, vx, vy]
        if actor_ok(state, actor):
            return actor
    raise RuntimeError("no admissible actor found")


def scenes():
    """(state, yaw_deg, yaw_rate_deg, actors) per scene: the required cases first, then random mixtures."""
    rng = np.random.default_rng(20261017)
    out = []

    def add(kinds, speed=None, dup=0):
        state, yaw, rate = make_state(rng, speed)
        actors = [draw_actor(rng, state, k) for k in kinds]
        for _ in range(dup):             # exact duplicates: same position, the stable sort keeps index order
            src = actors[int(rng.integers(0, len(actors)))]
            actors.insert(int(rng.integers(0, len(actors) + 1)), list(src))
        out.append((state, yaw, rate, actors[:MAX_ACT]))

    add([])
    add(["static"])
    add(["dynamic"])
    add(["any"] * 63)
    add(["any"] * 64)
    add(["wide"] * 64)
    add(["static"] * 9)
    add(["dynamic"] * 9)
    add(["behind", "static", "behind"], speed=8.0)
    add(["outside", "outside", "dynamic"])
    add(["beyond", "beyond", "static"])
    add(["far_static", "far_static", "far_static"])
    add(["far_static", "dynamic", "far_static", "dynamic"])
    add(["static", "static", "dynamic", "dynamic"], dup=3)
    add(["any"] * 20, dup=6)
    add(["wide"] * 12, speed=0.0)        # a stationary ego: along is 0 for everyone
    add(["behind", "any", "any"], speed=0.0)
    while len(out) < 96:
        n = int(rng.integers(0, 40))
        add([str(rng.choice(["any", "wide", "static", "dynamic", "behind", "outside", "beyond", "far_static"])) for _ in range(n)],
            dup=int(rng.integers(0, 3)) if n else 0)
    return out


def main():
    t9 = ref_loader.load_driver_reference()
    _, pu = ref_loader.load_reference()
    S = scenes()
    n = len(S)
    state = np.zeros((n, 6))
    actors = np.zeros((n, MAX_ACT, 4))
    n_act = np.zeros(n, np.int32)
    static_idx = np.full((n, MAX_ACT), -1, np.int32)
    dyn_idx = np.full((n, MAX_ACT), -1, np.int32)
    static_dis, dyn_dis, dyn_speed = (np.zeros((n, MAX_ACT)) for _ in range(3))
    n_static, n_dyn = np.zeros(n, np.int32), np.zeros(n, np.int32)
    pred = np.zeros((n, 3))
    for k, (st, yaw, rate, acts) in enumerate(S):
        assert all(actor_ok(st, a) for a in acts)
        state[k], n_act[k] = st, len(acts)
        if acts:
            actors[k, :len(acts)] = acts
        world = FakeWorld()
        wx, wy = port.world_velocity(st[2], st[3], st[5])
        ego = FakeVehicle(0, st[0], st[1], wx, wy, yaw, rate, world)
        others = [FakeVehicle(1 + i, *a) for i, a in enumerate(acts)]
        world.vehicles = others[:len(others) // 2] + [ego] + others[len(others) // 2:]    # the ego is one of the world's vehicles
        statics, dynamics = t9.get_actor_from_world(ego, dis_limitation=DIS_LIMITATION)
        n_static[k], n_dyn[k] = len(statics), len(dynamics)
        for r, (v, dis) in enumerate(statics):
            static_idx[k, r], static_dis[k, r] = v.id - 1, dis
        for r, (v, dis, speed) in enumerate(dynamics):
            dyn_idx[k, r], dyn_dis[k, r], dyn_speed[k, r] = v.id - 1, dis, speed
        pred[k] = pu.predict_block(ego, ts=PRED_TS)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "drive_request.npz"), state=state, actors=actors, n_act=n_act, static_idx=static_idx,
                        static_dis=static_dis, n_static=n_static, dyn_idx=dyn_idx, dyn_dis=dyn_dis, dyn_speed=dyn_speed, n_dyn=n_dyn,
                        pred=pred, margin=np.array(MARGIN), pred_ts=np.array(PRED_TS), dis_limitation=np.array(float(DIS_LIMITATION)))
    print("wrote", os.path.join(OUT, "drive_request.npz"), n, "scenes,", int(n_act.sum()), "actors,", int(n_static.sum()), "static,",
          int(n_dyn.sum()), "dynamic kept")


if __name__ == "__main__":
    main()
