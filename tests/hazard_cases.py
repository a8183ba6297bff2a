"""Inputs for the hazard rule (red lights and pedestrians in front of the car-following law) that the CPU suite
(tests/test_hazard_host.py: the g++ build of csrc/emp_hazard_core.h) and the GPU suite (tests/test_gpu_hazards.py) share: the
fixtures of tests/golden/hazards/ and their replay through the port, the seeded ragged batches with poison in every slot the rule
must not read, and hand-built worlds on the rule's thresholds.  A batch is tests/behavior_cases.py's dict plus the arrays of
emp_hazard_io, laid out (W, ...).  Test tool only."""
from __future__ import annotations

import math
import os
import sys

import numpy as np

from tests import agent_port as ap
from tests import behavior_cases as bc
from tests import behavior_port as bp
from tests import hazard_port as hp
from tests.agent_cases import same_bits  # noqa: F401  (re-exported)

GOLDEN = bc.GOLDEN
sys.path.insert(0, GOLDEN)
import make_golden_hazards as mkh  # noqa: E402

NAN = math.nan
NAMES = mkh.NAMES
HAZARD_IN = ("n_light", "light", "light_lane", "light_cycle", "n_walker", "walker", "walker_lane", "last_light")
HAZARD_OUT = ("last_light", "cause", "light_hit", "walker_hit", "walker_distance")
INT_OUT = bc.INT_OUT + ("last_light", "cause", "light_hit", "walker_hit")
POISON_INT = bc.POISON_INT
#: the seeded batches of the GPU suite: five worlds of 1, 2, 3, 64 and 7 agents with these lights and walkers
SIZES, LIGHTS, WALKERS = (1, 2, 3, 64, 7), (0, 1, 64, 5, 2), (0, 64, 1, 3, 9)
BATCHES = 12
SEED = 32                          # picked so that the port meets the coverage tests/test_hazard_host.py asserts
TICK0 = (0, 1, 7, 37, 100, 199, 200, 1234, 99999, 5, 64, 2000000000)
MIN_MARGIN = 1e-9


def fixture(name):
    with np.load(os.path.join(GOLDEN, "hazards", name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def lights_of(f):
    return [tuple(f["light"][q]) + (int(f["light_lane"][q]),) + tuple(int(v) for v in f["light_cycle"][q]) for q in range(len(f["light"]))]


def walkers_of(f):
    return [tuple(f["walker"][q]) + (int(f["walker_lane"][q]),) for q in range(len(f["walker"]))]


def replay(name):
    """The port on the recorded inputs of a fixture, each vehicle with its own agent state and sticky light: dict(control (T, V, 3),
    queue, target, mode, cause, last_light, light_hit, walker_hit (T, V))."""
    f = fixture(name)
    T, V = f["queue"].shape
    paths = bc.fixture_paths(f)
    prm, prb, hpp = ap.params(), bp.params(), hp.params()
    agents = [ap.Agent() for _ in range(V)]
    last = [-1] * V
    lights, walkers = lights_of(f), walkers_of(f)
    out = dict(control=np.zeros((T, V, 3)), queue=np.zeros((T, V), np.int32), target=np.zeros((T, V)))
    out.update({k: np.zeros((T, V), np.int32) for k in ("mode", "cause", "last_light", "light_hit", "walker_hit")})
    for t in range(T):
        heads = [g.head for g in agents]
        for i in range(V):
            cands = [(f["seen"][t, j, 0], f["seen"][t, j, 1], f["seen"][t, j, 4], f["extent"][j],
                      bp.lane_key(f["lane"][j], f["n_path"][j], heads[j])) for j in range(V) if j != i]
            x, y, c, s, kmh = f["seen"][t, i]
            r = hp.behave(prm, prb, hpp, paths[i], f["lane"][i], f["n_path"][i], x, y, c, s, kmh, f["speed_limit"][i], f["extent"][i], cands,
                          lights, walkers, t, agents[i], last[i])
            last[i] = r["last_light"]
            out["control"][t, i], out["queue"][t, i], out["target"][t, i] = r["control"], f["n_path"][i] - agents[i].head, r["target"]
            for k in ("mode", "cause", "last_light", "light_hit", "walker_hit"):
                out[k][t, i] = r[k]
    return f, out


def blank(W, N, M, K, ML, MW):
    """W worlds with nothing set: poison wherever the rule must not look."""
    b = bc.blank(W, N, M, K)
    b.update(n_light=np.zeros(W, np.int32), light=np.full((W, ML, 4), NAN), light_lane=np.full((W, ML), 1, np.int32),
             light_cycle=np.tile(np.array([1, 0, 1], np.int32), (W, ML, 1)), n_walker=np.zeros(W, np.int32),
             walker=np.full((W, MW, 5), NAN), walker_lane=np.full((W, MW), 1, np.int32), last_light=np.full((W, N), POISON_INT, np.int32))
    return b


def fixture_world(name):
    """A fixture's scenario as a one-world batch without forward / speed_kmh (the start of its closed loop)."""
    f = fixture(name)
    V, M = f["lane"].shape
    L_, K_ = len(f["light"]), len(f["walker"])
    b = blank(1, V, M, 0, L_, K_)
    b["n_world"][0] = V
    b["path"][0, :, :, :2], b["path"][0, :, :, 2:] = f["xy"], 0.0
    b["n_path"][0], b["lane"][0], b["state"][0], b["speed_limit"][0], b["extent"][0] = f["n_path"], f["lane"], f["state0"], f["speed_limit"], f["extent"]
    b["head"][0], b["past_steer"][0], b["n_lon"][0], b["n_lat"][0] = 0, 0.0, 0, 0
    b["n_light"][0], b["n_walker"][0], b["last_light"][0] = L_, K_, -1
    b["light"][0], b["light_lane"][0], b["light_cycle"][0] = f["light"], f["light_lane"], f["light_cycle"]
    b["walker"][0], b["walker_lane"][0] = f["walker"], f["walker_lane"]
    return f, b


def add_hazards(b, lights, walkers, ML, MW, tick0, rng):
    """Lights and walkers for the worlds of a tests/behavior_cases.random_worlds batch: most stand where an agent will meet them at
    tick index tick0.  Slots past the counts keep their poison (red, on every key, on top of an agent)."""
    W, N = b["n_path"].shape
    tau = float(tick0) * ap.params()["dt"]
    b.update({k: v for k, v in blank(W, N, 1, 0, ML, MW).items() if k in HAZARD_IN})
    for w in range(W):
        n = min(max(int(b["n_world"][w]), 0), N)
        nl, nk = lights[w], walkers[w]
        b["n_light"][w] = nl if rng.random() < 0.8 else nl + 1000 * (nl == ML)         # a count beyond the row is clamped
        b["n_walker"][w] = nk if rng.random() < 0.8 else nk + 1000 * (nk == MW)
        for q in range(ML):
            i = int(rng.integers(0, n)) if n else 0
            x, y, th = (b["state"][w, i, :3] if n else (0.0, 0.0, 0.0))
            d, off = rng.choice([0.0005, 1.0, 2.5, 4.0, 4.9, 5.1, 7.0, -2.0]), rng.normal(0, 0.8)
            tdir = th + rng.normal(0, 0.1) + (math.pi if rng.random() < 0.15 else 0.0)
            row = (x + d * math.cos(th) - off * math.sin(th), y + d * math.sin(th) + off * math.cos(th), math.cos(tdir), math.sin(tdir))
            period = int(rng.choice([0, -5, 1, 2, 7, 50, 400]))
            red_from = int(rng.integers(0, max(period, 1)))
            cycle = (period, red_from, red_from + int(rng.integers(0, max(period, 1) + 1))) if rng.random() < 0.5 else (max(period, 1), 0, max(period, 1))
            if q < nl:
                b["light"][w, q], b["light_lane"][w, q], b["light_cycle"][w, q] = row, rng.choice([1, 1, 1, 1, 2, -1]), cycle
            else:                                                  # never read: on top of agent i, red for ever, NaN direction
                b["light"][w, q], b["light_lane"][w, q], b["light_cycle"][w, q] = (x, y, NAN, NAN), 1, (1, 0, 1)
        for q in range(MW):
            i = int(rng.integers(0, n)) if n else 0
            x, y, th = (b["state"][w, i, :3] if n else (0.0, 0.0, 0.0))
            d, off = rng.choice([3.0, 6.5, 8.0, 8.5, 9.0, 9.5, 11.0, 12.0, 14.0, -3.0]), rng.normal(0, 1.5)
            vx, vy = rng.normal(0, 1.0, 2)
            ext = rng.uniform(0.3, 0.6)
            at = (x + d * math.cos(th) - off * math.sin(th), y + d * math.sin(th) + off * math.cos(th))
            if q < nk:
                b["walker"][w, q], b["walker_lane"][w, q] = (at[0] - vx * tau, at[1] - vy * tau, vx, vy, ext), rng.choice([1, 1, 1, 1, 2, -1])
            else:
                b["walker"][w, q], b["walker_lane"][w, q] = (x, y, NAN, 0.0, NAN), 1
        for i in range(n):
            u = rng.random()
            b["last_light"][w, i] = -1 if u < 0.6 else (int(rng.integers(0, nl)) if u < 0.75 and nl else int(rng.choice([-7, nl, nl + 3, 64, 9999])))
    return b


def gpu_batch(k):
    """Batch k of the GPU suite's twelve: (batch, tick0)."""
    rng = np.random.default_rng(SEED * 1000 + k)
    b = bc.random_worlds(SIZES, 64, 3, 40, seed=SEED * 100 + k)
    return add_hazards(b, LIGHTS, WALKERS, 64, 64, TICK0[k], rng), TICK0[k]


def world_of(b, w, n):
    return dict(bc.world_of(b, w, n), n_light=b["n_light"][w], light=b["light"][w], light_lane=b["light_lane"][w], light_cycle=b["light_cycle"][w],
                n_walker=b["n_walker"][w], walker=b["walker"][w], walker_lane=b["walker_lane"][w])


def port_behave(prm, prb, hpp, b, tick0=0, fill=None):
    """emp_agent_behave_hazards through the port: a dict of its outputs (W, N, ...), padding slots as in `fill` (default: the inputs
    for the agent state and last_light, 0 elsewhere), `margin` (W, N), the smallest margin of a comparison in the slot's tick, and
    `sticky`, `ignored`, `filter` (W, N) bool: the branches the tick met."""
    W, N = b["n_path"].shape
    out = {k: np.array(b[k], copy=True) for k in bc.STATE_OUT + ("last_light",)}
    out.update(status=np.zeros((W, N), np.int32), control=np.zeros((W, N, 3)), mode=np.zeros((W, N), np.int32), blocker=np.zeros((W, N), np.int32),
               distance=np.zeros((W, N)), ttc=np.zeros((W, N)), target_speed_out=np.zeros((W, N)), lat_error=np.zeros((W, N)),
               lon_command=np.zeros((W, N)), cause=np.zeros((W, N), np.int32), light_hit=np.zeros((W, N), np.int32),
               walker_hit=np.zeros((W, N), np.int32), walker_distance=np.zeros((W, N)))
    if fill:
        for k, v in fill.items():
            out[k] = np.array(v, copy=True)
    out["margin"] = np.full((W, N), np.inf)
    for k in ("sticky", "ignored", "filter"):
        out[k] = np.zeros((W, N), bool)
    for w in range(W):
        n = min(max(int(b["n_world"][w]), 0), N)
        agents = ap.agents_of(*[b[k][w, :n] for k in bc.STATE_OUT])
        margins, notes = [[] for _ in range(n)], [[] for _ in range(n)]
        last = [int(v) for v in b["last_light"][w, :n]]
        rows = hp.world_tick(prm, prb, hpp, world_of(b, w, n), agents, last, tick0, margins, notes)
        packed = ap.pack(agents, b["lon_err"][w, :n], b["lat_err"][w, :n]) if n else {}
        for k in bc.STATE_OUT:
            if n:
                out[k][w, :n] = packed[k]
        for i, r in enumerate(rows):
            out["status"][w, i], out["control"][w, i], out["mode"][w, i], out["blocker"][w, i] = r["status"], r["control"], r["mode"], r["blocker"]
            out["distance"][w, i], out["ttc"][w, i], out["target_speed_out"][w, i] = r["distance"], r["ttc"], r["target"]
            out["lat_error"][w, i], out["lon_command"][w, i] = r["lat_error"], r["lon_command"]
            for k in HAZARD_OUT:
                out[k][w, i] = r[k]
            out["margin"][w, i] = min(margins[i]) if margins[i] else np.inf
            for k in ("sticky", "ignored", "filter"):
                out[k][w, i] = k in notes[i]
    return out


live_mask = bc.live_mask


# ---- hand-built worlds on the thresholds ----------------------------------------------------------------------------------------------
EDGE_M = 12


def edge_cases():
    """(batch, names, tick0): one world per case, N = 2, K = 1, two lights, two walkers.  The ego is slot 0 at (0, 0) facing +x at
    36 km/h with limit 60 (th = 20 m) and extent 2 on a straight plan from (-2, 0) with head 1: its lane waypoint is (-2, 0), its
    chord (2, 0).  A hazard is placed by distance and bearing from the ego."""
    cases = []

    def add(name, lights=(), walkers=(), ego=None, tick0=0, last=-1, cands=()):
        cases.append(dict(name=name, lights=lights, walkers=walkers, ego=ego or {}, tick0=tick0, last=last, cands=cands))

    def light(dist, deg, dx=1.0, dy=0.0, key=1, cycle=(1, 0, 1)):
        r = math.radians(deg)
        return dict(x=dist * math.cos(r), y=dist * math.sin(r), dx=dx, dy=dy, key=key, cycle=cycle)

    def walker(dist, deg, ext=0.5, key=1, vx=0.0, vy=0.0, **kw):
        r = math.radians(deg)
        return dict(dict(x=dist * math.cos(r), y=dist * math.sin(r), vx=vx, vy=vy, ext=ext, key=key), **kw)

    up, dn = (lambda v: math.nextafter(v, math.inf)), (lambda v: math.nextafter(v, -math.inf))
    # the light's range: the waypoint stands on the y axis side so that the norm is exact (x = 0), and the ego looks along (0.6, 0.8)
    look = dict(c=0.6, s=0.8)
    for name, d in (("light norm == th", 5.0), ("light norm one ulp above th", up(5.0)), ("light norm one ulp below th", dn(5.0))):
        add(name, [dict(x=0.0, y=d, dx=1.0, dy=0.0, key=1, cycle=(1, 0, 1))], ego=look)
    for name, d in (("light norm == 0.001", 0.001), ("light norm one ulp below 0.001", dn(0.001)), ("light norm one ulp above 0.001 behind", up(0.001))):
        add(name, [dict(x=-d, y=0.0, dx=1.0, dy=0.0, key=1, cycle=(1, 0, 1))])
    add("light angle exactly 0: not seen", [dict(x=3.0, y=0.0, dx=1.0, dy=0.0, key=1, cycle=(1, 0, 1))])
    add("light angle just above 0", [dict(x=3.0, y=1e-6, dx=1.0, dy=0.0, key=1, cycle=(1, 0, 1))])
    add("light angle exactly 90: not seen", [dict(x=0.0, y=3.0, dx=1.0, dy=0.0, key=1, cycle=(1, 0, 1))])
    for name, deg in (("light angle near 90 inside", 89.999999), ("light angle near 90 outside", 90.000001), ("light angle 60.000001: seen", 60.000001)):
        add(name, [light(3.0, deg)])
    add("light dot == 0: not passed over", [light(3.0, 20.0, dx=0.0, dy=1.0)])
    add("light dot just below 0", [light(3.0, 20.0, dx=-1e-300, dy=1.0)])
    add("light dot -0.0: not passed over", [light(3.0, 20.0, dx=-0.0, dy=1.0)])
    add("light NaN direction: not passed over", [light(3.0, 20.0, dx=NAN, dy=0.0)])
    add("light on another key", [light(3.0, 20.0, key=2)])
    add("light keyed -1", [light(3.0, 20.0, key=-1)], ego=dict(lane_key=-1))
    add("light on key_next only", [light(3.0, 20.0, key=7)], ego=dict(lane_from=4, lane_key7=True))
    # the phase: period 10, red [3, 6)
    for name, k, in (("phase at red_from", 3), ("phase below red_from", 2), ("phase at red_to - 1", 5), ("phase at red_to", 6),
                     ("phase wraps: k mod period", 10 * 1000003 + 4), ("phase wraps to green", 10 * 1000003 + 6)):
        add(name, [light(3.0, 20.0, cycle=(10, 3, 6))], tick0=k)
    add("period 0: never red", [light(3.0, 20.0, cycle=(0, 0, 1))])
    add("period below 0: never red", [light(3.0, 20.0, cycle=(-4, 0, 1))], tick0=3)
    add("red_to beyond the period", [light(3.0, 20.0, cycle=(4, 2, 99))], tick0=7)
    add("two lights hit: the first wins", [light(4.0, 30.0), light(2.0, 10.0)])
    add("the first light is green: the second is taken", [light(4.0, 30.0, cycle=(2, 1, 2)), light(2.0, 10.0)], tick0=2)
    # the sticky light
    add("sticky: held by a red light far behind", [light(400.0, 180.0)], last=0)
    add("sticky: light 1 holds though light 0 would hit", [light(3.0, 20.0), light(400.0, 180.0)], last=1)
    add("sticky light went green: the scan finds the other", [light(400.0, 180.0, cycle=(2, 1, 2)), light(3.0, 20.0)], last=0, tick0=2)
    add("sticky light went green: nothing else", [light(400.0, 180.0, cycle=(2, 1, 2))], last=0, tick0=2)
    for name, v in (("last_light == n_light: counts as -1", 1), ("last_light far out of range", 9999), ("last_light -2", -2),
                    ("last_light INT_MIN", -2 ** 31)):
        add(name, [light(400.0, 180.0)], last=v)
    add("last_light points past n_light at a poisoned row", [light(400.0, 180.0)], last=1)
    add("DONE: lights and last_light are left alone", [light(3.0, 20.0)], ego=dict(done=True), last=9999)
    add("no plan: DONE", [light(3.0, 20.0)], ego=dict(n_path=0), last=0)
    add("n_path == 1: ve is (0, 0), the dot is 0", [light(3.0, 20.0, dx=-1.0, dy=0.0)], ego=dict(n_path=1, head=0))
    add("head 0: the chord is the first", [light(3.0, 20.0)], ego=dict(head=0))
    add("head n_path - 1: the chord is the last", [light(3.0, 20.0)], ego=dict(head=EDGE_M - 1))
    # walkers: the lane waypoint is (-2, 0); the 10 m filter is measured from there
    # (a 6-8-10 triangle from the waypoint, so that the filter's distance is exact; the ego looks along (0.6, 0.8))
    for name, y in (("filter == 10: rejected", 8.0), ("filter just below 10", 8.0 - 1e-9), ("filter just above 10", 8.0 + 1e-9)):
        add(name, walkers=[dict(x=4.0, y=y, vx=0.0, vy=0.0, ext=0.5, key=1)], ego=look)
    add("walker inside cone and th, outside the radius", walkers=[walker(15.0, 10.0)])
    # the walker's range: th = 20; the walker stands on the lane waypoint and the ego 12-16-20 away from it, so that the norm is exact
    for name, y in (("walker norm == th", 16.0), ("walker norm just above th", 16.0 + 1e-9), ("walker norm just below th", 16.0 - 1e-9)):
        add(name, walkers=[dict(x=-2.0, y=0.0, vx=0.0, vy=0.0, ext=0.5, key=1)], ego=dict(x=-14.0, y=-y))
    add("walker norm one ulp below 0.001", walkers=[dict(x=-dn(0.001), y=0.0, vx=0.0, vy=0.0, ext=0.5, key=1)])
    add("walker angle exactly 0: not seen", walkers=[dict(x=7.0, y=0.0, vx=0.0, vy=0.0, ext=0.5, key=1)])
    for name, deg in (("walker angle near 60 inside", 59.999999), ("walker angle near 60 outside", 60.000001), ("walker behind", 170.0)):
        add(name, walkers=[walker(7.0, deg)])
    # d against braking_distance: the walker stands on the x axis so that the distance is exact: d = dist + eps - 0.5 - 2
    skew = dict(c=math.cos(-0.1), s=math.sin(-0.1))
    for name, dist in (("walker d == braking_distance: ignored", 7.5), ("walker d one ulp below", dn(7.5)), ("walker d one ulp above", up(7.5))):
        add(name, walkers=[dict(x=dist, y=0.0, vx=0.0, vy=0.0, ext=0.5, key=1)], ego=skew)
    add("two walkers hit: the first wins though the second is nearer", walkers=[walker(7.9, 20.0), walker(4.0, 10.0)])
    add("the first walker is keyed -1", walkers=[walker(7.9, 20.0, key=-1), walker(4.0, 10.0)])
    add("the first walker is on another lane", walkers=[walker(7.9, 20.0, key=2), walker(4.0, 10.0)])
    add("walker on key_next", walkers=[walker(4.0, 10.0, key=7)], ego=dict(lane_from=4, lane_key7=True))
    add("walker walks into range at tick0", walkers=[dict(x=4.0, y=30.0, vx=0.0, vy=-2.9, ext=0.5, key=1)], tick0=200)
    add("an ignored walker, then the vehicle rule", walkers=[walker(7.9, 20.0)], cands=[dict(x=12.0 * math.cos(0.1), y=12.0 * math.sin(0.1))])
    add("an ignored walker, then the vehicle emergency", walkers=[walker(7.9, 20.0)], cands=[dict(x=8.0 * math.cos(0.1), y=8.0 * math.sin(0.1))])
    add("a red light comes before a walker", [light(3.0, 20.0)], [walker(4.0, 10.0)])
    add("alone")
    for fld in ("x", "y", "c", "s", "limit", "ext"):
        add(f"NaN ego {fld}", [light(3.0, 20.0)], [walker(4.0, 10.0)], ego={fld: NAN})
    for fld in ("x", "y"):
        add(f"NaN light {fld}", [dict(light(3.0, 20.0), **{fld: NAN}), light(2.0, 10.0)])
    for fld in ("x", "y", "vx", "ext"):
        add(f"NaN walker {fld}", walkers=[dict(walker(4.0, 10.0), **{fld: NAN}), walker(5.0, 12.0)])
    W, N, K, M, ML, MW = len(cases), 2, 1, EDGE_M, 2, 2
    b = blank(W, N, M, K, ML, MW)
    for w, c in enumerate(cases):
        e = dict(dict(x=0.0, y=0.0, c=1.0, s=0.0, kmh=36.0, limit=60.0, ext=2.0, n_path=M, done=False, head=1, lane_from=M, lane_key=1), **c["ego"])
        b["n_world"][w] = 1 + len(c["cands"])
        b["path"][w, 0, :, :2] = [(-2.0 + 2.0 * i, 0.0) for i in range(M)]
        b["n_path"][w, 0], b["head"][w, 0] = e["n_path"], (M if e["done"] else e["head"])
        b["lane"][w, 0] = e["lane_key"]
        if e.get("lane_key7"):
            b["lane"][w, 0, e["lane_from"]:] = 7
        b["state"][w, 0, :2], b["forward"][w, 0], b["speed_kmh"][w, 0] = (e["x"], e["y"]), (e["c"], e["s"]), e["kmh"]
        b["speed_limit"][w, 0], b["extent"][w, 0], b["past_steer"][w, 0] = e["limit"], e["ext"], 0.0
        b["n_lon"][w, 0], b["n_lat"][w, 0] = 0, 0
        b["last_light"][w, 0] = c["last"]
        for j, q in enumerate(c["cands"], 1):
            b["path"][w, j, :, :2] = [(q["x"] + 10.0 + 2.0 * i, q["y"]) for i in range(M)]
            b["n_path"][w, j], b["head"][w, j], b["lane"][w, j] = M, 0, 1
            b["state"][w, j, :2], b["forward"][w, j], b["speed_kmh"][w, j] = (q["x"], q["y"]), (1.0, 0.0), 18.0
            b["speed_limit"][w, j], b["extent"][w, j], b["past_steer"][w, j] = 60.0, 2.0, 0.0
            b["n_lon"][w, j], b["n_lat"][w, j], b["last_light"][w, j] = 0, 0, -1
        b["n_light"][w], b["n_walker"][w] = len(c["lights"]), len(c["walkers"])
        for q, r in enumerate(c["lights"]):
            b["light"][w, q], b["light_lane"][w, q], b["light_cycle"][w, q] = (r["x"], r["y"], r["dx"], r["dy"]), r["key"], r["cycle"]
        for q in range(len(c["lights"]), ML):                      # a poisoned row: on top of the ego, red for ever
            b["light"][w, q], b["light_lane"][w, q], b["light_cycle"][w, q] = (0.0, 0.0, NAN, NAN), 1, (1, 0, 1)
        for q, r in enumerate(c["walkers"]):
            b["walker"][w, q], b["walker_lane"][w, q] = (r["x"], r["y"], r["vx"], r["vy"], r["ext"]), r["key"]
        for q in range(len(c["walkers"]), MW):
            b["walker"][w, q], b["walker_lane"][w, q] = (0.0, 0.0, NAN, NAN, NAN), 1
    return b, [c["name"] for c in cases], [c["tick0"] for c in cases]
