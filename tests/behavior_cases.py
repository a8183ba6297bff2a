"""Inputs for the car-following law that the CPU suite (tests/test_behavior_host.py: the g++ build of csrc/emp_behavior_core.h) and
the GPU suite (tests/test_gpu_behavior.py) share: the fixtures of tests/golden/behavior/ and their replay through the port, ragged
random worlds with poison in every slot the rule must not read, and hand-built worlds on the rule's thresholds.  A batch is a dict
of the arrays emp_agent_behave takes, laid out (W, N, ...).  Test tool only."""
from __future__ import annotations

import math
import os
import sys

import numpy as np

from tests import agent_port as ap
from tests import behavior_port as bp
from tests.agent_cases import same_bits  # noqa: F401  (re-exported)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_golden_behavior as mkb  # noqa: E402

NAN = math.nan
IN_KEYS = ("n_world", "path", "n_path", "lane", "state", "forward", "speed_kmh", "speed_limit", "extent", "head", "past_steer", "lon_err",
           "n_lon", "lat_err", "n_lat", "n_other", "other", "other_lane")
STATE_OUT = ("head", "past_steer", "lon_err", "n_lon", "lat_err", "n_lat")
TICK_OUT = ("status", "control", "mode", "blocker", "distance", "ttc", "target_speed_out", "lat_error", "lon_command")
INT_OUT = ("head", "n_lon", "n_lat", "status", "mode", "blocker")
POISON_INT = -77


def fixture(name):
    """The arrays of a fixture as a dict (read once: an NpzFile would unpack an array again at every access)."""
    with np.load(os.path.join(GOLDEN, "behavior", name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def fixture_paths(f):
    return [np.c_[f["xy"][v, :f["n_path"][v]], np.zeros((f["n_path"][v], 2))] for v in range(len(f["n_path"]))]


def replay(name):
    """The port on the recorded inputs of a fixture, each vehicle with its own agent state: dict(control (T, V, 3), queue, target, mode,
    blocker (T, V)); rows of a vehicle that its agent does not drive hold the recorded values."""
    f = fixture(name)
    T, V = f["queue"].shape
    paths = fixture_paths(f)
    prm, prb = ap.params(), bp.params()
    agents = [ap.Agent() for _ in range(V)]
    out = dict(control=f["control"].copy(), queue=f["queue"].copy(), target=f["target"].copy(), mode=np.full((T, V), -1, np.int32),
               blocker=np.full((T, V), -1, np.int32), distance=np.full((T, V), np.inf))
    for t in range(T):
        heads = [g.head for g in agents]
        for i in range(V):
            if 0 <= f["brake_from"][i] <= t:
                agents[i].head = int(f["n_path"][i] - f["queue"][t, i])
                continue
            cands = [(f["seen"][t, j, 0], f["seen"][t, j, 1], f["seen"][t, j, 4], f["extent"][j],
                      bp.lane_key(f["lane"][j], f["n_path"][j], heads[j])) for j in range(V) if j != i]
            x, y, c, s, kmh = f["seen"][t, i]
            r = bp.behave(prm, prb, paths[i], f["lane"][i], f["n_path"][i], x, y, c, s, kmh, f["speed_limit"][i], f["extent"][i], cands, agents[i])
            out["control"][t, i], out["queue"][t, i], out["target"][t, i] = r["control"], f["n_path"][i] - agents[i].head, r["target"]
            out["mode"][t, i], out["blocker"][t, i], out["distance"][t, i] = r["mode"], r["blocker"], r["distance"]
    return f, out


def fixture_world(name):
    """A fixture's scenario as a one-world batch without forward / speed_kmh (the start of its closed loop)."""
    f = fixture(name)
    V, M = f["lane"].shape
    b = blank(1, V, M, 0)
    b["n_world"][0] = V
    b["path"][0, :, :, :2], b["path"][0, :, :, 2:] = f["xy"], 0.0
    b["n_path"][0], b["lane"][0], b["state"][0], b["speed_limit"][0], b["extent"][0] = f["n_path"], f["lane"], f["state0"], f["speed_limit"], f["extent"]
    b["head"][0], b["past_steer"][0], b["n_lon"][0], b["n_lat"][0] = 0, 0.0, 0, 0
    return f, b


def blank(W, N, M, K):
    """W worlds with nothing set: poison wherever the rule must not look."""
    return dict(n_world=np.zeros(W, np.int32), path=np.full((W, N, M, 4), NAN), n_path=np.full((W, N), 9999, np.int32),
                lane=np.full((W, N, M), 1, np.int32), state=np.full((W, N, 6), NAN), forward=np.full((W, N, 2), NAN),
                speed_kmh=np.full((W, N), NAN), speed_limit=np.full((W, N), NAN), extent=np.full((W, N), NAN),
                head=np.full((W, N), POISON_INT, np.int32), past_steer=np.full((W, N), NAN), lon_err=np.full((W, N, ap.BUFFER), NAN),
                n_lon=np.full((W, N), 99, np.int32), lat_err=np.full((W, N, ap.BUFFER), NAN), n_lat=np.full((W, N), POISON_INT, np.int32),
                n_other=np.zeros(W, np.int32), other=np.full((W, K, 5), NAN), other_lane=np.full((W, K), 1, np.int32))


def _track():
    return mkb.mk.polyline([("a", 100.0, 12.0)])                 # nearly two laps of a 100 m circle: 601 points 2 m apart


def random_worlds(sizes, N, K, M, seed):
    """Worlds of the given sizes on a circular track: vehicles 4 to 12 m apart in shuffled slots, mostly on lane 1, with ragged
    plans, heads and deques, and K slots of others near them."""
    rng = np.random.default_rng(seed)
    track = _track()
    W = len(sizes)
    b = blank(W, N, M, K)
    for w, n in enumerate(sizes):
        b["n_world"][w] = n if rng.random() < 0.8 else n + 1000 * (n == N)       # a count beyond the row is clamped
        at = (rng.integers(0, 30) + np.cumsum(rng.integers(2, 7, n))) % (len(track) - M - 1)
        slots = rng.permutation(n)
        for k, i in zip(at, slots):
            k = int(k)
            th = math.atan2(track[k + 1][1] - track[k][1], track[k + 1][0] - track[k][0]) + rng.normal(0, 0.05)
            off = rng.normal(0, 0.3)
            b["path"][w, i, :, :2] = track[k:k + M]
            b["n_path"][w, i] = rng.choice([M, M, M, M, M + 50, max(M - 3, 0), 2, 1, 0])
            b["lane"][w, i] = rng.choice([1, 1, 1, 1, 1, 1, 2, -1])
            if rng.random() < 0.2:
                b["lane"][w, i, M // 4:] = rng.choice([1, 2])
            b["state"][w, i] = (track[k][0] - off * math.sin(th), track[k][1] + off * math.cos(th), th, rng.normal(0, 0.1), rng.normal(0, 0.05),
                                rng.uniform(0, 14))
            b["speed_limit"][w, i] = rng.choice([23.0, 30.0, 60.0, 60.0, 90.0])
            b["extent"][w, i] = rng.uniform(1.0, 2.6)
            b["head"][w, i] = rng.choice([0, 0, 0, 1, 2, 3, -2, M, M + 7])
            b["past_steer"][w, i] = rng.uniform(-0.3, 0.3)
            for key in ("lon", "lat"):
                m = int(rng.choice([0, 1, 5, 9, 10]))
                b[key + "_err"][w, i, :m] = rng.uniform(-0.3, 0.3, m) * (10 if key == "lon" else 1)
                b["n_" + key][w, i] = m if rng.random() < 0.9 else (m and 10 + m)      # beyond 10: clamped (all ten must then be set)
                if b["n_" + key][w, i] > m:
                    b[key + "_err"][w, i, :] = rng.uniform(-0.3, 0.3, ap.BUFFER)
        obs = ap.observe_batch(b["state"][w, :n]) if n else None
        if n:
            b["forward"][w, :n], b["speed_kmh"][w, :n] = obs["forward"], obs["speed_kmh"]
        m = int(rng.integers(0, K + 1)) if K else 0
        b["n_other"][w] = m
        for o in range(m):
            k = int(rng.integers(0, len(track) - 2)) if not n else int(at[rng.integers(0, n)] + rng.integers(2, 6))
            th = math.atan2(track[k + 1][1] - track[k][1], track[k + 1][0] - track[k][0])
            v = rng.uniform(0, 8)
            b["other"][w, o] = (track[k][0], track[k][1], v * math.cos(th), v * math.sin(th), rng.uniform(1.0, 2.6))
            b["other_lane"][w, o] = rng.choice([1, 1, 2, -1])
    return b


def world_of(b, w, n):
    return dict(path=b["path"][w, :n], n_path=b["n_path"][w, :n], lane=b["lane"][w, :n], state=b["state"][w, :n], forward=b["forward"][w, :n],
                speed_kmh=b["speed_kmh"][w, :n], speed_limit=b["speed_limit"][w, :n], extent=b["extent"][w, :n],
                other=b["other"][w, :min(max(int(b["n_other"][w]), 0), b["other"].shape[1])], other_lane=b["other_lane"][w])


def port_behave(prm, prb, b, tick0=0, fill=None):
    """emp_agent_behave through the port: a dict of its outputs (W, N, ...), padding slots as in `fill` (a dict of arrays; default:
    the inputs for the agent state, 0 elsewhere), and `margin` (W, N): the smallest margin of a comparison in the slot's tick."""
    W, N = b["n_path"].shape
    out = {k: np.array(b[k], copy=True) for k in STATE_OUT}
    out.update(status=np.zeros((W, N), np.int32), control=np.zeros((W, N, 3)), mode=np.zeros((W, N), np.int32), blocker=np.zeros((W, N), np.int32),
               distance=np.zeros((W, N)), ttc=np.zeros((W, N)), target_speed_out=np.zeros((W, N)), lat_error=np.zeros((W, N)),
               lon_command=np.zeros((W, N)))
    if fill:
        for k, v in fill.items():
            out[k] = np.array(v, copy=True)
    out["margin"] = np.full((W, N), np.inf)
    for w in range(W):
        n = min(max(int(b["n_world"][w]), 0), N)
        agents = ap.agents_of(*[b[k][w, :n] for k in STATE_OUT])
        margins = [[] for _ in range(n)]
        rows = bp.world_tick(prm, prb, world_of(b, w, n), agents, tick0, margins)
        packed = ap.pack(agents, b["lon_err"][w, :n], b["lat_err"][w, :n]) if n else {}
        for k in STATE_OUT:
            if n:
                out[k][w, :n] = packed[k]
        for i, r in enumerate(rows):
            out["status"][w, i], out["control"][w, i], out["mode"][w, i], out["blocker"][w, i] = r["status"], r["control"], r["mode"], r["blocker"]
            out["distance"][w, i], out["ttc"][w, i], out["target_speed_out"][w, i] = r["distance"], r["ttc"], r["target"]
            out["lat_error"][w, i], out["lon_command"][w, i] = r["lat_error"], r["lon_command"]
            out["margin"][w, i] = min(margins[i]) if margins[i] else np.inf
    return out


def live_mask(b):
    W, N = b["n_path"].shape
    return np.arange(N)[None, :] < np.clip(b["n_world"], 0, N)[:, None]


# ---- hand-built worlds on the thresholds ----------------------------------------------------------------------------------------------
EDGE_M = 12


def edge_cases():
    """(batch, names): one world per case, N = 3, K = 2.  The ego is slot 0 at (0, 0) facing +x at 36 km/h with limit 60 (th = 20 m,
    normal target 50) on a straight plan from (10, 0); a candidate is placed by distance and bearing."""
    cases = []

    def add(name, cands=(), others=(), ego=None, tick0=0):
        cases.append(dict(name=name, cands=cands, others=others, ego=ego or {}, tick0=tick0))

    def at(dist, deg, kmh=18.0, ext=2.0, key=1, **kw):
        r = math.radians(deg)
        return dict(dict(x=dist * math.cos(r), y=dist * math.sin(r), kmh=kmh, ext=ext, key=key), **kw)

    up, dn = (lambda v: math.nextafter(v, math.inf)), (lambda v: math.nextafter(v, -math.inf))
    for name, d in (("norm == th", 20.0), ("norm one ulp above th", up(20.0)), ("norm one ulp below th", dn(20.0))):
        add(name, [dict(x=d * math.cos(0.2), y=d * math.sin(0.2), kmh=18.0, ext=2.0, key=1)])
    for name, d in (("norm == 0.001", 0.001), ("norm one ulp below 0.001", dn(0.001)), ("norm one ulp above 0.001 straight behind", up(0.001))):
        add(name, [dict(x=-d, y=0.0, kmh=18.0, ext=0.0, key=1)])
    add("angle exactly 0: not seen", [dict(x=12.0, y=0.0, kmh=18.0, ext=2.0, key=1)])
    add("angle just above 0", [dict(x=12.0, y=1e-6, kmh=18.0, ext=2.0, key=1)])
    for name, deg in (("angle near 30 inside", 29.999999), ("angle near 30 outside", 30.000001), ("behind", 170.0)):
        add(name, [at(12.0, deg)])
    # d against braking_distance: the ego's extent is 2, the candidate's 2: d = dist + eps - 4.  The candidate stands on the x axis, so
    # that the distance is exact, and the ego looks 0.1 rad to its right
    skew = dict(c=math.cos(-0.1), s=math.sin(-0.1))
    for name, dist in (("d == braking_distance", 9.0), ("d one ulp below", dn(9.0)), ("d one ulp above", up(9.0))):
        add(name, [dict(x=dist, y=0.0, kmh=18.0, ext=2.0, key=1)], ego=skew)
    # ttc = d / max(1, (36 - vs) / 3.6): vs = 18 gives dv = 5; d = 15, 30 puts ttc on safety_time and twice it
    for name, dist in (("ttc == safety_time", 19.0), ("ttc just below safety_time", 18.999), ("ttc just above safety_time", 19.001)):
        add(name, [dict(x=dist, y=0.0, kmh=18.0, ext=2.0, key=1)], ego=dict(skew, limit=90.0))
    for name, dist in (("ttc == 2 safety_time", 34.0), ("ttc just below 2 safety_time", 33.999), ("ttc just above 2 safety_time", 34.001)):
        add(name, [dict(x=dist, y=0.0, kmh=18.0, ext=2.0, key=1)], ego=dict(skew, limit=120.0))
    add("dv clipped to 1: the leader is faster", [at(14.0, 5.0, kmh=50.0)])
    add("positive() at 0: vs == speed_decrease", [at(12.0, 5.0, kmh=10.0)])
    add("positive() below 0", [at(12.0, 5.0, kmh=4.0)])
    add("follow below min_speed", [at(9.5, 5.0, kmh=2.0)], ego=dict(kmh=5.0))
    add("two hit: the first wins though the second is nearer", [at(15.0, 5.0), at(10.0, 4.0)])
    add("the first is keyed -1: the second is taken", [at(15.0, 5.0, key=-1), at(10.0, 4.0)])
    add("the first is on another lane", [at(15.0, 5.0, key=2), at(10.0, 4.0)])
    add("key_next matches", [at(15.0, 5.0, key=7)], ego=dict(lane_from=4, lane_key=7))
    add("a DONE blocker is still seen", [at(12.0, 5.0, done=True)])
    add("a blocker without a plan shows -1", [at(12.0, 5.0, n_path=0)])
    add("an other is hit", others=[at(12.0, 5.0)])
    add("an agent comes before an other", [at(15.0, 5.0)], others=[at(10.0, 4.0)])
    add("an other moves into range at tick0", others=[dict(x=40.0 * math.cos(0.1), y=40.0 * math.sin(0.1), vx=-2.5, vy=0.0, ext=2.0, key=1)], tick0=200)
    add("the ego is DONE", [at(12.0, 5.0)], ego=dict(done=True))
    add("the ego has no plan", [at(12.0, 5.0)], ego=dict(n_path=0))
    add("alone")
    for fld in ("x", "y", "c", "s", "kmh", "limit", "ext"):
        add(f"NaN ego {fld}", [at(12.0, 5.0)], ego={fld: NAN})
    for fld in ("x", "y", "kmh", "ext"):
        add(f"NaN candidate {fld}", [dict(at(12.0, 5.0), **{fld: NAN}), at(10.0, 4.0)])
    add("NaN other vx", others=[dict(at(12.0, 5.0), vx=NAN)])
    W, N, K, M = len(cases), 3, 2, EDGE_M
    b = blank(W, N, M, K)
    tick0 = []
    for w, c in enumerate(cases):
        e = dict(dict(x=0.0, y=0.0, c=1.0, s=0.0, kmh=36.0, limit=60.0, ext=2.0, n_path=M, done=False, lane_from=M, lane_key=1), **c["ego"])
        b["n_world"][w] = 1 + len(c["cands"])
        b["path"][w, 0, :, :2] = [(10.0 + 2.0 * i, 0.0) for i in range(M)]
        b["n_path"][w, 0], b["head"][w, 0] = e["n_path"], (M if e["done"] else 0)
        b["lane"][w, 0, e["lane_from"]:] = e["lane_key"]
        b["state"][w, 0, :2], b["forward"][w, 0], b["speed_kmh"][w, 0] = (e["x"], e["y"]), (e["c"], e["s"]), e["kmh"]
        b["speed_limit"][w, 0], b["extent"][w, 0], b["past_steer"][w, 0] = e["limit"], e["ext"], 0.0
        b["n_lon"][w, 0], b["n_lat"][w, 0] = 0, 0
        for j, q in enumerate(c["cands"], 1):
            b["path"][w, j, :, :2] = [(q["x"] + 10.0 + 2.0 * i, q["y"]) for i in range(M)]
            b["n_path"][w, j], b["head"][w, j] = q.get("n_path", M), (M if q.get("done") else 0)
            b["lane"][w, j] = q["key"]
            b["state"][w, j, :2], b["forward"][w, j], b["speed_kmh"][w, j] = (q["x"], q["y"]), (1.0, 0.0), q["kmh"]
            b["speed_limit"][w, j], b["extent"][w, j], b["past_steer"][w, j] = 60.0, q["ext"], 0.0
            b["n_lon"][w, j], b["n_lat"][w, j] = 0, 0
        b["n_other"][w] = len(c["others"])
        for o, q in enumerate(c["others"]):
            v = q["kmh"] / 3.6 if "kmh" in q and "vx" not in q else 0.0
            b["other"][w, o] = (q["x"], q["y"], q.get("vx", v), q.get("vy", 0.0), q["ext"])
            b["other_lane"][w, o] = q["key"]
        tick0.append(c["tick0"])
    return b, [c["name"] for c in cases], tick0
