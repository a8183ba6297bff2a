"""NumPy port of the exchange rule (csrc/emp_world_core.h: who sees whom in emp_world_exchange), as include/emplanner.h states it,
and the cases the CPU suite (tests/test_world_host.py: the g++ build of the core) and the GPU suite (tests/test_gpu_world.py) share.
The port does no arithmetic but d2 = (dx * dx) + (dy * dy) in binary64; an actor row is data it is given (``agent_observe``'s rows),
so the comparison with the device is bit for bit.  Test tool only."""
from __future__ import annotations

import numpy as np

ACT_TRUNCATED, NOT_LISTED, NO_WORLD = 1, 2, 4


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def world_egos(ego_off, w, B):
    e0 = clamp(int(ego_off[w]), 0, B)
    return e0, clamp(int(ego_off[w + 1]), e0, B)


def match(xy, path, n_global, pre_match_index, lane_window):
    """The windowed nearest match: the lowest index with the smallest d2 in [lo, hi]; a NaN never wins; all NaN: lo; n == 0: -1."""
    n = clamp(int(n_global), 0, len(path))
    if n == 0:
        return -1
    lo = clamp(int(pre_match_index), 0, n - 1)
    hi = min(lo + int(lane_window), n - 1)
    dx = path[lo:hi + 1, 0] - np.float64(xy[0])
    dy = path[lo:hi + 1, 1] - np.float64(xy[1])
    d2 = (dx * dx) + (dy * dy)
    best = None
    for i, d in enumerate(d2):
        if d == d and (best is None or d < d2[best]):
            best = i
    return lo + (0 if best is None else best)


def exchange(n_world, ego_off, ego_state, ego_extent, global_path, n_global, ego_lane, pre_match_index, agent_rows, ego_rows, max_act,
             max_other, see_egos=0, lane_window=50):
    """-> dict of actors (B, max_act, 4), n_act, other (W, max_other, 5), other_lane, n_other, wx_status, and match (B,) the index each
    listed ego's key was taken at (-1 where none).  agent_rows (W, N, 4) and ego_rows (B, 4): ``agent_observe``'s rows."""
    W, N = agent_rows.shape[:2]
    B = len(ego_state)
    actors, n_act = np.zeros((B, max_act, 4)), np.zeros(B, np.int32)
    other, other_lane = np.zeros((W, max_other, 5)), np.full((W, max_other), -1, np.int32)
    n_other, status, at = np.zeros(W, np.int32), np.zeros(B, np.int32), np.full(B, -1, np.int64)
    for w in range(W):
        nw = clamp(int(n_world[w]), 0, N)
        e0, e1 = world_egos(ego_off, w, B)
        for b in range(e0, e1):
            rows = [agent_rows[w, j] for j in range(nw)]
            if see_egos:
                rows += [ego_rows[j] for j in range(e0, e1) if j != b]
            n_act[b] = min(len(rows), max_act)
            for r, row in enumerate(rows[:max_act]):
                actors[b, r] = row
            status[b] = (ACT_TRUNCATED if len(rows) > max_act else 0) | (NOT_LISTED if b - e0 >= max_other else 0)
        no = min(e1 - e0, max_other)
        for j in range(no):
            b = e0 + j
            other[w, j, :4], other[w, j, 4] = ego_rows[b], ego_extent[b]
            at[b] = match(ego_state[b, :2], global_path[b], n_global[b], pre_match_index[b], lane_window)
            other_lane[w, j] = -1 if at[b] < 0 else ego_lane[b, at[b]]
        n_other[w] = no
    first, last = clamp(int(ego_off[0]), 0, B), clamp(int(ego_off[W]), 0, B)
    for b in range(B):
        if b < first or b >= last:
            actors[b], n_act[b], status[b] = 0.0, 0, NO_WORLD
    return dict(actors=actors, n_act=n_act, other=other, other_lane=other_lane, n_other=n_other, wx_status=status, match=at)


OUT = ("actors", "n_act", "other", "other_lane", "n_other", "wx_status")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def straight_path(G, x0=0.0, y0=0.0, step=2.0):
    s = np.arange(G) * step
    return np.column_stack([x0 + s, np.full(G, y0), np.zeros(G), np.zeros(G)])


def seeded(seed, W=3, N=4, per_world=(0, 1, 3), outside=1, G=12):
    """W worlds of up to N agents, per_world egos in each and `outside` egos behind every range; random rows (distinct, so a wrong
    gather order shows), wobbly paths, lane keys that differ per waypoint."""
    rng = np.random.default_rng(seed)
    B = sum(per_world) + outside
    off = np.concatenate([[0], np.cumsum(per_world)]).astype(np.int32)
    gp = np.stack([straight_path(G, rng.uniform(-20, 20), rng.uniform(-20, 20)) for _ in range(B)])
    gp[:, :, 1] += rng.normal(0.0, 0.3, (B, G))
    pre = rng.integers(-2, G + 2, B).astype(np.int32)
    st = np.zeros((B, 6))
    at = np.clip(pre + rng.integers(0, 4, B), 0, G - 1)
    st[:, :2] = gp[np.arange(B), at, :2] + rng.normal(0.0, 0.4, (B, 2))
    st[:, 2], st[:, 5] = rng.uniform(-3, 3, B), rng.uniform(0, 12, B)
    agents = np.zeros((W, N, 6))
    agents[..., :2], agents[..., 2], agents[..., 5] = rng.uniform(-30, 30, (W, N, 2)), rng.uniform(-3, 3, (W, N)), rng.uniform(0, 9, (W, N))
    return dict(n_world=rng.integers(0, N + 1, W).astype(np.int32), ego_off=off, ego_state=st, ego_extent=rng.uniform(1.5, 3.0, B),
                global_path=gp, n_global=rng.integers(G - 3, G + 1, B).astype(np.int32),
                ego_lane=rng.integers(0, 1000, (B, G)).astype(np.int32), pre_match_index=pre, agent_state=agents)


def gpu_case():
    """The GPU suite's sizes: W = 3, max_world = 4, egos per world 0, 1 and 3, one ego outside every range."""
    c = seeded(11)
    c["n_world"] = np.array([2, 4, 3], np.int32)
    return c


def rows_of(rng, shape):
    """Stand-ins for observe rows where no device is there to make them: random and distinct."""
    return rng.uniform(-100, 100, shape + (4,))


def hand_built():
    """name -> (case, settings, what must come out).  One world unless said; the ego stands at (x, 0) beside a straight path on y = 0."""
    G = 10

    def one(x=5.0, y=0.0, n_global=G, pre=0, n_world=2, egos=1, W=1, B=None, off=None, N=3):
        B = egos if B is None else B
        st = np.zeros((B, 6))
        st[:, 0], st[:, 1] = x, y
        return dict(n_world=np.full(W, n_world, np.int32), ego_off=np.array([0, egos] if off is None else off, np.int32), ego_state=st,
                    ego_extent=np.full(B, 2.0), global_path=np.stack([straight_path(G)] * B), n_global=np.full(B, n_global, np.int32),
                    ego_lane=np.tile(np.arange(100, 100 + G, dtype=np.int32), (B, 1)), pre_match_index=np.full(B, pre, np.int32),
                    agent_state=np.zeros((W, N, 6)))

    cases = {}
    cases["two waypoints at exactly equal distance: the lowest index wins"] = (one(x=5.0), dict(), dict(match=2))      # 4 and 6
    c = one(x=6.0)
    c["global_path"][0, 3, 0] = np.nan
    cases["a NaN waypoint inside the window"] = (c, dict(), dict(match=2))                                             # 4, not 6 (NaN)
    c = one(x=6.0, pre=2)
    c["global_path"][0, :, 1] = np.nan
    cases["all NaN: the window's first index"] = (c, dict(), dict(match=2))
    cases["the window cut by n_global"] = (one(x=18.0, n_global=6, pre=3), dict(lane_window=50), dict(match=5))
    cases["the window ends before the nearest waypoint"] = (one(x=18.0, pre=1), dict(lane_window=3), dict(match=4))
    cases["lane_window 0: the pre-match itself"] = (one(x=18.0, pre=1), dict(lane_window=0), dict(match=1))
    cases["pre_match_index negative"] = (one(x=0.4, pre=-7), dict(), dict(match=0))
    cases["pre_match_index past the end"] = (one(x=0.4, pre=99), dict(), dict(match=G - 1))
    cases["n_global == 0: key -1"] = (one(n_global=0), dict(), dict(match=-1, key=-1))
    cases["n_global beyond the row: clamped"] = (one(x=18.0, n_global=999), dict(), dict(match=9))
    cases["an empty world"] = (one(n_world=0, egos=2), dict(see_egos=1), dict(n_act=[1, 1]))
    cases["a world without egos"] = (one(egos=0, B=1), dict(), dict(status=[NO_WORLD], n_other=[0]))
    cases["an ego in no world"] = (one(egos=1, B=3, off=[1, 2]), dict(see_egos=1), dict(status=[NO_WORLD, 0, NO_WORLD], n_act=[0, 2, 0]))
    cases["max_act smaller than agents plus egos"] = (one(n_world=3, egos=3), dict(see_egos=1, max_act=4),
                                                      dict(status=[ACT_TRUNCATED] * 3, n_act=[4, 4, 4]))
    cases["max_act exactly agents plus egos"] = (one(n_world=3, egos=3), dict(see_egos=1, max_act=5), dict(status=[0] * 3, n_act=[5, 5, 5]))
    cases["more egos than max_other"] = (one(egos=4), dict(max_other=2), dict(status=[0, 0, NOT_LISTED, NOT_LISTED], n_other=[2]))
    cases["n_world beyond max_world: clamped"] = (one(n_world=99), dict(), dict(n_act=[3]))
    cases["n_world negative: clamped"] = (one(n_world=-5), dict(), dict(n_act=[0]))
    cases["two worlds share nothing"] = (one(W=2, egos=2, B=2, off=[0, 1, 2], n_world=1), dict(see_egos=1), dict(n_act=[1, 1], n_other=[1, 1]))
    return cases


SETTINGS = dict(max_act=6, max_other=3, see_egos=0, lane_window=50)


# ---- traffic for the GPU suite (NumPy only) -----------------------------------------------------------------------------------------
AGENT_BUFFER = 10
TRAFFIC_STATE = ("state", "head", "past_steer", "lon_err", "n_lon", "lat_err", "n_lat", "last_light")


def heading_path(x, y, rot, n, step=2.0):
    s = np.arange(n) * step
    return np.column_stack([x + s * np.cos(rot), y + s * np.sin(rot), np.full(n, rot), np.zeros(n)])


def place(x, y, rot, ahead, side):
    return x + ahead * np.cos(rot) - side * np.sin(rot), y + ahead * np.sin(rot) + side * np.cos(rot)


def traffic_of(worlds, N, M=40, extent=2.4):
    """worlds: per world a list of agents (x, y, rot, vx, speed_limit km/h, lane key), each at the start of its own straight path of M
    waypoints 2 m apart.  -> the arrays of ``traffic_rollout_hazards``; padding slots hold zeros and n_path 0."""
    W = len(worlds)
    t = dict(n_world=np.array([len(w) for w in worlds], np.int32), path=np.zeros((W, N, M, 4)), n_path=np.zeros((W, N), np.int32),
             lane=np.full((W, N, M), -1, np.int32), state=np.zeros((W, N, 6)), speed_limit=np.zeros((W, N)), extent=np.full((W, N), extent),
             head=np.zeros((W, N), np.int32), past_steer=np.zeros((W, N)), lon_err=np.zeros((W, N, AGENT_BUFFER)),
             n_lon=np.zeros((W, N), np.int32), lat_err=np.zeros((W, N, AGENT_BUFFER)), n_lat=np.zeros((W, N), np.int32),
             last_light=np.full((W, N), -1, np.int32))
    for w, agents in enumerate(worlds):
        for j, (x, y, rot, vx, limit, key) in enumerate(agents):
            t["path"][w, j], t["n_path"][w, j], t["lane"][w, j] = heading_path(x, y, rot, M), M, key
            t["state"][w, j], t["speed_limit"][w, j] = (x, y, rot, 0.0, 0.0, vx), limit
    return t


def live_mask(t):
    W, N = t["n_path"].shape
    return np.arange(N)[None, :] < np.clip(t["n_world"], 0, N)[:, None]


def chain_fleet(f, worlds_of_egos, N=4):
    """The GPU suite's world around tests/drive_timed_port.timed_fleet's egos `f`: ego b's world gets an agent where that fleet has
    its slow dynamic actor - 40 m along the ego's global path, 1.5 m to its right, at 6 m/s under a 25 km/h limit (so it stays near
    it) - on a lane key of its own.  worlds_of_egos: per world its ego indices (consecutive).  -> (traffic, ego extras)."""
    B = len(f["state"])
    worlds = []
    for egos in worlds_of_egos:
        agents = []
        for b in egos:
            x0, y0, rot = f["global_path"][b, 0, :3]
            agents.append((*place(x0, y0, rot, 40.0, -1.5), rot, 6.0, 25.0, 100 + b))
        worlds.append(agents)
    off = np.zeros(len(worlds_of_egos) + 1, np.int32)
    for w, egos in enumerate(worlds_of_egos):
        off[w], off[w + 1] = egos[0], egos[-1] + 1
    lane = np.tile((100 + np.arange(B, dtype=np.int32))[:, None], (1, f["global_path"].shape[1]))
    return traffic_of(worlds, N), dict(ego_off=off, ego_extent=np.full(B, 2.0), ego_lane=lane)
