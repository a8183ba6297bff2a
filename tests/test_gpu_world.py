"""GPU suite of the shared world.  emp_world_exchange against ``agent_observe``'s rows gathered by the NumPy port
(tests/world_port.py), bit for bit; emp_traffic_rollout_epoch against emp_traffic_rollout_hazards (other_tick0 = 0: the same bits; the
others' epoch moved with the clock: the same bits on shifted light phases; a moving other: different); emp_world_drive - K periods of
[exchange, the timed drive's period, the agents' ticks] in one call - against the chain of the three public calls BIT FOR BIT on every
output and log; a split run; the world closed in both directions; hostile arguments in a child process.

Set EMP_DRIVE_PRINT=1 to print every measured figure before it is asserted."""
from __future__ import annotations

import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import drive_timed_port as tport  # noqa: E402
import test_gpu_drive as base  # noqa: E402  (its parameter and comparison helpers; its tests are not re-exported)
import world_port as wp  # noqa: E402

pytestmark = pytest.mark.gpu

say, to_np, same_bits, up = base.say, base.to_np, base.same_bits, base.up
MAX_OBS, MAX_DYN = tport.MAX_OBS, tport.MAX_DYN
EGO_STATE = ("state", "accel", "actors", "pre_match_index", "track", "track_len", "held", "profile", "cursor", "speed_held")
EGO_LOGS = ("log_state", "log_plan_status", "log_roll_status", "log_held", "log_counts", "log_traj", "log_traj_len", "log_speed_status",
            "log_speed_held", "log_tgt_status", "log_cursor")
TRAFFIC_LAST = ("status", "done_tick", "mode_ticks", "min_gap", "actors", "cause_ticks", "min_walker_gap")
WORLD_LOGS = ("log_wx_status", "log_n_act", "log_agent_state", "log_agent_status", "log_done_tick", "log_mode_ticks", "log_cause_ticks",
              "log_min_gap", "log_min_walker_gap")
LOG_OF = dict(log_agent_status="status", log_done_tick="done_tick", log_mode_ticks="mode_ticks", log_cause_ticks="cause_ticks",
              log_min_gap="min_gap", log_min_walker_gap="min_walker_gap")
NORMAL = 0


@pytest.fixture(scope="module")
def pl():
    from emplanner_carla_amd.api import Planner
    return Planner(0)


def conv(d, dev):
    return {k: (up(v) if dev else np.array(v, copy=True)) for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------------------------
# 1. the exchange against the composition
# ---------------------------------------------------------------------------------------------------------------------
def run_exchange(pl, c, dev, **kw):
    g = conv(c, dev)
    r = pl.world_exchange(g["n_world"], g["agent_state"], g["ego_off"], g["ego_state"], g["ego_extent"], g["global_path"], g["n_global"],
                          g["ego_lane"], g["pre_match_index"], **kw)
    pl.synchronize()
    return r


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("max_act", [8, 3])
@pytest.mark.parametrize("see_egos", [0, 1])
def test_exchange_equals_observe_gathered_by_the_port(pl, see_egos, max_act, dev):
    c = wp.gpu_case()
    W, N = c["agent_state"].shape[:2]
    B = len(c["ego_state"])
    assert (W, N, B) == (3, 4, 5) and np.diff(c["ego_off"]).tolist() == [0, 1, 3]
    agent_rows = to_np(pl.agent_observe(c["agent_state"].reshape(W * N, 6)).actors).reshape(W, N, 4)
    ego_rows = to_np(pl.agent_observe(c["ego_state"]).actors)
    kw = dict(max_act=max_act, max_other=2, see_egos=see_egos, lane_window=3)
    want = wp.exchange(c["n_world"], c["ego_off"], c["ego_state"], c["ego_extent"], c["global_path"], c["n_global"], c["ego_lane"],
                       c["pre_match_index"], agent_rows, ego_rows, **kw)
    got = run_exchange(pl, c, dev, **kw)
    say(f"exchange see_egos={see_egos} max_act={max_act}: n_act {to_np(got.n_act).tolist()}, status {to_np(got.wx_status).tolist()}, "
        f"n_other {to_np(got.n_other).tolist()}, keys {to_np(got.other_lane).tolist()}")
    for k in wp.OUT:
        assert same_bits(getattr(got, k), want[k]), k
    st = want["wx_status"]
    assert st[4] == wp.NO_WORLD and st[3] & wp.NOT_LISTED and not st[1] & wp.NOT_LISTED      # world 2 has 3 egos, max_other 2
    if max_act == 3:
        assert st[0] & wp.ACT_TRUNCATED and to_np(got.n_act).max() == 3, "max_act = 3 must truncate"
    else:
        assert not (st & wp.ACT_TRUNCATED).any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the epoch rollout
# ---------------------------------------------------------------------------------------------------------------------
EPOCH_T = 7


def epoch_scene():
    """W = 2 worlds of 4 agents on parallel roads 50 m apart (keys 0-3, world 1: 10-13), 5 m/s under 60 km/h.  Agent 0: an other
    12 m ahead, moving at 2 m/s; agent 1: a light 3 m ahead; agent 2: a standing walker 6 m ahead; agent 3: alone."""
    worlds = [[(0.0, 50.0 * j + 1000.0 * w, 0.0, 5.0, 60.0, 10 * w + j) for j in range(4)] for w in range(2)]
    t = wp.traffic_of(worlds, 4)
    y = lambda w, j: 50.0 * j + 1000.0 * w
    other = np.array([[[12.0, y(w, 0) + 0.3, 2.0, 0.0, 2.0], [500.0, y(w, 0), 0.0, 0.0, 2.0]] for w in range(2)])
    others = (np.array([2, 2], np.int32), other, np.array([[0, 0], [10, 10]], np.int32))
    light = np.array([[[3.0, y(w, 1) + 0.2, 1.0, 0.0], [400.0, y(w, 1), 1.0, 0.0]] for w in range(2)])
    cycle = np.array([[[100, 40, 60], [50, 37, 50]]] * 2, np.int32)            # light 0 turns red 3 ticks after tick 37
    lights = (np.array([2, 2], np.int32), light, np.array([[1, 1], [11, 11]], np.int32), cycle)
    walker = np.array([[[6.0, y(w, 2) + 0.5, 0.0, 0.0, 0.5]] for w in range(2)])
    walkers = (np.array([1, 1], np.int32), walker, np.array([[2], [12]], np.int32))
    return t, others, lights, walkers


def run_epoch(pl, t, others, lights, walkers, tick0, other_tick0, dev=True):
    from emplanner_carla_amd import api
    g = conv(t, dev)
    c = (lambda x: tuple(up(v) for v in x)) if dev else (lambda x: x)
    args = (api.agent_params(), api.behavior_params(), api.hazard_params(), api.agent_vehicle_params(), g["n_world"], g["path"], g["n_path"],
            g["lane"], g["state"], g["speed_limit"], g["extent"], g["head"], g["past_steer"], g["lon_err"], g["n_lon"], g["lat_err"],
            g["n_lat"], g["last_light"], EPOCH_T)
    kw = dict(lights=c(lights), walkers=c(walkers), others=c(others), tick0=tick0, log_every=1)
    r = pl.traffic_rollout_hazards(*args, **kw) if other_tick0 is None else pl.traffic_rollout_epoch(*args, other_tick0, **kw)
    pl.synchronize()
    return r


def test_epoch_rollout(pl):
    t, others, lights, walkers = epoch_scene()
    assert wp.live_mask(t).all()
    fields = list(run_epoch(pl, t, others, lights, walkers, 0, None).__dataclass_fields__)
    for dev in (True, False):
        for tick0 in (0, 37):
            plain, epoch0 = run_epoch(pl, t, others, lights, walkers, tick0, None, dev), run_epoch(pl, t, others, lights, walkers, tick0, 0, dev)
            for k in fields:
                assert same_bits(getattr(epoch0, k), getattr(plain, k)), f"other_tick0 = 0, tick0 = {tick0}: {k}"
    # the others' epoch moved with the clock: the hazards call at tick 0 on light phases shifted by 37
    n, light, key, cycle = lights
    shifted = cycle.copy()
    shifted[..., 1:] -= 37
    assert (shifted[..., 1] >= 0).all() and (shifted[..., 2] <= shifted[..., 0]).all(), "the shifted phases must not wrap"
    want = run_epoch(pl, t, others, (n, light, key, shifted), walkers, 0, None)
    got = run_epoch(pl, t, others, lights, walkers, 37, 37)
    for k in fields:
        assert same_bits(getattr(got, k), getattr(want, k)), f"tick0 = other_tick0 = 37: {k}"
    causes = to_np(got.cause_ticks)
    say(f"epoch: cause ticks {causes.tolist()}, min_gap {to_np(got.min_gap).tolist()}, min_walker_gap {to_np(got.min_walker_gap).tolist()}")
    assert causes[:, 1, 0].tolist() == [EPOCH_T - 3] * 2, "agent 1 is held by the light from the tick it turns red"
    assert (causes[:, 2, 1] == EPOCH_T).all() and np.isfinite(to_np(got.min_gap)[:, 0]).all()
    # a moving other stands elsewhere when its rows are 37 ticks old: 3.7 m further ahead, so the agent behind it follows where it
    # would slow down (the brake saturates either way over these 7 ticks: the states agree, the gaps and targets do not)
    old = run_epoch(pl, t, others, lights, walkers, 37, 0)
    say(f"epoch: min_gap with 37 ticks old rows {to_np(old.min_gap)[:, 0].tolist()}, targets {to_np(old.log_target)[:, 0, 0].tolist()} against "
        f"{to_np(got.log_target)[:, 0, 0].tolist()}")
    assert (to_np(old.min_gap)[:, 0] > to_np(got.min_gap)[:, 0] + 3.0).all()
    assert not same_bits(old.log_target, got.log_target) and not same_bits(old.log_mode, got.log_mode)
    assert same_bits(to_np(old.state)[:, 1:], to_np(got.state)[:, 1:])       # lights and walkers stayed on the clock


# ---------------------------------------------------------------------------------------------------------------------
# 3. world_drive == the chain of the three public calls, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
MAX_ACT, MAX_OTHER = 6, 4


def agent_blocks(dt):
    from emplanner_carla_amd import api
    return api.agent_params(dt=dt), api.behavior_params(), api.hazard_params(), api.agent_vehicle_params(dt=dt)


def chain_world(T, M):
    """timed_fleet's five egos in two worlds (3 + 2) of up to 4 agents, with a light and a walker where no agent meets them (the
    arrays travel, the agents drive)."""
    f = tport.timed_fleet(5, T, M)
    t, extra = wp.chain_fleet(f, [[0, 1, 2], [3, 4]])
    f = {k: v for k, v in f.items() if k not in ("actors", "n_act")}
    f.update(extra)
    lights = (np.array([1, 1], np.int32), np.array([[[1e4, 1e4, 1.0, 0.0]]] * 2), np.array([[100], [103]], np.int32),
              np.array([[[50, 0, 25]]] * 2, np.int32))
    walkers = (np.array([1, 0], np.int32), np.array([[[1e4, -1e4, 0.0, 0.0, 0.5]]] * 2), np.array([[101], [104]], np.int32))
    return f, t, lights, walkers


def run_world(pl, law, f, t, K, T, Ta, adt, tick0=0, atick0=0, dev=False, in_place=False, logs=True, see_egos=False, lights=None,
              walkers=None, max_act=MAX_ACT, max_other=MAX_OTHER):
    from emplanner_carla_amd.api import drive_params
    from test_gpu_drive_timed import speed_params
    pr = base.params(law)
    sdp, sqp = speed_params()
    ap, bp, hp, avp = agent_blocks(adt)
    g, a = conv(f, dev), conv(t, dev)
    c = (lambda x: None if x is None else tuple(up(v) for v in x)) if dev else (lambda x: x)
    r = pl.world_drive(pr["p"], pr["q"], pr["sp"], sdp, sqp, drive_params(), pr["lat"], pr["pid"], pr["vp"], ap, bp, hp, avp,
                       g["global_path"], g["n_global"], g["state"], g["accel"], g["pre_match_index"], g["track"], g["track_len"], g["held"],
                       g["t0"], g["profile"], g["cursor"], g["speed_held"], g["target_speed"], g["ego_off"], g["ego_extent"], g["ego_lane"],
                       a["n_world"], a["path"], a["n_path"], a["lane"], a["state"], a["speed_limit"], a["extent"], a["head"],
                       a["past_steer"], a["lon_err"], a["n_lon"], a["lat_err"], a["n_lat"], a["last_light"], K, T, Ta, MAX_OBS, max_act,
                       max_other, max_dyn=MAX_DYN, tick0=tick0, atick0=atick0, lights=c(lights), walkers=c(walkers), see_egos=see_egos,
                       lane_window=8, lateral=law, logs=logs, in_place=in_place)
    pl.synchronize()
    if in_place:
        for name in EGO_STATE:
            assert name == "actors" or getattr(r.egos, name) is g[name], name
        for name in wp.TRAFFIC_STATE:
            assert getattr(r.traffic, name) is a[name], name
    return r


def carry(f, t, r):
    f2, t2 = dict(f), dict(t)
    for name in EGO_STATE:
        if name != "actors":
            f2[name] = to_np(getattr(r.egos, name)).copy()
    for name in wp.TRAFFIC_STATE:
        t2[name] = to_np(getattr(r.traffic, name)).copy()
    return f2, t2


def chain(pl, law, f, t, K, T, Ta, adt, tick0, atick0, see_egos, lights, walkers, max_act=MAX_ACT, max_other=MAX_OTHER):
    """What a user of the three public calls writes, one period at a time (NumPy arrays: every call stages them)."""
    from emplanner_carla_amd.api import drive_params
    from test_gpu_drive_timed import speed_params
    pr = base.params(law)
    sdp, sqp = speed_params()
    ap, bp, hp, avp = agent_blocks(adt)
    s = {k: np.array(f[k], copy=True) for k in EGO_STATE if k != "actors"}
    a = {k: np.array(t[k], copy=True) for k in wp.TRAFFIC_STATE}
    logs = {k: [] for k in EGO_LOGS + WORLD_LOGS}
    ego = tr = None
    for k in range(K):
        a_k = atick0 + k * Ta
        ex = pl.world_exchange(t["n_world"], a["state"], f["ego_off"], s["state"], f["ego_extent"], f["global_path"], f["n_global"],
                               f["ego_lane"], s["pre_match_index"], max_act, max_other, see_egos=see_egos, lane_window=8)
        ego = pl.drive_timed(pr["p"], pr["q"], pr["sp"], sdp, sqp, drive_params(), pr["lat"], pr["pid"], pr["vp"], f["global_path"],
                             f["n_global"], s["state"], s["accel"], ex.actors, ex.n_act, s["pre_match_index"], s["track"], s["track_len"],
                             s["held"], f["t0"], s["profile"], s["cursor"], s["speed_held"], f["target_speed"], 1, T, MAX_OBS, MAX_DYN,
                             tick0=tick0 + k * T, lateral=law)
        tr = pl.traffic_rollout_epoch(ap, bp, hp, avp, t["n_world"], t["path"], t["n_path"], t["lane"], a["state"], t["speed_limit"],
                                      t["extent"], a["head"], a["past_steer"], a["lon_err"], a["n_lon"], a["lat_err"], a["n_lat"],
                                      a["last_light"], Ta, a_k, lights=lights, walkers=walkers, others=(ex.n_other, ex.other, ex.other_lane),
                                      tick0=a_k)
        for name in EGO_LOGS:
            logs[name].append(getattr(ego, name)[0])
        logs["log_wx_status"].append(ex.wx_status)
        logs["log_n_act"].append(ex.n_act)
        logs["log_agent_state"].append(a["state"])
        for name, src in LOG_OF.items():
            logs[name].append(getattr(tr, src))
        s = {name: getattr(ego, name) for name in s}
        a = {name: getattr(tr, name) for name in a}
    out = dict(egos={name: getattr(ego, name) for name in EGO_STATE}, traffic={name: getattr(tr, name) for name in wp.TRAFFIC_STATE + TRAFFIC_LAST})
    out["egos"].update({k: np.array(logs[k]) for k in EGO_LOGS})
    out.update({k: np.array(logs[k]) for k in WORLD_LOGS})
    return out


def assert_equals_chain(r, want, live, what, padding=True, logs=True):
    """Every output and log; padding=False (device tensors: the call never writes a padding slot of the caller's memory, and a new
    output tensor starts uninitialised there): the agents' arrays on the live slots only."""
    pick = (lambda x: to_np(x)) if padding else (lambda x: to_np(x)[live])
    for name in EGO_STATE + (EGO_LOGS if logs else ()):
        assert same_bits(getattr(r.egos, name), want["egos"][name]), f"{what}: egos.{name}"
    for name in wp.TRAFFIC_STATE + TRAFFIC_LAST:
        assert same_bits(pick(getattr(r.traffic, name)), pick(want["traffic"][name])), f"{what}: traffic.{name}"
    for name in WORLD_LOGS if logs else ():
        got, ref = to_np(getattr(r, name)), want[name]
        if name in ("log_wx_status", "log_n_act") or padding:
            assert same_bits(got, ref), f"{what}: {name}"
        else:
            assert same_bits(got[:, live], ref[:, live]), f"{what}: {name}"


@pytest.mark.parametrize("law,T,Ta,ratio", [("mpc", 1, 1, 1.0), ("mpc", 5, 5, 1.0), ("lqr", 1, 1, 1.0), ("lqr", 5, 5, 1.0),
                                            ("mpc", 5, 2, 2.5)])          # the last: dt_agent = 2.5 * vp.dt
def test_world_drive_equals_the_chain_bit_for_bit(pl, law, T, Ta, ratio):
    K, tick0, atick0 = 3, 7, 37
    pr = base.params(law)
    adt = ratio * pr["vp"].dt
    f, t, lights, walkers = chain_world(T, pr["M"])
    live = wp.live_mask(t)
    assert live.sum(1).tolist() == [3, 2] and np.diff(f["ego_off"]).tolist() == [3, 2] and t["state"].shape[:2] == (2, 4)
    kw = dict(lights=lights, walkers=walkers)
    want = chain(pl, law, f, t, K, T, Ta, adt, tick0, atick0, False, **kw)
    r = run_world(pl, law, f, t, K, T, Ta, adt, tick0, atick0, **kw)
    e = r.egos
    say(f"world_drive {law} T={T} Ta={Ta}: n_dyn per period {e.log_counts[:, :, 1].tolist()}, n_act {r.log_n_act.tolist()}, plan status "
        f"{e.log_plan_status.tolist()}, speed status {e.log_speed_status.tolist()}, speed_held {e.log_speed_held.tolist()}, "
        f"agent modes {r.log_mode_ticks[:, live].tolist()}")
    adopted = e.log_speed_held == 0
    assert adopted.mean() >= 0.5, "the comparison must compare plans, not refusals"
    assert (e.log_counts[:, :, 1] >= 1).any(), "an exchanged agent must be some ego's dynamic actor"
    assert (r.log_n_act == np.array([3, 3, 3, 2, 2])).all() and not r.log_wx_status.any()
    assert_equals_chain(r, want, live, "NumPy")
    rd = run_world(pl, law, f, t, K, T, Ta, adt, tick0, atick0, dev=True, in_place=True, **kw)
    assert_equals_chain(rd, want, live, "device tensors, in place", padding=False)
    nolog = run_world(pl, law, f, t, K, T, Ta, adt, tick0, atick0, dev=True, logs=False, **kw)
    assert nolog.log_wx_status is None and nolog.log_min_gap is None and nolog.egos.log_state is None
    assert_equals_chain(nolog, want, live, "no logs", padding=False, logs=False)


# ---------------------------------------------------------------------------------------------------------------------
# 4. a split run equals one run
# ---------------------------------------------------------------------------------------------------------------------
def test_split_run_equals_one_run(pl):
    law, T, Ta, tick0, atick0 = "mpc", 5, 5, 3, 20
    pr = base.params(law)
    adt = pr["vp"].dt
    f, t, _, walkers = chain_world(T, pr["M"])
    # a light 3 m in front of world 0's first agent, red for agent ticks [30, 50): the second part of the run meets it
    x, y, rot = t["state"][0, 0, :3]
    lights = (np.array([1, 0], np.int32), np.array([[[*wp.place(x, y, rot, 3.0, 0.2), math.cos(rot), math.sin(rot)]]] * 2),
              np.array([[100], [103]], np.int32), np.array([[[1000, 30, 50]]] * 2, np.int32))
    kw = dict(lights=lights, walkers=walkers, dev=True)
    whole = run_world(pl, law, f, t, 3, T, Ta, adt, tick0, atick0, **kw)
    a = run_world(pl, law, f, t, 1, T, Ta, adt, tick0, atick0, **kw)
    f2, t2 = carry(f, t, a)
    b = run_world(pl, law, f2, t2, 2, T, Ta, adt, tick0 + T, atick0 + Ta, **kw)
    live = wp.live_mask(t)
    for name in EGO_STATE:
        assert same_bits(getattr(b.egos, name), getattr(whole.egos, name)), name
    for name in wp.TRAFFIC_STATE + TRAFFIC_LAST:
        assert same_bits(to_np(getattr(b.traffic, name))[live], to_np(getattr(whole.traffic, name))[live]), name
    for name in EGO_LOGS:
        assert same_bits(np.concatenate([to_np(getattr(a.egos, name)), to_np(getattr(b.egos, name))]), getattr(whole.egos, name)), name
    for name in WORLD_LOGS:
        both = np.concatenate([to_np(getattr(a, name)), to_np(getattr(b, name))])
        if name in ("log_wx_status", "log_n_act"):
            assert same_bits(both, getattr(whole, name)), name
        else:
            assert same_bits(both[:, live], to_np(getattr(whole, name))[:, live]), name
    causes = to_np(whole.log_cause_ticks)[:, 0, 0, 0]
    say(f"split: light ticks of world 0's first agent per period {causes.tolist()}")
    assert causes.tolist() == [0, 0, Ta], "the light turns red at agent tick 30: the run's third period"
    # ... and the agents' clock matters: resumed with atick0 not advanced, the light stays green
    wrong = run_world(pl, law, f2, t2, 2, T, Ta, adt, tick0 + T, atick0, **kw)
    assert to_np(wrong.log_cause_ticks)[:, 0, 0, 0].tolist() == [0, 0]
    assert not same_bits(to_np(wrong.log_cause_ticks)[:, live], to_np(whole.log_cause_ticks)[1:][:, live])


# ---------------------------------------------------------------------------------------------------------------------
# 5. the world is closed
# ---------------------------------------------------------------------------------------------------------------------
LOOP_K, LOOP_T = tport.LOOP_K, tport.LOOP_T


def closed_world(M):
    """loop_fleet's straight-road setting, each vehicle on a road of its own 1000 m from the next.  Ego 0 (10 m/s, cap 50 km/h)
    follows agent 0, 20 m ahead on its lane key under a limit that keeps it near 3 m/s; ego 1 stands still 15 m ahead of agent 1,
    which arrives at 8 m/s under 60 km/h.  Egos 2 and 3 are in no world."""
    f = tport.loop_fleet(M)
    B, G = f["global_path"].shape[:2]
    for b in range(B):
        rot = f["global_path"][b, 0, 2]
        f["global_path"][b] = wp.heading_path(1000.0 * b, 0.0, rot, G)
        f["state"][b] = [*wp.place(1000.0 * b, 0.0, rot, 10.0, 0.0), rot, 0.0, 0.0, 10.0]
    rot0, rot1 = f["global_path"][0, 0, 2], f["global_path"][1, 0, 2]
    f["state"][1] = [*wp.place(1000.0, 0.0, rot1, 30.0, 0.3), rot1, 0.0, 0.0, 0.0]
    f["target_speed"][1] = 0.0
    agents = [(*wp.place(0.0, 0.0, rot0, 30.0, 0.3), rot0, 3.0, 14.0, 7), (*wp.place(1000.0, 0.0, rot1, 15.0, 0.0), rot1, 8.0, 60.0, 9)]
    t = wp.traffic_of([agents], 2)
    f = {k: v for k, v in f.items() if k not in ("actors", "n_act")}
    lane = np.zeros((B, G), np.int32)
    lane[0], lane[1], lane[2:] = 7, 9, 5
    f.update(ego_off=np.array([0, 2], np.int32), ego_extent=np.full(B, 2.0), ego_lane=lane)
    return f, t


def test_the_world_is_closed(pl):
    """In the world the ego slows down behind the agent and the agent slows down behind the ego; with no ego in any world (ego_off
    all zero) neither does.  The ego's Vx difference control - world after K = 3 periods of T = 20 ticks is printed with
    EMP_DRIVE_PRINT=1 and recorded in DESIGN 3.14; no margin is fixed here beyond its sign."""
    law = "mpc"
    pr = base.params(law)
    f, t = closed_world(pr["M"])
    adt = pr["vp"].dt
    world = run_world(pl, law, f, t, LOOP_K, LOOP_T, LOOP_T, adt)
    g = dict(f, ego_off=np.zeros(2, np.int32))
    control = run_world(pl, law, g, t, LOOP_K, LOOP_T, LOOP_T, adt)
    we, ce = world.egos, control.egos
    say(f"closed world: ego 0 Vx {we.state[0, 5]} in the world, {ce.state[0, 5]} alone (difference {ce.state[0, 5] - we.state[0, 5]} m/s); "
        f"n_dyn {we.log_counts[:, :, 1].tolist()} / {ce.log_counts[:, :, 1].tolist()}; agent 1 min_gap {world.log_min_gap[:, 0, 1].tolist()}, "
        f"mode ticks {world.log_mode_ticks[:, 0, 1].tolist()}; speed status {we.log_speed_status.tolist()}, wx {world.log_wx_status.tolist()}")
    assert (world.log_wx_status == [0, 0, wp.NO_WORLD, wp.NO_WORLD]).all() and (control.log_wx_status == wp.NO_WORLD).all()
    # the ego sees the agent ...
    assert (we.log_counts[:, 0, 1] >= 1).all() and (world.log_n_act[:, 0] == 2).all()
    assert ((we.log_plan_status[:, 0] & ~1) == 0).all() and (we.log_speed_status[:, 0] == 0).all(), "ego 0 must be tracking plans"
    assert we.state[0, 5] < ce.state[0, 5]
    # ... and the agent sees the ego
    assert np.isfinite(world.log_min_gap[:, 0, 1]).all() and (world.log_mode_ticks[:, 0, 1, NORMAL] < LOOP_T).all()
    assert world.traffic.state[0, 1, 5] < control.traffic.state[0, 1, 5]
    # alone: nothing is seen
    assert (ce.log_counts[:, :, 1] == 0).all() and (control.log_n_act == 0).all()
    assert np.isinf(control.log_min_gap).all() and (control.log_mode_ticks[:, :, :, NORMAL] == LOOP_T).all()
    assert (control.log_mode_ticks[:, :, :, 1:] == 0).all()
    # the egos in no world are the control's, bit for bit
    assert same_bits(we.state[2:], ce.state[2:]) and same_bits(we.log_traj[:, 2:], ce.log_traj[:, 2:])


def test_a_convoy_sees_itself_only_when_asked(pl):
    """Two egos on one lane, 30 m apart, the front one at 3 m/s: with see_egos the rear one has it as a dynamic actor."""
    law, T = "mpc", 5
    pr = base.params(law)
    f, _ = closed_world(pr["M"])
    f = {k: v[:2].copy() if k != "ego_off" else v for k, v in f.items()}
    f["global_path"][1] = f["global_path"][0]
    rot = f["global_path"][0, 0, 2]
    f["state"][1] = [*wp.place(0.0, 0.0, rot, 40.0, 0.3), rot, 0.0, 0.0, 3.0]
    f["target_speed"][1] = 11.0
    f["ego_lane"][:] = 7
    t = wp.traffic_of([[]], 1, M=2)
    seen = run_world(pl, law, f, t, 1, T, T, pr["vp"].dt, see_egos=True)
    blind = run_world(pl, law, f, t, 1, T, T, pr["vp"].dt, see_egos=False)
    say(f"convoy: n_dyn {seen.egos.log_counts[0, :, 1].tolist()} with see_egos, {blind.egos.log_counts[0, :, 1].tolist()} without")
    assert seen.egos.log_counts[0, 0, 1] >= 1 and seen.log_n_act[0].tolist() == [1, 1]
    assert (blind.egos.log_counts[0, :, 1] == 0).all() and (blind.log_n_act == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 6. hostile arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_hostile_arguments_in_a_child_process():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "world_fuzz_child.py")], capture_output=True, text=True, timeout=300,
                         cwd=ROOT)
    tail = run.stdout[-3000:] + "\n" + run.stderr[-3000:]
    assert run.returncode == 0, f"the fuzz child died with {run.returncode}:\n{tail}"
    assert "WORLD-FUZZ-OK" in run.stdout, tail
    last = run.stdout.strip().splitlines()[-1].split()
    assert int(last[1]) >= 40 and int(last[3]) >= 35, last
