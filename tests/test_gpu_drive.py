"""GPU suite of the fleet loop.  emp_drive_request against the reference's recorded results (tests/golden/drive/) and
tests/drive_port.py: indices and order exact, dis and speed bit for bit, prediction and world velocity to 1e-12; emp_drive - K
periods of [request, plan, adopt, T ticks] in one call - against the chain of the separate calls BIT FOR BIT on every output and
every log; a split run against one run; held plans and coasting vehicles; a call with a pipeline set; hostile arguments in a
child process; and the whole loop against a CPU loop, stage by stage (DESIGN.md 3.9 says why not end to end).

Set EMP_DRIVE_PRINT=1 to print every measured figure before it is asserted."""
from __future__ import annotations

import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import drive_port as port  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(ROOT, "tests", "golden", "drive", "drive_request.npz")
G = 80                      # global path nodes, 2 m apart
DT = 0.01


def say(*a):
    if os.environ.get("EMP_DRIVE_PRINT"):
        print(*a, flush=True)


@pytest.fixture(scope="module")
def pl():
    from emplanner_carla_amd.api import Planner
    return Planner(0)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


def to_np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def same_bits(a, b):
    a, b = np.ascontiguousarray(to_np(a)), np.ascontiguousarray(to_np(b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def up(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def close(a, b, tol=1e-12):
    a, b = to_np(a), to_np(b)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the request against the fixture and the port
# ---------------------------------------------------------------------------------------------------------------------
def request_batch(B, A):
    """B vehicles from the fixture's scenes, their actor lists cut to the first A: the reference's kept lists, filtered to
    indices below A, are the expected ones (the order is stable).  Slots at or beyond n_act are poisoned with NaN and 1e300; a
    vehicle whose A slots are all live claims n_act = 1000."""
    fx = fixture()
    pick = [4, 0, 13] if B <= 3 else [(7 * i + 3) % len(fx["n_act"]) for i in range(B)]
    pick = pick[:B]
    state = fx["state"][pick].copy()
    actors = fx["actors"][pick][:, :A].copy()
    n_act = np.minimum(fx["n_act"][pick], A).astype(np.int32)
    for b in range(B):
        actors[b, n_act[b]:] = np.where(np.arange(A - n_act[b])[:, None] % 2 == 0, np.nan, 1e300)
    claimed = n_act.copy()
    claimed[(n_act == A) & (np.arange(B) % 2 == 0)] = 1000
    accel = np.random.default_rng(B * 100 + A).normal(0, 1, (B, 2))
    return pick, state, accel, actors, n_act, claimed


@pytest.mark.parametrize("max_obs", [1, 8])
@pytest.mark.parametrize("A", [1, 7, 64])
@pytest.mark.parametrize("B", [1, 3, 70])
def test_request_matches_the_reference_and_the_port(pl, B, A, max_obs):
    from emplanner_carla_amd.api import drive_params
    fx = fixture()
    max_dyn = 4
    pick, state, accel, actors, n_act, claimed = request_batch(B, A)
    assert B > 1 or claimed[0] == 1000                       # the 64-actor scene fills every slot: its count is clamped
    prm = drive_params(advance_s=0.05)
    r = pl.drive_request(prm, state, accel, actors, claimed, max_obs, max_dyn, advance=True)
    want = port.request_batch(state, accel, actors, n_act, max_obs, max_dyn, port.params(advance_s=0.05))
    for b, k in enumerate(pick):
        ns, nd = int(fx["n_static"][k]), int(fx["n_dyn"][k])
        s_keep = [(i, d) for i, d in zip(fx["static_idx"][k, :ns], fx["static_dis"][k, :ns]) if i < A]
        d_keep = [(i, d, v) for i, d, v in zip(fx["dyn_idx"][k, :nd], fx["dyn_dis"][k, :nd], fx["dyn_speed"][k, :nd]) if i < A]
        assert r.n_static[b] == min(len(s_keep), max_obs) and r.n_dyn[b] == min(len(d_keep), max_dyn)
        assert r.req_status[b] == (1 if len(s_keep) > max_obs or len(d_keep) > max_dyn else 0)
        for q, (i, d) in enumerate(s_keep[:max_obs]):                  # the reference's order and its bits
            assert same_bits(r.static_xy[b, q], actors[b, i, :2]) and r.static_dis[b, q] == d, (b, q)
        for q, (i, d, v) in enumerate(d_keep[:max_dyn]):
            assert same_bits(r.dyn[b, q], np.array([actors[b, i, 0], actors[b, i, 1], d, v])), (b, q)
        assert r.n_obs[b] == (r.n_static[b] if s_keep and s_keep[0][1] <= 30.0 else 0)
        assert same_bits(r.dyn_dis_speed[b], np.array(d_keep[0][1:] if d_keep else (np.nan, np.nan)))
        assert close(r.start_xy[b], fx["pred"][k, :2]) and close(r.pred_fi[b], fx["pred"][k, 2])
    # the port: everything exact but what libm touches
    for name in ("static_xy", "static_dis", "dyn", "dyn_dis_speed", "origin_xy", "start_a", "actors_next"):
        assert same_bits(getattr(r, name), want[name]), name
    for name in ("n_static", "n_dyn", "n_obs", "req_status"):
        assert np.array_equal(getattr(r, name), want[name]), name
    assert same_bits(r.start_a, accel) and same_bits(r.origin_xy, state[:, :2])
    worst = max(np.abs(to_np(getattr(r, n)) - want[n]).max() for n in ("start_xy", "pred_fi", "start_v"))
    say(f"request B={B} A={A} max_obs={max_obs}: worst |GPU - port| in start_xy / pred_fi / start_v {worst:.3g}")
    assert close(r.start_xy, want["start_xy"]) and close(r.pred_fi, want["pred_fi"]) and close(r.start_v, want["start_v"])
    # device tensors, honest counts instead of 1000, and actors_next aliasing actors: the same bits
    dev_actors = up(actors)
    rd = pl.drive_request(prm, up(state), up(accel), dev_actors, up(n_act), max_obs, max_dyn, in_place=True)
    pl.synchronize()
    assert rd.actors_next is dev_actors
    for name in r.__dataclass_fields__:
        assert same_bits(getattr(rd, name), getattr(r, name)), name
    none = pl.drive_request(drive_params(), state, None, actors, n_act, max_obs, max_dyn)
    assert none.actors_next is None and not none.start_a.any() and same_bits(none.static_dis, r.static_dis)


# ---------------------------------------------------------------------------------------------------------------------
# 2. drive == the chain of the separate calls, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
MAX_OBS, MAX_DYN, A_FLEET = 4, 2, 5


def params(law):
    from emplanner_carla_amd import api
    p = api.dp_params()
    return dict(p=p, q=api.qp_params(), sp=api.smooth_params(), lat=api.mpc_params() if law == "mpc" else api.lqr_params(),
                pid=api.pid_params(), vp=api.vehicle_params(), M=api.max_path_points(p))


def straight(rot, x0, y0, n=G):
    s = np.arange(n) * 2.0
    return np.column_stack([x0 + s * math.cos(rot), y0 + s * math.sin(rot), np.full(n, rot), np.zeros(n)])


def at(path_row0, rot, ahead, side):
    return (path_row0[0] + ahead * math.cos(rot) - side * math.sin(rot), path_row0[1] + ahead * math.sin(rot) + side * math.cos(rot))


def fleet(B, T, M, short=None, seed=3):
    """Straight 80-node global paths of several headings; the vehicle 10 m along its path, a little beside it, at 8-12 m/s.
    Scene 0: a dynamic actor just inside the 50 m range and faster than the ego (it leaves the range after the first period) and
    a static one just beyond the 30 m gate that the ego closes in on (the gate opens) - so n_dyn and n_obs change between
    periods.  Other scenes: a static actor 25 m ahead 1 m to the side, a dynamic one ahead, idle slots poisoned."""
    rng = np.random.default_rng(seed)
    gp = np.zeros((B, G, 4))
    state = np.zeros((B, 6))
    actors = np.full((B, A_FLEET, 4), np.nan)
    n_act = np.zeros(B, np.int32)
    for b in range(B):
        rot = [0.3, -2.0, 1.4, 3.0, -0.7][b % 5]
        gp[b] = straight(rot, rng.uniform(-50, 50), rng.uniform(-50, 50))
        v = 8.0 + b
        state[b] = [*at(gp[b, 0], rot, 10.0, 0.2 * (-1) ** b), rot, 0.0, 0.0, v]
        step = v * DT * T                                      # the ego's advance per period
        c, s = math.cos(rot), math.sin(rot)
        if b == 0:
            actors[b, 0] = [*at(gp[b, 0], rot, 10.0 + 50.0 - 0.3 * 30.0 * DT * T, 0.2), 38.0 * c, 38.0 * s]
            actors[b, 1] = [*at(gp[b, 0], rot, 10.0 + 30.0 + 0.5 * step, 1.2), 0.0, 0.0]
            n_act[b] = 2
        else:
            actors[b, 0] = [*at(gp[b, 0], rot, 35.0, 1.0), 0.0, 0.0]
            actors[b, 1] = [*at(gp[b, 0], rot, 40.0, -1.5), 6.0 * c, 6.0 * s]
            actors[b, 2] = [*at(gp[b, 0], rot, 20.0, 9.0), 0.0, 0.0]
            n_act[b] = 3
    n_global = np.full(B, G, np.int32)
    if short is not None:
        n_global[short] = 40
    return dict(global_path=gp, n_global=n_global, state=state, accel=np.zeros((B, 2)), actors=actors, n_act=n_act,
                pre_match_index=np.full(B, 5, np.int32), track=np.zeros((B, M + 1, 4)), track_len=np.zeros(B, np.int32),
                held=np.zeros(B, np.int32), target_speed=3.6 * state[:, 5] + 1.0)


def run_drive(pl, law, f, K, T, dev=False, in_place=False, logs=True):
    from emplanner_carla_amd.api import drive_params
    pr = params(law)
    g = {k: (up(v) if dev else np.array(v, copy=True)) for k, v in f.items()}
    r = pl.drive(pr["p"], pr["q"], pr["sp"], drive_params(), pr["lat"], pr["pid"], pr["vp"], g["global_path"], g["n_global"], g["state"],
                 g["accel"], g["actors"], g["n_act"], g["pre_match_index"], g["track"], g["track_len"], g["held"], g["target_speed"],
                 K, T, MAX_OBS, MAX_DYN, lateral=law, in_place=in_place, logs=logs)
    pl.synchronize()
    if in_place:
        for name in ("state", "accel", "actors", "pre_match_index", "track", "track_len", "held"):
            assert getattr(r, name) is g[name], name
    return r


def carry(f, r):
    """The next call's inputs from a result."""
    g = dict(f)
    for name in ("state", "accel", "actors", "pre_match_index", "track", "track_len", "held"):
        g[name] = to_np(getattr(r, name)).copy()
    return g


def chain(pl, law, f, K, T):
    """What a user of the separate calls writes, one period at a time (NumPy arrays: every call stages them)."""
    from emplanner_carla_amd.api import drive_params
    pr = params(law)
    M, B = pr["M"], len(f["state"])
    state, accel, actors, prem = f["state"].copy(), f["accel"].copy(), f["actors"].copy(), f["pre_match_index"].copy()
    track, tlen, held = f["track"].copy(), f["track_len"].copy(), f["held"].copy()
    w_of = lambda s: pl.drive_request(drive_params(), s, None, actors, f["n_act"], MAX_OBS, MAX_DYN).start_v
    logs = {k: [] for k in ("log_state", "log_plan_status", "log_roll_status", "log_held", "log_counts", "log_traj", "log_traj_len")}
    every = max(T - 1, 1)
    for _ in range(K):
        rq = pl.drive_request(drive_params(advance_s=T * pr["vp"].dt), state, accel, actors, f["n_act"], MAX_OBS, MAX_DYN, advance=True)
        cy = pl.plan_cycle(pr["p"], pr["q"], pr["sp"], None, None, rq.origin_xy, rq.start_xy, rq.start_v, rq.start_a, rq.static_xy,
                           rq.n_obs, max_pts=M, dyn_dis_speed=rq.dyn_dis_speed, global_path=f["global_path"], n_global=f["n_global"],
                           pre_match_index=prem)
        valid = (cy.ref_status == 0) & ((cy.status & ~1) == 0)
        take = valid[:, None] & (np.arange(M + 1)[None, :] < np.clip(cy.traj_len, 0, M + 1)[:, None])
        track = np.where(take[:, :, None], cy.traj, track)
        tlen = np.where(valid, cy.traj_len, tlen).astype(np.int32)
        held = np.where(valid, 0, held + 1).astype(np.int32)
        ro = pl.rollout(pr["lat"], pr["pid"], pr["vp"], track, tlen, state, np.zeros(B, np.int32), f["target_speed"], np.zeros((B, 60)),
                        np.zeros(B, np.int32), T, lateral=law, log_every=every)
        logs["log_state"].append(state)
        logs["log_plan_status"].append(cy.status | cy.ref_status)
        logs["log_roll_status"].append(ro.status)
        logs["log_held"].append(held)
        logs["log_counts"].append(np.column_stack([rq.n_obs, rq.n_dyn]))
        logs["log_traj"].append(cy.traj)
        logs["log_traj_len"].append(cy.traj_len)
        seen_last = ro.log_state[0 if T == 1 else 1]
        accel = (w_of(ro.state) - w_of(seen_last)) / pr["vp"].dt
        state, actors, prem = ro.state, rq.actors_next, cy.match_index
    out = dict(state=state, accel=accel, actors=actors, pre_match_index=prem, track=track, track_len=tlen, held=held)
    out.update({k: np.array(v) for k, v in logs.items()})
    return out


def counts_change_on_the_port(f, r, T):
    """On the port: scene 0's n_obs or n_dyn differs between two periods (from the logged states and the advanced actors)."""
    actors, seen = f["actors"][0].copy(), []
    for k in range(len(r.log_state)):
        q = port.request(to_np(r.log_state)[k, 0], None, actors, f["n_act"][0], MAX_OBS, MAX_DYN)
        seen.append((q["n_obs"], q["n_dyn"]))
        actors = port.advance(actors, f["n_act"][0], T * DT)
    return seen


@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("law", ["mpc", "lqr"])
def test_drive_equals_the_chain_bit_for_bit(pl, law, B, T):
    K = 3
    f = fleet(B, T, params(law)["M"])
    want = chain(pl, law, f, K, T)
    r = run_drive(pl, law, f, K, T)
    seen = counts_change_on_the_port(f, r, T)
    say(f"drive {law} B={B} T={T}: scene 0 (n_obs, n_dyn) per period on the port {seen}; GPU {to_np(r.log_counts)[:, 0].tolist()}")
    assert len(set(seen)) > 1, "the per-period request is not exercised: the counts never change"
    assert [tuple(c) for c in to_np(r.log_counts)[:, 0]] == seen
    assert ((to_np(r.log_plan_status) & ~1) == 0).all() and (to_np(r.log_roll_status) == 0).all() and (to_np(r.track_len) > 10).all()
    for name in r.__dataclass_fields__:
        assert same_bits(getattr(r, name), want[name]), name
    rd = run_drive(pl, law, f, K, T, dev=True, in_place=True)
    for name in r.__dataclass_fields__:
        assert same_bits(getattr(rd, name), want[name]), f"{name} (device tensors, in place)"
    nolog = run_drive(pl, law, f, K, T, dev=True, logs=False)
    assert nolog.log_state is None and same_bits(nolog.state, want["state"]) and same_bits(nolog.track, want["track"])


# ---------------------------------------------------------------------------------------------------------------------
# 3. a split run equals one run
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True])
def test_split_run_equals_one_run(pl, in_place):
    T, law = 5, "mpc"
    f = fleet(5, T, params(law)["M"])
    whole = run_drive(pl, law, f, 5, T, dev=True)
    a = run_drive(pl, law, f, 2, T, dev=True, in_place=in_place)
    b = run_drive(pl, law, carry(f, a), 3, T, dev=True, in_place=in_place)
    for name in ("state", "accel", "actors", "pre_match_index", "track", "track_len", "held"):
        assert same_bits(getattr(b, name), getattr(whole, name)), name
    for name in ("log_state", "log_plan_status", "log_roll_status", "log_held", "log_counts", "log_traj", "log_traj_len"):
        assert same_bits(np.concatenate([to_np(getattr(a, name)), to_np(getattr(b, name))]), getattr(whole, name)), name


# ---------------------------------------------------------------------------------------------------------------------
# 4. refused plans: hold the track, or coast
# ---------------------------------------------------------------------------------------------------------------------
def test_a_refused_vehicle_holds_its_track_or_coasts(pl):
    law, K, T, B, bad = "mpc", 3, 5, 4, 2
    pr = params(law)
    M = pr["M"]
    f = fleet(B, T, M, short=bad)
    good = fleet(B, T, M)
    # a valid plan for every vehicle from the full paths: the initial track
    from emplanner_carla_amd.api import drive_params
    rq = pl.drive_request(drive_params(), good["state"], None, good["actors"], good["n_act"], MAX_OBS, MAX_DYN)
    cy = pl.plan_cycle(pr["p"], pr["q"], pr["sp"], None, None, rq.origin_xy, rq.start_xy, rq.start_v, rq.start_a, rq.static_xy, rq.n_obs,
                       max_pts=M, dyn_dis_speed=rq.dyn_dis_speed, global_path=good["global_path"], n_global=good["n_global"],
                       pre_match_index=good["pre_match_index"])
    assert (cy.ref_status == 0).all() and ((cy.status & ~1) == 0).all()
    held_f = dict(f, track=cy.traj.copy(), track_len=cy.traj_len.copy())
    r = run_drive(pl, law, held_f, K, T)
    assert ((r.log_plan_status[:, bad] & ~1) != 0).all() and list(r.log_held[:, bad]) == [1, 2, 3] and r.held[bad] == K
    others = [b for b in range(B) if b != bad]
    assert (r.log_held[:, others] == 0).all() and ((r.log_plan_status[:, others] & ~1) == 0).all()
    assert same_bits(r.track[bad], cy.traj[bad]) and r.track_len[bad] == cy.traj_len[bad]
    state = f["state"][bad:bad + 1].copy()
    for k in range(K):                                        # a plain rollout chain on that track, a new controller each period
        assert same_bits(r.log_state[k, bad], state[0])
        ro = pl.rollout(pr["lat"], pr["pid"], pr["vp"], cy.traj[bad:bad + 1], cy.traj_len[bad:bad + 1], state, np.zeros(1, np.int32),
                        f["target_speed"][bad:bad + 1], np.zeros((1, 60)), np.zeros(1, np.int32), T, lateral=law)
        assert ro.status[0] == 0 and r.log_roll_status[k, bad] == 0
        state = ro.state
    assert same_bits(r.state[bad], state[0])
    # without a track it coasts: the rollout flags it every period, zero controls leave Vx alone (drag = 0)
    c = run_drive(pl, law, f, K, T)
    assert c.track_len[bad] == 0 and (c.log_roll_status[:, bad] != 0).all() and list(c.log_held[:, bad]) == [1, 2, 3]
    assert c.state[bad, 5] == f["state"][bad, 5] and (c.log_state[:, bad, 5] == f["state"][bad, 5]).all()
    assert np.isfinite(c.state).all() and c.state[bad, 0] != f["state"][bad, 0]
    # "zero controls": drive has no control log, so the same is asked of a plain rollout on an empty track - and the coasting
    # vehicle's state is that rollout chain's, bit for bit
    cs = f["state"][bad:bad + 1].copy()
    for k in range(K):
        ro = pl.rollout(pr["lat"], pr["pid"], pr["vp"], np.zeros((1, M + 1, 4)), np.zeros(1, np.int32), cs, np.zeros(1, np.int32),
                        f["target_speed"][bad:bad + 1], np.zeros((1, 60)), np.zeros(1, np.int32), T, lateral=law, log_every=1)
        assert ro.status[0] != 0 and not ro.log_control.any()
        cs = ro.state
    assert same_bits(c.state[bad], cs[0])
    # its neighbours do not notice it
    sub = {k: v[others] for k, v in f.items()}
    n = run_drive(pl, law, sub, K, T)
    for name in c.__dataclass_fields__:
        full = to_np(getattr(c, name))
        assert same_bits(full[others] if name in ("state", "accel", "actors", "pre_match_index", "track", "track_len", "held")
                         else full[:, others], getattr(n, name)), name


# ---------------------------------------------------------------------------------------------------------------------
# 5. against the CPU loop
# ---------------------------------------------------------------------------------------------------------------------
CPU_B, CPU_K, CPU_T = 4, 3, 20
DRIFT_BAR_M = 0.0           # 10 x the largest difference measured on the MI355X, which is 0 m: see the CPU-loop test's docstring
RTOL = 1e-6                 # |a - b| <= max(1e-6 |b|, 1e-9), conftest.assert_rel


def cpu_fleet(M):
    """Straight paths, one static actor 25 m ahead and 1 m to the side, one dynamic actor ahead at 5 m/s."""
    f = fleet(CPU_B, CPU_T, M)
    for b in range(CPU_B):
        rot = f["global_path"][b, 0, 2]
        c, s = math.cos(rot), math.sin(rot)
        f["actors"][b] = np.nan
        f["actors"][b, 0] = [*at(f["global_path"][b, 0], rot, 35.0, 1.0 + 0.2 * (-1) ** b), 0.0, 0.0]
        f["actors"][b, 1] = [*at(f["global_path"][b, 0], rot, 45.0, -1.0), 5.0 * c, 5.0 * s]
        f["n_act"][b] = 2
    return f


def check_plan_stage_by_stage(pl, pr, g, rq, what):
    """The planning half of one period against oracle/ref_port, stage by stage, each stage of the port fed with the device's
    previous one (tests/test_gpu_cycle.py's form; tests/test_drive_host.py shows why end to end is not possible: the
    reference sizes a densified segment with int(15 -+ 1 ulp)).  -> the two-call cycle's result."""
    from conftest import assert_rel
    from oracle import ref_port as op
    B, M = len(g["state"]), pr["M"]
    ref, n_ref, match, _, st_ref = pl.reference_line(pr["sp"], g["global_path"], g["n_global"], rq.start_xy, g["pre_match_index"])
    assert (st_ref == 0).all()
    cy = pl.plan_cycle(pr["p"], pr["q"], pr["sp"], ref, n_ref, rq.origin_xy, rq.start_xy, rq.start_v, rq.start_a, rq.static_xy, rq.n_obs,
                       max_pts=M, dyn_dis_speed=rq.dyn_dis_speed)
    sm, os_, ol_, bsl, start = pl.frenet_project(ref, n_ref, rq.origin_xy, rq.start_xy, rq.start_v, rq.start_a, rq.static_xy, rq.n_obs)
    for b in range(B):
        w = f"{what} vehicle {b}"
        path = [tuple(r) for r in g["global_path"][b, :g["n_global"][b]]]
        pred, veh, v, acc = tuple(rq.start_xy[b]), tuple(rq.origin_xy[b]), tuple(rq.start_v[b]), tuple(rq.start_a[b])
        # front end (test_9.py:99-110)
        want_match, _ = op.find_match_points([pred], path, False, int(g["pre_match_index"][b]))
        assert match[b] == want_match[0], w
        want_line = np.asarray(op.smooth_reference_line(op.sampling(want_match[0], path)), np.float64)
        P = int(n_ref[b])
        assert P == len(want_line), w
        assert_rel(ref[b, :P, :3], want_line[:, :3], RTOL, f"{w}: reference line")
        # projection (:113-177) on the device's reference line
        line = [tuple(r) for r in ref[b, :P]]
        s_map = op.cal_s_map_fun(line, origin_xy=veh)
        assert_rel(sm[b, :P], np.asarray(s_map), RTOL, f"{w}: s_map")
        k = int(rq.n_obs[b])
        if k:
            ws, wl = op.cal_s_l_fun([tuple(x) for x in rq.static_xy[b, :k]], line, s_map)
            assert_rel(os_[b, :k], np.asarray(ws), RTOL, f"{w}: obstacle s")
            assert_rel(ol_[b, :k], np.asarray(wl), RTOL, f"{w}: obstacle l")
        bs, bl = op.cal_s_l_fun([pred], line, s_map)
        assert_rel(bsl[b], np.asarray([bs[0], bl[0]]), RTOL, f"{w}: begin s, l")
        l0, _, _, _, dl0, _, ddl0 = op.cal_s_l_deri_fun([pred], [v], [acc], line, pred)
        assert_rel(start[b, 1:], np.asarray([l0[0], dl0[0], ddl0[0]]), RTOL, f"{w}: start l, dl, ddl")
        # DP (:180) on the device's projection: identical rows, the same stations
        obs_s, obs_l = list(os_[b, :k]), list(ol_[b, :k])
        dyn = None if np.isnan(rq.dyn_dis_speed[b, 0]) else tuple(rq.dyn_dis_speed[b])
        for vs, vl in op.virtual_obstacles(float(start[b, 0]), v, dyn):
            obs_s.append(vs)
            obs_l.append(vl)
        dp_s, dp_l, rows, _ = op.DP_algorithm(obs_s, obs_l, *(float(x) for x in start[b]), _return_rows=True, _verbose=False)
        assert np.array_equal(cy.dp_rows[b], np.asarray(rows, np.float64)), f"{w}: DP rows"
        n = int(cy.dp_len[b])
        assert n == len(dp_s), f"{w}: densified points"
        assert_rel(cy.dp_s[b, :n], np.asarray(dp_s), RTOL, f"{w}: dp_s")
        assert_rel(cy.dp_l[b, :n], np.asarray(dp_l), RTOL, f"{w}: dp_l")
        # bounds, path QP, midpoints (:187-210) on the device's densified path
        ds, dl = list(cy.dp_s[b, :n:2]), list(cy.dp_l[b, :n:2])
        l_min, l_max = op.cal_lmin_lmax(ds, dl, obs_s, obs_l, 5, 5)
        ql, _, _, status = op.Quadratic_planning(l_min, l_max, *(float(x) for x in start[b, 1:]), _return_status=True)
        if status != "optimal":              # the reference ignores cvxopt's status and sends its last iterate; here the plan is refused
            assert cy.status[b] & 8, f"{w}: the port's path QP ends '{status}', the device must refuse the plan"
            continue
        assert cy.status[b] == 0, w
        path_s = [ds[0]] + [(ds[j] + ds[j - 1]) / 2 for j in range(1, len(ql))] + [ds[-1]]
        path_l = [ql[0]] + [(ql[j] + ql[j - 1]) / 2 for j in range(1, len(ql))] + [ql[-1]]
        m = len(path_s)
        assert cy.path_len[b] == m, w
        assert_rel(cy.path_s[b, :m], np.asarray(path_s), RTOL, f"{w}: path s")
        assert_rel(cy.path_l[b, :m], np.asarray(path_l), RTOL, f"{w}: path l")
        # Cartesian tail (:212-218) on the device's path: the trajectory by SURVEY 8(d)'s rule
        want = np.asarray(op.frenet_2_x_y_theta_kappa(float(bsl[b, 0]), float(bsl[b, 1]), list(cy.path_s[b, :m]), list(cy.path_l[b, :m]),
                                                      line, list(sm[b, :P])), np.float64)
        assert cy.traj_len[b] == len(want), w
        assert_rel(cy.traj[b, :len(want), :3], want[:, :3], RTOL, f"{w}: trajectory x, y, theta")
        assert_rel(cy.traj[b, :len(want), 3], want[:, 3], RTOL, f"{w}: trajectory kappa")
    return cy, match


def test_drive_against_the_cpu_loop(pl):
    """B = 4, K = 3, T = 20, MPC, straight paths, a static actor 25 m ahead and 1 m to the side, a dynamic one: `drive`
    against drive_port, oracle/ref_port (motion_planning_body's stages) and oracle/mpc_lateral.py + PID + tests/vehicle_port.py.

    The comparison is staged, in every period: the request against the port (as the request test); the plan against ref_port
    stage by stage, each stage of the port fed with the device's previous one - identical DP rows, equal point counts, every
    array and the trajectory by SURVEY 8(d)'s rule |a - b| <= max(1e-6 |b|, 1e-9); the T ticks against the CPU controller and
    plant started from the device's state on the device's track.  An unstaged loop cannot be held to any bar: the reference
    sizes each densified segment with int(end_s - start_s) = int(15 -+ 1 ulp) (path_planning.py:405, :423), so which stations
    its path has follows the last bits of the planning start's s, and two correct computations of that s differ there
    (tests/test_drive_host.py::test_the_reference_path_follows_the_last_bits_of_its_start reproduces it on the CPU: metres
    of difference from 1e-13 m).  The chain of GPU periods is tied together by the bit-for-bit tests above: three K = 1
    calls equal the one K = 3 call here as well.

    The drift bar: the largest position difference, over all periods and vehicles, between the device's state after a
    period's T ticks and the CPU loop's from the same start.  Measured once on the MI355X over the 3 x 4 period ends:
    0 m in every one (x and y identical to the bit; Vx is asserted identical as well), so 10 x the largest difference seen is
    0 m and the bar asks for identical positions (the cap for such a bar is 1e-3 m).  It holds the device's sin / cos and the
    host's libm to the same bits along 20 ticks, as tests/test_gpu_rollout.py's drift bar does along 300: it was measured
    with one toolchain and HAS TO BE RE-MEASURED (same rule) when the ROCm or the C library version changes.  In the same run
    the device refused vehicle 1's plan of period 2 (EMP_ST_QP_FAILED) where the port's path QP does not reach 'optimal'
    either: that vehicle holds its track for the period, here and in the CPU loop."""
    import vehicle_port as vp
    from emplanner_carla_amd.api import drive_params
    pr = params("mpc")
    f = cpu_fleet(pr["M"])
    whole = run_drive(pl, "mpc", f, CPU_K, CPU_T)
    g, drift, actors_cpu = dict(f), np.zeros((CPU_K, CPU_B)), f["actors"].copy()
    for k in range(CPU_K):
        rq = pl.drive_request(drive_params(), g["state"], g["accel"], g["actors"], g["n_act"], MAX_OBS, MAX_DYN)
        want = port.request_batch(g["state"], g["accel"], g["actors"], g["n_act"], MAX_OBS, MAX_DYN)
        for name in ("static_xy", "static_dis", "dyn", "dyn_dis_speed", "origin_xy", "start_a"):
            assert same_bits(getattr(rq, name), want[name]), (k, name)
        for name in ("n_static", "n_dyn", "n_obs", "req_status"):
            assert np.array_equal(getattr(rq, name), want[name]), (k, name)
        assert close(rq.start_xy, want["start_xy"]) and close(rq.start_v, want["start_v"]) and close(rq.pred_fi, want["pred_fi"])
        assert same_bits(g["actors"], actors_cpu)                              # the actors moved as the port moves them
        assert (rq.n_obs == 1).all() and (rq.n_dyn == 1).all()
        cy, match = check_plan_stage_by_stage(pl, pr, g, rq, f"period {k}")
        one = run_drive(pl, "mpc", g, 1, CPU_T)
        assert same_bits(one.log_traj[0], cy.traj) and same_bits(one.log_traj_len[0], cy.traj_len)     # the plan drive made
        valid = (cy.status & ~1) == 0
        say(f"cpu loop: period {k}: plan status {cy.status.tolist()}")
        assert valid.sum() >= CPU_B - 1 and (k > 0 or valid.all())
        assert np.array_equal(one.track_len, np.where(valid, cy.traj_len, g["track_len"])) and same_bits(one.pre_match_index, match)
        assert np.array_equal(one.held, np.where(valid, 0, g["held"] + 1))
        for b in range(CPU_B):                                                 # the T ticks on that plan, on the CPU
            S, _, _, _, fin = vp.closed_loop_mpc(vp.params(), one.track[b, :one.track_len[b]], g["state"][b], 0,
                                                 float(f["target_speed"][b]), CPU_T)
            drift[k, b] = math.hypot(one.state[b, 0] - fin[0], one.state[b, 1] - fin[1])
            w1, w0 = port.world_velocity(fin[2], fin[3], fin[5]), port.world_velocity(S[-1][2], S[-1][3], S[-1][5])
            assert close(one.accel[b], np.array([(w1[0] - w0[0]) / DT, (w1[1] - w0[1]) / DT]), 1e-9), (k, b)
            assert one.state[b, 5] == fin[5], (k, b)                            # Vx: + - * only
        actors_cpu = np.array([port.advance(actors_cpu[b], f["n_act"][b], CPU_T * DT) for b in range(CPU_B)])
        g = carry(g, one)
    for name in ("state", "accel", "actors", "pre_match_index", "track", "track_len", "held"):
        assert same_bits(g[name], getattr(whole, name)), name
    say(f"cpu loop: largest position difference after a period's {CPU_T} ticks {drift.max():.3g} m (bar {DRIFT_BAR_M:.3g} m); "
        f"per period {drift.max(1).tolist()}")
    assert DRIFT_BAR_M <= 1e-3
    assert drift.max() <= DRIFT_BAR_M


# ---------------------------------------------------------------------------------------------------------------------
# with a pipeline set the call fences, runs its periods one at a time and leaves the setting alone
# ---------------------------------------------------------------------------------------------------------------------
def test_drive_with_a_pipeline_set(pl):
    from emplanner_carla_amd.api import Planner
    law, K, T = "mpc", 2, 2
    f = fleet(5, T, params(law)["M"])
    want = run_drive(pl, law, f, K, T, dev=True)
    p2 = Planner(0)
    try:
        p2.set_pipeline(1)
        form = p2.pipeline_form()
        got = run_drive(p2, law, f, K, T, dev=True)
        assert p2.pipeline_form() == form
        for name in want.__dataclass_fields__:
            assert same_bits(getattr(got, name), getattr(want, name)), name
    finally:
        p2.close()


# ---------------------------------------------------------------------------------------------------------------------
# hostile arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_hostile_arguments_in_a_child_process():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "drive_fuzz_child.py")], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    tail = run.stdout[-3000:] + "\n" + run.stderr[-3000:]
    assert run.returncode == 0, f"the fuzz child died with {run.returncode}:\n{tail}"
    assert "DRIVE-FUZZ-OK" in run.stdout, tail
    last = run.stdout.strip().splitlines()[-1].split()
    assert int(last[1]) >= 60 and int(last[3]) >= 55, last
