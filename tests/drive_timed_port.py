"""Python-float port of what emp_drive_request_timed and emp_drive_timed add to the fleet loop (csrc/emp_drive_kernels.h:
drive_request_kernel<Clock>, drive_adopt_kernel<Speed>; csrc/emp_dp_launch.h: plan_drive_clock), written from the text of
include/emplanner.h: the clock rule, the speed planner's inputs the request hands over, and the adopt rule for the track and the
profile.  tests/drive_port.py is the untimed request.  Test tool only: the package never imports it."""
from __future__ import annotations

import math

import numpy as np

import drive_port as port

INT32_MAX = 2 ** 31 - 1
PLAN_LEAD = 0.1                     # emp_drive_timed_params_default (test_10.py:325)
PROFILE_SHAPE = (7, 401)
DP_INFEASIBLE = 1                   # EMP_ST_DP_INFEASIBLE: the one path status bit a valid plan may carry


def clock_refusal(tick0, K, T):
    """None, or why emp_drive_timed refuses this clock (plan_drive_clock)."""
    if K < 1 or T < 1:
        return "K and T must be at least 1"
    if tick0 < 0:
        return "tick0 must be at least 0"
    if tick0 + K * T > INT32_MAX:
        return "tick0 + K * T must not exceed INT32_MAX"
    return None


def period_tick(tick0, k, T):
    """Period k's first tick: integers, nothing accumulates."""
    return tick0 + k * T


def clock(t0, tick, dt):
    """emp_rollout_timed's clock: the product rounded, then the sum."""
    return float(t0) + float(tick) * float(dt)


def plan_start_time(t0, tick, dt, plan_lead=PLAN_LEAD):
    return clock(t0, tick, dt) + float(plan_lead)


def request_timed(state, accel, actors, n_act, max_obs, max_dyn, t0, tick, dt, plan_lead=PLAN_LEAD, prm=None):
    """One vehicle's emp_drive_request_timed: drive_port.request's dict and the three extras."""
    out = port.request(state, accel, actors, n_act, max_obs, max_dyn, prm)
    actors = np.asarray(actors, np.float64)
    out["dyn_obs"] = np.zeros((max_dyn, 4))
    for r, i in enumerate(out["dyn_idx"]):
        out["dyn_obs"][r] = actors[i]                      # x, y, vx, vy before the advance
    _, _, fi, Vy, _, Vx = (float(v) for v in state)
    wx, wy = port.world_velocity(fi, Vy, Vx)
    out["start_heading"] = math.atan2(wy, wx)
    out["plan_start_time"] = plan_start_time(t0, tick, dt, plan_lead)
    return out


def request_timed_batch(state, accel, actors, n_act, max_obs, max_dyn, t0, tick, dt, plan_lead=PLAN_LEAD, prm=None):
    rows = [request_timed(state[b], None if accel is None else accel[b], actors[b], n_act[b], max_obs, max_dyn, t0[b], tick, dt,
                          plan_lead, prm) for b in range(len(state))]
    return {k: ([r[k] for r in rows] if k.endswith("_idx") else np.array([r[k] for r in rows])) for k in rows[0]}


def adopt(traj, traj_len, status, ref_status, trajectory, speed_status, track, track_len, held, profile, cursor, speed_held):
    """The adopt rule for a batch, on copies: -> dict(track, track_len, held, profile, cursor, speed_held).  The track by
    emp_drive's rule; the profile only when the path is valid AND speed_status == 0, else it and its cursor stay and speed_held
    counts.  The two are independent."""
    traj, track, profile = np.asarray(traj), np.array(track, copy=True), np.array(profile, copy=True)
    rows = track.shape[1]
    valid = (np.asarray(ref_status) == 0) & ((np.asarray(status) & ~DP_INFEASIBLE) == 0)
    take = valid[:, None] & (np.arange(rows)[None, :] < np.clip(traj_len, 0, rows)[:, None])
    track = np.where(take[:, :, None], traj, track)
    both = valid & (np.asarray(speed_status) == 0)
    profile = np.where(both[:, None, None], np.asarray(trajectory), profile)
    return dict(track=track, track_len=np.where(valid, traj_len, track_len).astype(np.int32),
                held=np.where(valid, 0, np.asarray(held) + 1).astype(np.int32), profile=profile,
                cursor=np.where(both, 0, cursor).astype(np.int32),
                speed_held=np.where(both, 0, np.asarray(speed_held) + 1).astype(np.int32))


# -----------------------------------------------------------------------------------------------------------------------------
# the whole timed loop through the CPU oracle alone: one vehicle, K periods (tests/test_drive_timed_host.py's tracking scenario)
# -----------------------------------------------------------------------------------------------------------------------------
STB_RANGE, STB_INDEX, STB_QP_FAILED, STB_NO_PROFILE = 2, 4, 8, 64


def oracle_speed_plan(traj_nodes, start_v, start_a, heading, dyn_obs, plan_time, width):
    """test_10.py:233-340 on a planned trajectory (a list of (x, y, heading, kappa)), composed from the oracle's restatements in
    the order tests/test_gpu_trajectory.py::test_trajectory_vs_cpu_port uses: -> (speed_status, trajectory (7, 401) or None)."""
    from oracle import ref_port as rp
    from oracle import st_backend as be
    from oracle import st_speed as ss
    nan, tl, k, slots = math.nan, len(traj_nodes), len(dyn_obs), max(len(dyn_obs), 1)
    nodes = [tuple(float(v) for v in row) for row in traj_nodes]
    rows = np.full((4, width), nan)
    rows[:, :tl] = np.asarray(nodes).T
    i2s = rp.trajectory_index2s(rows[0], rows[1])
    tor = (math.cos(heading), math.sin(heading))
    s1 = tor[0] * start_v[0] + tor[1] * start_v[1]
    s2 = tor[0] * start_a[0] + tor[1] * start_a[1]
    obs = [np.full(slots, nan) for _ in range(4)]
    if k:
        xy = [(float(o[0]), float(o[1])) for o in dyn_obs]
        try:
            _, proj = rp.find_match_points(xy, nodes, False, 0)
        except IndexError:
            return STB_INDEX, None
        s_list, l_list = rp.cal_s_l_fun(xy, nodes, i2s)
        sd, ld, _ = rp.cal_dy_obs_deri(l_list, [o[2] for o in dyn_obs], [o[3] for o in dyn_obs], [p[2] for p in proj], [p[3] for p in proj])
        obs[0][:k], obs[1][:k], obs[2][:], obs[3][:] = s_list, l_list, sd[:slots], ld[:slots]
    segs = ss.port_generate_st_graph(*obs)
    dp = ss.exact_speed_dp(*(x[None] for x in segs), np.array([s1]))
    dp_s, dp_t = dp["speed_s"][0], dp["speed_t"][0]
    try:
        cs = be.port_generate_convex_space(dp_s, dp_t, i2s, *segs, rows[3])
    except ValueError:
        return STB_RANGE, None
    except IndexError:
        return STB_INDEX, None
    try:
        prof, res, _ = be.speed_qp(s1, s2, dp_s, dp_t, *cs)
    except IndexError:
        return STB_INDEX, None
    if res is None or res.status != "optimal":
        return STB_QP_FAILED, None
    if tl <= 1:
        return (STB_NO_PROFILE if tl == 0 else STB_RANGE), None
    dense = be.port_increase_points(*prof)
    return 0, np.stack(be.port_path_speed_merge(dense[0], dense[1], dense[2], dense[3], plan_time, i2s, *rows))


def oracle_loop(global_path, state, actors, n_act, pre_match, cap_kmh, t0, K, T, max_obs, max_dyn, width, timed=True, tick0=0, dt=0.01):
    """K periods of ONE vehicle on the CPU: drive_port's request, oracle/ref_port's planning body, the speed plan above, the adopt
    rule, tests/speed_target_port.closed_loop_mpc_timed (oracle/mpc_lateral + PID + tests/vehicle_port), the acceleration, the
    actors advanced.  timed=False is emp_drive's loop: no speed plan, the constant target.  -> a list of per-period dicts."""
    from oracle import ref_port as rp
    import speed_target_port as stp
    import vehicle_port as vp
    path = [tuple(float(v) for v in r) for r in global_path]
    state, actors, accel = np.array(state, np.float64), np.array(actors, np.float64), (0.0, 0.0)
    track, profile, cursor, held, speed_held, log = None, None, 0, 0, 0, []
    for k in range(K):
        tick = period_tick(tick0, k, T)
        rq = request_timed(state, accel, actors, n_act, max_obs, max_dyn, t0, tick, dt, prm=port.params(advance_s=T * dt))
        statics = [(rq["static_xy"][i, 0], rq["static_xy"][i, 1], rq["static_dis"][i]) for i in range(rq["n_static"])]
        dynamics = [tuple(rq["dyn"][i]) for i in range(rq["n_dyn"])]
        traj, match, _, _, out = rp.motion_planning_body((statics, dynamics, tuple(rq["origin_xy"]), tuple(rq["start_xy"]),
                                                          tuple(rq["start_v"]), tuple(rq["start_a"]), path, [int(pre_match)]))
        # oracle/qp_dense reports "optimal" or "unknown".  The device's rule ref_status == 0 && (status & ~1) == 0: ref_status is the
        # front end, which raises in the port where the device refuses (no such input here); status bit 1 (EMP_ST_DP_INFEASIBLE) the
        # reference does not know; the other bits are the path QP's and the trajectory smoothing's, "optimal" on the port's side
        path_ok = out["qp_status"] == "optimal" and out["smooth_status"] == "optimal"
        speed_status, planned = -1, None
        if timed:
            speed_status, planned = oracle_speed_plan(traj, rq["start_v"], rq["start_a"], rq["start_heading"],
                                                      [rq["dyn_obs"][i] for i in range(rq["n_dyn"])], rq["plan_start_time"], width)
        if path_ok:
            track, held = np.asarray(traj, np.float64), 0
        else:
            held += 1
        if path_ok and speed_status == 0:
            profile, cursor, speed_held = planned, 0, 0
        else:
            speed_held += 1
        seen = state
        following = profile if profile is not None else np.full(PROFILE_SHAPE, math.nan)      # never had one: the caller's all-NaN start
        if track is not None:
            S, _, G, fin, cursor, bits = stp.closed_loop_mpc_timed(vp.params(), track, state, 0, cap_kmh, following if timed else None, t0, T,
                                                                   tick0=tick, cursor=cursor)
            w1, w0 = port.world_velocity(fin[2], fin[3], fin[5]), port.world_velocity(S[-1][2], S[-1][3], S[-1][5])
            accel, state = ((w1[0] - w0[0]) / dt, (w1[1] - w0[1]) / dt), fin
        else:
            G, bits = np.array([]), 0
        log.append(dict(start=seen, path_ok=path_ok, qp_status=out["qp_status"], speed_status=speed_status, held=held, speed_held=speed_held,
                        n_dyn=rq["n_dyn"], targets=G, tgt_bits=bits, state=np.array(state), track=track, profile=profile))
        actors, pre_match = rq["actors_next"], match[0]
    return log


# -----------------------------------------------------------------------------------------------------------------------------
# the fleets of tests/test_drive_timed_host.py and tests/test_gpu_drive_timed.py (NumPy only: no device, no package import)
# -----------------------------------------------------------------------------------------------------------------------------
G_NODES, A_FLEET, DT = 80, 5, 0.01
MAX_OBS, MAX_DYN = 4, 2
LOOP_B, LOOP_K, LOOP_T = 4, 3, 20
BLOCK_AHEAD, BLOCK_SPEED, BLOCK_VX = 24.0, 2.5, 16.0


def at(path_row0, rot, ahead, side):
    return (path_row0[0] + ahead * math.cos(rot) - side * math.sin(rot), path_row0[1] + ahead * math.sin(rot) + side * math.cos(rot))


def timed_fleet(B, T, M, seed=3):
    """Straight 80-node global paths (2 m apart) of several headings, the vehicle 10 m along its path and a little beside it at
    10 m/s and up (the speed planner's comfortable band: the CPU oracle run shows which plans succeed).  Vehicle 0: a fast dynamic
    actor just inside the 50 m range and a static one just beyond the 30 m gate; vehicle 1: no dynamic actor (its second actor
    stands still: the speed planner sees an empty S-T graph); vehicle 2: three, one more than MAX_DYN holds; 3, 4, ...: one.  Idle
    actor slots are NaN.  t0 differs per vehicle, the profile starts all NaN."""
    rng = np.random.default_rng(seed)
    gp, state = np.zeros((B, G_NODES, 4)), np.zeros((B, 6))
    actors, n_act = np.full((B, A_FLEET, 4), np.nan), np.zeros(B, np.int32)
    s = np.arange(G_NODES) * 2.0
    for b in range(B):
        rot = [0.3, -2.0, 1.4, 3.0, -0.7][b % 5]
        c, sn = math.cos(rot), math.sin(rot)
        x0, y0 = rng.uniform(-50, 50), rng.uniform(-50, 50)
        gp[b] = np.column_stack([x0 + s * c, y0 + s * sn, np.full(G_NODES, rot), np.zeros(G_NODES)])
        state[b] = [*at(gp[b, 0], rot, 10.0, 0.2 * (-1) ** b), rot, 0.0, 0.0, 10.0 + 0.2 * b]
        if b == 0:
            actors[b, 0] = [*at(gp[b, 0], rot, 10.0 + 50.0 - 0.3 * 30.0 * DT * T, 0.2), 38.0 * c, 38.0 * sn]
            actors[b, 1] = [*at(gp[b, 0], rot, 10.0 + 30.0 + 0.5 * 8.0 * DT * T, 1.2), 0.0, 0.0]
            n_act[b] = 2
        else:
            actors[b, 0] = [*at(gp[b, 0], rot, 35.0, 1.0), 0.0, 0.0]
            actors[b, 1] = [*at(gp[b, 0], rot, 40.0, -1.5), 6.0 * c, 6.0 * sn]
            actors[b, 2] = [*at(gp[b, 0], rot, 20.0, 9.0), 0.0, 0.0]
            n_act[b] = 3
        if b % 5 == 1:
            actors[b, 1, 2:] = 0.0
        if b % 5 == 2:
            actors[b, 3] = [*at(gp[b, 0], rot, 30.0, 1.0), 5.0 * c, 5.0 * sn]
            actors[b, 4] = [*at(gp[b, 0], rot, 46.0, -0.5), 7.0 * c, 7.0 * sn]
            n_act[b] = 5
    return dict(global_path=gp, n_global=np.full(B, G_NODES, np.int32), state=state, accel=np.zeros((B, 2)), actors=actors, n_act=n_act,
                pre_match_index=np.full(B, 5, np.int32), track=np.zeros((B, M + 1, 4)), track_len=np.zeros(B, np.int32),
                held=np.zeros(B, np.int32), target_speed=3.6 * state[:, 5] + 1.0, t0=100.0 + 0.37 * np.arange(B),
                profile=np.full((B,) + PROFILE_SHAPE, np.nan), cursor=np.zeros(B, np.int32), speed_held=np.zeros(B, np.int32))


def blocked(f, b):
    """Vehicle b arrives at 16 m/s behind a dynamic actor at 2.5 m/s 24 m ahead, in its lane: the path half still plans (the virtual
    obstacles of test_9.py:137-169 are its business), the speed QP has no feasible profile at this closing speed
    (EMP_STB_QP_FAILED).  tests/test_drive_timed_host.py shows both on the CPU oracle; asserted again where it is used."""
    g = {k: np.array(v, copy=True) for k, v in f.items()}
    rot = g["global_path"][b, 0, 2]
    g["actors"][b] = np.nan
    g["actors"][b, 0] = [*at(g["global_path"][b, 0], rot, 10.0 + BLOCK_AHEAD, 0.2), BLOCK_SPEED * math.cos(rot), BLOCK_SPEED * math.sin(rot)]
    g["n_act"][b] = 1
    g["state"][b, 5] = BLOCK_VX
    g["target_speed"][b] = 3.6 * BLOCK_VX + 1.0
    return g


def loop_fleet(M):
    """DESIGN 3.8's straight-path fleet: 10 m/s, cap 50 km/h; one dynamic actor 20 m ahead in the lane at 3 m/s."""
    f = timed_fleet(LOOP_B, LOOP_T, M)
    for b in range(LOOP_B):
        rot = f["global_path"][b, 0, 2]
        f["state"][b] = [*at(f["global_path"][b, 0], rot, 10.0, 0.0), rot, 0.0, 0.0, 10.0]
        f["actors"][b] = np.nan
        f["actors"][b, 0] = [*at(f["global_path"][b, 0], rot, 30.0, 0.3), 3.0 * math.cos(rot), 3.0 * math.sin(rot)]
        f["n_act"][b] = 1
    f["target_speed"] = np.full(LOOP_B, 50.0)
    return f


def loop_on_the_cpu(M):
    """loop_fleet through the CPU oracle alone (oracle_loop), timed and untimed: {timed: [vehicle][period] dicts}."""
    f = loop_fleet(M)
    return {timed: [oracle_loop(f["global_path"][b], f["state"][b], f["actors"][b], f["n_act"][b], f["pre_match_index"][b],
                                f["target_speed"][b], f["t0"][b], LOOP_K, LOOP_T, MAX_OBS, MAX_DYN, M + 2, timed=timed)
                    for b in range(LOOP_B)] for timed in (True, False)}
