"""Times the fleet loop: Planner.drive (K periods of [request, plan, adopt, T ticks] in ONE call, nothing leaving the device)
against what a user of the separate calls writes - per period a NumPy perceive-and-predict on the host (the state and the actors
come down, the request goes up; the acceleration, a pass-through, stays on the device), plan_cycle(global_path=...) and rollout on device tensors, the plan adopted with torch.where -
for both lateral laws and B in {1, 4096, 32768}, K = 10, T = 100.  Every run starts from the same fleet (made outside the timed
span); HIP events on the context's stream around each run; the two forms alternate block by block and each reports the median of
`--blocks` blocks with [min, max] after a warm-up run.  The host form's perception is vectorised NumPy with np.argsort(kind="stable")
and need not match the device's bits: it is timed, not compared.  As a sanity check the two forms' final positions must agree to
1e-6 m in the median over the fleet; the share of vehicles within 1e-6 m and the largest gap are reported (NumPy's and the device's
sin / cos differ in the last bit, and in a large fleet that flips a near-tie of the lattice DP for a few vehicles).  There is no
speed-up bar (launch counts alone buy nothing when the host runs ahead); the host form's cost is its round trip per
period.  Prints one JSON line per (law, B).

    python tools/drive_bench.py [--sizes 1,4096,32768] [--periods 10] [--ticks 100] [--reps 1] [--blocks 5] [--out drive_bench.json]

--timed times the timed fleet loop instead: Planner.drive_timed (one call) against the same loop written with the separate calls
(drive_request_timed, plan_cycle(global_path=..., speed=...), the adoption with torch.where, rollout_timed: all on device tensors, so
this form pays launches and Python, no round trip) and against Planner.drive on the same fleet (what the speed half and the profile
copy cost).  Same method: HIP events, the three forms alternated block by block, median of the blocks with [min, max].  The two
timed forms run the same kernels on the same bits: their final states must be identical.

    python tools/drive_bench.py --timed [--out profiles/drive/drive_timed_bench.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from emplanner_carla_amd import api  # noqa: E402

G, A, MAX_OBS, MAX_DYN = 80, 8, 4, 2


def fleet(B, seed=11):
    """Straight 80-node global paths (2 m apart) of every heading, the vehicle 10 m along at 6-12 m/s, three static actors ahead
    (one inside the 30 m gate) and two dynamic ones."""
    rng = np.random.default_rng(seed)
    rot = rng.uniform(-math.pi, math.pi, B)
    c, s = np.cos(rot), np.sin(rot)
    x0, y0 = rng.uniform(-500, 500, B), rng.uniform(-500, 500, B)
    d = np.arange(G) * 2.0
    gp = np.stack([x0[:, None] + d * c[:, None], y0[:, None] + d * s[:, None], np.broadcast_to(rot[:, None], (B, G)),
                   np.zeros((B, G))], -1)
    at = lambda ahead, side: (x0 + ahead * c - side * s, y0 + ahead * s + side * c)
    v = rng.uniform(6.0, 12.0, B)
    px, py = at(10.0, rng.uniform(-0.3, 0.3, B))
    state = np.column_stack([px, py, rot, np.zeros(B), np.zeros(B), v])
    actors = np.zeros((B, A, 4))
    for i, (ahead, side, speed) in enumerate(((32.0, 1.2, 0.0), (45.0, -1.5, 0.0), (70.0, 0.5, 0.0), (38.0, -1.0, 5.0), (52.0, 2.0, 9.0))):
        ax, ay = at(ahead + rng.uniform(-2, 2, B), side)
        actors[:, i] = np.column_stack([ax, ay, speed * c, speed * s])
    return dict(global_path=gp, n_global=np.full(B, G, np.int32), state=state, accel=np.zeros((B, 2)), actors=actors,
                n_act=np.full(B, 5, np.int32), pre_match_index=np.full(B, 5, np.int32), held=np.zeros(B, np.int32),
                target_speed=3.6 * v + 1.0)


def host_request(state, actors, n_act, ts=0.2):
    """The driver's perceive and predict on the host, vectorised (the cheapest form a user would write)."""
    x, y, fi, Vy, fi_dot, Vx = state.T
    c, s = np.cos(fi), np.sin(fi)
    wx, wy = Vx * c - Vy * s, Vx * s + Vy * c
    B, n = actors.shape[:2]
    live = np.arange(n)[None, :] < n_act[:, None]
    v1x, v1y = actors[:, :, 0] - x[:, None], actors[:, :, 1] - y[:, None]
    dis = np.sqrt(v1x * v1x + v1y * v1y)
    lat = v1x * (-s)[:, None] + v1y * c[:, None]
    along = v1x * wx[:, None] + v1y * wy[:, None]
    speed = np.sqrt(actors[:, :, 2] ** 2 + actors[:, :, 3] ** 2)
    kept = live & (dis < 50.0) & (lat > -5.0) & (lat < 5.0) & (along > -10.0)
    dyn, stat = kept & (speed > 1.0), kept & ~(speed > 1.0)
    rows = np.arange(B)[:, None]
    order = np.argsort(np.where(stat, dis, np.inf), 1, kind="stable")[:, :MAX_OBS]
    n_static = np.minimum(stat.sum(1), MAX_OBS).astype(np.int32)
    fill = np.arange(MAX_OBS)[None, :] < n_static[:, None]
    static_xy = np.where(fill[:, :, None], actors[rows, order, :2], 0.0)
    d0 = np.where(stat, dis, np.inf).min(1)
    n_obs = np.where((n_static > 0) & (d0 <= 30.0), n_static, 0).astype(np.int32)
    first = np.argmin(np.where(dyn, dis, np.inf), 1)
    any_dyn = dyn.any(1)
    dds = np.where(any_dyn[:, None], np.column_stack([dis[np.arange(B), first], speed[np.arange(B), first]]), np.nan)
    V = np.sqrt(wx * wx + wy * wy)
    beta = np.arctan2(wy, wx) - fi
    V_y, V_x = V * np.sin(beta), V * np.cos(beta)
    start = np.column_stack([x + V_x * ts * c - V_y * ts * s, y + V_y * ts * c + V_x * ts * s])
    return static_xy, n_obs, dds, state[:, :2].copy(), start, np.column_stack([wx, wy])


def main_timed(a):
    K, T = a.periods, a.ticks
    pl = api.Planner(0)
    stream = pl.torch_stream()
    p, q, sp, pid, vpar, dprm = api.dp_params(), api.qp_params(), api.smooth_params(), api.pid_params(), api.vehicle_params(), api.drive_params()
    sdp, sqp, adv = api.speed_dp_params(), api.speed_qp_params(), api.drive_params(advance_s=T * vpar.dt)
    M, N = api.max_path_points(p), 401
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    results = []
    for B in (int(s) for s in a.sizes.split(",")):
        f = fleet(B)
        f.update(track=np.zeros((B, M + 1, 4)), track_len=np.zeros(B, np.int32), profile=np.full((B, 7, N), np.nan),
                 cursor=np.zeros(B, np.int32), speed_held=np.zeros(B, np.int32))
        const = {k: up(f[k]) for k in ("global_path", "n_global", "n_act", "target_speed")}
        const["t0"] = torch.zeros(B, dtype=torch.float64, device="cuda")
        zeros = dict(mi=torch.zeros(B, dtype=torch.int32, device="cuda"), err=torch.zeros((B, 60), dtype=torch.float64, device="cuda"),
                     n_err=torch.zeros(B, dtype=torch.int32, device="cuda"))
        every = max(T - 1, 1)

        def fresh():
            g = {k: up(f[k]) for k in ("state", "accel", "actors", "pre_match_index", "track", "track_len", "held", "profile", "cursor",
                                       "speed_held")}
            torch.cuda.synchronize()
            return g

        def drive_timed(law, lat, g):
            return pl.drive_timed(p, q, sp, sdp, sqp, dprm, lat, pid, vpar, const["global_path"], const["n_global"], g["state"], g["accel"],
                                  g["actors"], const["n_act"], g["pre_match_index"], g["track"], g["track_len"], g["held"], const["t0"],
                                  g["profile"], g["cursor"], g["speed_held"], const["target_speed"], K, T, MAX_OBS, MAX_DYN, lateral=law,
                                  logs=False, in_place=True).state

        def drive(law, lat, g):
            return pl.drive(p, q, sp, dprm, lat, pid, vpar, const["global_path"], const["n_global"], g["state"], g["accel"], g["actors"],
                            const["n_act"], g["pre_match_index"], g["track"], g["track_len"], g["held"], const["target_speed"], K, T,
                            MAX_OBS, MAX_DYN, lateral=law, logs=False, in_place=True).state

        def separate(law, lat, g):
            state, accel, actors, prem, track, tlen, held, prof, cur, sheld = (g[k] for k in (
                "state", "accel", "actors", "pre_match_index", "track", "track_len", "held", "profile", "cursor", "speed_held"))
            w_of = lambda st_: pl.drive_request(dprm, st_, None, actors, const["n_act"], MAX_OBS, MAX_DYN).start_v
            for k in range(K):
                rq = pl.drive_request_timed(adv, state, accel, actors, const["n_act"], const["t0"], k * T, vpar.dt, MAX_OBS, MAX_DYN,
                                            in_place=True)
                cy = pl.plan_cycle(p, q, sp, None, None, rq.origin_xy, rq.start_xy, rq.start_v, rq.start_a, rq.static_xy, rq.n_obs,
                                   max_pts=M, dyn_dis_speed=rq.dyn_dis_speed, global_path=const["global_path"],
                                   n_global=const["n_global"], pre_match_index=prem,
                                   speed=api.TrajectoryInputs(sdp, sqp, rq.dyn_obs, rq.n_dyn, rq.plan_start_time,
                                                              start_heading=rq.start_heading, intermediates=False))
                valid = (cy.ref_status == 0) & ((cy.status & ~1) == 0)
                take = valid[:, None] & (torch.arange(M + 1, device="cuda")[None, :] < cy.traj_len[:, None])
                track = torch.where(take[:, :, None], cy.traj, track)
                tlen = torch.where(valid, cy.traj_len, tlen)
                held = torch.where(valid, torch.zeros_like(held), held + 1)
                both = valid & (cy.speed.speed_status == 0)
                prof = torch.where(both[:, None, None], cy.speed.trajectory, prof)
                cur = torch.where(both, torch.zeros_like(cur), cur)
                sheld = torch.where(both, torch.zeros_like(sheld), sheld + 1)
                ro = pl.rollout_timed(lat, pid, vpar, track, tlen, state, zeros["mi"], const["target_speed"], zeros["err"], zeros["n_err"],
                                      prof, const["t0"], T, tick0=k * T, cursor=cur, lateral=law, log_every=every)
                accel = (w_of(ro.state) - w_of(ro.log_state[0 if T == 1 else 1])) / vpar.dt
                state, prem, cur = ro.state, cy.match_index, ro.cursor
            return state

        def block(fn, law, lat):
            per = []
            for _ in range(a.reps):
                g = fresh()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn(law, lat, g)
                e1.record(stream)
                pl.synchronize()
                torch.cuda.synchronize()
                per.append(e0.elapsed_time(e1))
            return sum(per) / len(per)

        forms = (("drive_timed", drive_timed), ("separate_timed", separate), ("drive", drive))
        for law, lat in (("mpc", api.mpc_params()), ("lqr", api.lqr_params())):
            finals = {}
            for name, fn in forms:                                             # warm-up, and the two timed forms are one computation
                st = fn(law, lat, fresh())
                pl.synchronize()
                torch.cuda.synchronize()
                finals[name] = st.cpu().numpy()
            assert finals["drive_timed"].tobytes() == finals["separate_timed"].tobytes(), "drive_timed and the separate calls differ"
            ms = {name: [] for name, _ in forms}
            for _ in range(a.blocks):                                          # alternate: drift of the machine hits all alike
                for name, fn in forms:
                    ms[name].append(block(fn, law, lat))
            med = {name: statistics.median(v) for name, v in ms.items()}
            row = {"law": law, "B": B, "K": K, "T": T, "reps": a.reps, "blocks": a.blocks,
                   "separate_over_drive_timed": round(med["separate_timed"] / med["drive_timed"], 3),
                   "drive_timed_over_drive": round(med["drive_timed"] / med["drive"], 3),
                   "mean_vx_timed": float(finals["drive_timed"][:, 5].mean()), "mean_vx_drive": float(finals["drive"][:, 5].mean())}
            for name, v in ms.items():
                row[name + "_ms"] = round(med[name], 3)
                row[name + "_spread_ms"] = [round(min(v), 3), round(max(v), 3)]
            results.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)
    pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,4096,32768")
    ap.add_argument("--periods", type=int, default=10)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timed", action="store_true", help="time Planner.drive_timed against the separate timed calls and Planner.drive")
    a = ap.parse_args()
    if a.timed:
        return main_timed(a)
    K, T = a.periods, a.ticks
    pl = api.Planner(0)
    stream = pl.torch_stream()
    p, q, sp, pid, vpar, dprm = api.dp_params(), api.qp_params(), api.smooth_params(), api.pid_params(), api.vehicle_params(), api.drive_params()
    M = api.max_path_points(p)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    results = []
    for B in (int(s) for s in a.sizes.split(",")):
        f = fleet(B)
        f["track"] = np.zeros((B, M + 1, 4))
        f["track_len"] = np.zeros(B, np.int32)
        const = {k: up(f[k]) for k in ("global_path", "n_global", "n_act", "target_speed")}
        zeros = dict(mi=torch.zeros(B, dtype=torch.int32, device="cuda"), err=torch.zeros((B, 60), dtype=torch.float64, device="cuda"),
                     n_err=torch.zeros(B, dtype=torch.int32, device="cuda"))
        every = max(T - 1, 1)

        def fresh():
            g = {k: up(f[k]) for k in ("state", "accel", "actors", "pre_match_index", "track", "track_len", "held")}
            torch.cuda.synchronize()
            return g

        def drive(law, lat, g):
            r = pl.drive(p, q, sp, dprm, lat, pid, vpar, const["global_path"], const["n_global"], g["state"], g["accel"], g["actors"],
                         const["n_act"], g["pre_match_index"], g["track"], g["track_len"], g["held"], const["target_speed"], K, T,
                         MAX_OBS, MAX_DYN, lateral=law, logs=False, in_place=True)
            return r.state

        def separate(law, lat, g):
            state, actors, prem, track, tlen, held = (g[k] for k in ("state", "actors", "pre_match_index", "track", "track_len", "held"))
            accel = g["accel"]                                                             # pass-through: stays on the device
            for _ in range(K):
                h_state, h_actors = state.cpu().numpy(), actors.cpu().numpy()             # the round trip: down ...
                sxy, n_obs, dds, origin, start, v = host_request(h_state, h_actors, f["n_act"])
                cy = pl.plan_cycle(p, q, sp, None, None, up(origin), up(start), up(v), accel, up(sxy), up(n_obs), max_pts=M,
                                   dyn_dis_speed=up(dds), global_path=const["global_path"], n_global=const["n_global"],
                                   pre_match_index=prem)                                    # ... and up
                valid = (cy.ref_status == 0) & ((cy.status & ~1) == 0)
                take = valid[:, None] & (torch.arange(M + 1, device="cuda")[None, :] < cy.traj_len[:, None])
                track = torch.where(take[:, :, None], cy.traj, track)
                tlen = torch.where(valid, cy.traj_len, tlen)
                held = torch.where(valid, torch.zeros_like(held), held + 1)
                ro = pl.rollout(lat, pid, vpar, track, tlen, state, zeros["mi"], const["target_speed"], zeros["err"], zeros["n_err"], T,
                                lateral=law, log_every=every)
                last = ro.log_state[0 if T == 1 else 1]
                w = lambda st_: torch.stack([st_[:, 5] * torch.cos(st_[:, 2]) - st_[:, 3] * torch.sin(st_[:, 2]),
                                             st_[:, 5] * torch.sin(st_[:, 2]) + st_[:, 3] * torch.cos(st_[:, 2])], 1)
                accel = (w(ro.state) - w(last)) / vpar.dt
                actors = actors.clone()
                actors[:, :, :2] += actors[:, :, 2:] * (T * vpar.dt)
                state, prem = ro.state, cy.match_index
            return state

        def block(fn, law, lat):
            per = []
            for _ in range(a.reps):
                g = fresh()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn(law, lat, g)
                e1.record(stream)
                pl.synchronize()
                torch.cuda.synchronize()
                per.append(e0.elapsed_time(e1))
            return sum(per) / len(per)

        for law, lat in (("mpc", api.mpc_params()), ("lqr", api.lqr_params())):
            finals = []
            for fn in (drive, separate):                                       # warm-up, and the two forms agree (loosely)
                st = fn(law, lat, fresh())
                pl.synchronize()
                torch.cuda.synchronize()
                finals.append(st.cpu().numpy())
            gaps = np.hypot(*(finals[0][:, :2] - finals[1][:, :2]).T)
            gap, agree = float(np.median(gaps)), float((gaps <= 1e-6).mean())
            assert gap <= 1e-6, f"drive and the separate calls end {gap} m apart (median over the fleet)"
            dr, se = [], []
            for _ in range(a.blocks):                                          # alternate: drift of the machine hits both alike
                dr.append(block(drive, law, lat))
                se.append(block(separate, law, lat))
            d_ms, s_ms = statistics.median(dr), statistics.median(se)
            row = {"law": law, "B": B, "K": K, "T": T, "drive_ms": round(d_ms, 3), "separate_ms": round(s_ms, 3),
                   "drive_spread_ms": [round(min(dr), 3), round(max(dr), 3)], "separate_spread_ms": [round(min(se), 3), round(max(se), 3)],
                   "separate_over_drive": round(s_ms / d_ms, 3), "drive_ms_per_period": round(d_ms / K, 3),
                   "final_position_gap_median_m": gap, "final_position_gap_max_m": float(gaps.max()),
                   "vehicles_within_1e-6_m": round(agree, 5), "reps": a.reps, "blocks": a.blocks}
            results.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)
    pl.close()


if __name__ == "__main__":
    main()
