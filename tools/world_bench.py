"""Times K periods of a planning fleet in reacting traffic, two ways, in one run on one build:
  world_drive  one `traffic.World.drive(K)` call (emp_world_drive: exchange, the timed drive's period and the agents' ticks, K times,
               nothing leaving the device)
  host_loop    INTEGRATION.md's host loop of K single-period calls: agent_observe on the egos, torch.cat and set_others, the agents'
               rows expanded into every ego's actors, drive_timed(K=1), rollout
for W worlds x N agents with E egos a world (512 x 64 with 8 by default: 4096 egos, 32768 agents) on straight roads, one lane per
ego, eight agents ahead of it.  Device tensors; each measurement is a pair of HIP events on the planner's stream around the K
periods, host issue included; the mean of `--reps` per block and the median of `--blocks` blocks with [min, max], after a warm-up
of both.  Every repetition starts from the same state (restored outside the timed span).  The two are NOT the same computation to
the bit - the host loop resets the traffic's clock every period and takes each ego's lane key from a fixed array - so only times are
compared.  A timing tool only: no number is promised.  Prints one JSON line.

    python tools/world_bench.py [--worlds 512] [--agents 64] [--egos 8] [--periods 4] [--ticks 5] [--reps 5] [--blocks 5] [--out f.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from emplanner_carla_amd import api  # noqa: E402
from emplanner_carla_amd.traffic import BehaviorTraffic, World  # noqa: E402

G, M, MAX_OBS, MAX_DYN = 80, 40, 4, 2


def scene(W, N, E):
    """World w: E lanes 20 m apart along x; on each an ego at x = 10 at 10 m/s and N / E agents from x = 40 on, 20 m apart, 6 m/s."""
    per = N // E
    s = np.arange(G) * 2.0
    lane_y = (2000.0 * np.arange(W)[:, None] + 20.0 * np.arange(E)[None, :]).reshape(-1)           # (B,)
    B = W * E
    gp = np.zeros((B, G, 4))
    gp[:, :, 0], gp[:, :, 1] = s[None, :], lane_y[:, None]
    ego_state = np.zeros((B, 6))
    ego_state[:, 0], ego_state[:, 1], ego_state[:, 5] = 10.0, lane_y + 0.2, 10.0
    keys = np.arange(B, dtype=np.int32)
    path, state = np.zeros((W, N, M, 4)), np.zeros((W, N, 6))
    lane = np.zeros((W, N, M), np.int32)
    for j in range(N):
        e, i = j % E, j // E
        x0 = 40.0 + 20.0 * i
        y = lane_y.reshape(W, E)[:, e] + 0.5
        path[:, j, :, 0], path[:, j, :, 1] = x0 + np.arange(M)[None, :] * 2.0, y[:, None]
        state[:, j, 0], state[:, j, 1], state[:, j, 5] = x0, y, 6.0
        lane[:, j, :] = keys.reshape(W, E)[:, e][:, None]
    assert per >= 1
    return dict(global_path=gp, n_global=np.full(B, G, np.int32), ego_lane=np.tile(keys[:, None], (1, G)), ego_state=ego_state,
                ego_off=(np.arange(W + 1) * E).astype(np.int32), path=path, n_path=np.full((W, N), M, np.int32), lane=lane, state=state)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=512)
    ap.add_argument("--agents", type=int, default=64)
    ap.add_argument("--egos", type=int, default=8)
    ap.add_argument("--periods", type=int, default=4)
    ap.add_argument("--ticks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, N, E, K, T = a.worlds, a.agents, a.egos, a.periods, a.ticks
    B = W * E
    pl = api.Planner(0)
    stream = pl.torch_stream()
    p = api.dp_params()
    vp = api.vehicle_params()
    params = (p, api.qp_params(), api.smooth_params(), api.speed_dp_params(), api.speed_qp_params(), api.drive_params(), api.mpc_params(),
              api.pid_params(), vp)
    c = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in scene(W, N, E).items()}
    adt = vp.dt                                                # the agents tick with the egos: Ta = T
    mk = lambda: BehaviorTraffic(pl, c["path"], c["n_path"], c["lane"], c["state"], 25.0, params=api.agent_params(dt=adt),
                                 vehicle=api.agent_vehicle_params(dt=adt))
    tr_w, tr_h = mk(), mk()
    world = World(pl, tr_w, params, c["global_path"], c["n_global"], c["ego_lane"], c["ego_state"], 50.0, c["ego_off"], T, MAX_OBS,
                  max_act=N, max_other=E, max_dyn=MAX_DYN)
    host = World(pl, tr_h, params, c["global_path"], c["n_global"], c["ego_lane"], c["ego_state"], 50.0, c["ego_off"], T, MAX_OBS,
                 max_act=N, max_other=E, max_dyn=MAX_DYN)        # the host loop's ego arrays, held the same way
    n_act = torch.full((B,), N, dtype=torch.int32, device="cuda")
    half = torch.full((B, 1), 2.0, dtype=torch.float64, device="cuda")
    keys = c["ego_lane"][:, 0].reshape(W, E).contiguous()

    WORLD_KEYS = ("state", "accel", "pre_match_index", "track", "track_len", "held", "profile", "cursor", "speed_held")
    TRAFFIC_KEYS = ("state", "head", "past_steer", "lon_err", "n_lon", "lat_err", "n_lat", "last_light")

    def snapshot(w):
        return {k: getattr(w, k).clone() for k in WORLD_KEYS}, {k: getattr(w.traffic, k).clone() for k in TRAFFIC_KEYS}

    def restore(w, snap):
        for k, v in snap[0].items():
            getattr(w, k).copy_(v)
        for k, v in snap[1].items():
            getattr(w.traffic, k).copy_(v)
        w.tick, w.traffic.tick = 0, 0
        torch.cuda.synchronize()

    def world_drive():
        return world.drive(K, logs=False)

    def host_loop():
        h, t = host, tr_h
        for k in range(K):
            egos = pl.agent_observe(h.state).actors
            t.set_others(torch.cat([egos, half], 1).reshape(W, E, 5), keys)
            actors = t.actors().reshape(W, 1, N, 4).expand(W, E, N, 4).reshape(B, N, 4).contiguous()
            pl.drive_timed(*params, h.global_path, h.n_global, h.state, h.accel, actors, n_act, h.pre_match_index, h.track, h.track_len,
                           h.held, h.t0, h.profile, h.cursor, h.speed_held, h.target_speed, 1, T, MAX_OBS, MAX_DYN, tick0=k * T, logs=False,
                           in_place=True)
            t.rollout(T)

    s_w, s_h = snapshot(world), snapshot(host)
    with torch.cuda.stream(stream):                            # torch's own kernels of the host loop on the planner's stream
        for fn, w, s in ((world_drive, world, s_w), (host_loop, host, s_h)):     # warm-up
            fn()
            pl.synchronize()
            restore(w, s)
        r = world_drive()
        pl.synchronize()
        seen = dict(agents_with_a_gap=int((r.traffic.min_gap < float("inf")).sum().item()),
                    agents_not_normal=int((r.traffic.mode_ticks[..., 1:].sum(-1) > 0).sum().item()))
        restore(world, s_w)

        def timed(fn, w, s):
            out = []
            for _ in range(a.blocks):
                ms = 0.0
                for _ in range(a.reps):
                    restore(w, s)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    ms += e0.elapsed_time(e1)
                out.append(ms / a.reps)
            return round(statistics.median(out), 3), [round(min(out), 3), round(max(out), 3)]

        # alternate the two, block by block, so that a drift of the machine touches both
        w_ms, w_sp = timed(world_drive, world, s_w)
        h_ms, h_sp = timed(host_loop, host, s_h)
        w2_ms, w2_sp = timed(world_drive, world, s_w)
    row = {"worlds": W, "agents_per_world": N, "egos_per_world": E, "egos": B, "agents": W * N, "periods": K, "ego_ticks": T, "agent_ticks": T,
           "world_drive_ms": w_ms, "world_drive_spread_ms": w_sp, "world_drive_again_ms": w2_ms, "world_drive_again_spread_ms": w2_sp,
           "host_loop_ms": h_ms, "host_loop_spread_ms": h_sp, "host_loop_over_world_drive": round(h_ms / w_ms, 3), "reps": a.reps,
           "blocks": a.blocks, "seen": seen,
           "timed": "K periods between two HIP events on the planner's stream, host issue included; state restored outside the span"}
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(row, fh, indent=1)
    pl.close()


if __name__ == "__main__":
    main()
