"""Timed trajectories: what one ``plan_cycle(speed=...)`` call (emp_plan_trajectory) costs against the same work as
``plan_cycle`` followed by the Python chain of per-function calls, and against ``plan_cycle`` alone.

Inputs are device-resident torch tensors (the EMP_DEVICE form).  B = 1 and 4096 on configs[2] (40 x 9 lattice) and on the
cfg5 lattice (120 x 21, configs[4]), 8 dynamic-obstacle slots with ragged counts.  The three forms alternate block by block;
each block times `--reps` consecutive calls between two HIP events and the median block is reported (ms per call).  One JSON
line per (config, B).  `--once B` makes exactly one trajectory call of B scenes after a warm-up (for a `rocprofv3
--kernel-trace --stats` run: the launches of one call and no copies between its stages).

    python tools/trajectory_bench.py [--blocks 7] [--reps 5] [--sizes 1,4096] [--configs cfg2,cfg5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K = 8


def inputs(cfg, B, seed):
    import torch
    from emplanner_carla_amd import scenes as S
    b = S.make_batch(range(seed, seed + B), cfg)
    rng = np.random.default_rng(seed)
    P = b.ref.shape[1]
    dyn = np.zeros((B, K, 4))
    for s in range(B):
        for j in range(K):
            i = int(rng.integers(8, max(9, P - 20)))
            x, y, th = b.ref[s, i, :3]
            l, vt, vl = rng.uniform(-6, 6), rng.uniform(-4, 12), rng.uniform(-3, 3)
            dyn[s, j] = (x - l * np.sin(th), y + l * np.cos(th), vt * np.cos(th) - vl * np.sin(th), vt * np.sin(th) + vl * np.cos(th))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cyc = dict(ref_line=t(b.ref), n_ref=t(np.full(B, P, np.int32)), origin_xy=t(b.origin_xy), start_xy=t(b.start_xy),
               start_v=t(b.start_v), start_a=t(b.start_a), obs_xy=t(b.obs_xy), n_obs=t(b.n_obs.astype(np.int32)))
    n = rng.integers(0, K + 1, B).astype(np.int32)
    return cyc, t(dyn), t(n), t(100.0 + rng.uniform(0, 10, B))


def chain(pl, r, cyc, dyn, n_dyn, t0, dp, qp, M):
    """The speed half as the per-function calls on device tensors (torch glue between them)."""
    import torch
    B, W = r.traj_len.shape[0], M + 2
    idx = torch.arange(W, device=dyn.device)
    valid = idx[None, :] < r.traj_len[:, None]
    pad = torch.full((B, W - (M + 1), 4), float("nan"), dtype=torch.float64, device=dyn.device)
    rows = torch.where(valid[:, :, None], torch.cat([r.traj, pad], 1), torch.tensor(float("nan"), dtype=torch.float64,
                                                                                      device=dyn.device))
    x, y, h, k = (rows[:, :, c].contiguous() for c in range(4))
    wide = torch.full((B,), W, dtype=torch.int32, device=dyn.device)
    i2s = pl.trajectory_index2s(x, y, wide)
    v, a = cyc["start_v"], cyc["start_a"]
    heading = torch.atan2(v[:, 1], v[:, 0]).contiguous()
    s1, s2 = pl.speed_start_condition(v[:, 0].contiguous(), v[:, 1].contiguous(), a[:, 0].contiguous(), a[:, 1].contiguous(), heading)
    xy = dyn[:, :, :2].contiguous()
    zero = torch.zeros(B, dtype=torch.int32, device=dyn.device)
    _, proj = pl.find_match_points(r.traj, r.traj_len, xy, n_dyn, zero, zero)
    s, l = pl.s_l(r.traj, i2s[:, :M + 1].contiguous(), r.traj_len, xy, n_dyn)
    live = torch.arange(K, device=dyn.device)[None, :] < n_dyn[:, None].long()
    nan = torch.tensor(float("nan"), dtype=torch.float64, device=dyn.device)
    s, l = torch.where(live, s, nan), torch.where(live, l, nan)
    rows5 = torch.stack([l, dyn[:, :, 2], dyn[:, :, 3], proj[:, :, 2], proj[:, :, 3]], 2).reshape(-1, 5).contiguous()
    d3 = pl.dy_obs_deri(rows5).reshape(B, K, 3)
    alive = live & (torch.cumsum(torch.isnan(l).int(), 1) == 0)          # cal_dy_obs_deri stops at the first NaN l
    sd, ld = torch.where(alive, d3[:, :, 0], nan).contiguous(), torch.where(alive, d3[:, :, 1], nan).contiguous()
    si, so, ti, to = pl.st_graph(s.contiguous(), l.contiguous(), sd, ld)
    res = pl.speed_dp(dp, si, so, ti, to, s1, tables=False)
    cs = pl.speed_convex_space(res.speed_s, res.speed_t, i2s, k, wide, si, so, ti, to)
    q = pl.speed_qp(qp, s1, s2, res.speed_s, res.speed_t, *cs[:4])
    d = pl.speed_increase_points(*q[:4])
    return pl.path_speed_merge(*d[:4], t0, i2s, x, y, h, k, wide)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1,4096")
    ap.add_argument("--configs", default="cfg2,cfg5")
    ap.add_argument("--once", type=int, default=0, help="one trajectory call of this many scenes (cfg2) after a warm-up")
    args = ap.parse_args()
    import torch
    from emplanner_carla_amd import api as A
    from emplanner_carla_amd import scenes as S
    pl = A.Planner(0)
    cfgs = {"cfg2": S.CFG2, "cfg5": S.CFG5}
    sdp, sqp = A.speed_dp_params(), A.speed_qp_params()
    if args.once:
        cfg = S.CFG2
        p, q, sp = A.dp_params_from_cfg(cfg), A.qp_params(), A.smooth_params()
        cyc, dyn, n, t0 = inputs(cfg, args.once, 1)
        spd = A.TrajectoryInputs(sdp, sqp, dyn, n, t0, intermediates=False)
        for _ in range(3):
            pl.plan_cycle(p, q, sp, speed=spd, **cyc)
        torch.cuda.synchronize()
        pl.plan_cycle(p, q, sp, speed=spd, **cyc)
        torch.cuda.synchronize()
        print(json.dumps({"once": args.once}))
        pl.close()
        return
    for name in args.configs.split(","):
        cfg = cfgs[name]
        p, q, sp = A.dp_params_from_cfg(cfg), A.qp_params(obs_length=cfg.obs_length, obs_width=cfg.obs_width), A.smooth_params()
        M = A.max_path_points(p)
        for B in (int(x) for x in args.sizes.split(",")):
            cyc, dyn, n, t0 = inputs(cfg, B, 1000)
            spd = A.TrajectoryInputs(sdp, sqp, dyn, n, t0, intermediates=False)
            forms = {
                "trajectory_call": lambda: pl.plan_cycle(p, q, sp, speed=spd, **cyc),
                "cycle_then_chain": lambda: chain(pl, pl.plan_cycle(p, q, sp, **cyc), cyc, dyn, n, t0, sdp, sqp, M),
                "cycle_alone": lambda: pl.plan_cycle(p, q, sp, **cyc),
            }
            for f in forms.values():            # warm-up: every buffer allocated, every kernel loaded
                f()
            torch.cuda.synchronize()
            times = {k: [] for k in forms}
            for _ in range(args.blocks):
                for k, f in forms.items():      # the forms alternate block by block
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.reps):
                        f()
                    e1.record()
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1) / args.reps)
            print(json.dumps({"config": name, "B": B, "reps": args.reps, "blocks": args.blocks,
                              **{f"{k}_ms": round(float(np.median(v)), 4) for k, v in times.items()},
                              **{f"{k}_ms_spread": [round(float(min(v)), 4), round(float(max(v)), 4)] for k, v in times.items()}}),
                  flush=True)
    pl.close()


if __name__ == "__main__":
    main()
