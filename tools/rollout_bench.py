"""Times the closed loop for a fleet: emp_rollout (T ticks of lateral law + PID + actuation + vehicle model in ONE kernel launch)
against the chain it replaces (T x [emp_vehicle_control, emp_vehicle_step], 2 T launches), for both lateral laws and B in
{1, 4096, 32768}, T = 100.  Device-resident inputs (EMP_DEVICE), raw C-ABI calls, every run from the same initial fleet (restored
outside the timed span), HIP events on the context's stream around blocks of `--reps` runs; the two forms alternate block by
block and each reports the median of `--blocks` blocks after a warm-up run.  Both forms' final states are compared bit for bit
before anything is timed.  Prints one JSON line per (law, B).

    python tools/rollout_bench.py [--sizes 1,4096,32768] [--ticks 100] [--reps 2] [--blocks 7] [--out rollout_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from emplanner_carla_amd import _lib as L  # noqa: E402
from emplanner_carla_amd.api import Planner, lqr_params, mpc_params, pid_params, vehicle_params  # noqa: E402

MAX_PATH = 64


def fleet(B, seed=7):
    """B vehicles on 64-point paths (2.5 m spacing, straight to 1000 m radius), within 0.5 m of their path, 5-15 m/s (the LQR's
    Riccati iteration is slow for a creeping vehicle), targets near their speed."""
    rng = np.random.default_rng(seed)
    s = np.arange(MAX_PATH) * 2.5
    k = rng.uniform(-0.001, 0.001, (B, 1))
    h0 = rng.uniform(-math.pi, math.pi, (B, 1))
    th = h0 + k * s
    path = np.stack([np.cumsum(np.cos(th), 1) * 2.5, np.cumsum(np.sin(th), 1) * 2.5, th, np.broadcast_to(k, th.shape)], -1)
    idx = np.arange(B)
    off = rng.uniform(-0.5, 0.5, B)
    v = rng.uniform(5.0, 15.0, B)
    state = np.column_stack([path[idx, 2, 0] - off * np.sin(th[idx, 2]), path[idx, 2, 1] + off * np.cos(th[idx, 2]), th[idx, 2],
                             np.zeros(B), v * k[:, 0], v])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(path=d(path), n=d(np.full(B, MAX_PATH, np.int32)), state=d(state), mi=d(np.zeros(B, np.int32)),
                target=d(3.6 * v + rng.normal(0, 0.6, B)), err=torch.zeros((B, L.PID_BUFFER), dtype=torch.float64, device="cuda"),
                n_err=torch.zeros(B, dtype=torch.int32, device="cuda"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,4096,32768")
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T = a.ticks
    pl = Planner(0)
    lib, h = pl._lib, pl._h
    stream = pl.torch_stream()
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    pid, vpar = pid_params(), vehicle_params()
    results = []
    for B in (int(s) for s in a.sizes.split(",")):
        f = fleet(B)
        f64, i32 = torch.float64, torch.int32
        w = {k: torch.empty(s, dtype=dt, device="cuda") for k, s, dt in (
            ("state", (B, 6), f64), ("mi", (B,), i32), ("err", (B, L.PID_BUFFER), f64), ("n_err", (B,), i32), ("cs", (B, 5), f64),
            ("vx", (B,), f64), ("kmh", (B,), f64), ("control", (B, 3), f64), ("st", (B,), i32), ("ft", (B,), i32))}
        vx0 = torch.clamp(f["state"][:, 5], min=0.005)                       # the fleet moves forward: the clamp's >= 0 branch
        kmh0 = 3.6 * torch.sqrt(f["state"][:, 5] * f["state"][:, 5] + f["state"][:, 3] * f["state"][:, 3])

        def restore():
            for k in ("state", "mi", "err", "n_err"):
                w[k].copy_(f[k])
            w["cs"].copy_(f["state"][:, :5])
            w["vx"].copy_(vx0)
            w["kmh"].copy_(kmh0)
            torch.cuda.synchronize()

        def rollout(law, prm):
            rc = lib.emp_rollout(h, law, C.byref(prm), C.byref(pid), C.byref(vpar), B, MAX_PATH, P(f["path"]), P(f["n"]), P(w["state"]),
                                 P(w["mi"]), P(f["target"]), P(w["err"]), P(w["n_err"]), T, T + 1, P(w["state"]), P(w["mi"]),
                                 P(w["err"]), P(w["n_err"]), P(w["st"]), P(w["ft"]), None, None, None, None, L.EMP_DEVICE)
            assert rc == 0, rc

        def chain(law, prm):
            for _ in range(T):
                rc = lib.emp_vehicle_control(h, law, C.byref(prm), C.byref(pid), B, MAX_PATH, P(f["path"]), P(f["n"]), P(w["cs"]),
                                             P(w["vx"]), P(w["mi"]), P(w["kmh"]), P(f["target"]), P(w["err"]), P(w["n_err"]),
                                             P(w["control"]), None, None, P(w["mi"]), None, None, None, P(w["err"]), P(w["n_err"]),
                                             P(w["st"]), L.EMP_DEVICE)
                assert rc == 0, rc
                rc = lib.emp_vehicle_step(h, C.byref(vpar), B, P(w["state"]), P(w["control"]), P(w["state"]), P(w["cs"]), P(w["vx"]),
                                          P(w["kmh"]), L.EMP_DEVICE)
                assert rc == 0, rc

        def block(fn, law, prm):
            per = []
            for _ in range(a.reps):                                            # one event pair per run: the restore stays outside
                restore()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn(law, prm)
                e1.record(stream)
                e1.synchronize()
                per.append(e0.elapsed_time(e1))
            return sum(per) / len(per)

        for name, law, prm in (("mpc", L.EMP_LAT_MPC, mpc_params()), ("lqr", L.EMP_LAT_LQR, lqr_params())):
            finals = []
            for fn in (rollout, chain):                                        # warm-up, and the two forms agree
                restore()
                fn(law, prm)
                pl.synchronize()
                finals.append([w[k].clone() for k in ("state", "mi", "err", "n_err")])
            assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(*finals)), "rollout != chain"
            ro, ch = [], []
            for _ in range(a.blocks):                                          # alternate: drift of the machine hits both alike
                ro.append(block(rollout, law, prm))
                ch.append(block(chain, law, prm))
            r_ms, c_ms = statistics.median(ro), statistics.median(ch)
            row = {"law": name, "B": B, "T": T, "rollout_ms": round(r_ms, 4), "chain_ms": round(c_ms, 4),
                   "rollout_spread_ms": [round(min(ro), 4), round(max(ro), 4)], "chain_spread_ms": [round(min(ch), 4), round(max(ch), 4)],
                   "chain_over_rollout": round(c_ms / r_ms, 3), "rollout_us_per_tick": round(1000.0 * r_ms / T, 3),
                   "reps": a.reps, "blocks": a.blocks}
            results.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)
    pl.close()


if __name__ == "__main__":
    main()
