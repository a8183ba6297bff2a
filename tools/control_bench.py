"""Times Vehicle_control.run_step for a fleet: emp_vehicle_control (lateral law + PID + actuation in ONE kernel launch) against
the two separate calls it replaces (emp_mpc_lateral or emp_lqr_lateral, then emp_pid_longitudinal), for B in {1, 4096, 32768}
and both lateral laws, and emp_mpc_ff_lateral alone.  Device-resident inputs (EMP_DEVICE; the PID state is updated in place
across steps, as a fleet loop keeps it), raw C-ABI calls, HIP events on the context's stream around blocks of `--reps` calls;
the median of `--blocks` blocks after a warm-up block.  Prints one JSON line per (law, B).

    python tools/control_bench.py [--sizes 1,4096,32768] [--reps 20] [--blocks 7] [--out control_bench.json]
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
from emplanner_carla_amd.api import Planner, lqr_params, mpc_ff_params, mpc_params, pid_params  # noqa: E402

MAX_PATH = 64


def fleet(B, seed=7):
    """B vehicles on 64-point paths (2 m spacing, gentle curvature), near their path, 2-30 m/s, targets near their speed."""
    rng = np.random.default_rng(seed)
    t = np.arange(MAX_PATH) * 2.0
    k = rng.normal(0, 0.01, (B, 1))
    h0 = rng.uniform(-math.pi, math.pi, (B, 1))
    th = h0 + k * t
    path = np.stack([np.cumsum(np.cos(th), 1) * 2.0, np.cumsum(np.sin(th), 1) * 2.0, th, np.broadcast_to(k, th.shape)], -1)
    at = rng.integers(0, 20, B)
    idx = np.arange(B)
    state = np.column_stack([path[idx, at, 0] + rng.normal(0, 0.4, B), path[idx, at, 1] + rng.normal(0, 0.4, B),
                             th[idx, at] + rng.normal(0, 0.05, B), rng.normal(0, 0.2, B), rng.normal(0, 0.05, B)])
    vx = rng.uniform(2.0, 30.0, B)
    speed = vx * 3.6
    target = speed + rng.normal(0, 0.6, B)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(path=d(path), n=d(np.full(B, MAX_PATH, np.int32)), state=d(state), vx=d(vx), mi=d(np.maximum(at - 2, 0).astype(np.int32)),
                speed=d(speed), target=d(target), err=torch.zeros((B, L.PID_BUFFER), dtype=torch.float64, device="cuda"),
                n_err=torch.zeros(B, dtype=torch.int32, device="cuda"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,4096,32768")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pl = Planner(0)
    lib, h = pl._lib, pl._h
    stream = pl.torch_stream()
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    pid = pid_params()
    results = []
    for B in (int(s) for s in a.sizes.split(",")):
        f = fleet(B)
        o = {k: torch.empty(s, dtype=dt, device="cuda") for k, s, dt in (
            ("control", (B, 3), torch.float64), ("lat", (B,), torch.float64), ("lon", (B,), torch.float64),
            ("mo", (B,), torch.int32), ("e", (B, 4), torch.float64), ("k", (B,), torch.float64), ("pp", (B, 4), torch.float64),
            ("st", (B,), torch.int32), ("u", (B, 12), torch.float64), ("it", (B,), torch.int32), ("K", (B, 4), torch.float64))}
        torch.cuda.synchronize()

        def fused(law, prm):
            rc = lib.emp_vehicle_control(h, law, C.byref(prm), C.byref(pid), B, MAX_PATH, P(f["path"]), P(f["n"]), P(f["state"]),
                                         P(f["vx"]), P(f["mi"]), P(f["speed"]), P(f["target"]), P(f["err"]), P(f["n_err"]),
                                         P(o["control"]), P(o["lat"]), P(o["lon"]), P(o["mo"]), P(o["e"]), P(o["k"]), P(o["pp"]),
                                         P(f["err"]), P(f["n_err"]), P(o["st"]), L.EMP_DEVICE)
            assert rc == 0, rc

        def separate(law, prm):
            if law == L.EMP_LAT_MPC:
                rc = lib.emp_mpc_lateral(h, C.byref(prm), B, MAX_PATH, P(f["path"]), P(f["n"]), P(f["state"]), P(f["vx"]), P(f["mi"]),
                                         P(o["lat"]), None, P(o["e"]), P(o["k"]), P(o["mo"]), P(o["pp"]), None, None, None,
                                         P(o["st"]), L.EMP_DEVICE)
            else:
                rc = lib.emp_lqr_lateral(h, C.byref(prm), B, MAX_PATH, P(f["path"]), P(f["n"]), P(f["state"]), P(f["vx"]), P(f["mi"]),
                                         P(o["lat"]), None, P(o["e"]), P(o["k"]), P(o["mo"]), P(o["pp"]), None, P(o["st"]),
                                         L.EMP_DEVICE)
            assert rc == 0, rc
            rc = lib.emp_pid_longitudinal(h, C.byref(pid), B, P(f["speed"]), P(f["target"]), P(f["err"]), P(f["n_err"]),
                                          P(o["lon"]), P(f["err"]), P(f["n_err"]), L.EMP_DEVICE)
            assert rc == 0, rc

        ffp = mpc_ff_params()

        def ff_alone(law, prm):
            rc = lib.emp_mpc_ff_lateral(h, C.byref(ffp), B, MAX_PATH, P(f["path"]), P(f["n"]), P(f["state"]), P(f["vx"]), P(f["mi"]),
                                        P(o["lat"]), None, P(o["e"]), P(o["k"]), P(o["mo"]), P(o["pp"]), None, None, None,
                                        P(o["st"]), L.EMP_DEVICE)
            assert rc == 0, rc

        def timed(fn, law, prm):
            """ms per call: median over blocks of `reps` calls bracketed by events on the context's stream."""
            for _ in range(a.reps):
                fn(law, prm)
            per = []
            for _ in range(a.blocks):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.reps):
                    fn(law, prm)
                e1.record(stream)
                e1.synchronize()
                per.append(e0.elapsed_time(e1) / a.reps)
            return statistics.median(per), min(per), max(per)

        for name, law, prm in (("mpc", L.EMP_LAT_MPC, mpc_params()), ("lqr", L.EMP_LAT_LQR, lqr_params())):
            # alternate the two forms so that drift of the machine hits both alike
            fu1, se1 = timed(fused, law, prm), timed(separate, law, prm)
            fu2, se2 = timed(fused, law, prm), timed(separate, law, prm)
            fu = statistics.median([fu1[0], fu2[0]])
            se = statistics.median([se1[0], se2[0]])
            row = {"law": name, "B": B, "fused_ms": round(fu, 5), "separate_ms": round(se, 5),
                   "fused_spread_ms": [round(min(fu1[1], fu2[1]), 5), round(max(fu1[2], fu2[2]), 5)],
                   "separate_spread_ms": [round(min(se1[1], se2[1]), 5), round(max(se1[2], se2[2]), 5)],
                   "fused_over_separate": round(fu / se, 4), "reps": a.reps, "blocks": a.blocks}
            results.append(row)
            print(json.dumps(row), flush=True)
        ff = timed(ff_alone, None, None)
        row = {"law": "mpc_ff", "B": B, "ms": round(ff[0], 5), "spread_ms": [round(ff[1], 5), round(ff[2], 5)]}
        results.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)
    pl.close()


if __name__ == "__main__":
    main()
