"""Times routed traffic: emp_agent_rollout of T = 100 ticks (one launch) against the chain of the 300 separate launches
(emp_agent_observe, emp_agent_control, emp_vehicle_step per tick) for A in {1, 4096, 32768} agents on rotated copies of the short
corner path of tests/agent_cases.py.  Device-resident arrays (EMP_DEVICE), raw C-ABI calls, a pair of HIP events on the context's
stream around each rollout (or chain, host issue of its 300 calls included), the mean of `--reps` of them per block and the median
of `--blocks` blocks after a warm-up.  Every rollout and every chain starts from the same fleet state (the rollout's outputs go to
arrays of their own; the chain's state is reset outside the timed span), so each does the same work.  Before anything is timed the
rollout's outputs are compared bit for bit with the chain's.  A timing tool only: no number is promised.
Prints one JSON line per A.

    python tools/agent_bench.py [--sizes 1,4096,32768] [--ticks 100] [--reps 20] [--blocks 5] [--out agent_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from emplanner_carla_amd import _lib as L  # noqa: E402
from emplanner_carla_amd import api  # noqa: E402
from tests import agent_cases as ac  # noqa: E402

STATE = ("head", "past_steer", "lon_err", "n_lon", "lat_err", "n_lat")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,4096,32768")
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pl = api.Planner(0)
    lib, h, stream = pl._lib, pl._h, pl.torch_stream()
    prm, vp, T = api.agent_params(), api.agent_vehicle_params(), a.ticks
    P = lambda t: C.c_void_p(t.data_ptr())
    results = []
    for A in (int(x) for x in a.sizes.split(",")):
        b = ac.corner_fleet(A, ragged=False)
        M = b["path"].shape[1]
        g = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in b.items()}
        out = {k: torch.empty_like(g[k]) for k in ("state",) + STATE}                 # the rollout's outputs
        ch = {k: torch.empty_like(g[k]) for k in ("state",) + STATE}                  # the chain's state, updated in place
        status, done = torch.empty(A, dtype=torch.int32, device="cuda"), torch.empty(A, dtype=torch.int32, device="cuda")
        fw, kmh, ctl = (torch.empty(s, dtype=torch.float64, device="cuda") for s in ((A, 2), (A,), (A, 3)))
        io = L.AgentRolloutIO()
        for k in ("path", "n_path", "state", "target_speed") + STATE:
            setattr(io, k, P(g[k]))
        io.state_out = P(out["state"])
        for k in STATE:
            setattr(io, k + "_out", P(out[k]))
        io.status, io.done_tick, io.reserved = P(status), P(done), 0
        torch.cuda.synchronize()

        def rollout():
            r = lib.emp_agent_rollout(h, C.byref(prm), C.byref(vp), A, M, T, 1, C.byref(io), L.EMP_DEVICE)
            assert r == 0, lib.emp_last_error(h)

        def reset():
            for k in ch:
                ch[k].copy_(g[k])
            torch.cuda.current_stream().synchronize()

        def chain():
            for _ in range(T):
                r = lib.emp_agent_observe(h, A, P(ch["state"]), P(fw), P(kmh), None, L.EMP_DEVICE)
                r |= lib.emp_agent_control(h, C.byref(prm), A, M, P(g["path"]), P(g["n_path"]), P(ch["state"]), P(fw), P(kmh), P(g["target_speed"]),
                                           *[P(ch[k]) for k in STATE], P(ctl), P(status), *[P(ch[k]) for k in STATE], None, None, L.EMP_DEVICE)
                r |= lib.emp_vehicle_step(h, C.byref(vp), A, P(ch["state"]), P(ctl), P(ch["state"]), None, None, None, L.EMP_DEVICE)
                assert r == 0, lib.emp_last_error(h)

        rollout()
        reset()
        chain()
        pl.synchronize()
        for k in ch:                                                       # warm-up, and the two agree to the bit
            assert torch.equal(out[k], ch[k]), f"A={A}: {k} of the rollout differs from the chain"

        def timed(fn, reps, before=None):
            blocks = []
            for _ in range(a.blocks):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ms = 0.0
                for _ in range(reps):                                      # `before` (the chain's reset) stays outside the timed span
                    if before:
                        before()
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    ms += e0.elapsed_time(e1)
                blocks.append(ms / reps)
            return statistics.median(blocks), blocks

        r_ms, r_blocks = timed(rollout, a.reps)
        c_ms, c_blocks = timed(chain, max(1, a.reps // 4), reset)
        row = {"A": A, "ticks": T, "max_path": M, "rollout_ms": round(r_ms, 4), "rollout_spread_ms": [round(min(r_blocks), 4), round(max(r_blocks), 4)],
               "chain_launches": 3 * T, "chain_ms": round(c_ms, 4), "chain_spread_ms": [round(min(c_blocks), 4), round(max(c_blocks), 4)],
               "chain_over_rollout": round(c_ms / r_ms, 2), "us_per_agent_tick": round(1000.0 * r_ms / (A * T), 5), "reps": a.reps,
               "blocks": a.blocks, "timed": "one launch (or one chain of launches) between two HIP events, host issue included"}
        results.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)
    pl.close()


if __name__ == "__main__":
    main()
