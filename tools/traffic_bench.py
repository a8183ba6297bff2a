"""Times traffic that reacts to traffic: emp_traffic_rollout of T = 100 ticks (one launch) against the chain of the 300 separate
launches (emp_agent_observe, emp_agent_behave, emp_vehicle_step per tick) for W x N in {1 x 2, 512 x 8, 512 x 64} worlds x agents on
the circular track of tests/behavior_cases.py, and - in the same run, on the same build - emp_agent_rollout of as many agents on the
same paths, as information: the price of looking at each other.  Device-resident arrays (EMP_DEVICE), raw C-ABI calls, a pair of HIP
events on the context's stream around each rollout (or chain, host issue of its 300 calls included), the mean of `--reps` of them
per block and the median of `--blocks` blocks after a warm-up.  Every rollout and every chain starts from the same state (the
rollout's outputs go to arrays of their own; the chain's state is reset outside the timed span).  Before anything is timed the
rollout's outputs are compared bit for bit with the chain's.  A timing tool only: no number is promised.
Prints one JSON line per size.

    python tools/traffic_bench.py [--sizes 1x2,512x8,512x64] [--ticks 100] [--reps 20] [--blocks 5] [--out traffic_bench.json]
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
from tests import behavior_cases as bc  # noqa: E402

STATE = ("head", "past_steer", "lon_err", "n_lon", "lat_err", "n_lat")
IN = ("n_world", "path", "n_path", "lane", "speed_limit", "extent")


def clocks():
    """What the device says about its clocks, as far as this process can read it."""
    out = {"max_sclk_mhz": round(torch.cuda.get_device_properties(0).clock_rate / 1000.0, 1) if hasattr(torch.cuda.get_device_properties(0), "clock_rate") else None}
    try:
        out["sclk_mhz_now"] = int(torch.cuda.clock_rate())
    except Exception as e:                                                   # no SMI binding in this installation
        out["sclk_mhz_now"] = None
        out["sclk_note"] = type(e).__name__
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1x2,512x8,512x64")
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pl = api.Planner(0)
    lib, h, stream = pl._lib, pl._h, pl.torch_stream()
    prm, prb, vp, T = api.agent_params(), api.behavior_params(), api.agent_vehicle_params(), a.ticks
    P = lambda t: C.c_void_p(t.data_ptr())
    results = []
    for W, N in (tuple(int(v) for v in x.split("x")) for x in a.sizes.split(",")):
        M, A = 120, W * N
        b = bc.random_worlds((N,) * W, N, 0, M, seed=W + N)
        b["n_world"][:], b["n_path"][:], b["head"][:] = N, M, 0                    # full worlds, whole plans: nobody is DONE at once
        b["lane"][:] = 1
        g = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in b.items()}
        new = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device="cuda")
        out = {k: torch.empty_like(g[k]) for k in ("state",) + STATE}                 # the rollout's outputs
        ch = {k: torch.empty_like(g[k]) for k in ("state",) + STATE}                  # the chain's state, updated in place
        misc = dict(status=new((W, N), torch.int32), done_tick=new((W, N), torch.int32), mode_ticks=new((W, N, 5), torch.int32), min_gap=new((W, N)),
                    control=new((W, N, 3)), mode=new((W, N), torch.int32), blocker=new((W, N), torch.int32), distance=new((W, N)), ttc=new((W, N)),
                    target_speed_out=new((W, N)), forward=new((W, N, 2)), speed_kmh=new((W, N)))
        io, cio = L.BehaviorIO(), L.BehaviorIO()
        for k in IN:
            setattr(io, k, P(g[k]))
            setattr(cio, k, P(g[k]))
        for k in STATE:
            setattr(io, k, P(g[k]))
            setattr(io, k + "_out", P(out[k]))
            setattr(cio, k, P(ch[k]))
            setattr(cio, k + "_out", P(ch[k]))
        io.state, io.state_out, cio.state = P(g["state"]), P(out["state"]), P(ch["state"])
        for k in ("status", "done_tick", "mode_ticks", "min_gap"):
            setattr(io, k, P(misc[k]))
        for k in ("status", "control", "mode", "blocker", "distance", "ttc", "target_speed_out", "forward", "speed_kmh"):
            setattr(cio, k, P(misc[k]))
        io.reserved = cio.reserved = 0
        # the same agents without the law: emp_agent_rollout at the law's normal target
        flat = {k: g[k].reshape((A,) + tuple(g[k].shape[2:])) for k in ("path", "n_path", "state") + STATE}
        aout = {k: torch.empty_like(flat[k]) for k in ("state",) + STATE}
        target = torch.clamp(g["speed_limit"].reshape(A) - 3.0, max=50.0).contiguous()
        aio = L.AgentRolloutIO()
        for k in ("path", "n_path", "state") + STATE:
            setattr(aio, k, P(flat[k]))
        aio.target_speed, aio.state_out = P(target), P(aout["state"])
        for k in STATE:
            setattr(aio, k + "_out", P(aout[k]))
        a_status, a_done = new((A,), torch.int32), new((A,), torch.int32)
        aio.status, aio.done_tick, aio.reserved = P(a_status), P(a_done), 0
        torch.cuda.synchronize()

        def rollout():
            r = lib.emp_traffic_rollout(h, C.byref(prm), C.byref(prb), C.byref(vp), W, N, M, 0, T, 1, 0, C.byref(io), L.EMP_DEVICE)
            assert r == 0, lib.emp_last_error(h)

        def agents():
            r = lib.emp_agent_rollout(h, C.byref(prm), C.byref(vp), A, M, T, 1, C.byref(aio), L.EMP_DEVICE)
            assert r == 0, lib.emp_last_error(h)

        def reset():
            for k in ch:
                ch[k].copy_(g[k])
            torch.cuda.current_stream().synchronize()

        def chain():
            for t in range(T):
                r = lib.emp_agent_observe(h, A, P(ch["state"]), P(misc["forward"]), P(misc["speed_kmh"]), None, L.EMP_DEVICE)
                r |= lib.emp_agent_behave(h, C.byref(prm), C.byref(prb), W, N, M, 0, t, C.byref(cio), L.EMP_DEVICE)
                r |= lib.emp_vehicle_step(h, C.byref(vp), A, P(ch["state"]), P(misc["control"]), P(ch["state"]), None, None, None, L.EMP_DEVICE)
                assert r == 0, lib.emp_last_error(h)

        rollout()
        agents()
        reset()
        chain()
        pl.synchronize()
        bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t      # deque entries past the count are NaN: compare bits
        for k in ch:                                                       # warm-up, and the two agree to the bit
            assert torch.equal(bits(out[k]), bits(ch[k])), f"{W} x {N}: {k} of the rollout differs from the chain"
        ticks = misc["mode_ticks"].sum((0, 1)).tolist()

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
        g_ms, g_blocks = timed(agents, a.reps)
        c_ms, c_blocks = timed(chain, max(1, a.reps // 4), reset)
        row = {"W": W, "N": N, "agents": A, "ticks": T, "max_path": M, "rollout_ms": round(r_ms, 4),
               "rollout_spread_ms": [round(min(r_blocks), 4), round(max(r_blocks), 4)], "chain_launches": 3 * T, "chain_ms": round(c_ms, 4),
               "chain_spread_ms": [round(min(c_blocks), 4), round(max(c_blocks), 4)], "chain_over_rollout": round(c_ms / r_ms, 2),
               "agent_rollout_ms": round(g_ms, 4), "agent_rollout_spread_ms": [round(min(g_blocks), 4), round(max(g_blocks), 4)],
               "rollout_over_agent_rollout": round(r_ms / g_ms, 2), "us_per_agent_tick": round(1000.0 * r_ms / (A * T), 5),
               "mode_ticks": ticks, "reps": a.reps, "blocks": a.blocks, "clocks": clocks(),
               "timed": "one launch (or one chain of launches) between two HIP events, host issue included"}
        results.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)
    pl.close()


if __name__ == "__main__":
    main()
