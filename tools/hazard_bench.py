"""Times traffic that stops for red lights and pedestrians, by the method of tools/traffic_bench.py: for W x N in {1 x 2, 512 x 8,
512 x 64} worlds x agents on the circular track of tests/behavior_cases.py and T = 100 ticks, in one run on one build,
  hazards      emp_traffic_rollout_hazards with 4 lights and 8 walkers a world (tests/hazard_cases.add_hazards places them)
  no_hazards   the same call with none (n_light = n_walker = 0, max_light = max_walker = 0)
  rollout      emp_traffic_rollout on the same agents
  chain        the 300 separate launches (emp_agent_observe, emp_agent_behave_hazards, emp_vehicle_step per tick), hazards as above
Device-resident arrays (EMP_DEVICE), raw C-ABI calls, a pair of HIP events on the context's stream around each rollout (or chain,
host issue of its 300 calls included), the mean of `--reps` of them per block and the median of `--blocks` blocks with [min, max]
after a warm-up.  Every call starts from the same state (outputs go to arrays of their own; the chain's state is reset outside the
timed span).  Before anything is timed the hazard rollout's outputs are compared bit for bit with the chain's, and the no-hazard
rollout's with emp_traffic_rollout's.  A timing tool only: no number is promised.  Prints one JSON line per size.

    python tools/hazard_bench.py [--sizes 1x2,512x8,512x64] [--ticks 100] [--reps 20] [--blocks 5] [--out hazard_bench.json]
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
from tests import hazard_cases as hc  # noqa: E402
from tools.traffic_bench import IN, STATE, clocks  # noqa: E402

LIGHTS, WALKERS = 4, 8
HAZ_IN = ("n_light", "light", "light_lane", "light_cycle", "n_walker", "walker", "walker_lane")


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
    prm, prb, hpp, vp, T = api.agent_params(), api.behavior_params(), api.hazard_params(), api.agent_vehicle_params(), a.ticks
    P = lambda t: C.c_void_p(t.data_ptr())
    results = []
    for W, N in (tuple(int(v) for v in x.split("x")) for x in a.sizes.split(",")):
        M, A = 120, W * N
        b = bc.random_worlds((N,) * W, N, 0, M, seed=W + N)
        b["n_world"][:], b["n_path"][:], b["head"][:] = N, M, 0                    # full worlds, whole plans: nobody is DONE at once
        b["lane"][:] = 1
        b = hc.add_hazards(b, (LIGHTS,) * W, (WALKERS,) * W, LIGHTS, WALKERS, T // 2, np.random.default_rng(W + N))
        b["n_light"][:], b["n_walker"][:], b["last_light"][:] = LIGHTS, WALKERS, -1
        g = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in b.items()}
        new = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device="cuda")
        state_keys = ("state",) + STATE + ("last_light",)
        out = {k: torch.empty_like(g[k]) for k in state_keys}                         # the hazard rollout's outputs
        nout = {k: torch.empty_like(g[k]) for k in state_keys}                        # the no-hazard rollout's
        rout = {k: torch.empty_like(g[k]) for k in ("state",) + STATE}                # emp_traffic_rollout's
        ch = {k: torch.empty_like(g[k]) for k in state_keys}                          # the chain's state, updated in place
        misc = dict(status=new((W, N), torch.int32), done_tick=new((W, N), torch.int32), mode_ticks=new((W, N, 5), torch.int32), min_gap=new((W, N)),
                    control=new((W, N, 3)), mode=new((W, N), torch.int32), blocker=new((W, N), torch.int32), distance=new((W, N)), ttc=new((W, N)),
                    target_speed_out=new((W, N)), forward=new((W, N, 2)), speed_kmh=new((W, N)), cause=new((W, N), torch.int32),
                    light_hit=new((W, N), torch.int32), walker_hit=new((W, N), torch.int32), walker_distance=new((W, N)),
                    cause_ticks=new((W, N, 3), torch.int32), min_walker_gap=new((W, N)))

        def blocks(dst, in_place, hazards):
            io, hio = L.BehaviorIO(), L.HazardIO()
            src = dst if in_place else g
            for k in IN:
                setattr(io, k, P(g[k]))
            for k in STATE:
                setattr(io, k, P(src[k]))
                setattr(io, k + "_out", P(dst[k]))
            io.state, io.state_out = P(src["state"]), P(dst["state"])
            for k in ("status", "done_tick", "mode_ticks", "min_gap", "control", "mode", "blocker", "distance", "ttc", "target_speed_out", "forward",
                      "speed_kmh"):
                setattr(io, k, P(misc[k]))
            if hazards:
                for k in HAZ_IN:
                    setattr(hio, k, P(g[k]))
            if "last_light" in dst:
                hio.last_light, hio.last_light_out = P(src["last_light"]), P(dst["last_light"])
            for k in ("cause", "light_hit", "walker_hit", "walker_distance", "cause_ticks", "min_walker_gap"):
                setattr(hio, k, P(misc[k]))
            io.reserved = hio.reserved = 0
            return io, hio

        io, hio = blocks(out, False, True)
        nio, nhio = blocks(nout, False, False)
        rio, _ = blocks(rout, False, False)
        cio, chio = blocks(ch, True, True)
        torch.cuda.synchronize()

        def hazards():
            r = lib.emp_traffic_rollout_hazards(h, C.byref(prm), C.byref(prb), C.byref(vp), W, N, M, 0, T, 1, 0, C.byref(io), L.EMP_DEVICE,
                                                C.byref(hpp), LIGHTS, WALKERS, C.byref(hio))
            assert r == 0, lib.emp_last_error(h)

        def no_hazards():
            r = lib.emp_traffic_rollout_hazards(h, C.byref(prm), C.byref(prb), C.byref(vp), W, N, M, 0, T, 1, 0, C.byref(nio), L.EMP_DEVICE,
                                                C.byref(hpp), 0, 0, C.byref(nhio))
            assert r == 0, lib.emp_last_error(h)

        def rollout():
            r = lib.emp_traffic_rollout(h, C.byref(prm), C.byref(prb), C.byref(vp), W, N, M, 0, T, 1, 0, C.byref(rio), L.EMP_DEVICE)
            assert r == 0, lib.emp_last_error(h)

        def reset():
            for k in ch:
                ch[k].copy_(g[k])
            torch.cuda.current_stream().synchronize()

        def chain():
            for t in range(T):
                r = lib.emp_agent_observe(h, A, P(ch["state"]), P(misc["forward"]), P(misc["speed_kmh"]), None, L.EMP_DEVICE)
                r |= lib.emp_agent_behave_hazards(h, C.byref(prm), C.byref(prb), W, N, M, 0, t, C.byref(cio), L.EMP_DEVICE, C.byref(hpp), LIGHTS,
                                                  WALKERS, C.byref(chio))
                r |= lib.emp_vehicle_step(h, C.byref(vp), A, P(ch["state"]), P(misc["control"]), P(ch["state"]), None, None, None, L.EMP_DEVICE)
                assert r == 0, lib.emp_last_error(h)

        hazards()
        pl.synchronize()
        causes, ticks = misc["cause_ticks"].sum((0, 1)).tolist(), misc["mode_ticks"].sum((0, 1)).tolist()
        no_hazards()
        rollout()
        reset()
        chain()
        pl.synchronize()
        bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t      # deque entries past the count are NaN: compare bits
        for k in ch:                                                       # warm-up, and the calls agree to the bit
            assert torch.equal(bits(out[k]), bits(ch[k])), f"{W} x {N}: {k} of the hazard rollout differs from the chain"
        for k in rout:
            assert torch.equal(bits(nout[k]), bits(rout[k])), f"{W} x {N}: {k} of the no-hazard rollout differs from emp_traffic_rollout"

        def timed(fn, reps, before=None):
            blocks_ = []
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
                blocks_.append(ms / reps)
            return round(statistics.median(blocks_), 4), [round(min(blocks_), 4), round(max(blocks_), 4)]

        h_ms, h_sp = timed(hazards, a.reps)
        n_ms, n_sp = timed(no_hazards, a.reps)
        r_ms, r_sp = timed(rollout, a.reps)
        c_ms, c_sp = timed(chain, max(1, a.reps // 4), reset)
        row = {"W": W, "N": N, "agents": A, "ticks": T, "max_path": M, "lights": LIGHTS, "walkers": WALKERS, "hazards_ms": h_ms,
               "hazards_spread_ms": h_sp, "no_hazards_ms": n_ms, "no_hazards_spread_ms": n_sp, "traffic_rollout_ms": r_ms,
               "traffic_rollout_spread_ms": r_sp, "chain_launches": 3 * T, "chain_ms": c_ms, "chain_spread_ms": c_sp,
               "hazards_over_traffic_rollout": round(h_ms / r_ms, 3), "no_hazards_over_traffic_rollout": round(n_ms / r_ms, 3),
               "chain_over_hazards": round(c_ms / h_ms, 2), "mode_ticks": ticks, "cause_ticks": causes, "reps": a.reps, "blocks": a.blocks,
               "clocks": clocks(), "timed": "one launch (or one chain of launches) between two HIP events, host issue included"}
        results.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)
    pl.close()


if __name__ == "__main__":
    main()
