"""Times global routing for a fleet: emp_route_paths (one launch: A*, expansion, heading and curvature for B queries) on the
12 x 12 town of tests/golden/routing/sparse12.npz, B in {1, 4096, 32768} seeded queries.  Device-resident inputs (EMP_DEVICE), raw
C-ABI calls, HIP events on the context's stream around windows of `--reps` calls back to back (milliseconds per window at the
default), the median of `--blocks` windows after a warm-up call.  The same queries every call: the graph and the queries are warm
in cache, as they are for a fleet that routes on one map.  Beside it the Python port (tests/route_port.py) in this process on the
first `--port-queries` of the same queries: a reported baseline, not a target - its per-query time is what a drop-in user's interpreter would spend without networkx's
overhead.  The GPU's answers on those queries are compared with the port's before anything is timed.  The launch's LDS bytes and
its occupancy bound are plan_route's own (csrc/emp_route_launch.h, compiled with g++); the shader clock is read (never set) before
and after.
Prints one JSON line per B.

    python tools/route_bench.py [--sizes 1,4096,32768] [--reps 200] [--blocks 7] [--port-queries 256] [--out route_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from emplanner_carla_amd import _lib as L  # noqa: E402
from emplanner_carla_amd.api import Planner  # noqa: E402
from tests import route_cases as rc  # noqa: E402
from tests import route_port as port  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launch_plan(B, n_nodes, max_route, max_global):
    """grid, block, LDS bytes and wavefronts per compute unit (the LDS bound) as csrc/emp_route_launch.h's plan_route chooses them:
    the header itself, compiled with g++ through tests/host_check/route_check.cpp."""
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libroutecheck.so")
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", os.path.join(ROOT, "tests", "host_check", "route_check.cpp"),
                        "-o", so], check=True)
        lib = C.CDLL(so)
        lib.rc_plan.restype = C.c_char_p
        out = np.zeros(4, np.int64)
        err = lib.rc_plan(int(B), int(n_nodes), int(max_route), int(max_global), C.c_void_p(out.ctypes.data))
        assert err is None, err
    return dict(grid=int(out[0]), block=int(out[1]), lds_bytes_per_block=int(out[2]), waves_per_cu_by_lds=int(out[3]))


def queries(g, B, seed=5):
    """B (start node, end edge) pairs, the origin on an edge that leaves the start node, the destination on the end edge."""
    rng = np.random.default_rng(seed)
    has_out = np.nonzero(np.diff(g.succ_off) > 0)[0]
    s = rng.choice(has_out, B).astype(np.int32)
    e = rng.integers(0, g.n_edges, B).astype(np.int32)
    first = g.succ_off[s] + (rng.integers(0, 1 << 30, B) % np.diff(g.succ_off)[s])
    pick = lambda edges: g.wp_off[edges] + (rng.integers(0, 1 << 30, B) % np.diff(g.wp_off)[edges])
    return s, e, np.ascontiguousarray(g.wp[pick(first)]), np.ascontiguousarray(g.wp[pick(e)])


def shader_clock():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=30).stdout
        card = next(iter(json.loads(out).values()))
        return {k: v for k, v in card.items() if "sclk" in k.lower() or "mclk" in k.lower()}
    except Exception as err:       # the tool is optional: the timing stands without it, the clock is then "not read"
        return {"not read": type(err).__name__}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,4096,32768")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--port-queries", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g, want = rc.graph("sparse12"), rc.expected("sparse12")
    max_route, max_global = g.n_nodes + 1, 2 * int(want["n_global"].max())
    pl = Planner(0)
    lib, h, stream = pl._lib, pl._h, pl.torch_stream()
    dev = g.on_device(torch.device("cuda", 0))
    graph = g.struct([t.data_ptr() for t in dev])
    P = lambda t: C.c_void_p(t.data_ptr())
    results = []
    for B in (int(x) for x in a.sizes.split(",")):
        q = queries(g, B)
        ins = [torch.from_numpy(x).cuda() for x in q]
        outs = [torch.empty(sh, dtype=dt, device="cuda") for sh, dt in (
            ((B, max_route), torch.int32), ((B,), torch.int32), ((B, max_global), torch.int32), ((B, max_global, 4), torch.float64),
            ((B,), torch.int32), ((B,), torch.int32))]
        torch.cuda.synchronize()

        def call():
            r = lib.emp_route_paths(h, C.byref(graph), B, max_route, max_global, *[P(t) for t in ins], *[P(t) for t in outs], L.EMP_DEVICE)
            assert r == 0, lib.emp_last_error(h)

        clock0 = shader_clock()
        call()                                                             # warm-up, and the answers are the port's
        pl.synchronize()
        n = min(B, a.port_queries)
        t0 = time.perf_counter()
        p = port.run(g, *[x[:n] for x in q], max_route, max_global)
        port_s = time.perf_counter() - t0
        got = [t[:n].cpu().numpy() for t in outs]
        for k, x in zip(("route", "route_len", "wp_index", None, "n_global", "status"), got):
            if k:
                assert np.array_equal(x, p[k]), f"B={B}: {k} differs from the port"
        assert np.array_equal(got[3][..., :2].view(np.uint64), p["xy"].view(np.uint64))
        blocks = []
        for _ in range(a.blocks):                                          # one window = `reps` calls back to back between two events
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.reps):
                call()
            e1.record(stream)
            e1.synchronize()
            blocks.append(e0.elapsed_time(e1) / a.reps)
        ms = statistics.median(blocks)
        status = outs[5].cpu().numpy()
        row = {"town": "sparse12", "nodes": g.n_nodes, "edges": g.n_edges, "B": B, "route_paths_ms": round(ms, 4),
               "spread_ms": [round(min(blocks), 4), round(max(blocks), 4)], "us_per_query": round(1000.0 * ms / B, 3),
               "mean_route_len": round(float(outs[1].double().mean()), 2), "mean_n_global": round(float(outs[4].double().mean()), 2),
               "unreachable": int((status == L.ROUTE_UNREACHABLE).sum()), "truncated": int((status & L.ROUTE_TRUNCATED != 0).sum()),
               "max_route": max_route, "max_global": max_global, **launch_plan(B, g.n_nodes, max_route, max_global),
               "port_queries": n, "port_ms_per_query": round(1000.0 * port_s / n, 3),
               "port_ms_for_B_extrapolated": round(1000.0 * port_s / n * B, 1), "reps": a.reps, "blocks": a.blocks,
               "clock_before": clock0, "clock_after": shader_clock()}
        results.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)
    pl.close()


if __name__ == "__main__":
    main()
