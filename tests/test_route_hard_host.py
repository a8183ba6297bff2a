"""CPU suite of global routing on the hostile graphs of tests/route_hard_cases.py: the Python port against the reference's recorded
answers (tests/golden/routing_hard/, every query), the cases against what they were built to hold (asserted from the port's
statistics, whose table DESIGN.md 3.10 carries), mutants of the port that the cases must catch, the g++ builds of
csrc/emp_route_core.h - one lane (tests/host_check/route_check.cpp) and 64 threads behind barriers
(tests/host_check/route_wave64.cpp) - bit for bit against the port, the 64-thread program under ThreadSanitizer and under
AddressSanitizer + UBSan as plain subprocesses, and - where the reference tree is present - the fixtures regenerated bit for bit."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from emplanner_carla_amd import _lib as L
from tests import route_cases as rc
from tests import route_hard_cases as hc
from tests import route_port as port
from tests.test_routing_host import host_route, same

ROOT = rc.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden")
CHECK = os.path.join(ROOT, "tests", "host_check", "route_check.cpp")
WAVE = os.path.join(ROOT, "tests", "host_check", "route_wave64.cpp")
sys.path.insert(0, GOLDEN)


def _declare(fn):
    fn.restype = None
    fn.argtypes = [C.POINTER(L.RouteGraph), C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 10


class _As:
    """a library whose rc_route is another entry point, for test_routing_host.host_route"""

    def __init__(self, fn):
        self.rc_route = fn


@pytest.fixture(scope="module")
def one_lane(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("route_hard") / "libroutecheck.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", CHECK, "-o", out], check=True)
    lib = C.CDLL(out)
    _declare(lib.rc_route)
    return lib


@pytest.fixture(scope="module")
def wave64(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("route_wave64") / "libroutewave64.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-Wall", WAVE, "-o", out], check=True)
    lib = C.CDLL(out)
    _declare(lib.rw_route)
    return _As(lib.rw_route)


# ---- the port against the reference's recorded answers ---------------------------------------------------------------------------------
def test_every_recorded_case_has_its_file_and_fits():
    assert sorted(os.listdir(hc.HARD)) == sorted(n + ".npz" for n in hc.RECORDED)
    limit = os.path.getsize(os.path.join(rc.ROUTING, "sparse12.npz"))
    for n in hc.RECORDED:
        assert os.path.getsize(os.path.join(hc.HARD, n + ".npz")) < limit, n


@pytest.mark.parametrize("name", hc.RECORDED)
def test_port_equals_the_reference_on_every_recorded_query(name):
    """The recorded graph and queries are the case's own; route, _A_star's list, waypoint rows, xy to the bit: no query excluded."""
    f = hc.recorded(name)
    g, (s, e, ow, dw) = hc.case(name)
    for k, a in zip(("vertex", "succ_off", "succ", "length", "wp_off", "wp"), g.arrays()):
        assert a.dtype == f[k].dtype and np.array_equal(a, f[k]), f"{name}: {k}"
    for k, a in zip(("q_start_node", "q_end_edge", "q_origin_wp", "q_dest_wp"), (s, e, ow, dw)):
        assert a.dtype == f[k].dtype and np.array_equal(a, f[k], equal_nan=a.dtype.kind == "f"), f"{name}: {k}"
    got, st = hc.solved(name)
    Q = len(s)
    assert Q >= 40 and len(f["reachable"]) == Q
    np.testing.assert_array_equal(got["status"], np.where(f["reachable"] == 1, 0, port.UNREACHABLE), err_msg=name)
    np.testing.assert_array_equal(got["route_len"], np.diff(f["route_off"]), err_msg=f"{name}: route_len")
    np.testing.assert_array_equal(got["n_global"], np.diff(f["path_off"]), err_msg=f"{name}: n_global")
    for k in range(Q):
        a, b = f["route_off"][k:k + 2]
        assert list(got["route"][k, :b - a]) == list(f["route"][a:b]), f"{name}: route of query {k}"
        a, b = f["path_off"][k:k + 2]
        assert list(got["wp_index"][k, :b - a]) == list(f["path_row"][a:b]), f"{name}: waypoint rows of query {k}"
        assert np.array_equal(got["xy"][k, :b - a].view(np.uint64), f["path_xy"][a:b].view(np.uint64)), f"{name}: xy of query {k}"
        a, b = f["astar_off"][k:k + 2]
        n_end, _ = port.edge_ends(g, int(e[k]))
        assert (port.astar(g, int(s[k]), n_end) or []) == list(f["astar"][a:b]), f"{name}: _A_star of query {k}"
    assert np.array_equal(f["gap"], st["gap"])
    assert f["gap"].min() >= 1e-9, "a pop of this fixture is decided by less than hypot and sqrt may differ by"


def test_the_reference_index_of_no_distance_is_kept():
    """deep_wp's last three routed queries: a NaN origin and a -inf origin coordinate leave the reference's index at -1, so the
    first edge gives its exit alone; a +inf dest gives nothing of the last edge.  (Recorded: the test above compares them.)"""
    g, (s, e, ow, dw) = hc.case("deep_wp")
    got, st = hc.solved("deep_wp")
    nan_o = [k for k in range(len(s)) if np.isnan(ow[k]).any()]
    inf_o = [k for k in range(len(s)) if np.isinf(ow[k]).any()]
    inf_d = [k for k in range(len(s)) if np.isinf(dw[k]).any()]
    assert len(nan_o) == len(inf_o) == len(inf_d) == 1 and len({nan_o[0], inf_o[0], inf_d[0]}) == 3
    for k in nan_o + inf_o:
        assert got["status"][k] == 0 and st["tied"][k][0] == []
        first = port.find_edge(g, got["route"][k, 0], got["route"][k, 1])
        assert got["wp_index"][k, 0] == g.wp_off[first + 1] - 1 and g.wp_off[first + 1] - g.wp_off[first] >= 2
    k = inf_d[0]
    assert got["status"][k] == 0 and st["tied"][k][1] == []
    route = list(got["route"][k, :got["route_len"][k]])
    edges = [port.find_edge(g, u, v) for u, v in zip(route[:-2], route[1:-1])] or [int(e[k])]      # all but the last (two nodes: the one)
    count = np.diff(g.wp_off)
    assert got["n_global"][k] == count[edges[0]] - st["tied"][k][0][0] + sum(count[x] - 1 for x in edges[1:])


# ---- the cases hold what they are for -----------------------------------------------------------------------------------------------------
def test_cases_hold_what_they_are_for():
    """Conditions on the INPUTS, from the port's statistics.  Prints the table that DESIGN.md 3.10 carries, and holds it to it."""
    rows = [hc.stats_row(n) for n in hc.PORTED]
    print("\n" + hc.STATS_HEAD + "\n" + "\n".join(rows))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert hc.STATS_HEAD in design
    for r in rows:
        assert r + "\n" in design, f"DESIGN.md 3.10 does not carry this row:\n{r}"
    for n in hc.PORTED:
        g, q = hc.case(n)
        st = hc.solved(n)[1]
        assert len(q[0]) >= 40 and 2 * st["status"].get(0, 0) >= len(q[0]), n
        assert st["status"].get(port.UNREACHABLE, 0) >= 1 or n in ("grid_4096", "flat_h", "flat_h_zero"), n
    for n, N in (("lattice_63", 63), ("lattice_64", 64), ("lattice_65", 65), ("fans_300", 300), ("wide_1000", 1000), ("grid_4096", 4096)):
        assert hc.case(n)[0].n_nodes == N
    wide, grid = hc.solved("wide_1000")[1], hc.solved("grid_4096")[1]
    assert wide["updates"] >= 100 and wide["tie_pops"] >= 50 and wide["max_open"] > 192 and grid["max_open"] > 192
    assert sorted(hc.fan_nodes("wide_1000").values()) == [64, 64, 130, 130] and {64, 130} <= wide["popped_degree"]
    # fans: every size exists, is popped, and starts queries - the first one among them
    fans = hc.fan_nodes("fans_300")
    assert sorted(fans.values()) == sorted(hc.FANS) and set(hc.FANS) <= hc.solved("fans_300")[1]["popped_degree"]
    s = hc.case("fans_300")[1][0]
    assert int(s[0]) in fans and all((s == n).sum() >= 3 for n in fans)
    # updates of OPEN nodes and tie-decided pops in one search, on several cases
    assert sum(1 for n in hc.PORTED if hc.solved(n)[1]["updates"] >= 40 and hc.solved(n)[1]["tie_pops"] >= 10) >= 8
    # flat h: f = g, and with every length 0 every pop with a choice is a tie
    assert len(np.unique(hc.case("flat_h")[0].vertex, axis=0)) == 1 and not hc.case("flat_h_zero")[0].length.any()
    zero = hc.solved("flat_h_zero")[1]
    assert math.isinf(zero["min_gap"]) and zero["tie_pops"] >= 1000 and hc.solved("flat_h")[1]["min_gap"] == 1.0
    # huge: dx dx overflows, h is +inf or 0
    g = hc.case("huge")[0]
    hs = {port.dist3(g.vertex[a], g.vertex[b]) for a in range(g.n_nodes) for b in range(0, g.n_nodes, 7)}
    assert hs == {0.0, math.inf} and np.isfinite(g.vertex).all()
    assert set(np.unique(hc.case("long_len")[0].length)) == {0, hc.MAX_LEN - 1, hc.MAX_LEN}
    # deep_wp: every waypoint count, long edges first and last on routes, ties of closest a stride or more apart and in one lane
    g, (s, e, ow, dw) = hc.case("deep_wp")
    got, st = hc.solved("deep_wp")
    count = np.diff(g.wp_off)
    assert set(count) == set(hc.DEEP_COUNTS)
    routed = [k for k in range(len(s)) if got["status"][k] == 0]
    first = {int(count[port.find_edge(g, got["route"][k, 0], got["route"][k, 1])]) for k in routed}
    last = {int(count[e[k]]) for k in routed}
    assert set(hc.DEEP_COUNTS) <= first and set(hc.DEEP_COUNTS) <= last
    both = [max(a, b) for a, b in zip(hc.spans(st["tied"], 0), hc.spans(st["tied"], 1))]
    assert sum(1 for x in both if x >= 64) >= 5
    lane = lambda t: len(t) > 1 and any((b - a) % 64 == 0 for i, a in enumerate(t) for b in t[i + 1:])
    assert sum(1 for t in st["tied"] if t is not None and (lane(t[0]) or lane(t[1]))) >= 5
    assert sum(1 for t in st["tied"] if t is not None and len(t[1]) > 1 and t[1][0] == 0) >= 1       # the tie makes k = 0
    assert (got["n_global"] > 130).any()
    # empty lists at both ends of succ_off and in the middle; end_edge next to them
    g, (s, e, ow, dw) = hc.case("empty_ends")
    deg = np.diff(g.succ_off)
    N, E = g.n_nodes, g.n_edges
    assert not deg[[0, 1, 30, 31, 50, N - 2, N - 1]].any() and deg[2] and deg[N - 3]
    assert {0, E - 1, int(g.succ_off[30]) - 1, int(g.succ_off[32]), int(g.succ_off[50]) - 1, int(g.succ_off[51])} <= set(e.tolist())
    assert {0, 1, N - 1, N - 2} <= set(s.tolist())
    # NaN vertices: at the n_end of some queries; on the way of others
    g, (s, e, ow, dw) = hc.case("nan_vertex_end")
    at_end = np.isnan(g.vertex[np.repeat(np.arange(g.n_nodes), np.diff(g.succ_off))[e]]).any(1)
    assert at_end.sum() >= 10 and (~at_end).sum() >= 10 and (hc.solved("nan_vertex_end")[0]["status"][at_end] == 0).sum() >= 10
    g, (s, e, ow, dw) = hc.case("nan_vertex_way")
    assert np.isnan(g.vertex).any(1).sum() == 6
    assert not np.isnan(g.vertex[np.repeat(np.arange(g.n_nodes), np.diff(g.succ_off))[e]]).any()


# ---- the cases have teeth -------------------------------------------------------------------------------------------------------------------
def mutant_astar(g, start, n_end, m):
    """route_port.astar with one rule changed: ``tie_index`` (equal f: the smallest node index), ``tie_newest`` (the newest
    insertion), ``update_restamps`` (an update of an OPEN node renews its stamp), ``relax_le`` (<= in the relaxation),
    ``chunk_stamps`` (the stamps start again with every 64 successors of a node), ``nan_first`` (a NaN f orders first).
    None: no change."""
    N = g.n_nodes
    h = {}
    state, gc, parent, stamp, nxt = [0] * N, [0] * N, [-1] * N, [0] * N, 1
    state[start], opened = 1, [start]

    def key(n):
        if n not in h:
            h[n] = port.dist3(g.vertex[n], g.vertex[n_end])
        f = float(gc[n]) + h[n]
        if f != f:
            f = -math.inf if m == "nan_first" else math.inf
        return f, (n if m == "tie_index" else -stamp[n] if m == "tie_newest" else stamp[n]), n

    for _ in range(N):
        if not opened:
            return None
        c = min(opened, key=key)
        opened.remove(c)
        if c == n_end:
            break
        base = nxt
        for i, ed in enumerate(range(g.succ_off[c], g.succ_off[c + 1])):
            if m == "chunk_stamps" and i and i % 64 == 0:
                nxt = base
            v, ng = int(g.succ[ed]), gc[c] + int(g.length[ed])
            if state[v] == 1:
                if ng < gc[v] or (m == "relax_le" and ng == gc[v] and v != c):
                    gc[v], parent[v] = ng, c
                    if m == "update_restamps":
                        stamp[v], nxt = nxt, nxt + 1
            elif state[v] == 0:
                state[v], gc[v], parent[v], stamp[v], nxt = 1, ng, c, nxt, nxt + 1
                opened.append(v)
        state[c] = 2
    else:
        return None
    route = [n_end]
    while parent[route[-1]] != -1 and len(route) <= N:
        route.append(parent[route[-1]])
    return route[::-1]




@pytest.mark.parametrize("m", (None, "tie_index", "tie_newest", "update_restamps", "relax_le", "chunk_stamps", "nan_first"))
def test_mutants_of_the_search_change_routes(m):
    """Each wrong rule returns other routes than the port on at least ten queries of the set; the unchanged copy on none."""
    wrong = {}
    for name in hc.PORTED:
        g, (s, e, _, _) = hc.case(name)
        want = hc.solved(name)[0]
        for k in range(len(s)):
            n_end, _ = port.edge_ends(g, int(e[k]))
            r = mutant_astar(g, int(s[k]), n_end, m)
            n = int(want["route_len"][k])
            wrong[name] = wrong.get(name, 0) + ((r or []) != list(want["route"][k, :max(n - 1, 0)]))
    print(f"\nmutant {m}: queries with another route, per case: {wrong}")
    total = sum(wrong.values())
    assert total == 0 if m is None else total >= 10, wrong
    if m == "chunk_stamps":
        assert wrong["flat_h"] >= 10          # only a list of more than 64 successors can tell
    if m == "nan_first":
        assert wrong["nan_vertex_way"] >= 10 and total == wrong["nan_vertex_way"] + wrong["nan_vertex_end"]


def test_a_mutant_of_closest_changes_paths(monkeypatch):
    """closest with <= (the LAST index of the smallest distance) emits other waypoints on at least ten queries."""
    def closest_le(g, p, a, b, tied=None):
        best, k = math.inf, -1
        for j in range(a, b):
            d = port.dist3(g.wp[j], p)
            if d <= best and d < math.inf:
                best, k = d, j - a
        return k

    monkeypatch.setattr(port, "closest", closest_le)
    wrong = {}
    for name in hc.PORTED:
        g, (s, e, ow, dw) = hc.case(name)
        want = hc.solved(name)[0]
        for k in range(len(s)):
            if want["status"][k]:
                continue
            rows = port.expand(g, list(want["route"][k, :want["route_len"][k]]), ow[k], dw[k])
            wrong[name] = wrong.get(name, 0) + (rows != list(want["wp_index"][k, :want["n_global"][k]]))
    print(f"\nmutant closest <=: queries with other waypoints, per case: {wrong}")
    assert wrong["deep_wp"] >= 10


# ---- the core, one lane and 64 threads, against the port ---------------------------------------------------------------------------------------
def core_equals_port(lib, name, search_only_on=slice(None)):
    g, (s, e, ow, dw) = hc.case(name)
    want = hc.solved(name)[0]
    R, G = want["route"].shape[1], want["wp_index"].shape[1]
    got = host_route(lib, g, s, e, ow, dw, R, G)
    same(got, want, name)
    rc.padded_ok(got, R, G, name)
    k = search_only_on
    only = host_route(lib, g, s[k], e[k], ow[k], dw[k], R, 1, search_only=True)
    same(only, {x: want[x][k] for x in ("route", "route_len", "status")}, name + " (search only)", keys=("route", "route_len", "status"))
    assert not only["wp_index"].any() and not only["n_global"].any() and not only["global_path"].any()
    return got


@pytest.mark.parametrize("name", hc.PORTED)
def test_one_lane_core_equals_the_port_bit_for_bit(one_lane, name):
    core_equals_port(one_lane, name)


@pytest.mark.parametrize("name", hc.WAVE64)
def test_wave_of_64_threads_equals_the_port_and_the_one_lane_core_bit_for_bit(one_lane, wave64, name):
    """routes, counts, statuses, waypoint rows, xy - and every byte, theta and kappa included, against the one-lane build.  (64
    threads on a few cores pay for every barrier: the A*-only form runs every third query here, and all of them on one lane.)"""
    a, b = core_equals_port(wave64, name, slice(None, None, 3)), core_equals_port(one_lane, name)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"{name}: {k}"


def test_one_lane_core_on_the_long_chain(one_lane):
    """4096 nodes, every length 2^18: g reaches 4095 * 2^18 = 2^30 - 2^18 and stays an int32"""
    g, (s, e, ow, dw), want = hc.chain_long()
    n = g.n_nodes
    got = host_route(one_lane, g, s, e, ow, dw, n, n)
    check_chain(got, g, want)


def check_chain(got, g, want):
    n = g.n_nodes
    assert (n - 1) * hc.MAX_LEN < 2 ** 31 and (g.length == hc.MAX_LEN).all()
    for b, w in enumerate(want):
        if w is None:
            assert got["status"][b] == port.UNREACHABLE and got["route_len"][b] == 0 and got["n_global"][b] == 0
            continue
        route, rows = w
        assert got["status"][b] == 0 and got["route_len"][b] == len(route) and got["n_global"][b] == len(rows), b
        np.testing.assert_array_equal(got["route"][b, :len(route)], route)
        np.testing.assert_array_equal(got["wp_index"][b, :len(rows)], rows)
        assert np.array_equal(np.ascontiguousarray(got["global_path"][b, :len(rows), :2]).view(np.uint64), g.wp[rows, :2].copy().view(np.uint64))
    rc.padded_ok(got, n, n, "chain_4096_long")


# ---- the 64-thread wave as a program of its own, under sanitizers ----------------------------------------------------------------------------------
def write_case(path, name):
    g, (s, e, ow, dw) = hc.case(name)
    want = hc.solved(name)[0]
    head = np.array([g.n_nodes, g.n_edges, g.n_wp, len(s), want["route"].shape[1], want["wp_index"].shape[1], 0, 0], np.int32)
    with open(path, "wb") as f:
        for a in (head,) + g.arrays() + (s, e, ow, dw):
            raw = np.ascontiguousarray(a).tobytes()
            f.write(raw + b"\0" * (-len(raw) % 8))


@pytest.mark.parametrize("sanitizer", ("thread", "address,undefined"))
def test_wave64_program_under_sanitizers(tmp_path, sanitizer):
    """-DROUTE_WAVE64_MAIN: 64 threads against one lane, byte for byte, on fans_300 and deep_wp.  A ThreadSanitizer report is a
    missing barrier in csrc/emp_route_core.h."""
    exe = str(tmp_path / "route_wave64")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off", f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all",
                    "-DROUTE_WAVE64_MAIN", WAVE, "-o", exe], check=True)
    for name in ("fans_300", "deep_wp"):
        path = str(tmp_path / (name + ".bin"))
        write_case(path, name)
        run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        print(f"\n-fsanitize={sanitizer} {name}: exit {run.returncode}: {run.stdout.strip()}")
        assert run.returncode == 0 and "agree" in run.stdout and "Sanitizer" not in run.stderr, run.stdout + run.stderr[-3000:]


# ---- live: the fixtures regenerate ---------------------------------------------------------------------------------------------------------------------
def test_hard_routing_fixtures_regenerate_bit_for_bit(tmp_path):
    import ref_loader
    if not ref_loader.reference_available():
        pytest.skip("the reference tree is not present")
    env = dict(os.environ, EMP_GOLDEN_OUT=str(tmp_path))
    run = subprocess.run([sys.executable, "-B", os.path.join(GOLDEN, "make_golden_routing_hard.py")], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert sorted(os.listdir(hc.HARD)) == sorted(os.listdir(tmp_path / "routing_hard")) == sorted(n + ".npz" for n in hc.RECORDED)
    for name in hc.RECORDED:
        want, got = np.load(os.path.join(hc.HARD, name + ".npz")), np.load(tmp_path / "routing_hard" / (name + ".npz"))
        assert sorted(want.files) == sorted(got.files), name
        for k in want.files:
            a, b = want[k], got[k]
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), f"{name}: {k}"
