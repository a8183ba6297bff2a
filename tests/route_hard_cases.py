"""Hostile graphs for global routing, shared by the CPU and the GPU suite: exact ties in f and in ``closest``, successor lists on
either side of one and two 64-lane chunks, open sets of several strides, lengths 0 and 2^18, edges of up to 200 waypoints, a
heuristic that overflows, NaN vertices on device graphs, empty successor lists at both ends of ``succ_off``.  Everything is seeded
and built from small integers (halves for query points), so every sum of squares is exact and equal distances are equal in bits.
No GPU and no reference tree is needed to import this.

``case(name)`` is ``(RoadGraph, (start_node, end_edge, origin_wp, dest_wp))``; ``solved(name)`` the port's answer to it in the
C-ABI's padded layout together with ``stats``.  RECORDED are the cases the reference was asked about
(tests/golden/make_golden_routing_hard.py -> tests/golden/routing_hard/<name>.npz)."""
from __future__ import annotations

import functools
import math
import os

import numpy as np

from emplanner_carla_amd.routing import RoadGraph
from tests import route_cases as rc
from tests import route_port as port

HARD = os.path.join(rc.ROOT, "tests", "golden", "routing_hard")
LENGTHS = (0, 0, 1, 1, 2, 3, 7)
DEGREES = (0, 1, 2, 3, 5)
FANS = (64, 65, 128, 129, 200)
DEEP_COUNTS = (2, 3, 63, 64, 65, 66, 128, 129, 200)
RECORDED = ("lattice_63", "lattice_64", "lattice_65", "fans_300", "wide_1000", "flat_h", "flat_h_zero", "long_len", "deep_wp",
            "empty_ends")
DEVICE_ONLY = ("nan_vertex_end", "nan_vertex_way")
PORTED = RECORDED + ("huge", "grid_4096") + DEVICE_ONLY          # every case the port answers (chain_4096_long: analytic)
WAVE64 = tuple(n for n in PORTED if n != "grid_4096")            # what the 64-thread library runs as well
MAX_LEN = 1 << 18


def _assemble(vertex, adj, length, wps, checked=True):
    """adj[u]: successors in CSR order; length[u][i], wps[u][i] ([n][3]) belong to adj[u][i]."""
    succ_off = np.concatenate([[0], np.cumsum([len(a) for a in adj])]).astype(np.int32)
    succ = np.array([v for a in adj for v in a], np.int32)
    ln = np.array([x for a in length for x in a], np.int32)
    flat = [w for a in wps for w in a]
    wp_off = np.concatenate([[0], np.cumsum([len(w) for w in flat])]).astype(np.int32)
    wp = np.concatenate(flat).astype(np.float64).reshape(-1, 3) if flat else np.zeros((0, 3))
    arrs = (np.asarray(vertex, np.float64).reshape(-1, 3), succ_off, succ, ln, wp_off, wp)
    return RoadGraph(*arrs) if checked else unchecked(arrs)


def unchecked(arrs):
    """A RoadGraph that skips the constructor's checks: what only EMP_DEVICE arrays can bring (NaN vertices)."""
    g = RoadGraph.__new__(RoadGraph)
    g.vertex, g.succ_off, g.succ, g.length, g.wp_off, g.wp = [np.ascontiguousarray(a) for a in arrs]
    g._device = {}
    return g


def _lattice(rng, N, box, fans=(), degrees=DEGREES, lengths=LENGTHS, wp_counts=(2, 2, 3, 4), wp_box=None, zs=(-1, 0, 1), empty=(),
             periodic=0.0):
    """N nodes on integer points of a box of +-box, random successor lists (``fans``: out-degrees forced on the first nodes a
    seeded permutation names; ``empty``: nodes without successors), waypoints on integer points: the entry at the node, the exit
    at the successor, the others anywhere in +-wp_box.  ``periodic``: the share of edges whose waypoints repeat every 64."""
    wp_box = box if wp_box is None else wp_box
    vertex = np.stack([rng.integers(-box, box + 1, N), rng.integers(-box, box + 1, N), rng.choice(zs, N)], 1).astype(np.float64)
    fan_nodes = [int(n) for n in rng.permutation([n for n in range(N) if n not in empty])[:len(fans)]]
    adj, length, wps = [], [], []
    for u in range(N):
        d = int(rng.choice(degrees))
        if u in fan_nodes:
            d = fans[fan_nodes.index(u)]
        if u in empty:
            d = 0
        d = min(d, N)
        a = [int(v) for v in rng.permutation(N)[:d]]
        adj.append(a)
        length.append([int(rng.choice(lengths)) for _ in a])
        ws = []
        for v in a:
            n = int(rng.choice(wp_counts))
            w = np.stack([rng.integers(-wp_box, wp_box + 1, n), rng.integers(-wp_box, wp_box + 1, n), np.zeros(n, np.int64)], 1).astype(np.float64)
            if n > 64 and rng.uniform() < periodic:
                w = w[np.arange(n) % 64]
            else:
                w[0], w[-1] = vertex[u], vertex[v]
            ws.append(w)
        wps.append(ws)
    return vertex, adj, length, wps, fan_nodes


def _reach(adj, s):
    seen, todo = {s}, [s]
    while todo:
        for v in adj[todo.pop()]:
            if v not in seen:
                seen.add(v)
                todo.append(v)
    return seen


def _queries(rng, adj, count, box, starts=(), unreachable=0.2):
    """``count`` queries: about ``unreachable`` of them without a route; ``starts``: start nodes the first queries take in turn.
    origin and dest lie on points and half-points of +-box."""
    edge_u = [u for u, a in enumerate(adj) for _ in a]
    N, E = len(adj), len(edge_u)
    reach = {}
    s_, e_ = [], []
    want_bad = int(round(count * unreachable))
    tries = 0
    while len(s_) < count:
        tries += 1
        s = int(starts[len(s_)]) if len(s_) < len(starts) else int(rng.integers(N))
        e = int(rng.integers(E))
        if s not in reach:
            reach[s] = _reach(adj, s)
        ok = edge_u[e] in reach[s]
        bad_so_far = sum(1 for a, b in zip(s_, e_) if edge_u[b] not in reach[a])
        if not ok and (bad_so_far >= want_bad or len(s_) < len(starts)) and tries < 100000:
            continue
        if ok and count - len(s_) <= want_bad - bad_so_far and tries < 100000:
            continue
        s_.append(s)
        e_.append(e)
    half = lambda: rng.integers(-2 * box, 2 * box + 1, (count, 3)) / 2.0
    ow, dw = half(), half()
    ow[:, 2], dw[:, 2] = 0.0, 0.0
    return np.array(s_, np.int32), np.array(e_, np.int32), np.ascontiguousarray(ow), np.ascontiguousarray(dw)


def _lattice_case(seed, N, box=6, count=48, per_fan=4, **kw):
    rng = np.random.default_rng(seed)
    vertex, adj, length, wps, fan_nodes = _lattice(rng, N, box, **kw)
    starts = [fan_nodes[i % len(fan_nodes)] for i in range(per_fan * len(fan_nodes))] if fan_nodes else ()
    return (vertex, adj, length, wps), _queries(rng, adj, max(count, len(starts) + 20), box, starts), fan_nodes


def _deep_wp():
    """Edges of 2 ... 200 waypoints on a +-3 lattice (z = 0), half of the long ones periodic in 64: the minimum of ``closest``
    is attained again a stride later, in the same lane.  A third of the destinations sit on a waypoint of the last edge itself:
    its first (the tie then makes k = 0), or the one 64 behind it."""
    rng = np.random.default_rng(905)
    N = 36
    vertex, adj, length, wps, _ = _lattice(rng, N, 3, degrees=(1, 2, 2, 3), wp_counts=DEEP_COUNTS, zs=(0,), periodic=0.5)
    s, e, ow, dw = _queries(rng, adj, 60, 3, unreachable=0.05)
    g = _assemble(vertex, adj, length, wps)
    for k in range(len(s)):
        a, b = int(g.wp_off[e[k]]), int(g.wp_off[e[k] + 1])
        if k % 3 == 0:
            dw[k] = g.wp[a + 1]
        elif k % 3 == 1 and b - a > 66:
            dw[k] = g.wp[a + 1 + 64]
    ok = [k for k in range(len(s)) if port.astar(g, int(s[k]), port.edge_ends(g, int(e[k]))[0]) is not None]
    ow[ok[-1]] = (np.nan, 1.0, 0.0)                    # no distance is a number: the reference's index stays -1
    dw[ok[-2]] = (0.5, np.inf, 0.0)
    ow[ok[-3]] = (-np.inf, 0.0, 0.0)
    return g, (s, e, ow, dw)


def _grid_4096():
    """64 x 64 nodes, an edge each way between neighbours.  The positions fold the grid into +-6 (so h says little and ties a
    lot): a search floods its neighbourhood and leaves hundreds of nodes open.  Queries end within 15 hops of their start."""
    rng = np.random.default_rng(4096)
    n = 64
    idx = lambda i, j: i * n + j
    vertex = np.array([((5 * i + 3 * j) % 13 - 6, (7 * i + 11 * j) % 13 - 6, 0) for i in range(n) for j in range(n)], np.float64)
    adj, length, wps = [], [], []
    for i in range(n):
        for j in range(n):
            a = [idx(i + di, j + dj) for di, dj in ((1, 0), (0, 1), (-1, 0), (0, -1)) if 0 <= i + di < n and 0 <= j + dj < n]
            adj.append(a)
            length.append([int(rng.choice(LENGTHS)) for _ in a])
            wps.append([np.array([vertex[idx(i, j)], vertex[v]]) for v in a])
    g = _assemble(vertex, adj, length, wps)
    s_, e_ = [], []
    while len(s_) < 40:
        i, j = int(rng.integers(n)), int(rng.integers(n))
        di = int(rng.integers(-15, 16))
        dj = int(rng.integers(-(15 - abs(di)), 15 - abs(di) + 1))
        if 0 <= i + di < n and 0 <= j + dj < n and abs(di) + abs(dj) >= 8:
            s_.append(idx(i, j))
            e_.append(int(g.succ_off[idx(i + di, j + dj)]) + int(rng.integers(2)))
    B = len(s_)
    ow, dw = rng.integers(-12, 13, (B, 3)) / 2.0, rng.integers(-12, 13, (B, 3)) / 2.0
    return g, (np.array(s_, np.int32), np.array(e_, np.int32), np.ascontiguousarray(ow), np.ascontiguousarray(dw))


def _empty_ends():
    """Nodes 0, 1 and N-2, N-1 list nothing, nor do 30, 31 and 50: edge ids next to empty lists are where edge_ends bisects."""
    N = 70
    (vertex, adj, length, wps), (s, e, ow, dw), _ = _lattice_case(707, N, degrees=(1, 2, 3), empty=(0, 1, 30, 31, 50, N - 2, N - 1), count=56)
    g = _assemble(vertex, adj, length, wps)
    E = g.n_edges
    ids = [0, E - 1, 1, E - 2] + [int(g.succ_off[m]) - 1 for m in (30, 50)] + [int(g.succ_off[m + 1]) for m in (31, 50)]
    for k, x in enumerate(ids * 2):
        e[k] = x
    for k, x in enumerate((0, 1, 30, N - 1, N - 2, 50)):          # starts without a successor
        s[len(s) - 1 - k] = x
    return g, (s, e, ow, dw)


def _nan_vertex(way):
    """lattice_65's shape with NaN in a few vertices.  ``way`` False: in the n_end of every second query (all of its h and so
    every f is NaN: +inf, the stamps decide); True: in six nodes with many successors that no query ends at."""
    (vertex, adj, length, wps), (s, e, ow, dw), _ = _lattice_case(6502 if way else 6501, 65, degrees=(1, 2, 3, 5), count=48)
    g = _assemble(vertex, adj, length, wps)
    vertex = g.vertex.copy()
    n_end = g.edge_u[e]
    if way:
        rich = [int(n) for n in np.argsort(-np.diff(g.succ_off), kind="stable") if n not in set(n_end.tolist())][:6]
        vertex[rich, 0] = np.nan
    else:
        vertex[np.unique(n_end[::2]), 1] = np.nan
    return unchecked((vertex,) + g.arrays()[1:]), (s, e, ow, dw)


@functools.lru_cache(maxsize=None)
def case(name):
    """(graph, (start_node, end_edge, origin_wp, dest_wp))"""
    if name.startswith("lattice_"):
        N = int(name[len("lattice_"):])
        parts, q, _ = _lattice_case(1000 + N, N)
    elif name == "fans_300":
        parts, q, _ = _lattice_case(300, 300, box=3, zs=(0,), fans=FANS)
    elif name == "wide_1000":
        parts, q, _ = _lattice_case(1000, 1000, fans=(64, 130, 64, 130), count=40)
    elif name in ("flat_h", "flat_h_zero"):
        parts, q, _ = _lattice_case(11, 240, degrees=(3, 5, 8, 12), fans=(65, 129, 200), per_fan=10,
                                    lengths=(0,) if name == "flat_h_zero" else LENGTHS)
        parts = (np.tile([2.0, -1.0, 1.0], (240, 1)),) + parts[1:]
    elif name == "huge":
        parts, q, _ = _lattice_case(1064, 64, box=2, degrees=(1, 2, 3, 5))
        parts = (parts[0] * 1e200,) + parts[1:]
    elif name == "long_len":
        parts, q, _ = _lattice_case(218, 100, degrees=(1, 2, 3, 5), lengths=(0, MAX_LEN - 1, MAX_LEN))
    elif name == "deep_wp":
        return _deep_wp()
    elif name == "grid_4096":
        return _grid_4096()
    elif name == "empty_ends":
        return _empty_ends()
    elif name in DEVICE_ONLY:
        return _nan_vertex(name == "nan_vertex_way")
    else:
        raise KeyError(name)
    return _assemble(*parts), q


def fan_nodes(name):
    """node -> out-degree of the forced fans of a case"""
    g, _ = case(name)
    deg = np.diff(g.succ_off)
    return {int(n): int(deg[n]) for n in np.nonzero(deg >= 64)[0]}


@functools.lru_cache(maxsize=None)
def chain_long():
    """``route_cases.chain(4096)`` with every length 2^18 (g reaches 4095 * 2^18), five queries and their analytic answers:
    (graph, queries, [(route, rows) or None])."""
    c = rc.chain(4096)
    g = RoadGraph(c.vertex, c.succ_off, c.succ, np.full(c.n_edges, MAX_LEN, np.int32), c.wp_off, c.wp)
    n = g.n_nodes
    s = np.array([0, 4000, n - 1, 17, 2048], np.int32)
    e = np.array([n - 2, 4090, 0, 17, 1000], np.int32)              # edge k leaves node k
    ow = np.ascontiguousarray(g.wp[2 * np.minimum(s, n - 2)])        # the entry of the first edge
    want = []
    for b in range(len(s)):
        if s[b] > e[b]:
            want.append(None)
            continue
        want.append((list(range(s[b], e[b] + 2)), [2 * s[b], 2 * s[b] + 1] + [2 * i + 1 for i in range(s[b] + 1, e[b])]))
    return g, (s, e, ow, ow.copy()), want


def stats(g, queries):
    """What the port meets on these queries: ``updates`` (an OPEN node took a smaller g), ``tie_pops`` (pops whose best f two
    or more open nodes held), ``max_open``, ``min_gap`` (the smallest non-zero gap between the best and the second-best f of any
    pop; inf: none), ``status`` {status: count}, ``popped_degree`` (the out-degrees of the expanded nodes), ``gap`` per query, and
    per query ``tied``: None without a route, else (origin's, dest's) lists of the positions at which ``closest`` attains its
    minimum - more than one entry is a tie, their differences say how far apart."""
    return _solve(g, queries)[1]


def _solve(g, queries):
    s, e, ow, dw = queries
    B = len(s)
    probe = dict(updates=0, tie_pops=0, max_open=0, pops=0, popped_degree=set())
    routes, tied, gap, status = [], [], np.full(B, np.inf), {}
    for b in range(B):
        gaps = []
        route, rows = port.search_path_way(g, int(s[b]), int(e[b]), ow[b], dw[b], gaps, probe)
        nz = [x for x in gaps if x > 0.0]
        gap[b] = min(nz) if nz else np.inf
        routes.append((route, rows))
        tied.append(None if route is None else (list(probe["origin_tied"]), list(probe["dest_tied"])))
        st = port.UNREACHABLE if route is None else 0
        status[st] = status.get(st, 0) + 1
    R = max([len(r) for r, _ in routes if r is not None] + [2])
    G = max([len(w) for r, w in routes if r is not None] + [1])
    o = dict(route=np.zeros((B, R), np.int32), route_len=np.zeros(B, np.int32), wp_index=np.zeros((B, G), np.int32), xy=np.zeros((B, G, 2)),
             n_global=np.zeros(B, np.int32), status=np.zeros(B, np.int32))
    for b, (route, rows) in enumerate(routes):
        if route is None:
            o["status"][b] = port.UNREACHABLE
            continue
        o["route_len"][b], o["n_global"][b] = len(route), len(rows)
        o["route"][b, :len(route)] = route
        o["wp_index"][b, :len(rows)] = rows
        o["xy"][b, :len(rows)] = g.wp[rows, :2]
    st = dict(updates=probe["updates"], tie_pops=probe["tie_pops"], max_open=probe["max_open"], pops=probe["pops"],
              popped_degree=probe["popped_degree"], min_gap=float(gap.min()) if B else math.inf, gap=gap, status=status, tied=tied)
    return o, st


@functools.lru_cache(maxsize=None)
def solved(name):
    """(the port's answer with capacities that hold everything - route, route_len, wp_index, xy, n_global, status -, stats)"""
    return _solve(*case(name))


def spans(tied, which):
    """per query with a route: the distance between the first and the last tied position of closest (0: no tie); which 0 origin, 1 dest"""
    return [t[which][-1] - t[which][0] if t is not None and t[which] else 0 for t in tied]


@functools.lru_cache(maxsize=None)
def recorded(name):
    return dict(np.load(os.path.join(HARD, name + ".npz")))


def stats_row(name):
    st = solved(name)[1]
    g, q = case(name)
    gap = "-" if not np.isfinite(st["min_gap"]) else f"{st['min_gap']:.1e}"
    far = sum(1 for w in (0, 1) for x in spans(st["tied"], w) if x >= 64)
    return (f"| {name} | {g.n_nodes} | {int(np.diff(g.succ_off).max())} | {int(np.diff(g.wp_off).min())}-{int(np.diff(g.wp_off).max())} | "
            f"{len(q[0])} | {st['status'].get(0, 0)} | {st['updates']} | {st['tie_pops']} of {st['pops']} | {st['max_open']} | {gap} | {far} |")


STATS_HEAD = ("| case | N | max out-degree | waypoints per edge | queries | with a route | OPEN-node updates | pops decided by a tie | "
              "largest open set | smallest non-zero f gap | closest ties 64 or more apart |\n|---|---|---|---|---|---|---|---|---|---|---|")
