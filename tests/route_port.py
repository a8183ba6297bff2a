"""The routing procedure of include/emplanner.h (emp_route_graph's block) in plain Python on a ``RoadGraph``'s arrays: ``astar``,
``expand``, ``search_path_way`` and ``run``, the batched form with the C-ABI's statuses, capacities and zero padding.  The tests
compare it with the reference's recorded routes (tests/golden/routing/) on one side and with the g++ build of csrc/emp_route_core.h
and the GPU on the other.  Python floats are binary64 and ``math.sqrt`` is IEEE, so every f and every distance here carries the
bits the library computes."""
from __future__ import annotations

import math

import numpy as np

UNREACHABLE, TRUNCATED, BAD_QUERY = 1, 2, 4


def dist3(p, q):
    dx, dy, dz = float(p[0]) - float(q[0]), float(p[1]) - float(q[1]), float(p[2]) - float(q[2])
    return math.sqrt(((dx * dx) + (dy * dy)) + (dz * dz))


def edge_ends(g, e):
    """(n_end, n_exit) of edge id e, None for an id outside [0, E)."""
    if not 0 <= e < len(g.succ):
        return None
    return int(np.searchsorted(g.succ_off, e, side="right")) - 1, int(g.succ[e])


def astar(g, start, n_end, gaps=None, probe=None):
    """The route from start to n_end as a list of node ids, None when the open set runs empty.  ``gaps``: a list that receives,
    per pop with at least two open nodes, the difference between the second-best and the best f (0.0 for equal ones).  ``probe``:
    a dict whose counters this search adds to - ``updates`` (an OPEN node took a smaller g), ``tie_pops`` (the best f was held by
    two or more open nodes), ``max_open``, ``pops``, and ``popped_degree``, the set of out-degrees of the nodes it expanded.
    The open nodes are kept as a list in the order of their first insertion - the order of their stamps - so the first strict
    minimum of f over it is the header's "smallest f, then smallest stamp"."""
    N = len(g.vertex)
    h = [None] * N
    state = [0] * N                     # 0 NEW, 1 OPEN, 2 CLOSED
    gc, parent = [0] * N, [-1] * N
    state[start], opened = 1, [start]
    for _ in range(N):
        if not opened:
            return None
        best, at, fs = None, 0, []
        for i, n in enumerate(opened):
            if h[n] is None:
                h[n] = dist3(g.vertex[n], g.vertex[n_end])
            f = float(gc[n]) + h[n]
            if f != f:                  # a NaN f orders as +inf
                f = math.inf
            fs.append(f)
            if best is None or f < best:
                best, at = f, i
        if len(fs) > 1 and (gaps is not None or probe is not None):
            fs.sort()
            if gaps is not None:
                gaps.append(0.0 if fs[1] == fs[0] else fs[1] - fs[0])
            if probe is not None and fs[1] == fs[0]:
                probe["tie_pops"] = probe.get("tie_pops", 0) + 1
        if probe is not None:
            probe["max_open"] = max(probe.get("max_open", 0), len(opened))
            probe["pops"] = probe.get("pops", 0) + 1
        c = opened.pop(at)
        if c == n_end:
            state[c] = 2
            break
        if probe is not None:
            probe.setdefault("popped_degree", set()).add(int(g.succ_off[c + 1]) - int(g.succ_off[c]))
        for e in range(g.succ_off[c], g.succ_off[c + 1]):
            suc, ng = int(g.succ[e]), gc[c] + int(g.length[e])
            if state[suc] == 2:
                continue
            if state[suc] == 1:
                if ng < gc[suc]:
                    gc[suc], parent[suc] = ng, c
                    if probe is not None:
                        probe["updates"] = probe.get("updates", 0) + 1
            else:
                state[suc], gc[suc], parent[suc] = 1, ng, c
                opened.append(suc)
        state[c] = 2
    else:
        return None
    route = [n_end]
    while parent[route[-1]] != -1:
        route.append(parent[route[-1]])
    return route[::-1]


def find_edge(g, u, v):
    for e in range(g.succ_off[u], g.succ_off[u + 1]):
        if g.succ[e] == v:
            return e
    raise KeyError((u, v))


def closest(g, p, a, b, tied=None):
    """The first index of wp[a:b] with the strictly smallest distance to p, relative to a; -1 when no distance is below inf (the
    reference's initial index).  ``tied``: a list that receives every relative index at which that smallest distance is attained."""
    best, k = math.inf, -1
    for j in range(a, b):
        d = dist3(g.wp[j], p)
        if d < best:
            best, k = d, j - a
            if tied is not None:
                del tied[:]
        if tied is not None and d == best and k >= 0:
            tied.append(j - a)
    return k


def expand(g, route, origin_wp, dest_wp, probe=None):
    """search_path_way's waypoints as rows of g.wp.  An index of -1 is read as Python reads it: path[-1:] is the first edge's exit
    alone, path[:0] nothing.  ``probe``: a dict that receives ``origin_tied`` and ``dest_tied`` (closest's tied indices)."""
    out = []
    ot, dt = ([], []) if probe is not None else (None, None)
    e = find_edge(g, route[0], route[1])
    a, b = int(g.wp_off[e]), int(g.wp_off[e + 1])
    k = closest(g, origin_wp, a, b, ot)
    out += range(a + k if k >= 0 else b - 1, b)
    if len(route) > 3:
        for i in range(1, len(route) - 2):
            e = find_edge(g, route[i], route[i + 1])
            out += range(int(g.wp_off[e]) + 1, int(g.wp_off[e + 1]))
    e = find_edge(g, route[-2], route[-1])
    a, b = int(g.wp_off[e]) + 1, int(g.wp_off[e + 1])
    k = closest(g, dest_wp, a, b, dt)
    if k > 0:
        out += range(a, a + k + 1)
    if probe is not None:
        probe["origin_tied"], probe["dest_tied"] = ot, dt
    return out


def search_path_way(g, start_node, end_edge, origin_wp, dest_wp, gaps=None, probe=None):
    """(route, rows of g.wp), or (None, None) for an unreachable end.  The route ends with n_exit."""
    n_end, n_exit = edge_ends(g, end_edge)
    route = astar(g, start_node, n_end, gaps, probe)
    if route is None:
        return None, None
    route = route + [n_exit]
    return route, expand(g, route, origin_wp, dest_wp, probe)


def run(g, start_node, end_edge, origin_wp, dest_wp, max_route, max_global):
    """emp_route_paths on the CPU, without theta and kappa: dict of route, route_len, wp_index, xy, n_global, status."""
    B = len(start_node)
    o = dict(route=np.zeros((B, max_route), np.int32), route_len=np.zeros(B, np.int32), wp_index=np.zeros((B, max_global), np.int32),
             xy=np.zeros((B, max_global, 2)), n_global=np.zeros(B, np.int32), status=np.zeros(B, np.int32))
    for b in range(B):
        ends = edge_ends(g, int(end_edge[b]))
        if ends is None or not 0 <= start_node[b] < len(g.vertex):
            o["status"][b] = BAD_QUERY
            continue
        route, rows = search_path_way(g, int(start_node[b]), int(end_edge[b]), origin_wp[b], dest_wp[b])
        if route is None:
            o["status"][b] = UNREACHABLE
            continue
        o["route_len"][b], o["n_global"][b] = len(route), len(rows)
        if len(route) > max_route or len(rows) > max_global:
            o["status"][b] = TRUNCATED
        route, rows = route[:max_route], rows[:max_global]
        o["route"][b, :len(route)] = route
        o["wp_index"][b, :len(rows)] = rows
        o["xy"][b, :len(rows)] = g.wp[rows, :2]
    return o
