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


def astar(g, start, n_end, gaps=None):
    """The route from start to n_end as a list of node ids, None when the open set runs empty.  ``gaps``: a list that receives,
    per pop with at least two open nodes, the difference between the second-best and the best f."""
    N = len(g.vertex)
    h = [dist3(g.vertex[n], g.vertex[n_end]) for n in range(N)]
    state = [0] * N                     # 0 NEW, 1 OPEN, 2 CLOSED
    gc, parent, stamp = [0] * N, [-1] * N, [0] * N
    state[start], next_stamp = 1, 1
    for _ in range(N):
        best = None
        fs = []
        for n in range(N):
            if state[n] != 1:
                continue
            f = float(gc[n]) + h[n]
            fs.append(f)
            if best is None or f < best[0] or (f == best[0] and stamp[n] < best[1]):
                best = (f, stamp[n], n)
        if best is None:
            return None
        if gaps is not None and len(fs) > 1:
            fs.sort()
            gaps.append(fs[1] - fs[0])
        c = best[2]
        if c == n_end:
            state[c] = 2
            break
        for e in range(g.succ_off[c], g.succ_off[c + 1]):
            suc, ng = int(g.succ[e]), gc[c] + int(g.length[e])
            if state[suc] == 2:
                continue
            if state[suc] == 1:
                if ng < gc[suc]:
                    gc[suc], parent[suc] = ng, c
            else:
                state[suc], gc[suc], parent[suc], stamp[suc] = 1, ng, c, next_stamp
                next_stamp += 1
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


def closest(g, p, a, b):
    """The first index of wp[a:b] with the strictly smallest distance to p, relative to a; 0 when no distance is below inf."""
    best, k = math.inf, 0
    for j in range(a, b):
        d = dist3(g.wp[j], p)
        if d < best:
            best, k = d, j - a
    return k


def expand(g, route, origin_wp, dest_wp):
    """search_path_way's waypoints as rows of g.wp."""
    out = []
    e = find_edge(g, route[0], route[1])
    a, b = int(g.wp_off[e]), int(g.wp_off[e + 1])
    out += range(a + closest(g, origin_wp, a, b), b)
    if len(route) > 3:
        for i in range(1, len(route) - 2):
            e = find_edge(g, route[i], route[i + 1])
            out += range(int(g.wp_off[e]) + 1, int(g.wp_off[e + 1]))
    e = find_edge(g, route[-2], route[-1])
    a, b = int(g.wp_off[e]) + 1, int(g.wp_off[e + 1])
    k = closest(g, dest_wp, a, b)
    if k != 0:
        out += range(a, a + k + 1)
    return out


def search_path_way(g, start_node, end_edge, origin_wp, dest_wp):
    """(route, rows of g.wp), or (None, None) for an unreachable end.  The route ends with n_exit."""
    n_end, n_exit = edge_ends(g, end_edge)
    route = astar(g, start_node, n_end)
    if route is None:
        return None, None
    route = route + [n_exit]
    return route, expand(g, route, origin_wp, dest_wp)


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
