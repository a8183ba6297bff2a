"""The reference's word on the hostile routing graphs of tests/route_hard_cases.py, recorded under tests/golden/routing_hard/.

    python tests/golden/make_golden_routing_hard.py        (EMP_GOLDEN_OUT=<dir>: write to <dir>/routing_hard/ instead)

The reference (``planner.global_planning``, loaded as make_golden_routing.py loads it, real networkx) is not given a map to build
a graph from: each case's arrays become a ``networkx.DiGraph`` directly - nodes in id order with ``vertex``, edges in CSR order with
``length``, ``entry_waypoint``, ``path``, ``exit_waypoint`` and ``type``, which is all ``_A_star`` and ``search_path_way`` read - and
the two map look-ups (``get_waypoint`` and the road / section / lane table behind ``_find_location_edge``) are a stub that hands
back the query's own numbers.  The searches, the closest-index scans and the slicing are the reference's own code.

Per case ``<name>.npz`` holds:
  vertex, succ_off, succ, length, wp_off, wp                     the case's arrays, as the reference was given them
  q_start_node, q_end_edge [Q], q_origin_wp, q_dest_wp [Q][3]    the queries
  reachable [Q], route_off [Q+1], route                          _route_search (with n_exit), nothing where NetworkXNoPath
  astar_off [Q+1], astar                                         _A_star alone
  path_off [Q+1], path_row, path_xy [.][2]                       search_path_way: rows of wp
  gap [Q]                                                        smallest non-zero (second-best f - best f) at any pop (inf: none)
Not asked: ``huge`` (math.hypot does not overflow where the stated sqrt of a sum of squares does, so that case pins the project's
own header), the NaN-vertex graphs (the library refuses them from the host; on device arrays the header's "a NaN f orders as
+inf" is the project's own rule) and the two 4096-node graphs (their size).  A gap below 1e-9 stops the run, as in
make_golden_routing.py.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden_routing as mk      # noqa: E402


class _Waypoint:
    def __init__(self, xyz, key=None):
        self.transform = mk.Transform(mk.Location(*xyz), mk.Rotation(0.0))
        self.road_id, self.section_id, self.lane_id = key, 0, 0
        self.is_intersection = False


class _Map:
    """get_waypoint hands back the waypoint the query location carries"""

    def get_waypoint(self, loc):
        return loc.waypoint


def planner_of(gp, g):
    """The reference's planner around the DiGraph of RoadGraph ``g``, and the waypoint object -> row of g.wp table."""
    import networkx as nx
    pl = gp.global_path_planner.__new__(gp.global_path_planner)
    pl._map, pl._sampling_resolution, pl._topology, pl._id_map, pl._road_to_edge = _Map(), 1.0, [], {}, {}
    graph, row_of = nx.DiGraph(), {}
    for n in range(g.n_nodes):
        graph.add_node(n, vertex=tuple(float(c) for c in g.vertex[n]))
    for u in range(g.n_nodes):
        for e in range(int(g.succ_off[u]), int(g.succ_off[u + 1])):
            a, b = int(g.wp_off[e]), int(g.wp_off[e + 1])
            wps = [_Waypoint(g.wp[j]) for j in range(a, b)]
            for j, w in zip(range(a, b), wps):
                row_of[id(w)] = j
            graph.add_edge(u, int(g.succ[e]), length=int(g.length[e]), path=wps[1:-1], entry_waypoint=wps[0], exit_waypoint=wps[-1],
                           type=gp.RoadOption.LANE_FOLLOW)
            pl._road_to_edge[("edge", e)] = {0: {0: (u, int(g.succ[e]))}}
        pl._road_to_edge[("node", u)] = {0: {0: (u, -1)}}         # _route_search reads the start edge's first node only
    pl._graph = graph
    pl._keep = graph                                               # (the waypoint objects live as long as the graph)
    return pl, row_of


def _location(xyz, key):
    loc = mk.Location(*xyz)
    loc.waypoint = _Waypoint(xyz, key)
    return loc


def record(name, gp):
    import networkx as nx
    from tests import route_hard_cases as hc
    from tests import route_port
    g, (s, e, ow, dw) = hc.case(name)
    pl, row_of = planner_of(gp, g)
    Q = len(s)
    o = dict(zip(("vertex", "succ_off", "succ", "length", "wp_off", "wp"), g.arrays()))
    o.update(q_start_node=s, q_end_edge=e, q_origin_wp=ow, q_dest_wp=dw)
    o["reachable"], o["gap"] = np.zeros(Q, np.int32), np.full(Q, np.inf)
    route_off, route, astar_off, astar, path_off, path_row, path_xy = [0], [], [0], [], [0], [], []
    for k in range(Q):
        origin, destination = _location(ow[k], ("node", int(s[k]))), _location(dw[k], ("edge", int(e[k])))
        n_end = int(g.edge_u[e[k]])
        assert pl._find_location_edge(origin)[0] == s[k] and pl._find_location_edge(destination) == (n_end, int(g.succ[e[k]]))
        astar += pl._A_star(int(s[k]), n_end) or []
        astar_off.append(len(astar))
        gaps = []
        route_port.astar(g, int(s[k]), n_end, gaps)
        nz = [x for x in gaps if x > 0.0]
        o["gap"][k] = min(nz) if nz else np.inf
        try:
            r = pl._route_search(origin, destination)
            pw = pl.search_path_way(origin, destination)
            o["reachable"][k] = 1
        except nx.NetworkXNoPath:
            r, pw = [], []
        route += r
        route_off.append(len(route))
        for w, option in pw:
            assert option == gp.RoadOption.LANE_FOLLOW
            path_row.append(row_of[id(w)])
            path_xy.append((w.transform.location.x, w.transform.location.y))
        path_off.append(len(path_row))
    o["route_off"], o["route"] = np.array(route_off, np.int32), np.array(route, np.int32)
    o["astar_off"], o["astar"] = np.array(astar_off, np.int32), np.array(astar, np.int32)
    o["path_off"], o["path_row"] = np.array(path_off, np.int32), np.array(path_row, np.int32)
    o["path_xy"] = np.array(path_xy, np.float64).reshape(-1, 2)
    return o


def main():
    from tests import route_hard_cases as hc
    gp, _ = mk.load_global_planning()
    out = os.path.join(os.environ.get("EMP_GOLDEN_OUT", HERE), "routing_hard")
    os.makedirs(out, exist_ok=True)
    for name in hc.RECORDED:
        o = record(name, gp)
        low = o["gap"].min() if len(o["gap"]) else np.inf
        if low < mk.GAP_FLOOR:
            raise SystemExit(f"{name}: a pop decided by {low:.3e} (< {mk.GAP_FLOOR}): change this case's seed")
        np.savez_compressed(os.path.join(out, name + ".npz"), **o)
        print(f"{name}: {len(o['vertex'])} nodes, {len(o['succ'])} edges, {len(o['q_start_node'])} queries, "
              f"{int((o['reachable'] == 0).sum())} unreachable, {len(o['path_row'])} path rows, smallest gap {low:.3e}")


if __name__ == "__main__":
    sys.exit(main())
