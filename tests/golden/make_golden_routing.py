"""Routing fixtures: fake towns from seeds, run through the reference's ``planner.global_planning`` (real networkx, a fake
``carla.Map``), recorded as arrays under tests/golden/routing/.

    python tests/golden/make_golden_routing.py        (EMP_GOLDEN_OUT=<dir>: write to <dir>/routing/ instead)

The town half of this file needs nothing but NumPy: tests rebuild a town from its seed (``town(name)``) to get the very map the
fixture was recorded on.  The recording half imports the reference (``ref_loader._install_stubs()`` supplies ``carla`` and
``cvxopt``; ``planner.global_planning`` is imported here because ``ref_loader.load_driver_reference`` stubs it out).

A town is a list of directed segments, each a polyline from its entry to its exit.  ``Waypoint.next(d)`` walks the polyline by
arc length (and on along its last leg beyond the exit), ``Location.distance`` is sqrt(((dx dx) + (dy dy)) + (dz dz)), and a query
location carries the segment it was sampled on, which is what ``Map.get_waypoint`` resolves it to (two lanes of one road share
their end points here, so geometry alone would not tell them apart).

Per town ``<name>.npz`` holds, all from the reference's objects:
  seg_entry, seg_exit [S][3], seg_path_off [S+1], seg_path [P][3]   _build_topology's segments (what RoadGraph.from_segments takes)
  vertex, succ_off, succ, length, wp_off, wp                        the DiGraph in networkx order (nodes by id, successors as
                                                                    DiGraph.successors yields them, waypoints from the edge data)
  seg_uv [S][2]                                                     the (n1, n2) of every segment
  q_seg [Q][2], q_s [Q][2]                                          origin and destination: segment and arc length
  q_start_node, q_end_edge [Q], q_origin_wp, q_dest_wp [Q][3]       the query as emp_route_paths takes it
  reachable [Q], route_off [Q+1], route                             _route_search (with n_exit), nothing where NetworkXNoPath
  astar_off [Q+1], astar                                            _A_star alone
  path_off [Q+1], path_edge, path_idx, path_xy [.][2]               search_path_way: edge id and index in that edge's waypoints
  theta, kappa                                                      waypoint_list_2_target_path on it (NaN rows where it raises)
  gap [Q]                                                           smallest non-zero (second-best f - best f) at any pop (inf: none)
No query is excluded.  If a seed ever gives a query with a gap below 1e-9 - where math.hypot and the 3-term sqrt might order two
nodes differently - main() stops: change that town's seed, and say here which and why.  (None so far.)
"""
from __future__ import annotations

import importlib
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GAP_FLOOR = 1e-9


# ---- the fake CARLA map ---------------------------------------------------------------------------------------------------------
class Location:
    def __init__(self, x, y, z, seg=None, s=None):
        self.x, self.y, self.z = float(x), float(y), float(z)
        self.seg, self.s = seg, s            # a query location: the lane it lies on

    def distance(self, other):
        dx, dy, dz = self.x - other.x, self.y - other.y, self.z - other.z
        return math.sqrt(((dx * dx) + (dy * dy)) + (dz * dz))


class Vector:
    def __init__(self, x, y, z):
        self.x, self.y, self.z = x, y, z


class Rotation:
    def __init__(self, yaw):
        self.yaw = yaw

    def get_forward_vector(self):
        return Vector(math.cos(self.yaw), math.sin(self.yaw), 0.0)


class Transform:
    def __init__(self, location, rotation):
        self.location, self.rotation = location, rotation


class Waypoint:
    def __init__(self, town, seg, s):
        self._town, self.seg, self.s = town, seg, s
        p, yaw = town.point(seg, s)
        self.transform = Transform(Location(*p), Rotation(yaw))
        self.road_id, self.section_id, self.lane_id = town.lane_ids[seg]
        self.is_intersection = False

    def next(self, d):
        return [Waypoint(self._town, self.seg, self.s + d)]


class Map:
    """segments: a list of polylines [[x, y, z], ...]; lane_ids: (road_id, section_id, lane_id) per segment."""

    def __init__(self, segments, lane_ids=None):
        self.segments = [np.asarray(p, np.float64) for p in segments]
        self.lane_ids = lane_ids or [(i, 0, 1) for i in range(len(segments))]
        self.cum = [np.concatenate([[0.0], np.cumsum(np.sqrt((np.diff(p, axis=0) ** 2).sum(1)))]) for p in self.segments]

    def point(self, seg, s):
        p, cum = self.segments[seg], self.cum[seg]
        if cum[-1] == 0.0:                                  # a segment that ends where it starts and has no way points
            return tuple(p[0]), 0.0
        i = min(max(int(np.searchsorted(cum, s, side="right")) - 1, 0), len(p) - 2)
        while cum[i + 1] == cum[i] and i > 0:
            i -= 1
        t = (s - cum[i]) / (cum[i + 1] - cum[i])            # beyond the exit: on along the last leg
        q = p[i] + t * (p[i + 1] - p[i])
        return (float(q[0]), float(q[1]), float(q[2])), math.atan2(p[i + 1][1] - p[i][1], p[i + 1][0] - p[i][0])

    def length(self, seg):
        return float(self.cum[seg][-1])

    def get_topology(self):
        return [(Waypoint(self, i, 0.0), Waypoint(self, i, self.length(i))) for i in range(len(self.segments))]

    def get_waypoint(self, loc):
        return Waypoint(self, loc.seg, loc.s)

    def location(self, seg, s):
        p, _ = self.point(seg, s)
        return Location(*p, seg=seg, s=s)


def grid_town(n, spacing, seed=None, jitter=0.0, bend=0.0, z_amp=0.0, removed=0.0):
    """n x n intersections, a directed segment each way between neighbours.  Intersections sit on whole centimetres and every
    segment end is moved off them by up to 3 mm, so that only the reference's 2-decimal rounding joins them into nodes."""
    rng = np.random.default_rng(seed)
    pts = np.zeros((n, n, 3))
    for i in range(n):
        for j in range(n):
            pts[i, j] = (i * spacing, j * spacing, 0.0)
    if seed is not None:
        pts[..., :2] += rng.uniform(-jitter, jitter, (n, n, 2))
        pts[..., 2] = rng.uniform(-z_amp, z_amp, (n, n))
        pts = np.round(pts, 2)
    segments = []
    for i in range(n):
        for j in range(n):
            for di, dj in ((1, 0), (0, 1)):
                if i + di >= n or j + dj >= n:
                    continue
                for a, b in ((pts[i, j], pts[i + di, j + dj]), (pts[i + di, j + dj], pts[i, j])):
                    if seed is not None and rng.uniform() < removed:
                        continue
                    off = rng.uniform(-0.003, 0.003, (2, 3)) if seed is not None else np.zeros((2, 3))
                    poly = [a + off[0]]
                    if seed is not None and bend > 0.0 and rng.uniform() < 0.5:        # a bent edge: one knee to the side
                        d = b - a
                        side = np.array([-d[1], d[0], 0.0]) / max(math.hypot(d[0], d[1]), 1e-9)
                        poly.append(a + rng.uniform(0.3, 0.7) * d + rng.uniform(-bend, bend) * side)
                    poly.append(b + off[1])
                    segments.append(poly)
    return Map(segments)


def micro_towns():
    """Hand-built graphs, name -> (Map, resolution, [(origin seg, s, destination seg, s), ...])."""
    A, B, Cc = (0.0, 0.0, 0.0), (10.0, 0.0, 0.0), (10.0, 10.0, 0.5)
    out = {}
    out["two_nodes"] = (Map([[A, B]]), 2.0, [(0, 3.0, 0, 7.0), (0, 7.0, 0, 3.0), (0, 0.0, 0, 10.0), (0, 9.5, 0, 0.2)])
    # A -> A (no way points: its ends coincide), A -> B, B -> A
    out["self_loop"] = (Map([[A, (3.0, 4.0, 0.0), (-3.0, 4.0, 0.0), A], [A, B], [B, A]]), 2.0,
                        [(0, 1.0, 1, 5.0), (1, 5.0, 0, 2.0), (2, 5.0, 0, 0.0), (0, 0.0, 0, 0.0), (2, 1.0, 1, 9.0)])
    # two segments A -> B: the later one's attributes win, the successor keeps its first position (before C)
    out["duplicate"] = (Map([[A, B], [A, Cc], [A, (5.0, 3.0, 0.0), B], [B, Cc], [Cc, A]]), 1.0,
                        [(0, 2.0, 3, 5.0), (2, 6.0, 3, 5.0), (4, 3.0, 0, 8.0), (4, 3.0, 2, 4.0), (1, 3.0, 2, 4.0), (3, 1.0, 1, 9.0)])
    # a ring A -> B -> C -> A and B -> A: the destination's edge leads back to the start node
    out["back_over_start"] = (Map([[A, B], [B, Cc], [Cc, A], [B, A]]), 2.0,
                              [(3, 4.0, 0, 6.0), (1, 4.0, 0, 6.0), (0, 6.0, 0, 2.0), (1, 2.0, 1, 1.0), (0, 1.0, 2, 13.0), (3, 9.0, 3, 1.0)])
    # a hub with 70 successors on a ring round the target T, the hub straight above T: leaves 5 and 65 are mirror images and tie
    hub, T, src = (0.0, 0.0, 50.0), (0.0, 0.0, 0.0), (0.0, 0.0, 60.0)
    segs = [[src, hub]]
    for i in range(70):
        r, th = 20.0 + 0.5 * min(abs(i - 5), abs(i - 65)), 2.0 * math.pi * i / 70
        leaf = (round(r * math.cos(th), 2), round(r * math.sin(th), 2), 0.0)
        segs += [[hub, leaf], [leaf, T]]
    segs.append([T, src])
    q = [(0, 2.0, len(segs) - 1, 30.0), (0, 2.0, 2 * 65 + 2, 3.0), (0, 9.0, 2 * 5 + 2, 11.0), (2 * 40 + 1, 5.0, len(segs) - 1, 1.0)]
    out["degree_70"] = (Map(segs), 2.0, q)
    for n in (63, 64, 65):       # a ring of n nodes, both ways, and a chord
        P = [(round(40.0 * math.cos(2 * math.pi * k / n), 2), round(40.0 * math.sin(2 * math.pi * k / n), 2), 0.1 * (k % 3)) for k in range(n)]
        segs = []
        for k in range(n):
            segs += [[P[k], P[(k + 1) % n]], [P[(k + 1) % n], P[k]]]
        segs.append([P[0], P[n // 2]])
        out[f"ring_{n}"] = (Map(segs), 1.0, [(0, 1.0, 2 * (n - 2), 2.0), (2 * 7 + 1, 1.0, 2 * (n // 2 + 5), 1.5), (2 * (n - 1), 0.5, 2 * 30, 3.0),
                                             (2 * 20, 2.0, 2 * 20, 1.0), (2 * (n - 1) + 1, 1.0, 1, 2.0)])
    return out


def _all_pairs(m, first_out):
    """every (start node, end node) pair as (origin seg, s, destination seg, s): each node by the first segment that leaves it"""
    return [(first_out[u], 1.5, first_out[v], 2.5) for u in sorted(first_out) for v in sorted(first_out)]


def _seeded_pairs(m, seed, count):
    rng = np.random.default_rng(seed)
    S = len(m.segments)
    q = []
    for _ in range(count):
        a, b = int(rng.integers(S)), int(rng.integers(S))
        q.append((a, float(rng.uniform(0.0, m.length(a))), b, float(rng.uniform(0.0, m.length(b)))))
    return q


TOWNS = {"grid6": dict(n=6, spacing=5.0, res=1.0),
         "jitter8": dict(n=8, spacing=12.0, res=2.0, seed=811, jitter=2.0, bend=2.5, z_amp=1.5, queries=300),
         "sparse12": dict(n=12, spacing=12.0, res=2.0, seed=1213, jitter=2.0, bend=2.5, z_amp=1.5, removed=0.15, queries=300)}


def town(name):
    """(Map, sampling resolution, queries) of a fixture: the grid towns above, or ``micro_<name>``."""
    if name.startswith("micro_"):
        return micro_towns()[name[len("micro_"):]]
    t = TOWNS[name]
    m = grid_town(t["n"], t["spacing"], t.get("seed"), t.get("jitter", 0.0), t.get("bend", 0.0), t.get("z_amp", 0.0), t.get("removed", 0.0))
    if "queries" in t:
        return m, t["res"], _seeded_pairs(m, t["seed"] + 1, t["queries"])
    first_out = {}
    for s, p in enumerate(m.segments):         # (the regular grid: exact positions, so the key is the node)
        first_out.setdefault(tuple(np.round(p[0], 2)), s)
    return m, t["res"], _all_pairs(m, first_out)


def names():
    return list(TOWNS) + ["micro_" + k for k in micro_towns()]


# ---- recording ----------------------------------------------------------------------------------------------------------------------
def load_global_planning():
    sys.path.insert(0, HERE)
    import ref_loader
    if not ref_loader.reference_available():
        raise RuntimeError("reference tree not present")
    sys.dont_write_bytecode = True
    ref_loader._install_stubs()
    sys.path.insert(0, ref_loader.REFERENCE_ROOT)
    try:
        for name in ("planner", "planner.planning_utils", "planner.global_planning"):
            sys.modules.pop(name, None)
        gp = importlib.import_module("planner.global_planning")
        pu = importlib.import_module("planner.planning_utils")
    finally:
        sys.path.remove(ref_loader.REFERENCE_ROOT)
        for name in ("planner", "planner.planning_utils", "planner.global_planning"):
            sys.modules.pop(name, None)
    return gp, pu


def _xyz(w):
    loc = w.transform.location
    return (loc.x, loc.y, loc.z)


def record(name, gp, pu):
    import networkx as nx
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import route_port
    m, res, queries = town(name)
    planner = gp.global_path_planner(m, res)
    topology, graph, id_map, _ = planner.get_topology_and_graph_info()
    o = {}
    o["seg_entry"] = np.array([_xyz(t["entry"]) for t in topology], np.float64).reshape(-1, 3)
    o["seg_exit"] = np.array([_xyz(t["exit"]) for t in topology], np.float64).reshape(-1, 3)
    o["seg_path_off"] = np.concatenate([[0], np.cumsum([len(t["path"]) for t in topology])]).astype(np.int32)
    o["seg_path"] = np.array([_xyz(w) for t in topology for w in t["path"]], np.float64).reshape(-1, 3)
    N = graph.number_of_nodes()
    assert sorted(graph.nodes) == list(range(N))
    o["vertex"] = np.array([graph.nodes[n]["vertex"] for n in range(N)], np.float64).reshape(-1, 3)
    succ_off, succ, length, wp_off, wp, edge_id, edge_wps = [0], [], [], [0], [], {}, []
    for u in range(N):
        for v in graph.successors(u):
            d = graph.get_edge_data(u, v)
            edge_id[(u, v)] = len(succ)
            succ.append(v)
            length.append(d["length"])
            wps = [d["entry_waypoint"]] + d["path"] + [d["exit_waypoint"]]
            edge_wps.append(wps)
            wp += [_xyz(w) for w in wps]
            wp_off.append(len(wp))
        succ_off.append(len(succ))
    o["succ_off"], o["succ"], o["length"] = np.array(succ_off, np.int32), np.array(succ, np.int32), np.array(length, np.int32)
    o["wp_off"], o["wp"] = np.array(wp_off, np.int32), np.array(wp, np.float64).reshape(-1, 3)
    rnd = lambda w: tuple(np.round(c, 2) for c in _xyz(w))
    o["seg_uv"] = np.array([(id_map[rnd(t["entry"])], id_map[rnd(t["exit"])]) for t in topology], np.int32).reshape(-1, 2)
    where = {}                                  # waypoint object -> (edge, index): the first edge that holds it
    for e, wps in enumerate(edge_wps):
        for i, w in enumerate(wps):
            where.setdefault(id(w), (e, i))

    class G:                                    # the recorded arrays, for the port's gap probe
        vertex, succ_off, succ, length = o["vertex"], o["succ_off"], o["succ"], o["length"]

    Q = len(queries)
    o["q_seg"] = np.array([(q[0], q[2]) for q in queries], np.int32)
    o["q_s"] = np.array([(q[1], q[3]) for q in queries], np.float64)
    o["q_start_node"], o["q_end_edge"] = np.zeros(Q, np.int32), np.zeros(Q, np.int32)
    o["q_origin_wp"], o["q_dest_wp"] = np.zeros((Q, 3)), np.zeros((Q, 3))
    o["reachable"], o["gap"] = np.zeros(Q, np.int32), np.full(Q, np.inf)
    route_off, route, astar_off, astar, path_off, path_edge, path_idx, path_xy, theta, kappa = [0], [], [0], [], [0], [], [], [], [], []
    for k, (sa, s_a, sb, s_b) in enumerate(queries):
        origin, destination = m.location(sa, s_a), m.location(sb, s_b)
        start_edge, end_edge = planner._find_location_edge(origin), planner._find_location_edge(destination)
        o["q_start_node"][k], o["q_end_edge"][k] = start_edge[0], edge_id[end_edge]
        o["q_origin_wp"][k], o["q_dest_wp"][k] = _xyz(m.get_waypoint(origin)), _xyz(m.get_waypoint(destination))
        a = planner._A_star(start_edge[0], end_edge[0])
        astar += a or []
        astar_off.append(len(astar))
        gaps = []
        route_port.astar(G, start_edge[0], end_edge[0], gaps)
        nz = [x for x in gaps if x > 0.0]
        o["gap"][k] = min(nz) if nz else np.inf
        try:
            r = planner._route_search(origin, destination)
            pw = planner.search_path_way(origin, destination)
            o["reachable"][k] = 1
        except nx.NetworkXNoPath:
            r, pw = [], []
        route += r
        route_off.append(len(route))
        for w, option in pw:
            assert option == gp.RoadOption.LANE_FOLLOW
            e, i = where[id(w)]
            path_edge.append(e)
            path_idx.append(i)
            path_xy.append((w.transform.location.x, w.transform.location.y))
        path_off.append(len(path_edge))
        if pw:
            try:
                with np.errstate(all="ignore"):
                    tp = pu.waypoint_list_2_target_path(pw)
                th, ka = [p[2] for p in tp], [p[3] for p in tp]
                assert len(th) == len(pw)
            except (ZeroDivisionError, IndexError):
                th = ka = [np.nan] * len(pw)
            theta += th
            kappa += ka
    o["route_off"], o["route"] = np.array(route_off, np.int32), np.array(route, np.int32)
    o["astar_off"], o["astar"] = np.array(astar_off, np.int32), np.array(astar, np.int32)
    o["path_off"], o["path_edge"], o["path_idx"] = np.array(path_off, np.int32), np.array(path_edge, np.int32), np.array(path_idx, np.int32)
    o["path_xy"] = np.array(path_xy, np.float64).reshape(-1, 2)
    o["theta"], o["kappa"] = np.array(theta, np.float64), np.array(kappa, np.float64)
    return o


def signatures():
    """The reference module's surface, read with ``ast`` as make_signatures.py reads the others (names and default literals only)."""
    sys.path.insert(0, HERE)
    import make_signatures
    import ref_loader
    rel = "planner/global_planning.py"
    text = open(os.path.join(ref_loader.REFERENCE_ROOT, rel), encoding="utf-8").read()
    return {rel: dict(dropin="emplanner_carla_amd.planner.global_planning", scope="full", **make_signatures.surface_of_source(text))}


def main():
    import json
    gp, pu = load_global_planning()
    out = os.path.join(os.environ.get("EMP_GOLDEN_OUT", HERE), "routing")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "signatures_global_planning.json"), "w") as f:
        json.dump(signatures(), f, indent=1, sort_keys=True)
        f.write("\n")
    for name in names():
        o = record(name, gp, pu)
        low = o["gap"].min() if len(o["gap"]) else np.inf
        if low < GAP_FLOOR:
            raise SystemExit(f"{name}: a pop decided by {low:.3e} (< {GAP_FLOOR}): change this town's seed and note it in the docstring")
        np.savez_compressed(os.path.join(out, name + ".npz"), **o)
        print(f"{name}: {len(o['vertex'])} nodes, {len(o['succ'])} edges, {len(o['q_start_node'])} queries, "
              f"{int((o['reachable'] == 0).sum())} unreachable, {len(o['path_edge'])} path rows, smallest gap {low:.3e}")


if __name__ == "__main__":
    sys.exit(main())
