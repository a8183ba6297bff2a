"""The road graph of global routing as arrays: the data model shared by the kernels behind ``emp_route_search`` /
``emp_route_paths`` (include/emplanner.h states the layout and the procedure), ``Planner.route`` and the drop-in
``planner/global_planning.py``.

``RoadGraph.from_segments`` reproduces the reference's ``global_path_planner._build_graph`` (global_planning.py:78-134) on arrays,
``RoadGraph.from_carla_map`` its ``_build_topology`` (:43-76) on anything that quacks like a ``carla.Map``.  Neither imports
``networkx`` or ``carla``; nothing here searches a graph - that is the library's work.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _lib as L

MAX_NODES = L.ROUTE_MAX_NODES
MAX_LENGTH = L.ROUTE_MAX_LENGTH


def _arr(x, dtype, shape, name):
    a = np.ascontiguousarray(x, dtype=dtype)
    if a.ndim != len(shape) or any(s is not None and a.shape[i] != s for i, s in enumerate(shape)):
        raise ValueError(f"{name}: expected shape {tuple('?' if s is None else s for s in shape)}, got {a.shape}")
    return a


class RoadGraph:
    """vertex [N][3] f64, succ_off [N+1], succ [E], length [E], wp_off [E+1] i32, wp [W][3] f64 - all contiguous, checked here the
    way the library checks host arrays: a violation raises ``ValueError``.  An edge id is a position in ``succ``."""

    def __init__(self, vertex, succ_off, succ, length, wp_off, wp):
        self.vertex = _arr(vertex, np.float64, (None, 3), "vertex")
        N = self.vertex.shape[0]
        self.succ_off = _arr(succ_off, np.int32, (N + 1,), "succ_off")
        self.succ = _arr(succ, np.int32, (None,), "succ")
        E = self.succ.shape[0]
        self.length = _arr(length, np.int32, (E,), "length")
        self.wp_off = _arr(wp_off, np.int32, (E + 1,), "wp_off")
        self.wp = _arr(wp, np.float64, (None, 3), "wp")
        W = self.wp.shape[0]
        if not 1 <= N <= MAX_NODES:
            raise ValueError(f"a road graph has 1 to {MAX_NODES} nodes (EMP_ROUTE_MAX_NODES), not {N}")
        if not np.isfinite(self.vertex).all() or not np.isfinite(self.wp).all():
            raise ValueError("vertex and wp must be finite")
        for off, n, name in ((self.succ_off, E, "succ_off"), (self.wp_off, W, "wp_off")):
            if off[0] != 0 or off[-1] != n or (np.diff(off.astype(np.int64)) < 0).any():
                raise ValueError(f"{name} must rise monotonically from 0 to {n}")
        if E and (self.succ.min() < 0 or self.succ.max() >= N):
            raise ValueError("a successor index lies outside [0, N)")
        if E and (self.length.min() < 0 or self.length.max() > MAX_LENGTH):
            raise ValueError(f"an edge length lies outside [0, {MAX_LENGTH}]")
        if E and np.diff(self.wp_off.astype(np.int64)).min() < 2:
            raise ValueError("every edge has at least 2 waypoints (entry and exit)")
        #: the node each edge leaves (the CSR row of its id)
        self.edge_u = np.repeat(np.arange(N, dtype=np.int32), np.diff(self.succ_off))
        if len(np.unique(self.edge_u.astype(np.int64) * N + self.succ)) != E:
            raise ValueError("a node lists the same successor twice (one edge per (u, v), as in a DiGraph)")
        self._device = {}
        #: [E] int32 lane key of each edge: what stands in for CARLA's (road_id, lane_id) in the car-following law
        #: (emp_agent_behave).  The edge id unless a builder knows better; a key below 0 never matches.
        self.edge_key = np.arange(E, dtype=np.int32)
        # what from_segments / from_carla_map add
        self.seg_edge = None          # [S] the edge each segment became (a duplicate (u, v) shares its edge)
        self.edge_seg = None          # [E] the segment whose attributes the edge carries (the LAST add_edge of the pair)
        self.id_map = None            # {(x, y, z) rounded: node id}
        self.topology = None          # from_carla_map: the reference's list of {"entry", "exit", "path"} dicts
        self.waypoints = None         # from_carla_map: the waypoint objects, one per row of wp
        self.road_to_edge = None      # from_carla_map: {road_id: {section_id: {lane_id: (n1, n2)}}}

    n_nodes = property(lambda self: self.vertex.shape[0])
    n_edges = property(lambda self: self.succ.shape[0])
    n_wp = property(lambda self: self.wp.shape[0])

    def arrays(self):
        return self.vertex, self.succ_off, self.succ, self.length, self.wp_off, self.wp

    def edge_id(self, u: int, v: int) -> int:
        """The id of edge (u, v): the first match in u's list.  KeyError without one."""
        a, b = int(self.succ_off[u]), int(self.succ_off[u + 1])
        hit = np.nonzero(self.succ[a:b] == v)[0]
        if not len(hit):
            raise KeyError((u, v))
        return a + int(hit[0])

    def max_edge_waypoints(self) -> int:
        return int(np.diff(self.wp_off).max()) if self.n_edges else 0

    def on_device(self, device):
        """The six arrays as torch tensors on ``device`` (copied once, kept)."""
        import torch
        key = str(device)
        if key not in self._device:
            self._device[key] = tuple(torch.from_numpy(a).to(device) for a in self.arrays())
        return self._device[key]

    def struct(self, pointers) -> "L.RouteGraph":
        g = L.RouteGraph()
        g.vertex, g.succ_off, g.succ, g.length, g.wp_off, g.wp = pointers
        g.n_nodes, g.n_edges, g.n_wp, g.reserved = self.n_nodes, self.n_edges, self.n_wp, 0
        return g

    # ---- builders -------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_segments(cls, entry_xyz, exit_xyz, path_off, path_xyz) -> "RoadGraph":
        """``_build_graph`` on arrays.  Segment s runs from ``entry_xyz[s]`` to ``exit_xyz[s]`` (the waypoints' own, unrounded
        positions) over the waypoints ``path_xyz[path_off[s]:path_off[s + 1]]``.  Node positions are rounded to 2 decimals and
        numbered in order of first appearance, entry before exit; the successors of a node keep the order of the FIRST segment
        of each (u, v); a later segment with the same (u, v) replaces the edge's length and waypoints (networkx's add_edge
        updates the attributes in place).  A segment may start and end at the same node."""
        entry = _arr(entry_xyz, np.float64, (None, 3), "entry_xyz")
        S = entry.shape[0]
        exit_ = _arr(exit_xyz, np.float64, (S, 3), "exit_xyz")
        path_off = _arr(path_off, np.int64, (S + 1,), "path_off")
        path = _arr(path_xyz, np.float64, (None, 3), "path_xyz")
        if path_off[0] != 0 or path_off[-1] != path.shape[0] or (np.diff(path_off) < 0).any():
            raise ValueError("path_off must rise monotonically from 0 to len(path_xyz)")
        r_entry, r_exit = np.round(entry, 2), np.round(exit_, 2)
        id_map, vertex = {}, []
        adj = []                       # per node: {v: segment}, insertion-ordered like DiGraph's adjacency
        seg_uv = np.zeros((S, 2), np.int32)
        for s in range(S):
            for k, xyz in enumerate((r_entry[s], r_exit[s])):
                key = (float(xyz[0]), float(xyz[1]), float(xyz[2]))
                if key not in id_map:
                    id_map[key] = len(id_map)
                    vertex.append(key)
                    adj.append({})
                seg_uv[s, k] = id_map[key]
            adj[seg_uv[s, 0]][int(seg_uv[s, 1])] = s
        succ_off, succ, edge_seg = [0], [], []
        for u, row in enumerate(adj):
            succ.extend(row.keys())
            edge_seg.extend(row.values())
            succ_off.append(len(succ))
        n_path = np.diff(path_off)
        edge_seg = np.asarray(edge_seg, np.int64)
        wp_off = np.concatenate([[0], np.cumsum(n_path[edge_seg] + 2)]) if len(edge_seg) else np.zeros(1, np.int64)
        wp = np.zeros((int(wp_off[-1]), 3))
        for e, s in enumerate(edge_seg):
            a = int(wp_off[e])
            wp[a] = entry[s]
            wp[a + 1:a + 1 + n_path[s]] = path[path_off[s]:path_off[s + 1]]
            wp[a + 1 + n_path[s]] = exit_[s]
        g = cls(np.asarray(vertex, np.float64).reshape(-1, 3), succ_off, np.asarray(succ, np.int32), n_path[edge_seg] + 1, wp_off, wp)
        g.edge_seg = edge_seg.astype(np.int32)
        g.seg_edge = np.array([g.edge_id(u, v) for u, v in seg_uv], np.int32)
        g.id_map = id_map
        return g

    @staticmethod
    def topology_of(world_map, sampling_resolution) -> list:
        """``_build_topology``: one {"entry", "exit", "path"} dict per (entry, exit) pair of ``world_map.get_topology()``.  The
        path holds the waypoints met by stepping ``sampling_resolution`` metres at a time from the entry for as long as the
        exit is farther than one step away; an exit within one step of the entry leaves it empty."""
        def between(entry, goal):
            far = lambda w: w.transform.location.distance(goal) > sampling_resolution
            if not far(entry):
                return
            w = entry.next(sampling_resolution)[0]
            while far(w):
                yield w
                w = w.next(sampling_resolution)[0]

        return [{"entry": pair[0], "exit": pair[1], "path": list(between(pair[0], pair[1].transform.location))}
                for pair in world_map.get_topology()]

    @classmethod
    def from_topology(cls, topology) -> "RoadGraph":
        """``_build_graph`` on a topology list.  The waypoint objects, the topology and the road / section / lane table stay on
        the host (``waypoints``, ``topology``, ``road_to_edge``)."""
        xyz = lambda w: (w.transform.location.x, w.transform.location.y, w.transform.location.z)
        rows = lambda pts: np.asarray(pts, np.float64).reshape(-1, 3)
        path_off = np.concatenate([[0], np.cumsum([len(t["path"]) for t in topology])]).astype(np.int64)
        g = cls.from_segments(rows([xyz(t["entry"]) for t in topology]), rows([xyz(t["exit"]) for t in topology]), path_off,
                              rows([xyz(w) for t in topology for w in t["path"]]))
        g.topology = topology
        g.waypoints = []
        for s in g.edge_seg:
            t = topology[s]
            g.waypoints += [t["entry"]] + t["path"] + [t["exit"]]
        g.road_to_edge = {}
        for t, e in zip(topology, g.seg_edge):
            w = t["entry"]
            g.road_to_edge.setdefault(w.road_id, {}).setdefault(w.section_id, {})[w.lane_id] = (int(g.edge_u[e]), int(g.succ[e]))
        g.edge_key = np.array([pack_lane_key(topology[s]["entry"].road_id, topology[s]["entry"].lane_id) for s in g.edge_seg],
                              np.int32).reshape(g.n_edges)
        return g

    @classmethod
    def from_carla_map(cls, world_map, sampling_resolution) -> "RoadGraph":
        """``_build_topology`` then ``_build_graph`` on ``world_map.get_topology()``.  Duck-typed: a waypoint needs
        ``transform.location`` (``x``, ``y``, ``z``, ``distance``), ``next(d)``, ``road_id``, ``section_id``, ``lane_id``."""
        return cls.from_topology(cls.topology_of(world_map, sampling_resolution))


def pack_lane_key(road_id: int, lane_id: int) -> int:
    """(road_id, lane_id) as one non-negative int32: road_id * 256 + (lane_id + 128), lane ids in [-128, 127] and road ids below
    2^23 (OpenDRIVE lanes are small signed numbers)."""
    road_id, lane_id = int(road_id), int(lane_id)
    if not (0 <= road_id < 1 << 23 and -128 <= lane_id <= 127):
        raise ValueError(f"(road_id, lane_id) = ({road_id}, {lane_id}) does not fit a lane key")
    return road_id * 256 + (lane_id + 128)


@dataclass
class RouteResult:
    """What ``Planner.route`` returns (``Planner.route_search``: the first three).  Arrays of the kind that went in."""
    route: object            # (B, max_route) int32 node ids
    route_len: object        # (B,)
    status: object           # (B,) EMP_ROUTE_* bits
    wp_index: object = None      # (B, max_global) int32 rows of graph.wp
    global_path: object = None   # (B, max_global, 4) x, y, theta, kappa
    n_global: object = None      # (B,)

    def lane_key(self, graph: "RoadGraph"):
        """(B, max_global) int32: the lane key (``graph.edge_key``) of the edge each waypoint of ``global_path`` lies on, -1 past
        ``n_global`` - the ``lane`` array of ``Planner.agent_behave`` / ``traffic.BehaviorTraffic``, of the kind ``wp_index`` is."""
        if self.wp_index is None:
            raise ValueError("lane_key needs the wp_index of Planner.route")
        torch_ = hasattr(self.wp_index, "data_ptr")
        wi = self.wp_index.detach().cpu().numpy() if torch_ else np.asarray(self.wp_index)
        ng = self.n_global.detach().cpu().numpy() if torch_ else np.asarray(self.n_global)
        edge = np.clip(np.searchsorted(graph.wp_off, np.clip(wi, 0, max(graph.n_wp - 1, 0)), side="right") - 1, 0, max(graph.n_edges - 1, 0))
        key = np.where(np.arange(wi.shape[1])[None, :] < ng[:, None], np.asarray(graph.edge_key, np.int32)[edge], -1).astype(np.int32)
        if torch_:
            import torch
            return torch.from_numpy(key).to(self.wp_index.device)
        return key


UNREACHABLE, TRUNCATED, BAD_QUERY = L.ROUTE_UNREACHABLE, L.ROUTE_TRUNCATED, L.ROUTE_BAD_QUERY
