"""Drop-in for reference planner/global_planning.py: ``RoadOption`` and ``global_path_planner`` with the reference's method names,
argument names and defaults.  The road graph is a ``routing.RoadGraph`` (arrays, no networkx), the CARLA look-ups stay on the
host, and every route is searched and expanded by the HIP kernel behind ``emp_route_search`` / ``emp_route_paths`` as a batch of
one.  A fleet routes all its vehicles in one call through ``Planner.route`` on the same graph.

Neither ``networkx`` nor ``carla`` is imported.  An unreachable destination raises ``networkx.NetworkXNoPath`` where networkx is
installed (so a driver's ``except`` clause keeps working) and a local class of that name otherwise.
"""
from __future__ import annotations

from enum import Enum

import numpy as np

from .. import routing
from . import _runtime


class RoadOption(Enum):
    """How an edge of a route is to be driven.  Members and values are the reference's; every edge built here is LANE_FOLLOW."""
    VOID = -1
    LEFT = 1
    RIGHT = 2
    STRAIGHT = 3
    LANE_FOLLOW = 4
    CHANGE_LANE_LEFT = 5
    CHANGE_LANE_RIGHT = 6


class _LocalNoPath(Exception):
    """No route between two nodes: what is raised where networkx is not installed."""


_LocalNoPath.__name__ = _LocalNoPath.__qualname__ = "NetworkXNoPath"


def __getattr__(name):
    """``global_planning.NetworkXNoPath``: networkx's class where networkx is installed, the local one otherwise - resolved on
    first use, so that importing this module never imports networkx."""
    if name != "NetworkXNoPath":
        raise AttributeError(name)
    import importlib.util
    if importlib.util.find_spec("networkx") is None:
        return _LocalNoPath
    import networkx
    return networkx.NetworkXNoPath


def _no_path(start_node, end_node):
    return __getattr__("NetworkXNoPath")(f"no route from node {start_node} to node {end_node}")


def _require_ok(status):
    if status:
        raise RuntimeError(f"routing failed with status {int(status)} (EMP_ROUTE_* bits)")


def _xyz(location):
    return [location.x, location.y, location.z]


class global_path_planner(object):
    def __init__(self, world_map, sampling_resolution):
        self._map, self._sampling_resolution = world_map, sampling_resolution
        # filled by the two builders; _graph is a routing.RoadGraph where the reference holds a networkx.DiGraph
        self._topology = self._graph = self._id_map = self._road_to_edge = None
        self._build_topology()
        self._build_graph()

    def get_topology_and_graph_info(self):
        return self._topology, self._graph, self._id_map, self._road_to_edge

    def _build_topology(self):
        self._topology = routing.RoadGraph.topology_of(self._map, self._sampling_resolution)

    def _build_graph(self):
        self._graph = routing.RoadGraph.from_topology(self._topology)
        self._id_map = self._graph.id_map
        self._road_to_edge = self._graph.road_to_edge

    def _find_location_edge(self, loc):
        """(n1, n2) of the edge ``loc`` lies on, None for a lane the graph does not hold."""
        wp = self._map.get_waypoint(loc)
        return self._road_to_edge.get(wp.road_id, {}).get(wp.section_id, {}).get(wp.lane_id)

    def _route_search(self, origin, destination):
        start_edge = self._find_location_edge(origin)
        end_edge = self._find_location_edge(destination)
        g = self._graph
        r = _runtime.planner().route_search(g, np.array([start_edge[0]], np.int32), np.array([g.edge_id(*end_edge)], np.int32),
                                            g.n_nodes + 1)
        if r.status[0] & routing.UNREACHABLE:
            raise _no_path(start_edge[0], end_edge[0])
        _require_ok(r.status[0])
        return [int(n) for n in r.route[0, :r.route_len[0]]]

    def _A_star(self, n_begin, n_end):
        """The route from ``n_begin`` to ``n_end`` as a list of node ids, None when there is none.  The library's query ends at
        an edge, so ``n_end`` needs at least one edge leaving it (every node ``_find_location_edge(...)[0]`` returns has one)."""
        g = self._graph
        if g.succ_off[n_end] == g.succ_off[n_end + 1]:
            raise ValueError(f"node {n_end} has no outgoing edge to name it by")
        r = _runtime.planner().route_search(g, np.array([n_begin], np.int32), np.array([g.succ_off[n_end]], np.int32), g.n_nodes + 1)
        if r.status[0] & routing.UNREACHABLE:
            return None
        _require_ok(r.status[0])
        return [int(n) for n in r.route[0, :r.route_len[0] - 1]]

    @staticmethod
    def _closest_index(current_waypoint, waypoint_list):
        """The first index whose waypoint is strictly nearest to ``current_waypoint``; -1 for an empty list or when no distance
        is below infinity (a NaN distance never wins)."""
        here = current_waypoint.transform.location
        d = [w.transform.location.distance(here) for w in waypoint_list]
        best = min((x for x in d if x == x), default=float("inf"))
        return d.index(best) if best < float("inf") else -1

    def search_path_way(self, origin, destination):
        """[(waypoint, RoadOption.LANE_FOLLOW), ...] from ``origin`` to ``destination`` (``carla.Location``-like)."""
        start_edge = self._find_location_edge(origin)
        end_edge = self._find_location_edge(destination)
        start_node, end_id = start_edge[0], self._graph.edge_id(*end_edge[:2])      # (TypeError for a location off every edge)
        origin_wp = self._map.get_waypoint(origin)
        destination_wp = self._map.get_waypoint(destination)
        g = self._graph
        r = _runtime.planner().route(g, np.array([start_node], np.int32), np.array([end_id], np.int32),
                                     np.array([_xyz(origin_wp.transform.location)]), np.array([_xyz(destination_wp.transform.location)]),
                                     g.n_nodes + 1, g.n_wp + g.max_edge_waypoints())
        if r.status[0] & routing.UNREACHABLE:
            raise _no_path(start_edge[0], end_edge[0])
        _require_ok(r.status[0])
        return [(g.waypoints[i], RoadOption.LANE_FOLLOW) for i in r.wp_index[0, :r.n_global[0]]]
