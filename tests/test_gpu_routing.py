"""GPU suite of global routing, through the C-ABI (emp_route_search / emp_route_paths): the towns and micro graphs of
tests/golden/routing/ against the reference's recorded routes and waypoint sequences, theta and kappa bit for bit against
Planner.heading_kappa on the same xy, ragged batches on poisoned outputs, the node limit, host arrays against device tensors, the
chain into Planner.reference_line, and the drop-in search_path_way on a fake map."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import pytest

from emplanner_carla_amd import _lib as L
from emplanner_carla_amd.api import smooth_params
from emplanner_carla_amd.routing import RoadGraph
from tests import route_cases as rc
from tests import route_port as port
from tests.conftest import make_planner

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(rc.ROOT, "tests", "golden"))
KEYS = ("route", "route_len", "wp_index", "global_path", "n_global", "status")


@pytest.fixture(scope="module")
def planner():
    pl = make_planner()
    yield pl
    pl.close()


def as_dict(r):
    get = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else x
    return {k: get(getattr(r, k)) for k in KEYS if getattr(r, k) is not None}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check(planner, got, want, what):
    """routes, rows, counts and statuses equal; xy in bits; theta and kappa the bits of Planner.heading_kappa on the same xy"""
    for k in ("route", "route_len", "wp_index", "n_global", "status"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")
    gp = got["global_path"]
    assert np.array_equal(bits(gp[..., :2]), bits(want["xy"])), f"{what}: xy differs in bits"
    n = np.minimum(got["n_global"], gp.shape[1]).astype(np.int32)
    if gp.shape[1] >= 2:
        th, ka = planner.heading_kappa(np.ascontiguousarray(gp[..., :2]), n)
        assert np.array_equal(bits(gp[..., 2]), bits(th)), f"{what}: theta is not emp_heading_kappa's"
        assert np.array_equal(bits(gp[..., 3]), bits(ka)), f"{what}: kappa is not emp_heading_kappa's"
    rc.padded_ok(got, got["route"].shape[1], gp.shape[1], what)


@pytest.mark.parametrize("name", rc.TOWNS + rc.MICRO)
def test_fixture_queries_equal_the_reference(planner, name):
    g, want = rc.graph(name), rc.expected(name)
    R, G = want["route"].shape[1], want["wp_index"].shape[1]
    got = as_dict(planner.route(g, *rc.queries(name), R, G))
    check(planner, got, want, name)
    s, e, _, _ = rc.queries(name)
    only = as_dict(planner.route_search(g, s, e, R))                 # emp_route_search: the route part of emp_route_paths
    for k in ("route", "route_len", "status"):
        np.testing.assert_array_equal(only[k], got[k], err_msg=f"{name}: emp_route_search {k}")


def raw_paths(planner, g, s, e, ow, dw, max_route, max_global, device):
    """emp_route_paths on output buffers pre-filled with 0xCC bytes, in host memory or (device) on torch tensors."""
    B = len(s)
    shapes = dict(route=((B, max_route), np.int32), route_len=((B,), np.int32), wp_index=((B, max_global), np.int32),
                  global_path=((B, max_global, 4), np.float64), n_global=((B,), np.int32), status=((B,), np.int32))
    outs = {k: np.full(sh, rc.POISON_I if dt == np.int32 else rc.POISON_F, dt) for k, (sh, dt) in shapes.items()}
    ins = [np.ascontiguousarray(s, np.int32), np.ascontiguousarray(e, np.int32), np.ascontiguousarray(ow, np.float64),
           np.ascontiguousarray(dw, np.float64)]
    if device:
        import torch
        outs = {k: torch.from_numpy(v).cuda() for k, v in outs.items()}
        ins = [torch.from_numpy(v).cuda() for v in ins]
        graph = g.struct([t.data_ptr() for t in g.on_device(ins[0].device)])
        torch.cuda.synchronize()
        ptr = lambda t: C.c_void_p(t.data_ptr())
    else:
        graph = g.struct([a.ctypes.data for a in g.arrays()])
        ptr = lambda a: C.c_void_p(a.ctypes.data)
    rcode = planner._lib.emp_route_paths(planner._h, C.byref(graph), B, max_route, max_global, *[ptr(x) for x in ins],
                                         *[ptr(outs[k]) for k in ("route", "route_len", "wp_index", "global_path", "n_global", "status")],
                                         L.EMP_DEVICE if device else L.EMP_HOST)
    assert rcode == 0, planner._lib.emp_last_error(planner._h)
    planner.synchronize()
    return {k: (v.cpu().numpy() if device else v) for k, v in outs.items()}


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("B", (1, 3, 65, 130))
def test_ragged_batches_on_poisoned_outputs(planner, B, device):
    """Reachable, unreachable, truncated (one short of need, and exactly enough) and bad queries in one batch: the port's answer,
    every unused slot 0 where 0xCC bytes were, and every query alone is itself in the batch, bit for bit."""
    g = rc.graph("sparse12")
    s, e, ow, dw, max_route, max_global, want = rc.ragged(B)
    got = raw_paths(planner, g, s, e, ow, dw, max_route, max_global, device)
    check(planner, got, want, f"ragged {B}")
    alone = range(B) if not device else sorted({0, 1, 2, 3, 7, B - 1} & set(range(B)))      # device tensors: one query of each kind
    for b in alone:
        one = raw_paths(planner, g, s[b:b + 1], e[b:b + 1], ow[b:b + 1], dw[b:b + 1], max_route, max_global, device)
        for k in KEYS:
            assert np.array_equal(one[k][0:1].view(np.uint8), got[k][b:b + 1].view(np.uint8)), f"query {b} alone differs from the batch in {k}"


@pytest.mark.parametrize("name", ("jitter8", "micro_degree_70", "micro_ring_65"))
def test_host_arrays_and_device_tensors_agree(planner, name):
    import torch
    g, want = rc.graph(name), rc.expected(name)
    R, G = want["route"].shape[1], want["wp_index"].shape[1]
    host = as_dict(planner.route(g, *rc.queries(name), R, G))
    r = planner.route(g, *[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in rc.queries(name)], R, G)
    assert r.global_path.is_cuda and r.route.is_cuda
    torch.cuda.synchronize()
    dev = as_dict(r)
    for k in KEYS:
        assert np.array_equal(host[k].view(np.uint8), dev[k].view(np.uint8)), f"{name}: {k}"
    s, e, _, _ = rc.queries(name)
    only = as_dict(planner.route_search(g, torch.from_numpy(s).cuda(), torch.from_numpy(e).cuda(), R))
    for k in ("route", "route_len", "status"):
        np.testing.assert_array_equal(only[k], host[k])


def test_node_limit(planner):
    """4096 nodes are accepted (a chain: 96 KiB of LDS, 4095 pops), 4097 refused with EMP_ERR_INVALID before anything is read."""
    n = L.ROUTE_MAX_NODES
    g = rc.chain(n)
    s = np.array([0, 4000, n - 1, 17, 2048], np.int32)
    e = np.array([n - 2, 4090, 0, 17, 1000], np.int32)              # edge k leaves node k
    ow = np.ascontiguousarray(g.wp[2 * np.minimum(s, n - 2)])        # the entry of the first edge
    got = as_dict(planner.route(g, s, e, ow, ow, n, n))
    for b in range(len(s)):
        if s[b] > e[b]:
            assert got["status"][b] == L.ROUTE_UNREACHABLE and got["route_len"][b] == 0 and got["n_global"][b] == 0
            continue
        route = np.arange(s[b], e[b] + 2)
        rows = [2 * s[b], 2 * s[b] + 1] + [2 * i + 1 for i in range(s[b] + 1, e[b])]
        assert got["status"][b] == 0 and got["route_len"][b] == len(route) and got["n_global"][b] == len(rows), b
        np.testing.assert_array_equal(got["route"][b, :len(route)], route)
        np.testing.assert_array_equal(got["wp_index"][b, :len(rows)], rows)
        assert np.array_equal(bits(got["global_path"][b, :len(rows), :2]), bits(g.wp[rows, :2]))
    rc.padded_ok(got, n, n, "chain")
    st = g.struct([a.ctypes.data for a in g.arrays()])
    st.n_nodes = n + 1
    out = [np.zeros(8, np.int32) for _ in range(3)]
    args = [s[:1].ctypes.data, e[:1].ctypes.data] + [o.ctypes.data for o in out]
    assert planner._lib.emp_route_search(planner._h, C.byref(st), 1, 8, *args, L.EMP_HOST) == -1       # EMP_ERR_INVALID
    assert b"EMP_ROUTE_MAX_NODES" in planner._lib.emp_last_error(planner._h)
    st.n_nodes = n
    for max_route, B in ((1, 1), (1, 0)):
        assert planner._lib.emp_route_search(planner._h, C.byref(st), B, max_route, *args, L.EMP_HOST) == -1
    assert planner._lib.emp_route_search(planner._h, C.byref(st), 0, 8, *args, L.EMP_HOST) == 0         # an empty batch
    st.reserved = 1
    assert planner._lib.emp_route_search(planner._h, C.byref(st), 1, 8, *args, L.EMP_HOST) == -1
    st.reserved = 0
    bad = g.succ.copy()
    bad[5] = n
    st.succ = bad.ctypes.data
    assert planner._lib.emp_route_search(planner._h, C.byref(st), 1, 8, *args, L.EMP_HOST) == -1       # host graphs are checked
    assert b"successor" in planner._lib.emp_last_error(planner._h)


def test_device_graphs_with_bad_indices_are_never_followed(planner):
    """EMP_DEVICE: the graph cannot be checked up front; an index out of range met during a query ends that query."""
    import torch
    g = rc.graph("micro_ring_63")
    s, e, ow, dw = rc.queries("micro_ring_63")
    for i, idx, v in ((2, 0, 10 ** 6), (2, 3, -5), (1, 1, -4), (1, 2, 10 ** 6), (4, 3, 10 ** 7), (4, 2, -9)):
        arrs = [x.copy() for x in g.arrays()]
        arrs[i][idx] = v
        broken = RoadGraph.__new__(RoadGraph)
        broken.vertex, broken.succ_off, broken.succ, broken.length, broken.wp_off, broken.wp = arrs
        broken._device = {}
        got = raw_paths(planner, broken, s, e, ow, dw, 64, 256, True)
        bad = got["status"] == L.ROUTE_BAD_QUERY
        assert set(got["status"]) <= {0, L.ROUTE_BAD_QUERY} and bad.any(), (i, idx, v)
        assert not got["route_len"][bad].any() and not got["n_global"][bad].any() and not got["wp_index"][bad].any()
        assert not got["route"][bad].any() and not bits(got["global_path"][bad]).any()
    torch.cuda.synchronize()


def test_routed_paths_feed_the_reference_line(planner):
    """The chain holds: the routed global_path goes into Planner.reference_line and gives, bit for bit, what the port's path does
    (the port's waypoints with Planner.heading_kappa's theta and kappa)."""
    g, want = rc.graph("sparse12"), rc.expected("sparse12")
    long = np.nonzero(want["n_global"] >= 60)[0][:24]
    assert len(long) >= 8
    s, e, ow, dw = (np.ascontiguousarray(a[long]) for a in rc.queries("sparse12"))
    G = int(want["n_global"][long].max())
    r = planner.route(g, s, e, ow, dw, want["route"].shape[1], G)
    assert not r.status.any()
    p = port.run(g, s, e, ow, dw, want["route"].shape[1], G)
    th, ka = planner.heading_kappa(p["xy"], p["n_global"])
    path = np.concatenate([p["xy"], th[..., None], ka[..., None]], axis=2)
    pred = np.ascontiguousarray(p["xy"][:, 20] + 0.3)
    pre = np.full(len(long), 18, np.int32)
    first = np.ones(len(long), np.int32)
    a = planner.reference_line(smooth_params(), r.global_path, r.n_global, pred, pre, first)
    b = planner.reference_line(smooth_params(), path, p["n_global"], pred, pre, first)
    assert (a[4] == 0).any()
    for x, y, what in zip(a, b, ("ref_line", "n_ref", "match_index", "iters", "status")):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), what


def test_dropin_search_path_way_on_a_fake_map(planner):
    """global_path_planner on the fake map of town jitter8: the graph the reference built, and search_path_way returns the map's
    waypoint objects the reference returned, in order, each with RoadOption.LANE_FOLLOW; failures raise what the reference raises."""
    import make_golden_routing as mk
    from emplanner_carla_amd.planner import global_planning as gp
    m, res, queries = mk.town("jitter8")
    f, want = rc.fixture("jitter8"), rc.expected("jitter8")
    pl = gp.global_path_planner(m, res)
    topology, graph, id_map, road_to_edge = pl.get_topology_and_graph_info()
    for k, a in zip(("vertex", "succ_off", "succ", "length", "wp_off", "wp"), graph.arrays()):
        assert np.array_equal(a, f[k]), k
    assert len(topology) == len(f["seg_uv"]) and len(id_map) == graph.n_nodes
    for k in list(range(0, 300, 13)):
        sa, s_a, sb, s_b = queries[k]
        origin, destination = m.location(sa, s_a), m.location(sb, s_b)
        way = pl.search_path_way(origin, destination)
        n = int(want["n_global"][k])
        assert len(way) == n and all(o is gp.RoadOption.LANE_FOLLOW for _, o in way)
        assert [w for w, _ in way] == [graph.waypoints[i] for i in want["wp_index"][k, :n]]
        xy = np.array([(w.transform.location.x, w.transform.location.y) for w, _ in way])
        assert np.array_equal(bits(xy), bits(want["xy"][k, :n]))
        assert pl._route_search(origin, destination) == list(want["route"][k, :want["route_len"][k]])
        assert pl._A_star(int(f["q_start_node"][k]), int(graph.edge_u[f["q_end_edge"][k]])) == list(want["route"][k, :want["route_len"][k] - 1])
        assert pl._find_location_edge(origin) == tuple(f["seg_uv"][sa])
    assert pl._closest_index(m.get_waypoint(m.location(3, 2.0)), [w for w in graph.waypoints[:6]]) in range(6)
    # an unreachable destination, on the town with removed segments
    m2, res2, q2 = mk.town("sparse12")
    f2 = rc.fixture("sparse12")
    pl2 = gp.global_path_planner(m2, res2)
    k = int(np.nonzero(f2["reachable"] == 0)[0][0])
    try:
        import networkx
        no_path = networkx.NetworkXNoPath
    except ImportError:
        no_path = Exception
    with pytest.raises(no_path) as err:
        pl2.search_path_way(m2.location(q2[k][0], q2[k][1]), m2.location(q2[k][2], q2[k][3]))
    assert type(err.value).__name__ == "NetworkXNoPath"
    assert pl2._A_star(int(f2["q_start_node"][k]), int(pl2._graph.edge_u[f2["q_end_edge"][k]])) is None
    # a location that lies on no edge of the graph: the reference's TypeError
    m.lane_ids[5] = (9999, 0, 1)
    with pytest.raises(TypeError):
        pl.search_path_way(m.location(5, 1.0), m.location(7, 1.0))
