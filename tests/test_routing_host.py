"""CPU suite of global routing: the Python port (tests/route_port.py) against the reference's recorded routes and waypoint
sequences (tests/golden/routing/, every query of every town), RoadGraph.from_segments against the reference's recorded graph, the
g++ build of csrc/emp_route_core.h and csrc/emp_route_launch.h (tests/host_check/route_check.cpp) bit for bit against the port,
the ctypes layout of emp_route_graph, RoadGraph's refusals, the drop-in's surface, and - where the reference tree is present -
every routing fixture regenerated bit for bit."""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from emplanner_carla_amd import _lib as L
from emplanner_carla_amd.routing import RoadGraph
from tests import route_cases as rc
from tests import route_port as port
from tests.conftest import assert_rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(ROOT, "tests", "host_check", "route_check.cpp")
RTOL = 1e-6                  # cal_heading_kappa against the reference: the rule of tests/test_gpu_frenet_batch.py::test_heading_kappa
ALL = rc.TOWNS + rc.MICRO
sys.path.insert(0, GOLDEN)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("route_check") / "libroutecheck.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", SRC, "-o", out], check=True)
    lib = C.CDLL(out)
    p, i = C.c_void_p, C.c_int
    lib.rc_plan.restype = C.c_char_p
    lib.rc_plan.argtypes = [i, i, i, i, p]
    lib.rc_graph_error.restype = C.c_char_p
    lib.rc_graph_error.argtypes = [C.POINTER(L.RouteGraph)]
    lib.rc_layout.restype = None
    lib.rc_layout.argtypes = [p]
    lib.rc_route.restype = None
    lib.rc_route.argtypes = [C.POINTER(L.RouteGraph), i, i, i] + [p] * 10
    return lib


def host_route(lib, g, s, e, ow, dw, max_route, max_global, search_only=False):
    """rc_route on NumPy arrays, outputs as a dict (theta and kappa in global_path)."""
    B = len(s)
    s, e = np.ascontiguousarray(s, np.int32), np.ascontiguousarray(e, np.int32)
    ow, dw = np.ascontiguousarray(ow, np.float64), np.ascontiguousarray(dw, np.float64)
    o = dict(route=np.zeros((B, max_route), np.int32), route_len=np.zeros(B, np.int32), wp_index=np.zeros((B, max_global), np.int32),
             global_path=np.zeros((B, max_global, 4)), n_global=np.zeros(B, np.int32), status=np.zeros(B, np.int32))
    st = g.struct([a.ctypes.data for a in g.arrays()])
    ptr = lambda a: a.ctypes.data
    lib.rc_route(C.byref(st), B, max_route, max_global, ptr(s), ptr(e), None if search_only else ptr(ow), None if search_only else ptr(dw),
                 ptr(o["route"]), ptr(o["route_len"]), ptr(o["wp_index"]), ptr(o["global_path"]), ptr(o["n_global"]), ptr(o["status"]))
    return o


def same(got, want, what, keys=("route", "route_len", "wp_index", "n_global", "status")):
    for k in keys:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")
    if "wp_index" in keys and "xy" in want and "global_path" in got:
        assert np.array_equal(got["global_path"][..., :2].view(np.uint64), want["xy"].view(np.uint64)), f"{what}: xy differs in bits"


# ---- the port against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_port_equals_the_reference_on_every_recorded_query(name):
    """route, _A_star's own list, waypoint sequence as rows of wp, xy to the bit: no query excluded."""
    f, g, want = rc.fixture(name), rc.graph(name), rc.expected(name)
    s, e, ow, dw = rc.queries(name)
    R, G = want["route"].shape[1], want["wp_index"].shape[1]
    got = port.run(g, s, e, ow, dw, R, G)
    for k in ("route", "route_len", "wp_index", "n_global", "status"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name}: {k}")
    assert np.array_equal(got["xy"].view(np.uint64), want["xy"].view(np.uint64)), f"{name}: xy differs in bits"
    for k in range(len(s)):                    # _A_star alone: the route without n_exit, nothing where unreachable
        a, b = f["astar_off"][k:k + 2]
        n_end, _ = port.edge_ends(g, int(e[k]))
        assert (port.astar(g, int(s[k]), n_end) or []) == list(f["astar"][a:b]), f"{name}: _A_star of query {k}"
    assert f["gap"].min() >= 1e-9, "a pop of this fixture is decided by less than hypot and sqrt may differ by"


def test_fixtures_cover_what_they_are_for():
    f = rc.fixture("grid6")
    assert len(f["q_start_node"]) == 36 * 36 and len(set(zip(f["q_start_node"], rc.graph("grid6").edge_u[f["q_end_edge"]]))) == 1296
    assert len(rc.fixture("jitter8")["q_start_node"]) == 300 and len(rc.fixture("sparse12")["q_start_node"]) == 300
    assert (rc.fixture("sparse12")["reachable"] == 0).sum() >= 1 and rc.graph("sparse12").n_nodes == 144
    assert np.diff(rc.graph("micro_degree_70").succ_off).max() == 70
    assert [rc.graph(f"micro_ring_{n}").n_nodes for n in (63, 64, 65)] == [63, 64, 65]
    two = rc.expected("micro_two_nodes")
    assert (two["route_len"] == 2).all()                       # start_node == n_end: the one edge is emitted twice
    g = rc.graph("micro_self_loop")
    assert (g.succ == g.edge_u).any()
    back = rc.expected("micro_back_over_start")
    assert any(r[0] == r[n - 1] and n > 2 for r, n in zip(back["route"], back["route_len"]))      # n_exit is the start node again


def test_the_tie_rule_decides_routes_on_the_regular_grid():
    """Smallest f, then OLDEST first insertion.  On the regular grid a port that breaks ties by node index, or by newest insertion,
    returns other routes than the reference on many pairs - so this fixture would catch either."""
    g, want = rc.graph("grid6"), rc.expected("grid6")
    s, e, _, _ = rc.queries("grid6")

    def astar_with(tie):                        # route_port.astar with another tie-break
        wrong = 0
        for k in range(len(s)):
            n_end, _ = port.edge_ends(g, int(e[k]))
            N = g.n_nodes
            h = [port.dist3(g.vertex[n], g.vertex[n_end]) for n in range(N)]
            state, gc, parent, stamp, nxt = [0] * N, [0] * N, [-1] * N, [0] * N, 1
            state[s[k]] = 1
            while True:
                opened = [n for n in range(N) if state[n] == 1]
                c = min(opened, key=lambda n: (gc[n] + h[n], tie(n, stamp[n])))
                if c == n_end:
                    break
                for ed in range(g.succ_off[c], g.succ_off[c + 1]):
                    v, ng = int(g.succ[ed]), gc[c] + int(g.length[ed])
                    if state[v] == 1 and ng < gc[v]:
                        gc[v], parent[v] = ng, c
                    elif state[v] == 0:
                        state[v], gc[v], parent[v], stamp[v], nxt = 1, ng, c, nxt, nxt + 1
                state[c] = 2
            route = [n_end]
            while parent[route[-1]] != -1:
                route.append(parent[route[-1]])
            wrong += route[::-1] != list(want["route"][k, :want["route_len"][k] - 1])
        return wrong

    assert astar_with(lambda n, st: st) == 0
    assert astar_with(lambda n, st: n) > 100
    assert astar_with(lambda n, st: -st) > 100


# ---- RoadGraph ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_from_segments_rebuilds_the_reference_graph(name):
    """ids, successor order, lengths and waypoints of the reference's DiGraph from _build_topology's segments; micro_duplicate holds
    two segments of one (u, v): the successor keeps its first position, the later segment's length and waypoints win."""
    f = rc.fixture(name)
    g = RoadGraph.from_segments(f["seg_entry"], f["seg_exit"], f["seg_path_off"], f["seg_path"])
    for k, a in zip(("vertex", "succ_off", "succ", "length", "wp_off", "wp"), g.arrays()):
        assert a.dtype == f[k].dtype and np.array_equal(a, f[k]), f"{name}: {k}"
    np.testing.assert_array_equal(np.stack([g.edge_u[g.seg_edge], g.succ[g.seg_edge]], 1), f["seg_uv"])
    if name == "micro_duplicate":
        assert len(f["seg_uv"]) == g.n_edges + 1 and g.seg_edge[0] == g.seg_edge[2] == 0 and g.edge_seg[0] == 2
        assert g.length[0] == f["seg_path_off"][3] - f["seg_path_off"][2] + 1


@pytest.mark.parametrize("name", ("jitter8", "micro_duplicate", "micro_self_loop"))
def test_from_carla_map_rebuilds_the_reference_graph(name):
    import make_golden_routing as mk
    m, res, _ = mk.town(name)
    f, g = rc.fixture(name), RoadGraph.from_carla_map(m, res)
    for k, a in zip(("vertex", "succ_off", "succ", "length", "wp_off", "wp"), g.arrays()):
        assert np.array_equal(a, f[k]), f"{name}: {k}"
    assert len(g.waypoints) == g.n_wp and len(g.topology) == len(f["seg_uv"])
    for i in (0, g.n_wp // 2, g.n_wp - 1):
        loc = g.waypoints[i].transform.location
        assert (loc.x, loc.y, loc.z) == tuple(g.wp[i])
    for t, (u, v) in zip(g.topology, f["seg_uv"]):
        w = t["entry"]
        assert g.road_to_edge[w.road_id][w.section_id][w.lane_id] == (u, v)


def test_road_graph_refusals():
    g = rc.graph("micro_duplicate")
    a = lambda: [x.copy() for x in g.arrays()]
    RoadGraph(*a())

    def refused(i, edit, match):
        arrs = a()
        edit(arrs[i])
        with pytest.raises(ValueError, match=match):
            RoadGraph(*arrs)

    def put(idx, v):
        def f(x):
            x[idx] = v
        return f

    refused(0, put((1, 2), np.nan), "finite")
    refused(5, put((3, 0), np.inf), "finite")
    refused(1, put(1, g.succ_off[2] + 1), "succ_off")
    refused(1, put(-1, g.n_edges + 1), "succ_off")
    refused(2, put(0, g.n_nodes), "successor")
    refused(2, put(1, -1), "successor")
    refused(2, put(1, g.succ[0]), "twice")                 # node 0 would list one successor twice
    refused(3, put(0, -1), "length")
    refused(3, put(0, 2 ** 18 + 1), "length")
    refused(4, put(1, g.wp_off[0] + 1), "2 waypoints")
    refused(4, put(-1, g.n_wp - 1), "wp_off")
    RoadGraph(*[x if i != 3 else np.full_like(x, 2 ** 18) for i, x in enumerate(a())])
    rc.chain(L.ROUTE_MAX_NODES)
    with pytest.raises(ValueError, match="EMP_ROUTE_MAX_NODES"):
        rc.chain(L.ROUTE_MAX_NODES + 1)
    with pytest.raises(ValueError, match="shape"):
        RoadGraph(g.vertex[:, :2], *g.arrays()[1:])


# ---- the core and the launch plan, compiled with g++ ---------------------------------------------------------------------------------------
def test_route_graph_struct_layout(lib):
    got = np.zeros(11, np.int64)
    lib.rc_layout(got.ctypes.data)
    want = [C.sizeof(L.RouteGraph)] + [getattr(L.RouteGraph, n).offset for n, _ in L.RouteGraph._fields_]
    assert list(got) == want and [n for n, _ in L.RouteGraph._fields_] == ["vertex", "succ_off", "succ", "length", "wp_off", "wp", "n_nodes",
                                                                          "n_edges", "n_wp", "reserved"]


def test_launch_plan(lib):
    out = np.zeros(4, np.int64)
    for B, N in ((1, 1), (3, 63), (130, 144), (32768, 4096)):
        assert lib.rc_plan(B, N, 2, 1, out.ctypes.data) is None
        assert list(out[:3]) == [B, 64, 24 * N]
        assert out[3] == min(32, (160 * 1024) // (24 * N)) and out[2] <= 160 * 1024
    assert out[2] == 96 * 1024 and out[3] == 1                 # the node limit: 96 KiB, one wavefront per compute unit
    for args in ((4, 4097, 2, 1), (4, 0, 2, 1), (0, 4097, 2, 1), (4, 10, 1, 1), (4, 10, 2, 0), (0, 10, 1, 1)):
        assert lib.rc_plan(*args, out.ctypes.data) is not None, args
    assert lib.rc_plan(0, 10, 2, 1, out.ctypes.data) is None and not out.any()      # an empty batch: nothing to launch


def test_graph_check_of_the_library_agrees_with_road_graph(lib):
    g = rc.graph("micro_duplicate")
    ok = g.struct([a.ctypes.data for a in g.arrays()])
    assert lib.rc_graph_error(C.byref(ok)) is None
    for i, idx, v in ((0, (1, 2), np.nan), (5, (3, 0), np.inf), (1, 1, 5), (2, 0, 3), (2, 1, -1), (2, 1, int(g.succ[0])), (3, 0, -1), (3, 0, 2 ** 18 + 1), (4, 1, 1)):
        arrs = [x.copy() for x in g.arrays()]
        arrs[i][idx] = v
        with pytest.raises(ValueError):
            RoadGraph(*arrs)
        assert lib.rc_graph_error(C.byref(g.struct([a.ctypes.data for a in arrs]))) is not None, (i, idx, v)


@pytest.mark.parametrize("name", ("grid6",) + rc.MICRO + ("jitter8", "sparse12"))
def test_core_equals_the_port_bit_for_bit(lib, name):
    """The functions route_kernel compiles, on one lane: routes, counts, statuses, waypoint rows, xy bits - and the A*-only form."""
    g, want = rc.graph(name), rc.expected(name)
    s, e, ow, dw = rc.queries(name)
    R, G = want["route"].shape[1], want["wp_index"].shape[1]
    got = host_route(lib, g, s, e, ow, dw, R, G)
    same(got, want, name)
    rc.padded_ok(got, R, G, name)
    only = host_route(lib, g, s, e, ow, dw, R, 1, search_only=True)
    same(only, want, name + " (search only)", keys=("route", "route_len", "status"))
    assert not only["wp_index"].any() and not only["n_global"].any()


@pytest.mark.parametrize("name", ALL)
def test_heading_and_curvature_against_the_reference(lib, name):
    """theta and kappa of the expanded path against the reference's waypoint_list_2_target_path at the suite's rule for
    cal_heading_kappa, and bit for bit against emp_frenet_core.h's heading_kappa on the same xy (what emp_heading_kappa runs)."""
    from tests import host_check
    hc = host_check.load()
    f, g, want = rc.fixture(name), rc.graph(name), rc.expected(name)
    G = want["wp_index"].shape[1]
    got = host_route(lib, g, *rc.queries(name), want["route"].shape[1], G)
    for k in range(len(want["n_global"])):
        m = int(want["n_global"][k])
        gp = got["global_path"][k]
        if m < 2:
            assert not gp[:, 2:].any()
            continue
        a, b = f["path_off"][k:k + 2]
        xy = np.ascontiguousarray(gp[:m, :2])
        th, ka = np.zeros(m), np.zeros(m)
        hc.hc_heading_kappa(xy.ctypes.data, m, th.ctypes.data, ka.ctypes.data)
        assert np.array_equal(gp[:m, 2].view(np.uint64), th.view(np.uint64)) and np.array_equal(gp[:m, 3].view(np.uint64), ka.view(np.uint64))
        for mine, ref, what in ((gp[:m, 2], f["theta"][a:b], "theta"), (gp[:m, 3], f["kappa"][a:b], "kappa")):
            fin = np.isfinite(ref)
            assert_rel(mine[fin], ref[fin], RTOL, f"{name} query {k} {what}")
            assert not np.isfinite(mine[~fin]).any(), f"{name} query {k}: {what} is finite where the reference divides by zero"
    if name in rc.TOWNS:
        assert np.isfinite(f["theta"]).all() and np.isfinite(f["kappa"]).all()


@pytest.mark.parametrize("B", (1, 3, 65, 130))
def test_core_on_ragged_batches_with_short_capacities(lib, B):
    s, e, ow, dw, max_route, max_global, want = rc.ragged(B)
    got = host_route(lib, rc.graph("sparse12"), s, e, ow, dw, max_route, max_global)
    same(got, want, f"ragged {B}")
    rc.padded_ok(got, max_route, max_global, f"ragged {B}")
    if B >= 65:
        st = want["status"]
        assert (st == port.TRUNCATED).any() and (st == port.UNREACHABLE).any() and (st == port.BAD_QUERY).sum() == 4 and (st == 0).any()
        assert ((want["route_len"] == max_route + 1) & (st == port.TRUNCATED)).any() and (want["route_len"] == max_route).any()


def test_core_refuses_to_follow_bad_indices(lib):
    """What only EMP_DEVICE arrays can bring: offsets and successor indices out of range end the query with EMP_ROUTE_BAD_QUERY."""
    g = rc.graph("micro_ring_63")
    s, e, ow, dw = rc.queries("micro_ring_63")
    for i, idx, v in ((2, 0, 10 ** 6), (2, 3, -5), (1, 1, -4), (1, 2, 10 ** 6), (4, 3, 10 ** 7), (4, 2, -9)):
        arrs = [x.copy() for x in g.arrays()]
        arrs[i][idx] = v
        broken = RoadGraph.__new__(RoadGraph)
        broken.vertex, broken.succ_off, broken.succ, broken.length, broken.wp_off, broken.wp = arrs
        got = host_route(lib, broken, s, e, ow, dw, 64, 256)
        assert set(got["status"]) <= {0, port.BAD_QUERY} and (got["status"] == port.BAD_QUERY).any(), (i, idx, v)
        bad = got["status"] == port.BAD_QUERY
        assert not got["route_len"][bad].any() and not got["n_global"][bad].any() and not got["wp_index"][bad].any()
        assert not got["global_path"][bad].any()


def test_route_check_as_a_program_of_its_own(tmp_path):
    """-DROUTE_CHECK_MAIN: the self-checking program a sanitizer build runs (here: address and undefined behaviour, on the CPU)."""
    exe = str(tmp_path / "route_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DROUTE_CHECK_MAIN", SRC, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "route_check: 0 bad" in run.stdout, run.stdout + run.stderr[-2000:]


# ---- the drop-in's surface and the binding ------------------------------------------------------------------------------------------------
def test_dropin_surface_matches_the_reference_signature_fixture():
    """tests/golden/routing/signatures_global_planning.json by the rules of tests/test_cabi_and_host.py's surface test: same names,
    same argument names in order, same defaults; trailing keyword arguments with defaults may be added."""
    import importlib
    import inspect
    from tests.test_cabi_and_host import _callable_args, _same_default
    sig = json.load(open(os.path.join(rc.ROUTING, "signatures_global_planning.json")))
    assert set(sig) == {"planner/global_planning.py"}
    entry = sig["planner/global_planning.py"]
    mod = importlib.import_module(entry["dropin"])
    assert entry["scope"] == "full" and set(entry["classes"]) == {"RoadOption", "global_path_planner"} and not entry["functions"]
    problems, checked = [], 0
    for cname, methods in entry["classes"].items():
        cls = getattr(mod, cname)
        for mname, want in methods.items():
            got = _callable_args(getattr(cls, mname))
            if len(got) < len(want):
                problems.append(f"{cname}.{mname}: {len(got)} arguments, the reference has {len(want)}")
                continue
            for (gn, gd), (wn, wd) in zip(got, want):
                if gn != wn or not _same_default(gd, wd):
                    problems.append(f"{cname}.{mname}: {gn!r} = {gd!r} where the reference has {wn!r} = {wd}")
            problems += [f"{cname}.{mname}: extra argument {gn!r} without a default" for gn, gd in got[len(want):]
                         if gd is inspect.Parameter.empty and not gn.startswith("*")]
            checked += 1
    assert not problems, "\n".join(problems)
    assert checked == 9
    assert [(o.name, o.value) for o in mod.RoadOption] == [("VOID", -1), ("LEFT", 1), ("RIGHT", 2), ("STRAIGHT", 3), ("LANE_FOLLOW", 4),
                                                            ("CHANGE_LANE_LEFT", 5), ("CHANGE_LANE_RIGHT", 6)]


def test_the_package_imports_neither_networkx_nor_carla():
    code = ("import sys\nimport emplanner_carla_amd.planner, emplanner_carla_amd.routing\n"
            "from emplanner_carla_amd.planner.global_planning import global_path_planner, RoadOption\n"
            "print('LOADED', [m for m in ('networkx', 'carla') if m in sys.modules])\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert "LOADED []" in out.stdout, out.stdout + out.stderr
    from emplanner_carla_amd.planner import global_planning as gp
    assert gp.NetworkXNoPath is gp.NetworkXNoPath and gp.NetworkXNoPath.__name__ == "NetworkXNoPath"      # one class to catch
    assert gp._LocalNoPath.__name__ == "NetworkXNoPath" and issubclass(gp._LocalNoPath, Exception)
    with pytest.raises(gp.NetworkXNoPath):
        raise gp._no_path(1, 2)


def test_binding_speaks_the_header():
    text = open(os.path.join(ROOT, "include", "emplanner.h")).read()
    for name, value in (("EMP_ROUTE_MAX_NODES", L.ROUTE_MAX_NODES), ("EMP_ROUTE_UNREACHABLE", L.ROUTE_UNREACHABLE),
                        ("EMP_ROUTE_TRUNCATED", L.ROUTE_TRUNCATED), ("EMP_ROUTE_BAD_QUERY", L.ROUTE_BAD_QUERY)):
        assert f"#define {name} {value}\n" in text
    assert "#define EMP_ROUTE_MAX_LENGTH (1 << 18)" in text and L.ROUTE_MAX_LENGTH == 1 << 18
    assert (port.UNREACHABLE, port.TRUNCATED, port.BAD_QUERY) == (L.ROUTE_UNREACHABLE, L.ROUTE_TRUNCATED, L.ROUTE_BAD_QUERY)
    assert len(L.PROTOTYPES["emp_route_search"][1]) == 10 and len(L.PROTOTYPES["emp_route_paths"][1]) == 16


# ---- live: the fixtures regenerate ------------------------------------------------------------------------------------------------------------
def test_routing_fixtures_regenerate_bit_for_bit(tmp_path):
    import ref_loader
    if not ref_loader.reference_available():
        pytest.skip("the reference tree is not present")
    env = dict(os.environ, EMP_GOLDEN_OUT=str(tmp_path))
    run = subprocess.run([sys.executable, "-B", os.path.join(GOLDEN, "make_golden_routing.py")], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    committed = sorted(os.listdir(rc.ROUTING))
    assert committed == sorted(os.listdir(tmp_path / "routing")) == sorted([n + ".npz" for n in ALL] + ["signatures_global_planning.json"])
    for name in ALL:
        want, got = np.load(os.path.join(rc.ROUTING, name + ".npz")), np.load(tmp_path / "routing" / (name + ".npz"))
        assert sorted(want.files) == sorted(got.files), name
        for k in want.files:
            a, b = want[k], got[k]
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), f"{name}: {k}"
    assert json.load(open(os.path.join(rc.ROUTING, "signatures_global_planning.json"))) == \
        json.load(open(tmp_path / "routing" / "signatures_global_planning.json"))
