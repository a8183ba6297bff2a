"""GPU suite of global routing on the hostile graphs of tests/route_hard_cases.py, through the C-ABI on 0xCC-poisoned outputs, with
EMP_HOST arrays and with EMP_DEVICE tensors: every case against the Python port (routes, counts, statuses, waypoint rows, xy in
bits, theta and kappa the bits of Planner.heading_kappa, every unused slot 0), emp_route_search on the same queries, one long
query alone and inside batches of 65 and 130, a sweep of both capacities across the 64-lane strides and the true lengths, and the
4096-node chain whose g reaches 4095 * 2^18.  The port's answers are computed once (route_hard_cases.solved caches them); what
the port itself is held to - the reference's recorded answers - is tests/test_route_hard_host.py's."""
from __future__ import annotations

import numpy as np
import pytest

from emplanner_carla_amd import _lib as L
from tests import route_hard_cases as hc
from tests import route_port as port
from tests.conftest import make_planner
from tests.test_gpu_routing import KEYS, as_dict, bits, check, raw_paths

pytestmark = pytest.mark.gpu
MODES = [(n, d) for n in hc.PORTED for d in (False, True) if d or n not in hc.DEVICE_ONLY]


@pytest.fixture(scope="module")
def planner():
    pl = make_planner()
    yield pl
    pl.close()


def search_only(planner, g, s, e, R, device):
    if device:
        import torch
        s, e = torch.from_numpy(np.ascontiguousarray(s)).cuda(), torch.from_numpy(np.ascontiguousarray(e)).cuda()
    r = as_dict(planner.route_search(g, s, e, R))
    if device:
        import torch
        torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("name,device", MODES, ids=[f"{n}-{'device' if d else 'host'}" for n, d in MODES])
def test_hard_cases_equal_the_port(planner, name, device):
    g, (s, e, ow, dw) = hc.case(name)
    want = hc.solved(name)[0]
    R, G = want["route"].shape[1], want["wp_index"].shape[1]
    got = raw_paths(planner, g, s, e, ow, dw, R, G, device)
    check(planner, got, want, name)
    only = search_only(planner, g, s, e, R, device)                  # emp_route_search: the route part of emp_route_paths
    for k in ("route", "route_len", "status"):
        np.testing.assert_array_equal(only[k], got[k], err_msg=f"{name}: emp_route_search {k}")


def long_query():
    """a query of deep_wp with more than 130 waypoints and a route of at least four nodes: the one with the longest path"""
    want = hc.solved("deep_wp")[0]
    ok = np.nonzero((want["n_global"] > 130) & (want["route_len"] >= 4))[0]
    assert len(ok)
    return int(ok[np.argmax(want["n_global"][ok])])


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_one_query_alone_and_in_batches_of_65_and_130(planner, device):
    """the same bytes each time, wherever the query stands among the others"""
    g, (s, e, ow, dw) = hc.case("deep_wp")
    want = hc.solved("deep_wp")[0]
    q = long_query()
    R, G = want["route"].shape[1], want["wp_index"].shape[1]
    alone = raw_paths(planner, g, s[q:q + 1], e[q:q + 1], ow[q:q + 1], dw[q:q + 1], R, G, device)
    check(planner, alone, {k: v[q:q + 1] for k, v in want.items()}, "deep_wp alone")
    assert alone["n_global"][0] > 130
    for B, at in ((65, 64), (130, 71)):
        pick = np.arange(B) % len(s)
        pick[at] = q
        batch = raw_paths(planner, g, s[pick], e[pick], ow[pick], dw[pick], R, G, device)
        for k in KEYS:
            assert np.array_equal(batch[k][at:at + 1].view(np.uint8), alone[k].view(np.uint8)), f"batch of {B}: {k} of the query differs"
        check(planner, batch, {k: v[pick] for k, v in want.items()}, f"deep_wp batch of {B}")


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_capacity_sweep(planner, device):
    """max_global on either side of one stride and of the true count, max_route down to 2: the written prefix is the full answer's,
    EMP_ROUTE_TRUNCATED exactly when a capacity is short, the counts the true ones, theta and kappa those of the shorter xy."""
    g, (s, e, ow, dw) = hc.case("deep_wp")
    want = hc.solved("deep_wp")[0]
    q = long_query()
    n, ln = int(want["n_global"][q]), int(want["route_len"][q])
    one = [a[q:q + 1] for a in (s, e, ow, dw)]
    full = raw_paths(planner, g, *one, ln, n, device)
    assert full["status"][0] == 0
    for max_global in (1, 2, 63, 64, 65, n - 1, n, n + 1):
        for max_route in (2, ln - 1, ln):
            what = f"max_global {max_global} max_route {max_route}"
            got = raw_paths(planner, g, *one, max_route, max_global, device)
            check(planner, got, port.run(g, *one, max_route, max_global), what)
            short = max_global < n or max_route < ln
            assert got["status"][0] == (L.ROUTE_TRUNCATED if short else 0), what
            assert got["route_len"][0] == ln and got["n_global"][0] == n, what
            m = min(max_global, n)
            np.testing.assert_array_equal(got["route"][0, :min(max_route, ln)], full["route"][0, :min(max_route, ln)], err_msg=what)
            np.testing.assert_array_equal(got["wp_index"][0, :m], full["wp_index"][0, :m], err_msg=what)
            assert np.array_equal(bits(got["global_path"][0, :m, :2]), bits(full["global_path"][0, :m, :2])), what
            if max_global < 2:
                assert not bits(got["global_path"][0, :, 2:]).any(), what          # no heading below 2 points


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_long_chain_at_the_node_limit(planner, device):
    """4096 nodes, every length 2^18: g reaches 4095 * 2^18 and stays an int32; the answer is written down, not searched"""
    from tests.test_route_hard_host import check_chain
    g, (s, e, ow, dw), want = hc.chain_long()
    n = g.n_nodes
    got = raw_paths(planner, g, s, e, ow, dw, n, n, device)
    check_chain(got, g, want)
    only = search_only(planner, g, s, e, n, device)
    for k in ("route", "route_len", "status"):
        np.testing.assert_array_equal(only[k], got[k], err_msg=f"emp_route_search {k}")
