"""The three forms of the nearest-node match scan - the serial match_scan (emp_frenet_core.h), the value-only wave scan for lines of
at most 64 nodes and the chunked wave scan (emp_tail_kernels.h) - on the tables of tests/match_cases.py: exact ties (the first wins),
the stop after 50 (5) consecutive non-improvements one node either side of it, a local minimum that is not the global one,
non-finite nodes and queries, the windowed search's direction at flag = +-0, one ulp and NaN, and the 51-node window at either end
of a global path.  Indices equal the constructed labels exactly; projections and Frenet outputs agree with oracle/ref_port.py
within 1e-6 (the tolerance contract at the top of emp_frenet_core.h) and are NaN where the port's are; the wave forms agree with
the chain of serial kernels on the same arrays; and every scene gives the same bits alone, in the batch, in the reversed batch,
from host arrays and device tensors, and whatever lies behind its counts.  tests/test_match_cases_host.py shows that a match on
any other candidate index moves these outputs by at least 1e-3 relative."""
import functools

import numpy as np
import pytest

from oracle import ref_port as op
from tests import match_cases as M
from tests import match_truth as T
from tests.conftest import assert_rel

pytestmark = pytest.mark.gpu

RTOL = 1e-6                      # emp_frenet_core.h: device sin / cos / atan2 differ from libm in the last ulp
POISONS = ("nan", "hostile")
WIN_WIDTH = M.WP + 4             # the windowed lines in rows with four slots of padding


@pytest.fixture(scope="module")
def planner():
    from tests.conftest import make_planner
    p = make_planner(0)
    yield p
    p.close()


def close(got, want, what):
    """Within RTOL where the port is finite; NaN where it is NaN; the same infinity where it is infinite."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    fin = np.isfinite(want)
    assert np.isnan(got[np.isnan(want)]).all(), f"{what}: the port is NaN, the device is not"
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)]), f"{what}: the port is infinite"
    assert_rel(got[fin], want[fin], RTOL, what)


def same_bits(a, b, what):
    assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), what


# ---- the whole-line table as arrays ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def line_rows(poison):
    cs = M.whole_line()
    ref = M.padded([c["nodes"] for c in cs], [c["P"] for c in cs], M.MAX_REF, poison, [c["q"] for c in cs])
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def line_arrays():
    cs = M.whole_line()
    out = dict(n_ref=np.array([c["P"] for c in cs], np.int32), q=np.stack([c["q"] for c in cs]), label=np.array([c["label"] for c in cs], np.int32),
               benign=np.stack([c["nodes"][c["label"], :2] for c in cs]), one=np.ones(len(cs), np.int32))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def port_projections():
    """match_projection_points of every whole-line case: the projection of the query on the labelled node."""
    out = []
    with np.errstate(all="ignore"):
        for c in M.whole_line():
            match, proj = op.match_projection_points([tuple(float(v) for v in c["q"])], T.node_list(c["nodes"]))
            assert int(match[0]) == c["label"]
            out.append(np.array(proj[0], np.float64))
    return np.stack(out)


@pytest.mark.parametrize("poison", POISONS)
def test_serial_scan_indices_are_the_labels_and_projections_the_ports(planner, poison):
    a, ref = line_arrays(), line_rows(poison)
    xy = a["q"][:, None, :]
    B = len(a["label"])
    mi, pr = planner.match_projection(ref, a["n_ref"], xy, a["one"])
    bad = np.nonzero(mi[:, 0] != a["label"])[0]
    assert bad.size == 0, [(M.whole_line()[b]["name"], int(mi[b, 0]), int(a["label"][b])) for b in bad[:8]]
    close(pr[:, 0], port_projections(), "match_projection: projection")
    # find_match_points on a first run is the same scan; pre_match_index is not looked at
    mi2, pr2 = planner.find_match_points(ref, a["n_ref"], xy, a["one"], np.ones(B, np.int32), np.full(B, -5, np.int32))
    same_bits(mi2, mi, "find_match_points (first run): index")
    same_bits(pr2, pr, "find_match_points (first run): projection")


def _windowed_arrays(poison):
    cs = M.windowed()
    ref = M.padded([c["nodes"] for c in cs], [c["n_ref"] for c in cs], WIN_WIDTH, poison, [c["q"] for c in cs])
    return (ref, np.array([c["n_ref"] for c in cs], np.int32), np.stack([c["q"] for c in cs]), np.array([c["st"] for c in cs], np.int32),
            np.array([c["label"] for c in cs], np.int32))


@pytest.mark.parametrize("poison", POISONS)
def test_windowed_search_direction_limit_and_ends(planner, poison):
    cs = M.windowed()
    ref, n_ref, q, st, label = _windowed_arrays(poison)
    B = len(cs)
    mi, pr = planner.find_match_points(ref, n_ref, q[:, None, :], np.ones(B, np.int32), np.zeros(B, np.int32), st)
    bad = np.nonzero(mi[:, 0] != label)[0]
    assert bad.size == 0, [(cs[b]["name"], int(mi[b, 0]), int(label[b])) for b in bad]
    for b, c in enumerate(cs):
        if not c["in_range"]:
            assert np.isnan(pr[b, 0]).all(), c["name"]
            continue
        with np.errstate(all="ignore"):
            _, proj = op.find_match_points([tuple(float(v) for v in c["q"])], T.node_list(c["nodes"][:c["n_ref"]]), False, c["st"])
        close(pr[b, 0], np.array(proj[0], np.float64), f"{c['name']}: projection")


@pytest.mark.parametrize("poison", POISONS)
def test_serial_s_map_and_s_l_follow_the_match(planner, poison):
    a, ref = line_arrays(), line_rows(poison)
    cs = M.whole_line()
    sm = planner.s_map(ref, a["n_ref"], a["q"])                         # the query as origin of the s axis
    for b, (c, t) in enumerate(zip(cs, T.projection_truth("origin"))):
        close(sm[b, :c["P"]], t["s_map"], f"{c['name']}: s_map")
    sm0 = planner.s_map(ref, a["n_ref"], a["benign"])                   # the origin on the labelled node, the query as a point
    s, l = planner.s_l(ref, sm0, a["n_ref"], a["q"][:, None, :], a["one"])
    want = np.stack([t["begin"] for t in T.projection_truth("start")])
    close(s[:, 0], want[:, 0], "s_l: s")
    close(l[:, 0], want[:, 1], "s_l: l")
    assert sum(c["finite"] for c in cs) >= 250 and np.isfinite(want[[c["finite"] for c in cs]]).all()


# ---- the projection kernel: both wave forms ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def role_arrays(role):
    cs = M.whole_line()
    sc = [T.scene(c, role) for c in cs]
    B = len(cs)
    out = dict(origin=np.stack([s["origin"] for s in sc]), start=np.stack([s["start"] for s in sc]), obs=np.stack([s["obs"] for s in sc]),
               n_obs=np.array([s["n_obs"] for s in sc], np.int32), v=np.tile(np.array(T.START_V), (B, 1)), a=np.tile(np.array(T.START_A), (B, 1)))
    for v in out.values():
        v.setflags(write=False)
    return out


def _project(planner, ref, n_ref, r, idx=slice(None), to=lambda x: x):
    return planner.frenet_project(ref_line=to(ref[idx]), n_ref=to(n_ref[idx]), origin_xy=to(r["origin"][idx]), start_xy=to(r["start"][idx]),
                                  start_v=to(r["v"][idx]), start_a=to(r["a"][idx]), obs_xy=to(r["obs"][idx]), n_obs=to(r["n_obs"][idx]))


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("role", [r for r, _ in T.ROLES])
def test_projection_kernel_against_the_port_and_the_serial_chain(planner, role, poison):
    a, ref, r = line_arrays(), line_rows(poison), role_arrays(role)
    cs, truth = M.whole_line(), T.projection_truth(role)
    sm, os_, ol_, bsl, start = _project(planner, ref, a["n_ref"], r)
    # the chain of the serial kernels on the same arrays
    sm2 = planner.s_map(ref, a["n_ref"], r["origin"])
    os2, ol2 = planner.s_l(ref, sm2, a["n_ref"], r["obs"], r["n_obs"])
    bs2, bl2 = planner.s_l(ref, sm2, a["n_ref"], r["start"][:, None, :], a["one"])
    nan_match = 0
    for b, (c, t) in enumerate(zip(cs, truth)):
        P = c["P"]
        for got, want, what in ((sm[b, :P], t["s_map"], "s_map"), (os_[b], t["obs_s"], "obs_s"), (ol_[b], t["obs_l"], "obs_l"),
                                (bsl[b], t["begin"], "begin_sl"), (start[b], t["start"], "start")):
            close(got, want, f"{c['name']} as {role}: {what} against the port")
        for got, want, what in ((sm[b, :P], sm2[b, :P], "s_map"), (os_[b], os2[b], "obs_s"), (ol_[b], ol2[b], "obs_l"),
                                (bsl[b], [bs2[b, 0], bl2[b, 0]], "begin_sl")):
            close(got, want, f"{c['name']} as {role}: {what} against s_map -> s_l")
        if np.isnan(c["nodes"][c["label"], :2]).any():                 # the matched node is NaN: both forms say NaN
            nan_match += 1
            assert np.isnan(sm[b, :P]).all() and np.isnan(sm2[b, :P]).all() and np.isnan(bsl[b]).all() and np.isnan([bs2[b, 0], bl2[b, 0]]).all()
    assert nan_match == 2 * len(M.P_ALL)


# ---- the front end of the cycle --------------------------------------------------------------------------------------------
def _window_arrays(poison):
    cs = M.window()
    gp = M.padded([c["path"] for c in cs], [c["G"] for c in cs], M.MAX_GLOBAL, poison, [c["q"] for c in cs])
    return (gp, np.array([c["n_global"] for c in cs], np.int32), np.stack([c["q"] for c in cs]), np.array([c["st"] for c in cs], np.int32),
            np.array([c["first_run"] for c in cs], np.int32))


@pytest.mark.parametrize("poison", POISONS)
def test_reference_line_window_at_either_end_of_the_path(planner, poison):
    from emplanner_carla_amd.api import smooth_params
    cs, truth = M.window(), T.window_truth()
    gp, n_global, q, st, first = _window_arrays(poison)
    ref, n_ref, mi, it, status = planner.reference_line(smooth_params(), gp, n_global, q, st, first)
    for b, (c, (want_status, want_n, line)) in enumerate(zip(cs, truth)):
        assert mi[b] == c["label"] and status[b] == want_status and n_ref[b] == want_n, (c["name"], int(mi[b]), int(status[b]), int(n_ref[b]))
        if want_n == 0:
            assert not ref[b].any(), c["name"]
            continue
        assert_rel(ref[b, :, :2], line[:, :2], RTOL, f"{c['name']}: reference line xy")       # one node off is 2 m off
        assert_rel(ref[b, :, 2], line[:, 2], RTOL, f"{c['name']}: theta")
        assert_rel(ref[b, :, 3], line[:, 3], RTOL, f"{c['name']}: kappa")
    assert sum(t[1] == 0 for t in truth) == sum(c["G"] < M.REF_POINTS for c in cs) >= 12


@pytest.mark.parametrize("poison", POISONS)
def test_reference_line_runs_the_windowed_search(planner, poison):
    """The windowed table through the front end (match_scan on lane 0, limit 5).  Its lines are distance profiles, not roads: the
    match index is exact; of the status only EMP_ST_S_OUT_OF_RANGE is looked at, which does not depend on the smoothing."""
    from emplanner_carla_amd.api import smooth_params
    cs = M.windowed()
    ref, n_ref, q, st, label = _windowed_arrays(poison)
    _, _, mi, _, status = planner.reference_line(smooth_params(), ref, n_ref, q, st, np.zeros(len(cs), np.int32))
    for b, c in enumerate(cs):
        assert mi[b] == max(c["label"], 0), (c["name"], int(mi[b]))                           # a refused search reports node 0
        assert bool(status[b] & 2) == (not c["in_range"] or c["n_ref"] < M.REF_POINTS), (c["name"], int(status[b]))


def test_cycle_from_the_global_path_matches_like_the_two_call_form(planner):
    """The window table's windowed rows through emp_plan_cycle with emp_cycle_io.global_path: match index and front-end status equal
    emp_reference_line's bit for bit (the fused front end is always windowed)."""
    from emplanner_carla_amd.api import dp_params, qp_params, smooth_params
    gp, n_global, q, st, first = _window_arrays("nan")
    rows = np.nonzero(first == 0)[0]
    B = len(rows)
    _, _, mi, _, status = planner.reference_line(smooth_params(), gp[rows], n_global[rows], q[rows], st[rows], first[rows])
    res = planner.plan_cycle(dp_params(), qp_params(), smooth_params(), None, None, origin_xy=q[rows], start_xy=q[rows],
                             start_v=np.tile(np.array(T.START_V), (B, 1)), start_a=np.tile(np.array(T.START_A), (B, 1)),
                             obs_xy=np.zeros((B, 1, 2)), n_obs=np.zeros(B, np.int32), global_path=gp[rows], n_global=n_global[rows],
                             pre_match_index=st[rows])
    planner.synchronize()
    same_bits(res.match_index, mi, "match_index")
    same_bits(res.ref_status, status, "ref_status")
    assert np.array_equal(mi, [M.window()[b]["label"] for b in rows])
    assert np.array_equal(status != 0, [M.window()[b]["G"] < M.REF_POINTS for b in rows]) and 6 <= (status != 0).sum() < B


# ---- batch invariance: bit for bit -------------------------------------------------------------------------------------------
def test_every_scene_alone_in_the_batch_and_in_the_reversed_batch(planner):
    a, ref = line_arrays(), line_rows("nan")
    B = len(a["label"])
    xy = a["q"][:, None, :]
    r = role_arrays("obs_slot64")
    rev = np.arange(B)[::-1]
    mi, pr = planner.match_projection(ref, a["n_ref"], xy, a["one"])
    mir, prr = planner.match_projection(ref[rev], a["n_ref"][rev], xy[rev], a["one"])
    same_bits(mir[rev], mi, "match_projection reversed: index")
    same_bits(prr[rev], pr, "match_projection reversed: projection")
    batch = _project(planner, ref, a["n_ref"], r)
    for x, y in zip(_project(planner, ref, a["n_ref"], r, rev), batch):
        same_bits(x[rev], y, "frenet_project reversed")
    for b in range(B):
        one = slice(b, b + 1)
        m1, p1 = planner.match_projection(ref[one], a["n_ref"][one], xy[one], a["one"][one])
        assert m1[0, 0] == mi[b, 0] and np.array_equal(p1[0], pr[b], equal_nan=True), M.whole_line()[b]["name"]
        P = int(a["n_ref"][b])
        for x, y, n in zip(_project(planner, ref, a["n_ref"], r, one), batch, (P, 65, 65, 2, 4)):
            assert np.array_equal(x[0, :n], y[b, :n], equal_nan=True), M.whole_line()[b]["name"]
    # the windowed search and the front end
    from emplanner_carla_amd.api import smooth_params
    wref, wn, wq, wst, _ = _windowed_arrays("nan")
    W = len(wn)
    zero, ones = np.zeros(W, np.int32), np.ones(W, np.int32)
    wm, wp = planner.find_match_points(wref, wn, wq[:, None, :], ones, zero, wst)
    wrev = np.arange(W)[::-1]
    wmr, wpr = planner.find_match_points(wref[wrev], wn[wrev], wq[wrev][:, None, :], ones, zero, wst[wrev])
    same_bits(wmr[wrev], wm, "find_match_points reversed: index")
    same_bits(wpr[wrev], wp, "find_match_points reversed: projection")
    gp, ng, gq, gst, gfirst = _window_arrays("nan")
    full = planner.reference_line(smooth_params(), gp, ng, gq, gst, gfirst)
    grev = np.arange(len(ng))[::-1]
    for x, y in zip(planner.reference_line(smooth_params(), gp[grev], ng[grev], gq[grev], gst[grev], gfirst[grev]), full):
        same_bits(x[grev], y, "reference_line reversed")
    for b in range(W):
        one = slice(b, b + 1)
        m1, p1 = planner.find_match_points(wref[one], wn[one], wq[one][:, None, :], ones[one], zero[one], wst[one])
        assert m1[0, 0] == wm[b, 0] and np.array_equal(p1[0], wp[b], equal_nan=True), M.windowed()[b]["name"]
    for b in range(len(ng)):
        one = slice(b, b + 1)
        for x, y in zip(planner.reference_line(smooth_params(), gp[one], ng[one], gq[one], gst[one], gfirst[one]), full):
            assert np.array_equal(x[0], y[b], equal_nan=True), M.window()[b]["name"]


def test_host_arrays_and_device_tensors_give_the_same_bits(planner):
    import torch
    from emplanner_carla_amd.api import smooth_params
    dev = lambda x: torch.from_numpy(np.array(x)).cuda()

    def host(xs):
        planner.synchronize()
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in xs]

    a, ref = line_arrays(), line_rows("hostile")
    xy = np.ascontiguousarray(a["q"][:, None, :])
    for x, y in zip(host(planner.match_projection(dev(ref), dev(a["n_ref"]), dev(xy), dev(a["one"]))), planner.match_projection(ref, a["n_ref"], xy, a["one"])):
        same_bits(x, y, "match_projection")
    for role in ("start", "obs_last"):
        r = role_arrays(role)
        for x, y in zip(host(_project(planner, ref, a["n_ref"], r, to=dev)), _project(planner, ref, a["n_ref"], r)):
            same_bits(x, y, f"frenet_project, {role}")
    wref, wn, wq, wst, _ = _windowed_arrays("hostile")
    W = len(wn)
    args = (wref, wn, np.ascontiguousarray(wq[:, None, :]), np.ones(W, np.int32), np.zeros(W, np.int32), wst)
    for x, y in zip(host(planner.find_match_points(*map(dev, args))), planner.find_match_points(*args)):
        same_bits(x, y, "find_match_points")
    gargs = _window_arrays("hostile")
    for x, y in zip(host(planner.reference_line(smooth_params(), *map(dev, gargs))), planner.reference_line(smooth_params(), *gargs)):
        same_bits(x, y, "reference_line")


def test_what_lies_behind_the_counts_changes_no_bit(planner):
    from emplanner_carla_amd.api import smooth_params
    a = line_arrays()
    xy = a["q"][:, None, :]
    n_ref = a["n_ref"]
    for x, y in zip(planner.match_projection(line_rows("nan"), n_ref, xy, a["one"]), planner.match_projection(line_rows("hostile"), n_ref, xy, a["one"])):
        same_bits(x, y, "match_projection")
    for role, _ in T.ROLES:
        r = role_arrays(role)
        for k, (x, y) in enumerate(zip(_project(planner, line_rows("nan"), n_ref, r), _project(planner, line_rows("hostile"), n_ref, r))):
            if k == 0:                                                   # s_map: the line's own P entries
                for b in range(len(n_ref)):
                    same_bits(x[b, :n_ref[b]], y[b, :n_ref[b]], f"frenet_project, {role}: s_map")
            else:
                same_bits(x, y, f"frenet_project, {role}")
    W = len(M.windowed())
    outs = []
    for poison in POISONS:
        wref, wn, wq, wst, _ = _windowed_arrays(poison)
        outs.append(planner.find_match_points(wref, wn, wq[:, None, :], np.ones(W, np.int32), np.zeros(W, np.int32), wst))
    for x, y in zip(*outs):
        same_bits(x, y, "find_match_points")
    for x, y in zip(planner.reference_line(smooth_params(), *_window_arrays("nan")), planner.reference_line(smooth_params(), *_window_arrays("hostile"))):
        same_bits(x, y, "reference_line")
