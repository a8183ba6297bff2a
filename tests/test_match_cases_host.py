"""CPU suite of the match scans' case tables (tests/match_cases.py): the tables say what they claim to say before the GPU suite
(tests/test_gpu_match_cases.py) relies on them.  oracle/ref_port.py (match_projection_points, find_match_points, sampling) and the
g++ build of match_scan (tests/host_check, hc_match) return the constructed label on every case; every tie is exact in bits, every
other distance is at least 1e-3 m away from the labelled one, every stop-boundary case has its deciding node at the stated offset;
a match on any other candidate index would move the Frenet outputs by at least 1e-3 relative, a thousand times what the GPU
comparison allows; and every family is present at every line length it is meant for.  No case is left out of any condition."""
from __future__ import annotations

import collections
import ctypes as C
import struct

import numpy as np
import pytest

from oracle import ref_port as op
from tests import match_cases as M
from tests import match_truth as T

GAP = 1e-3              # metres between the labelled distance and every other one that is not an exact tie
MARGIN = 1e-3           # relative move of an output under any other candidate index: 1000 x the GPU suite's 1e-6


def bits(v):
    return struct.pack("<d", float(v))


@pytest.fixture(scope="module")
def hc():
    from tests import host_check
    return host_check.load()


def hc_match(hc, nodes, n, q, first, step, limit):
    line = np.ascontiguousarray(nodes, np.float64)
    return hc.hc_match(line.ctypes.data, int(n), float(q[0]), float(q[1]), int(first), int(step), int(limit))


def test_the_port_and_the_host_scan_return_every_whole_line_label(hc):
    seen = 0
    for c in M.whole_line():
        nodes, q = T.node_list(c["nodes"]), tuple(float(v) for v in c["q"])
        with np.errstate(all="ignore"):
            assert int(op.match_projection_points([q], nodes)[0][0]) == c["label"], c["name"]
            assert int(op.find_match_points([q], nodes, True, 0)[0][0]) == c["label"], c["name"]
        assert hc_match(hc, c["nodes"], c["P"], q, 0, 1, M.LIMIT) == c["label"], c["name"]
        seen += 1
    assert seen == len(M.whole_line()) >= 300


def test_the_port_and_the_host_scan_return_every_windowed_label(hc):
    seen = collections.Counter()
    for c in M.windowed():
        if not c["in_range"]:
            assert c["label"] == -1, c["name"]                      # the library's contract where the reference raises IndexError
            seen["out"] += 1
            continue
        n = c["n_ref"]
        nodes, q = T.node_list(c["nodes"][:n]), tuple(float(v) for v in c["q"])
        with np.errstate(all="ignore"):
            assert int(op.find_match_points([q], nodes, False, c["st"])[0][0]) == c["label"], c["name"]
            px, py, th = nodes[c["st"]][:3]
            flag = np.dot(np.array([q[0] - px, q[1] - py]), np.array([np.cos(th), np.sin(th)]))
        if c["name"] == "flag_minus_zero":
            assert flag == 0.0 and np.cos(th) < 0.0 and np.sin(th) < 0.0 and q[0] - px == 0.0 and q[1] - py == 0.0
        if c["flag"] is not None:
            assert bits(flag) == bits(c["flag"]), (c["name"], float(flag).hex())       # the sign of a zero included
        assert hc_match(hc, c["nodes"], n, q, c["st"], 1 if flag > 0.0 else -1, M.WINDOW_LIMIT) == c["label"], c["name"]
        seen["fwd" if flag > 0.0 else "back"] += 1
    assert sum(seen.values()) == len(M.windowed()) and min(seen["fwd"], seen["back"]) >= 8 and seen["out"] >= 5


def test_the_port_returns_every_window_label():
    firsts = collections.defaultdict(set)
    for c, (status, n_ref, line) in zip(M.window(), T.window_truth()):
        G = c["G"]                                                  # (a count beyond the row's capacity: the row's G nodes)
        nodes, q = T.node_list(c["path"]), tuple(float(v) for v in c["q"])
        assert int(op.find_match_points([q], nodes, bool(c["first_run"]), c["st"] if not c["first_run"] else 0)[0][0]) == c["label"] == c["m"]
        if G < M.REF_POINTS:
            assert c["first"] is None and status == 2 and n_ref == 0 and not line.any(), c["name"]
            continue
        win = op.sampling(c["label"], nodes)
        assert win == nodes[c["first"]:c["first"] + M.REF_POINTS] and len(win) == M.REF_POINTS, c["name"]
        assert 0 <= c["first"] <= c["m"] <= c["first"] + M.REF_POINTS - 1
        assert status == 0 and n_ref == M.REF_POINTS and np.isfinite(line).all()
        firsts[G].add(c["first"])
    assert firsts[51] == {0} and firsts[52] == {0, 1} and firsts[140] >= {0, 1, 88, 89}
    assert {c["G"] for c in M.window()} == set(M.WINDOW_G)
    for G in M.WINDOW_G:
        for first_run in (0, 1):
            assert {c["m"] for c in M.window() if c["G"] == G and c["first_run"] == first_run and c["n_global"] == G} == \
                {0, 9, 10, 11, G - 42, G - 41, G - 40, G - 1}
    assert sum(c["n_global"] > M.MAX_GLOBAL for c in M.window()) == 2


def test_ties_are_exact_and_every_other_distance_is_clear_of_the_label():
    tied_cases = widest = checked = 0
    for c in M.whole_line():
        d = M.distances(c)
        lab = c["label"]
        if c["tied"]:
            assert lab == min(c["tied"]), c["name"]
            assert len({bits(d[i]) for i in c["tied"]}) == 1, c["name"]
            assert len({tuple(c["nodes"][i, 2:]) for i in c["tied"]}) == len(c["tied"]), c["name"]       # every node its own heading
            tied_cases += 1
            widest = max(widest, len(c["tied"]))
        if not np.isfinite(d[lab]):
            assert not c["finite"] and lab == 0 and c["family"] == "nonfinite", c["name"]
            assert not (d[:min(M.LIMIT, c["P"])] < np.inf).any(), c["name"]              # the first `limit` distances: none is `< inf`
            checked += 1
            continue
        for i in range(c["P"]):
            if i != lab and i not in c["tied"] and np.isfinite(d[i]):
                assert abs(d[i] - d[lab]) >= GAP, (c["name"], i)
        checked += 1
    assert checked == len(M.whole_line()) and tied_cases >= 8 * len(M.P_ALL) and widest == max(M.P_ALL)
    for c in M.windowed():
        if c["in_range"] and c["name"].startswith("tie_"):
            d = M.distances(dict(nodes=c["nodes"][:c["n_ref"]], q=c["q"]))
            assert int((d == d[c["label"]]).sum()) >= 2 and d[c["label"]] == np.nanmin(d), c["name"]


def test_every_stop_boundary_case_has_its_deciding_node_at_the_stated_offset():
    seen = collections.Counter()
    for c in M.whole_line():
        if c["stop"] is None:
            assert c["family"] in ("ties", "nonfinite"), c["name"]
            continue
        L, off, taken = c["stop"]
        d = M.distances(c)
        reach = L - 49 if "two_stage" in c["kind"] else L                     # two stages: L is the improvement 49 behind the first minimum
        assert (np.diff(d[:reach + 1]) < 0).all(), c["name"]                   # the scan gets there: every node before it improves
        assert reach == L or (d[L] + GAP <= d[reach] and (d[reach + 1:L] >= d[reach] + GAP).all()), c["name"]
        if taken is None:                                                      # never stops: the line ends first
            assert c["P"] - 1 - L < M.LIMIT and c["label"] == L and (d[L + 1:] > d[L]).all(), c["name"]
            seen["never"] += 1
            continue
        decider = L + off
        assert decider <= c["P"] - 1 and d[decider] + GAP <= d[L] and (d[L + 1:decider] >= d[L] + GAP).all(), c["name"]
        assert taken == (off <= M.LIMIT) and c["label"] == (decider if taken else L), c["name"]
        seen[(L + M.LIMIT, off) if c["kind"].startswith("stop") and "two" not in c["kind"] else c["kind"]] += 1
    for node in M.STOP_NODES:
        assert seen[node, 49] >= 1 and seen[node, 50] >= 1 and seen[node, 51] >= 1, (node, seen)
    assert all(seen[f"stop{node}_two_stage"] >= 1 for node in (50, 63, 64)) and seen["hairpin"] >= 9 and seen["never"] == len(M.P_ALL)


def _moved(a, b):
    """|a - b| relative to the larger of the two, 1 at the least: how far an output moves, in units the 1e-6 comparison uses."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    assert np.array_equal(np.isnan(a), np.isnan(b))                 # (behind a NaN node the chord sums are NaN in both)
    keep = ~np.isnan(a)
    return float(np.max(np.abs(a - b)[keep] / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1.0)[keep]))


def test_any_other_candidate_index_moves_the_frenet_outputs():
    checked = pairs = 0
    smallest = np.inf
    for c in M.whole_line():
        if not c["finite"]:
            continue
        want = T.forced(c, c["label"])
        for idx in c["candidates"]:
            if not np.isfinite(c["nodes"][idx]).all():
                continue
            other = T.forced(c, idx)
            for k in ("s_map", "s"):
                smallest = min(smallest, _moved(other[k], want[k]))
                assert _moved(other[k], want[k]) >= MARGIN, (c["name"], idx, k)
            pairs += 1
        assert len(c["candidates"]) >= 1, c["name"]
        checked += 1
    assert checked == sum(c["finite"] for c in M.whole_line()) and pairs >= 2 * checked - 40
    # a hairpin's two candidates are more than 100 m of s apart
    for c in M.whole_line():
        if c["kind"] == "hairpin":
            far = c["stop"][0] + c["stop"][1]
            assert abs(T.forced(c, far)["s"] - T.forced(c, 8)["s"]) > 100.0, c["name"]


def test_the_projection_scenes_see_the_match_through_s_and_l():
    """In every role the port's outputs on the case differ from its outputs with the scan's answer replaced by a candidate - checked
    on the outputs of the whole call: the s_map under the origin role, begin (s, l) under the start role, obs_s under the obstacle roles."""
    for role, key in (("origin", "s_map"), ("start", "begin"), ("obs_slot0", "obs_s")):
        truth = T.projection_truth(role)
        assert len(truth) == len(M.whole_line())
        for c, t in zip(M.whole_line(), truth):
            if not c["finite"]:
                continue
            want = T.forced(c, c["label"])
            got = {"s_map": t["s_map"], "begin": t["begin"][0], "obs_s": t["obs_s"][0]}[key]
            # the role's own output is the forced-label value (the other points sit on the labelled node: the origin there makes
            # s_map[label] = 0, so s of the query is the projection term alone)
            if key == "s_map":
                assert _moved(got, want["s_map"]) <= 1e-12, c["name"]
            else:
                assert abs(got - want["s"]) <= 1e-12 * max(1.0, abs(got)), c["name"]


def test_coverage_of_families_and_line_lengths():
    by = collections.defaultdict(set)
    for c in M.whole_line():
        by[c["P"]].add(c["kind"])
        assert c["nodes"].shape == (c["P"], 4) and 0 <= c["label"] < c["P"] and c["family"] in M.FAMILIES
    assert set(by) == set(M.P_ALL)
    common = {"tie2", "tie3", "tie51", "whole", "seam15_16", "seam31_32", "seam47_48", "stop50_plus49", "stop50_plus50", "never_stops",
              "last_node_improves", "query_nan", "query_inf", "nan_before_min", "nan_at_min", "nan_after_min", "inf_x_at_min", "nan_first49",
              "nan_first50", "inf_first50", "nan_all"}
    for P in M.P_ALL:
        assert common <= by[P], (P, common - by[P])
        assert ("stop50_plus51" in by[P]) == (P >= 52) and ("hairpin" in by[P]) == (P >= 63)
        assert ("seam63_64" in by[P]) == (P >= 65) and ("seam127_128" in by[P]) == (P >= 129)
        assert ("stop63_plus50" in by[P]) == (P >= 64) and ("stop64_plus50" in by[P]) == (P >= 65) and ("stop64_plus51" in by[P]) == (P >= 66)
        assert ("stop127_plus50" in by[P]) == (P >= 128) and ("stop128_plus50" in by[P]) == (P >= 129) and ("stop128_plus51" in by[P]) == (P >= 130)
        assert ("stop50_two_stage" in by[P]) == (P >= 101)
    shifted = sum(bool(c["q"][0] == M.OFFSET[0]) for c in M.whole_line())
    assert 0.3 < shifted / len(M.whole_line()) < 0.7
    names = {c["name"] for c in M.windowed()}
    assert {"flag_plus_zero", "flag_minus_zero", "flag_plus_ulp", "flag_minus_ulp", "flag_nan", "backward_from_0", "forward_from_last",
            "forward_after_4", "forward_after_5", "backward_after_4", "backward_after_5", "tie_forward", "tie_backward", "st_minus_1",
            "st_equals_P", "empty_line", "flag_positive_ignores_the_back", "flag_negative_ignores_the_front"} <= names
