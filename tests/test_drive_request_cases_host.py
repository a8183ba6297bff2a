"""CPU suite of the drive request's case table (tests/drive_request_cases.py): the table says what it claims to say before the GPU
suite (tests/test_gpu_drive_request_cases.py) relies on it.  tests/drive_port.py reproduces every constructed label; on the
threshold family each probed decision variable has exactly the bits written down and exact rational arithmetic on the inputs agrees
with the float decision; tied distances are bit-equal; outside the threshold family no finite decision variable comes within 1e-9 of
its threshold, for every case (none is left out); and the table covers every family, both sides of every comparison, every listed
n_act and kept count, and truncation on and off."""
from __future__ import annotations

import collections
import math
import os
import struct
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import drive_port as port  # noqa: E402
import drive_request_cases as D  # noqa: E402

CONFIGS = ((1, 1), (8, 4), (63, 64), (64, 63), (65, 63), (130, 64), (256, 64))       # the GPU suite's (max_obs, max_dyn)


def bits(v):
    return struct.pack("<d", float(v))


def kept_lists(c):
    s, d = port.perceive(c["state"], c["actors"], c["n_act"], D.params(c))
    return s, d


def test_the_table_is_a_few_hundred_vehicles_of_every_family():
    t = D.table()
    count = collections.Counter(c["family"] for c in t)
    assert set(count) == set(D.FAMILIES) and 200 <= len(t) <= 400, count
    assert count["plain"] >= 36 and min(count.values()) >= 8
    assert len({c["name"] for c in t}) == len(t)
    for c in t:
        assert c["actors"].shape == (D.A, 4) and c["state"].shape == (6,) and c["accel"].shape == (2,) and c["params"] in D.PARAM_SETS
        n = D.live(c["n_act"])
        pad = c["actors"][n:]
        assert np.isnan(pad[0::2]).all() and (pad[1::2] == 1e300).all(), c["name"]          # poisoned beyond n_act
        assert (c["label"] is not None) == (c["family"] in ("threshold", "ties")), c["name"]
    # the plain ones sit between the others
    fam = [c["family"] for c in t[:150]]
    assert all("plain" in fam[i:i + 3] for i in range(0, 147))


def test_the_port_reproduces_every_constructed_label():
    seen = 0
    for c in D.table():
        if c["label"] is None:
            continue
        s, d = kept_lists(c)
        assert [i for i, _ in s] == c["label"]["static"], c["name"]
        assert [i for i, _, _ in d] == c["label"]["dyn"], c["name"]
        r = port.request(c["state"], c["accel"], c["actors"], c["n_act"], 256, 64, D.params(c))
        assert r["n_obs"] == c["label"]["n_obs"] and r["req_status"] == 0, c["name"]
        seen += 1
    assert seen >= 25


def test_threshold_probes_have_the_bits_written_down():
    seen = collections.Counter()
    for c in D.table():
        if c["family"] != "threshold":
            continue
        assert c["state"][2] == 0.0 and c["state"][3] == 0.0 and c["state"][5] == 8.0
        for i, var, val in c["probes"]:
            m = dict(zip(("dis", "lat", "along", "speed"), port.measure(c["state"], c["actors"][i])))
            assert bits(m[var]) == bits(val), (c["name"], i, var, m[var].hex(), float(val).hex())
            seen[var] += 1
    assert set(seen) == {"dis", "lat", "along", "speed"} and min(seen.values()) >= 6


def test_exact_rational_arithmetic_agrees_with_the_float_decisions():
    """dis^2 against limit^2, lat, along and speed^2 from the exact values of the inputs (fi = 0: cos = 1, sin = 0, w = (Vx, 0))."""
    F = Fraction
    on_value = 0
    for c in D.table():
        if c["family"] != "threshold":
            continue
        prm = D.params(c)
        x, y, _, _, _, Vx = (F(float(v)) for v in c["state"])
        kept_s, kept_d = [], []
        for i in range(D.live(c["n_act"])):
            ax, ay, avx, avy = (F(float(v)) for v in c["actors"][i])
            dis2, lat, along, speed2 = (ax - x) ** 2 + (ay - y) ** 2, ay - y, (ax - x) * Vx, avx ** 2 + avy ** 2
            exact = (dis2 < F(prm["dis_limitation"]) ** 2, -F(prm["lateral_band"]) < lat, lat < F(prm["lateral_band"]), along > F(prm["behind"]),
                     speed2 > F(prm["dynamic_speed"]) ** 2)
            dis, flat, falong, speed = port.measure(c["state"], c["actors"][i])
            got = (dis < prm["dis_limitation"], -prm["lateral_band"] < flat, flat < prm["lateral_band"], falong > prm["behind"],
                   speed > prm["dynamic_speed"])
            if (i, "speed", 1.0) in c["probes"] and avx != 1:
                # (0.6, 0.8): the exact square sum of the two doubles is not 1; the FLOAT sum rounds to exactly 1, which is the point
                assert speed == 1.0 and speed2 != 1 and abs(speed2 - 1) < F(1, 2 ** 52)
                exact = exact[:4] + (False,)
            assert exact == got, (c["name"], i, exact, got)
            on_value += dis2 == F(prm["dis_limitation"]) ** 2 or abs(lat) == F(prm["lateral_band"]) or along == F(prm["behind"]) or speed2 == 1
            if all(exact[:4]):
                (kept_d if exact[4] else kept_s).append((dis2, i))
        assert [i for _, i in sorted(kept_s)] == c["label"]["static"] and [i for _, i in sorted(kept_d)] == c["label"]["dyn"], c["name"]
        gate = kept_s and min(kept_s)[0] <= F(prm["static_gate"]) ** 2
        assert c["label"]["n_obs"] == (len(kept_s) if gate else 0), c["name"]
    assert on_value >= 10


def test_tied_distances_are_bit_equal():
    widest = 0
    for c in D.table():
        if c["family"] != "ties":
            continue
        for tied in c["label"]["tied"]:
            dis = {bits(port.measure(c["state"], c["actors"][i])[0]) for i in tied}
            assert len(dis) <= 1, c["name"]
            widest = max(widest, len(tied))
        if "distinct" in c["name"]:
            assert len({tuple(r[:2]) for r in c["actors"]}) == D.A, c["name"]
        if "same" in c["name"]:
            for cls in c["label"]["tied"]:
                assert len({c["actors"][i].tobytes() for i in cls}) <= 1, c["name"]           # duplicates: all four fields
    assert widest == D.A
    assert len(set(D.tied_points(D.A))) == D.A


def test_no_case_outside_the_threshold_family_is_undecided():
    """Every case is checked; the share left out is 0 (a random case that came too close was drawn again where it was made)."""
    checked = 0
    for c in D.table():
        if c["family"] == "threshold":
            continue
        assert not D.undecided(c), (c["name"], D.undecided(c)[:3])
        checked += 1
    assert checked == sum(c["family"] != "threshold" for c in D.table())


def test_coverage_of_sides_counts_and_truncation():
    t = D.table()
    sides = collections.Counter()
    for c in t:
        for _, var, val, thr in D.decisions(c):
            if math.isfinite(val):
                sides[var, thr, "eq" if val == thr else "lt" if val < thr else "gt"] += 1
    for pset in D.PARAM_SETS:
        prm = D.params(pset)
        for var, thr in (("dis", prm["dis_limitation"]), ("lat", prm["lateral_band"]), ("lat", -prm["lateral_band"]), ("along", prm["behind"]),
                         ("speed", prm["dynamic_speed"]), ("gate", prm["static_gate"])):
            for side in ("lt", "eq", "gt"):
                assert sides[var, thr, side] >= 1, (pset, var, thr, side)
    assert {c["n_act"] for c in t} >= set(D.N_ACT_LISTED)
    kept = [tuple(len(k) for k in kept_lists(c)) for c in t]
    assert {s for s, _ in kept} >= set(D.KEPT_LISTED) | {0, 32} and {d for _, d in kept} >= set(D.KEPT_LISTED) | {0, 32}
    for mo, md in CONFIGS:
        trunc = [s > mo or d > md for s, d in kept]
        assert any(trunc) == (mo < 64 or md < 64) and not all(trunc), (mo, md)
        if mo <= 64:
            assert {mo, min(mo + 1, 64), 64} <= {s for s, _ in kept}, mo                     # exactly at, one above, and 64
        if md <= 64:
            assert {md, min(md + 1, 64), 64} <= {d for _, d in kept}, md
    names = {c["name"] for c in t}
    assert {"only_lane_0", "only_lane_63", "ascending", "descending", "zeros_np", "reversing", "sideways", "heading_1e6", "60_m_per_s",
            "actor_at_the_ego", "pair_across_classes", "actor_vx_nan", "ego_x_nan", "accel0_nan"} <= names


def test_what_the_port_returns_on_non_finite_input():
    """The sentences of include/emplanner.h, on the port."""
    by = {c["name"]: c for c in D.table()}
    rq = lambda c: port.request(c["state"], c["accel"], c["actors"], c["n_act"], 8, 4, D.params(c))
    for tag in ("nan", "pinf", "ninf"):
        for f in ("vx", "vy"):
            r = rq(by[f"actor_{f}_{tag}"])
            if tag == "nan":                                                   # NaN velocity: static
                assert D.NONFINITE_ACTOR in r["static_idx"] and D.NONFINITE_ACTOR not in r["dyn_idx"]
                assert np.isnan(r["actors_next"][D.NONFINITE_ACTOR, 0 if f == "vx" else 1])
            else:                                                              # infinite velocity: dynamic, advanced by inf * advance_s
                assert D.NONFINITE_ACTOR in r["dyn_idx"]
                assert np.isinf(r["actors_next"][D.NONFINITE_ACTOR, 0 if f == "vx" else 1])
        for f in ("x", "y"):
            r = rq(by[f"actor_{f}_{tag}"])
            assert D.NONFINITE_ACTOR not in r["static_idx"] + r["dyn_idx"] and r["n_static"] == 2 and r["n_dyn"] == 2
            r = rq(by[f"ego_{f}_{tag}"])                                       # a non-finite ego position keeps nothing
            assert r["n_static"] == 0 and r["n_dyn"] == 0 and r["n_obs"] == 0 and np.isnan(r["dyn_dis_speed"]).all()
            assert not np.isfinite(r["start_xy"][0 if f == "x" else 1])
        r = rq(by[f"ego_fi_dot_{tag}"])                                        # fi_dot reaches pred_fi only
        assert not np.isfinite(r["pred_fi"]) and np.isfinite(r["start_xy"]).all() and r["n_static"] == 2 and r["n_dyn"] == 3
        for j in range(2):                                                     # accel reaches start_a only
            r = rq(by[f"accel{j}_{tag}"])
            assert not np.isfinite(r["start_a"][j]) and np.isfinite(r["start_a"][1 - j]) and np.isfinite(r["start_xy"]).all()
            assert r["n_static"] == 2 and r["n_dyn"] == 3
    assert np.isnan(rq(by["ego_x_nan"])["start_xy"][0])
    import drive_timed_port as tport
    c = by["zeros_np"]                                                         # Vx = -0.0 at fi = 0: the heading is pi
    t = tport.request_timed(c["state"], c["accel"], c["actors"], c["n_act"], 8, 4, 0.0, 0, 0.01, prm=D.params(c))
    assert t["start_heading"] == math.pi
    # Vx = Vy = -0.0: wx = -0 - (-0) = +0 and wy = -0 + -0 = -0, so the heading is -0.0; the other two are +0.0
    for name, want in (("zeros_nn", -0.0), ("zeros_pp", 0.0), ("zeros_pn", 0.0), ("standstill", 0.0)):
        c = by[name]
        h = tport.request_timed(c["state"], c["accel"], c["actors"], c["n_act"], 8, 4, 0.0, 0, 0.01, prm=D.params(c))["start_heading"]
        assert bits(h) == bits(want), name
