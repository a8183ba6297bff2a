"""Case table of the hard-input tests of emp_drive_request / emp_drive_request_timed (tests/test_drive_request_cases_host.py on the
CPU, tests/test_gpu_drive_request_cases.py on the device).  A plain helper module: no fixtures, no hooks, NumPy and tests/drive_port.py
only.  Each case is ONE vehicle with all 64 actor slots allocated: state[6], actors[64][4], n_act, accel[2], the name of a parameter
set and a family.  Slots at or beyond n_act are poisoned, alternately NaN and 1e300.

Families
  threshold  fi = 0, Vy = 0, Vx = 8 and a dyadic position: cos = 1, sin = 0, lat = y_a - y, along = 8 (x_a - x), every subtraction
             exact.  For each comparison of the kernel three actors: on the value, one ulp to each side.  LABELLED.
  ties       the ego at the origin (dis does not depend on the heading); two to 64 actors at one computed distance.  LABELLED.
  capacity   kept counts at and around the output capacities, every n_act of interest, ascending and descending distances.
  nonfinite  NaN, +inf, -inf in every actor field, every ego field and the acceleration.
  ego        standstill, signed zeros, reversing, sideways, fi = +-pi and 1e6, 60 m/s, an actor at the ego's position.
  plain      random vehicles at general headings: the neighbours of the others in every batch.
A label is WRITTEN DOWN where the case is constructed - the kept actor indices of each class in output order and the gated static
count - never computed from the inputs; `probes` name the decision variable that sits on a threshold and the value it must have.

Outside `threshold` no finite decision variable lies within MARGIN (relative to max(1, |threshold|)) of its threshold: the device's
sin / cos may differ from the host's in the last bit, which moves lat and along by some 1e-12 at these magnitudes.  A random case
that comes closer is drawn again, so no case is ever left out as undecided."""
from __future__ import annotations

import functools
import math

import numpy as np

import drive_port as port

A = 64
NAN, INF = math.nan, math.inf
MARGIN = 1e-9
ADVANCE_S = 0.05
PARAM_SETS = {"default": {}, "wide": dict(lateral_band=45.0, behind=0.0)}
FAMILIES = ("threshold", "ties", "capacity", "nonfinite", "ego", "plain")
N_ACT_LISTED = (0, -3, 1, 63, 64, 1000)
KEPT_LISTED = (1, 2, 63, 64)                 # kept statics / dynamics: max_obs and max_obs + 1 for 1 and 63, and 64
NONFINITE = (("nan", NAN), ("pinf", INF), ("ninf", -INF))


def params(case_or_name, **kw):
    """drive_port's parameter dict of a case (or of a parameter set's name)."""
    name = case_or_name if isinstance(case_or_name, str) else case_or_name["params"]
    return port.params(**dict(PARAM_SETS[name], advance_s=ADVANCE_S, **kw))


def live(n_act):
    return min(max(int(n_act), 0), A)


def _case(family, name, state, rows, n_act=None, accel=(0.25, -0.5), pset="default", label=None, probes=()):
    """rows: the live actors (x, y, vx, vy); n_act: what the caller claims (default: len(rows))."""
    rows = [tuple(float(v) for v in r) for r in rows]
    assert len(rows) <= A
    n_act = len(rows) if n_act is None else int(n_act)
    assert live(n_act) <= len(rows) or not rows
    actors = np.zeros((A, 4))
    if rows:
        actors[:len(rows)] = rows
    n = live(n_act)
    actors[n:] = np.where(np.arange(A - n)[:, None] % 2 == 0, NAN, 1e300)
    return dict(family=family, name=name, state=np.array(state, np.float64), actors=actors, n_act=n_act, accel=np.array(accel, np.float64),
                params=pset, label=label, probes=tuple(probes))


def place(state, ahead, side):
    """The point `ahead` metres in front of and `side` metres to the left of a vehicle."""
    x, y, fi = (float(v) for v in state[:3])
    return x + ahead * math.cos(fi) - side * math.sin(fi), y + ahead * math.sin(fi) + side * math.cos(fi)


def off(base, d):
    """base + d where the sum, and the difference that gives d back, are exact."""
    v = base + d
    assert v - base == d and base - v == -d, (base, d)
    return v


# ---------------------------------------------------------------------------------------------------------------------
# threshold
# ---------------------------------------------------------------------------------------------------------------------
EGO_T = (0.5, -0.25, 0.0, 0.0, 0.125, 8.0)
nx = math.nextafter
ONE_UP, ONE_DOWN = nx(1.0, INF), nx(1.0, 0.0)


def _offsets(state, rows):
    return [(off(state[0], r[0]), off(state[1], r[1])) + tuple(r[2:]) + (0.0,) * (4 - len(r)) for r in rows]


def _threshold():
    out = []
    # the six actor comparisons, default parameters: (x_a - x, y_a - y[, vx, vy])
    rows = [(50.0, 0.0), (nx(50.0, 0.0), 0.0), (nx(50.0, INF), 0.0),                       # 0-2   dis < 50
            (10.0, 5.0), (10.0, nx(5.0, 0.0)), (10.0, nx(5.0, INF)),                       # 3-5   lat < 5
            (12.0, -5.0), (12.0, nx(-5.0, 0.0)), (12.0, nx(-5.0, -INF)),                   # 6-8   -5 < lat
            (-1.25, 0.0), (nx(-1.25, 0.0), 0.0), (nx(-1.25, -INF), 0.0),                   # 9-11  along > -10
            (20.0, 1.0, 1.0, 0.0), (21.0, 1.0, 0.6, 0.8), (22.0, 1.0, ONE_UP, 0.0), (23.0, 1.0, ONE_DOWN, 0.0)]   # 12-15 speed > 1
    probes = [(0, "dis", 50.0), (1, "dis", nx(50.0, 0.0)), (2, "dis", nx(50.0, INF)),
              (3, "lat", 5.0), (4, "lat", nx(5.0, 0.0)), (5, "lat", nx(5.0, INF)),
              (6, "lat", -5.0), (7, "lat", nx(-5.0, 0.0)), (8, "lat", nx(-5.0, -INF)),
              (9, "along", -10.0), (10, "along", nx(-10.0, 0.0)), (11, "along", nx(-10.0, -INF)),
              (12, "speed", 1.0), (13, "speed", 1.0), (14, "speed", ONE_UP), (15, "speed", ONE_DOWN)]
    # kept: 1 (just inside 50), 4, 7 (just inside the band), 10 (just in front of `behind`), 12, 13, 15 static, 14 dynamic
    out.append(_case("threshold", "six_comparisons", EGO_T, _offsets(EGO_T, rows), probes=probes,
                     label=dict(static=[10, 4, 7, 12, 13, 15, 1], dyn=[14], n_obs=7)))
    # the gate static_dis[0] <= 30
    far = (40.0, 1.0)
    out.append(_case("threshold", "gate_on_30", EGO_T, _offsets(EGO_T, [(30.0, 0.0), far]), probes=[(0, "dis", 30.0)],
                     label=dict(static=[0, 1], dyn=[], n_obs=2)))
    out.append(_case("threshold", "gate_inside_30", EGO_T, _offsets(EGO_T, [(nx(30.0, 0.0), 0.0), far]), probes=[(0, "dis", nx(30.0, 0.0))],
                     label=dict(static=[0, 1], dyn=[], n_obs=2)))
    out.append(_case("threshold", "gate_beyond_30", EGO_T, _offsets(EGO_T, [far, (nx(30.0, INF), 0.0)]), probes=[(1, "dis", nx(30.0, INF))],
                     label=dict(static=[1, 0], dyn=[], n_obs=0)))
    out.append(_case("threshold", "gate_dynamic_inside_static_beyond", EGO_T,
                     _offsets(EGO_T, [(20.0, 0.0, 3.0, 0.0), (nx(30.0, INF), 0.0), far]), probes=[(1, "dis", nx(30.0, INF))],
                     label=dict(static=[1, 2], dyn=[0], n_obs=0)))
    # lateral_band = 45, behind = 0: (30, 40) lies at dis == 50 off the axis; the neighbours of `behind` = 0 are one ulp of x_a
    rows = [(30.0, 40.0), (30.0, nx(40.0, 0.0)), (30.0, nx(40.0, INF)),
            (10.0, 45.0), (10.0, nx(45.0, 0.0)), (10.0, nx(45.0, INF)),
            (12.0, -45.0), (12.0, nx(-45.0, 0.0)), (12.0, nx(-45.0, -INF)),
            (0.0, 2.0), (2.0 ** -53, 2.0), (-2.0 ** -54, 2.0),
            (20.0, 1.0, 1.0, 0.0), (21.0, 1.0, 0.6, 0.8), (22.0, 1.0, ONE_UP, 0.0), (23.0, 1.0, ONE_DOWN, 0.0)]
    probes = [(0, "dis", 50.0), (1, "dis", nx(50.0, 0.0)), (2, "dis", nx(50.0, INF)),
              (3, "lat", 45.0), (4, "lat", nx(45.0, 0.0)), (5, "lat", nx(45.0, INF)),
              (6, "lat", -45.0), (7, "lat", nx(-45.0, 0.0)), (8, "lat", nx(-45.0, -INF)),
              (9, "along", 0.0), (10, "along", 2.0 ** -50), (11, "along", -2.0 ** -51),
              (12, "speed", 1.0), (13, "speed", 1.0), (14, "speed", ONE_UP), (15, "speed", ONE_DOWN)]
    out.append(_case("threshold", "six_comparisons_wide", EGO_T, _offsets(EGO_T, rows), pset="wide", probes=probes,
                     label=dict(static=[10, 12, 13, 15, 4, 7, 1], dyn=[14], n_obs=7)))
    out.append(_case("threshold", "gate_on_30_wide", EGO_T, _offsets(EGO_T, [(18.0, 24.0), far]), pset="wide", probes=[(0, "dis", 30.0)],
                     label=dict(static=[0, 1], dyn=[], n_obs=2)))
    out.append(_case("threshold", "gate_beyond_30_wide", EGO_T, _offsets(EGO_T, [(18.0, nx(24.0, INF)), far]), pset="wide",
                     probes=[(0, "dis", nx(30.0, INF))], label=dict(static=[0, 1], dyn=[], n_obs=0)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# ties
# ---------------------------------------------------------------------------------------------------------------------
HEADINGS = (0.0, 0.7, -2.5, math.pi)
IMAGES = ((3, 4), (4, 3), (-3, 4), (4, -3), (-4, -3), (-3, -4), (3, -4), (-4, 3))      # sign and swap images of (3, 4)
IMAGE_SCALE = 0.125              # radius 0.625: |lat| < 5 and along >= -5 > -10 at every heading
MOVING = (3.0, 0.0)


@functools.lru_cache(maxsize=None)
def tied_points(n):
    """n DISTINCT points of one computed distance: integer solutions of a^2 + b^2 = 1105^2 (108 of them) over 1024.  The squares
    and their sum are exact and so is the root, 1105 / 1024 = 1.079 m: inside the band and in front of `behind` at every heading.
    Shuffled, so that the index order is no geometric order."""
    R = 1105
    pts = []
    for a in range(-R, R + 1):
        b = math.isqrt(R * R - a * a)
        if b * b == R * R - a * a:
            pts.extend({(a, b), (a, -b)})
    pts.sort()
    assert len(pts) >= n
    pick = np.random.default_rng(1105).permutation(len(pts))[:n]
    return tuple((pts[i][0] / 1024.0, pts[i][1] / 1024.0) for i in pick)


def _ties():
    out = []
    for h in HEADINGS:
        ego = (0.0, 0.0, h, 0.0, 0.0, 8.0)
        for k in (2, 3, 8):
            # 0: a static far ahead; 1..k: the tied ones (with k = 8 every second one moves); k + 1: a static nearer than all
            rows = [place(ego, 20.0, 1.0) + (0.0, 0.0)]
            moving = [k == 8 and j % 2 == 1 for j in range(k)]
            rows += [(IMAGE_SCALE * IMAGES[j][0], IMAGE_SCALE * IMAGES[j][1]) + (MOVING if moving[j] else (0.0, 0.0)) for j in range(k)]
            rows.append(place(ego, 0.25, 0.0) + (0.0, 0.0))
            tied_s = [1 + j for j in range(k) if not moving[j]]
            tied_d = [1 + j for j in range(k) if moving[j]]
            out.append(_case("ties", f"images_{k}_heading_{h:.1f}", ego, rows,
                             label=dict(static=[k + 1] + tied_s + [0], dyn=tied_d, n_obs=len(tied_s) + 2, tied=[tied_s, tied_d])))
    # equal dis in different classes: neither counts for the other's rank
    ego = (0.0, 0.0, 0.7, 0.0, 0.0, 8.0)
    p, q, r = tied_points(3)
    out.append(_case("ties", "pair_across_classes", ego, [p + MOVING, p + (0.0, 0.0), q + (0.0, 0.0), r + MOVING],
                     label=dict(static=[1, 2], dyn=[0, 3], n_obs=2, tied=[[1, 2], [0, 3]])))
    # 64 at one distance: one identical position (duplicates identical in all four fields) and 64 distinct positions
    layouts = dict(interleaved=lambda i: i % 2 == 1, blocks=lambda i: i >= 32, all_static=lambda i: False, all_dynamic=lambda i: True)
    for f, (form, pts) in enumerate((("same", (tied_points(1)[0],) * A), ("distinct", tied_points(A)))):
        for j, (lname, dyn) in enumerate(layouts.items()):
            ego = (0.0, 0.0, HEADINGS[(j + f) % 4], 0.0, 0.0, 8.0)
            rows = [pts[i] + (MOVING if dyn(i) else (0.0, 0.0)) for i in range(A)]
            s, d = [i for i in range(A) if not dyn(i)], [i for i in range(A) if dyn(i)]
            out.append(_case("ties", f"tie64_{form}_{lname}", ego, rows, n_act=1000 if j % 2 else A,
                             label=dict(static=s, dyn=d, n_obs=len(s), tied=[s, d])))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# capacity
# ---------------------------------------------------------------------------------------------------------------------
EGO_C = (12.5, -7.25, 0.3, 0.1, 0.02, 9.0)


def _lanes(order, cls, n_kept=A, kept_from=0):
    """64 actors 1 m beside the axis; those in [kept_from, kept_from + n_kept) between 1.5 and 45.6 m ahead (ascending or descending
    with the index), the others 60 m and more ahead: out of range.  cls(i) -> moving?"""
    rows = []
    for i in range(A):
        kept = kept_from <= i < kept_from + n_kept
        step = i if order == "ascending" else A - 1 - i
        ahead = 1.5 + 0.7 * step if kept else 60.0 + step
        rows.append(place(EGO_C, ahead, 1.0 if i % 2 else -1.0) + ((2.0, 1.0) if cls(i) else (0.0, 0.0)))
    return rows


def _capacity():
    out = []
    for n in KEPT_LISTED:
        out.append(_case("capacity", f"kept_static_{n}", EGO_C, _lanes("ascending", lambda i: False, n, kept_from=(A - n) // 2)))
        out.append(_case("capacity", f"kept_dynamic_{n}", EGO_C, _lanes("descending", lambda i: True, n, kept_from=(A - n) // 3)))
    for n_act in N_ACT_LISTED:
        rows = _lanes("ascending" if n_act % 2 else "descending", lambda i: i % 3 == 0)
        out.append(_case("capacity", f"n_act_{n_act}", EGO_C, rows[:live(n_act)], n_act=n_act))
    out.append(_case("capacity", "only_lane_0", EGO_C, _lanes("ascending", lambda i: False, 1, kept_from=0)))
    out.append(_case("capacity", "only_lane_63", EGO_C, _lanes("ascending", lambda i: True, 1, kept_from=63), n_act=1000))
    out.append(_case("capacity", "descending", EGO_C, _lanes("descending", lambda i: i % 2 == 1)))
    out.append(_case("capacity", "ascending", EGO_C, _lanes("ascending", lambda i: i % 2 == 1)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# nonfinite
# ---------------------------------------------------------------------------------------------------------------------
EGO_N = (3.0, -2.0, 0.3, 0.2, 0.05, 7.0)
NONFINITE_ACTOR = 2


def _around(ego):
    return [place(ego, 10.0, 1.0) + (0.0, 0.0), place(ego, 15.0, -1.0) + (4.0, 1.0), place(ego, 20.0, 0.5) + (2.0, 1.0),
            place(ego, 28.0, 2.0) + (0.0, 0.0), place(ego, 35.0, -2.0) + (0.0, -3.0), place(ego, 60.0, 0.0) + (0.0, 0.0)]


def _nonfinite():
    out = []
    for tag, v in NONFINITE:
        for f, fname in enumerate(("x", "y", "vx", "vy")):
            rows = [list(r) for r in _around(EGO_N)]
            rows[NONFINITE_ACTOR][f] = v
            out.append(_case("nonfinite", f"actor_{fname}_{tag}", EGO_N, rows))
        for f, fname in enumerate(("x", "y", "fi", "Vy", "fi_dot", "Vx")):
            ego = list(EGO_N)
            ego[f] = v
            out.append(_case("nonfinite", f"ego_{fname}_{tag}", ego, _around(EGO_N)))
        for j in range(2):
            accel = [0.25, -0.5]
            accel[j] = v
            out.append(_case("nonfinite", f"accel{j}_{tag}", EGO_N, _around(EGO_N), accel=accel))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# ego
# ---------------------------------------------------------------------------------------------------------------------
def _neighbours(ego):
    """(ahead, side, moving) around any vehicle: in front and behind, inside and outside the band and the range."""
    spots = ((5.0, 0.5, 0), (12.0, -2.0, 1), (25.0, 1.0, 0), (31.0, 3.0, 0), (45.0, -1.0, 1), (-0.5, 0.5, 0), (-3.0, 1.0, 1),
             (20.0, 6.0, 0), (55.0, 0.0, 0))
    return [place(ego, a, s) + ((1.5, -2.5) if m else (0.0, 0.0)) for a, s, m in spots]


def _ego():
    out = []
    pos = (1.5, 2.25)
    for name, fi, Vy, Vx in (("standstill", 0.0, 0.0, 0.0), ("standstill_heading_0.3", 0.3, 0.0, 0.0),
                             ("zeros_pp", 0.0, 0.0, 0.0), ("zeros_np", 0.0, 0.0, -0.0), ("zeros_pn", 0.0, -0.0, 0.0), ("zeros_nn", 0.0, -0.0, -0.0),
                             ("reversing", 0.0, 0.0, -3.0), ("reversing_heading_0.7", 0.7, 0.1, -3.0), ("sideways", 0.0, 2.0, 0.0),
                             ("heading_pi", math.pi, 0.1, 8.0), ("heading_minus_pi", -math.pi, -0.1, 8.0), ("heading_1e6", 1e6, 0.1, 8.0),
                             ("60_m_per_s", -1.1, 0.3, 60.0)):
        ego = pos + (fi, Vy, 0.03, Vx)
        out.append(_case("ego", name, ego, _neighbours(ego)))
    ego = pos + (0.4, 0.0, 0.0, 8.0)
    out.append(_case("ego", "actor_at_the_ego", ego, _neighbours(ego) + [pos + (0.0, 0.0), pos + (0.0, 2.0)]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# plain, and the margin rule
# ---------------------------------------------------------------------------------------------------------------------
def decisions(c):
    """Every decision variable of a case against its threshold: (actor index or -1, name, value, threshold).  The gate's variable is
    the nearest kept static's dis (index -1)."""
    prm = params(c)
    out = []
    for i in range(live(c["n_act"])):
        dis, lat, along, speed = port.measure(c["state"], c["actors"][i])
        out += [(i, "dis", dis, prm["dis_limitation"]), (i, "lat", lat, prm["lateral_band"]), (i, "lat", lat, -prm["lateral_band"]),
                (i, "along", along, prm["behind"]), (i, "speed", speed, prm["dynamic_speed"])]
    statics, _ = port.perceive(c["state"], c["actors"], c["n_act"], prm)
    if statics:
        out.append((-1, "gate", statics[0][1], prm["static_gate"]))
    return out


def undecided(c, margin=MARGIN):
    """The finite decision variables within `margin` of their thresholds."""
    return [d for d in decisions(c) if math.isfinite(d[2]) and abs(d[2] - d[3]) <= margin * max(1.0, abs(d[3]))]


def _plain(n_default=96, n_wide=24):
    rng = np.random.default_rng(389)
    out = []
    for k in range(n_default + n_wide):
        pset = "default" if k < n_default else "wide"
        while True:
            ego = (rng.uniform(-100, 100), rng.uniform(-100, 100), rng.uniform(-math.pi, math.pi), rng.normal(0, 0.3), rng.normal(0, 0.1),
                   rng.uniform(2.0, 20.0))
            n = int(rng.integers(0, A + 1))
            rows = []
            for _ in range(n):
                kind = rng.integers(0, 3)
                v = 0.0 if kind == 0 else rng.uniform(0.2, 0.9) if kind == 1 else rng.uniform(1.2, 15.0)
                th = rng.uniform(-math.pi, math.pi)
                rows.append(place(ego, rng.uniform(-15.0, 60.0), rng.uniform(-8.0, 8.0) if pset == "default" else rng.uniform(-60.0, 60.0))
                            + (v * math.cos(th), v * math.sin(th)))
            c = _case("plain", f"plain_{k}", ego, rows, accel=rng.normal(0, 1, 2), pset=pset)
            if not undecided(c):
                break
        out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def table():
    """All cases, the plain ones spread between the others so that every hostile vehicle has ordinary neighbours."""
    special = _threshold() + _ties() + _capacity() + _nonfinite() + _ego()
    plain = _plain()
    out, per = [], max(1, len(special) // len(plain) + 1)
    it = iter(plain)
    for i, c in enumerate(special):
        out.append(c)
        if i % per == per - 1:
            nxt_plain = next(it, None)
            if nxt_plain is not None:
                out.append(nxt_plain)
    out.extend(it)
    return tuple(out)


def group(pset):
    """The cases of one parameter set and their arrays: (cases, state, accel, actors, n_act)."""
    cases = [c for c in table() if c["params"] == pset]
    return (cases, np.array([c["state"] for c in cases]), np.array([c["accel"] for c in cases]), np.array([c["actors"] for c in cases]),
            np.array([c["n_act"] for c in cases], np.int32))
